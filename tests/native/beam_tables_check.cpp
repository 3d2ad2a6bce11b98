// Stand-alone check of the beam-table compiler (csrc/mc_beams.h
// compile_beams, build_fan), for a host-only build with sanitizers
// (tests/test_beam_tables_host.py builds and runs it; no HIP call).
//
// Input (a text file): per case one line "beams range H Wp Lp N lanes fan"
// (fan: build_fan must accept the set), then per beam its increment row
// "xinc yinc distinc" and the test's own record "K axis sign msign bits".
// compile_beams' records must equal the test's, its flags, kmax, kmin and k1
// a brute force over the per-start words; build_fan's words are decoded by
// their layout comments alone (mc_internal.h State::fan_data, "Fan march")
// and every beam's path must be in them once.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "mc_beams.h"

static int fails = 0;
#define CHECK(c, ...)                     \
  do {                                    \
    if (!(c)) {                           \
      if (++fails <= 20) {                \
        std::printf("FAIL " __VA_ARGS__); \
        std::printf("\n");                \
      }                                   \
    }                                     \
  } while (0)

struct Rec {
  int K, axis, sign, msign;
  unsigned bits;
};
struct Case {
  int nb, H, Wp, Lp, N, lanes, fan;
  double range;
  std::vector<double> tab;
  std::vector<Rec> recs;
};

// minor cell after steps 1..K from start c0 with step word w
static std::vector<int> path(uint64_t w, int c0, int K, int msign) {
  std::vector<int> p;
  for (int k = 0, c = c0; k < K; ++k) p.push_back(c += ((w >> k) & 1) ? msign : 0);
  return p;
}

// start c0's own march differs from the common word's at or before the step
// that reaches a border cell of the minor axis (0 or cm - 1)
static bool diverges(uint64_t own, uint64_t common, int c0, int cm, int K, int msign) {
  const std::vector<int> a = path(own, c0, K, msign), c = path(common, c0, K, msign);
  for (int k = 0; k < K; ++k) {
    if (a[k] != c[k]) return true;
    if (a[k] <= 0 || a[k] >= cm - 1) return false;
  }
  return false;
}

// what a sector slot or a beam contributes to the march: its class (FAN_COLS,
// FAN_NEG, minor side), and per step the signed minor offset and "in range"
struct Sig {
  std::vector<int> v;
  bool operator<(const Sig& o) const { return v < o.v; }
  bool operator==(const Sig& o) const { return v == o.v; }
};
static Sig beam_sig(const mc::Beam& o, int kmax) {
  Sig s;
  s.v = {(o.axis & 1) ? 1 : 0, o.sign < 0 ? 1 : 0, o.msign < 0 ? 1 : 0};
  for (int k = 1; k <= kmax; ++k) {
    s.v.push_back(o.msign * __builtin_popcount(o.bits & ((1u << k) - 1u)));
    s.v.push_back(o.K >= k);
  }
  return s;
}

static void check_tables(const Case& c, const mc::BeamTables& T) {
  const int nb = c.nb;
  CHECK((int)T.bt.size() == nb && T.cmax == std::max(c.Wp, c.Lp) && T.bits.size() == (size_t)nb * T.cmax, "sizes");
  int kmax = 0, kmin = 1 << 30;
  uint32_t k1 = 1u << 4;
  bool common = true;
  for (int b = 0; b < nb; ++b) {
    const mc::Beam& o = T.bt[b];
    const Rec& r = c.recs[b];
    kmax = std::max(kmax, r.K);
    kmin = std::min(kmin, r.K);
    CHECK(o.K == r.K && (o.axis & 1) == r.axis && o.sign == r.sign && o.msign == r.msign,
          "beam %d: K %d axis %d sign %d msign %d, want %d %d %d %d", b, o.K, o.axis & 1, o.sign, o.msign, r.K, r.axis,
          r.sign, r.msign);
    const int cm = r.axis == 0 ? c.Lp : c.Wp;
    const uint64_t* row = &T.bits[(size_t)b * T.cmax];
    bool flag = false;
    for (int c0 = 1; c0 + 1 < cm; ++c0) flag = flag || diverges(row[c0], o.bits, c0, cm, r.K, r.msign);
    CHECK(((o.axis & 2) != 0) == flag, "beam %d: flagged %d, brute force %d", b, (o.axis & 2) != 0, (int)flag);
    if (flag && nb == 360) std::printf("360 beams: beam %d (%d degrees) is flagged\n", b, b);
    common = common && !flag;
    const unsigned low = r.K >= 32 ? ~0u : (1u << r.K) - 1u;
    if (!flag) CHECK((o.bits & low) == (r.bits & low), "beam %d: common bits %x, want %x", b, o.bits & low, r.bits & low);
    if (r.K >= 1) {  // the step-1 cell around the robot, bit 3 * (dx + 1) + (dy + 1)
      const int mv = (o.bits & 1u) ? r.msign : 0;
      k1 |= 1u << (r.axis == 0 ? 3 * (r.sign + 1) + (mv + 1) : 3 * (mv + 1) + (r.sign + 1));
    }
  }
  CHECK(T.kmax == kmax && T.kmin == kmin, "kmax %d kmin %d, want %d %d", T.kmax, T.kmin, kmax, kmin);
  CHECK(T.k1 == k1, "k1 %x, want %x", T.k1, k1);
  CHECK(T.common == common, "common %d, want %d", (int)T.common, (int)common);
}

static void check_fan(const Case& c, const mc::BeamTables& T) {
  std::vector<uint32_t> w(3, 7u);
  int nsec = -1, nspec = -1;
  const bool on = mc::build_fan(T, c.Wp, c.Lp, c.N, c.lanes, w, nsec, nspec);
  CHECK(on == (c.fan != 0), "%d beams: build_fan returned %d", c.nb, (int)on);
  if (!on || !c.fan) return;
  const int kt = T.kmax, pair_words = 2 * (kt + 1), lutw = mc::kFanLutBytes / 4;
  CHECK(w.size() % 4 == 0, "%zu words are no multiple of 4", w.size());
  CHECK(nsec % 2 == 0 && w.size() >= (size_t)lutw + (size_t)nsec / 2 * pair_words + 8 * (size_t)nspec &&
            w.size() < (size_t)lutw + (size_t)nsec / 2 * pair_words + 8 * (size_t)nspec + 4,
        "%zu words for %d sectors, %d specials", w.size(), nsec, nspec);
  if (fails) return;
  // the LUTs: beam i of a sector stands popcount(D & low i bits) cells past beam 0
  const uint8_t* lut = reinterpret_cast<const uint8_t*>(w.data());
  for (int D = 0; D < 32; ++D)
    for (int A = 0; A < 64; ++A) {
      int lit = 0, on_cells = 0;
      for (int i = 0; i < mc::kFanS; ++i) {
        const int cell = __builtin_popcount(D & ((1 << i) - 1));
        if ((A >> i) & 1) lit |= 1 << cell;
        if ((A >> cell) & 1) on_cells |= 1 << i;
      }
      CHECK(lut[D * 64 + A] == lit && lut[2048 + D * 64 + A] == on_cells, "LUT D %d A %d", D, A);
    }
  std::vector<Sig> slots, beams;
  std::vector<int> spec_refs(nspec, 0);
  const uint32_t* specs = &w[lutw + (size_t)nsec / 2 * pair_words];
  for (int p = 0; p < nsec / 2; ++p) {
    const uint32_t* rec = &w[lutw + (size_t)p * pair_words];
    CHECK((rec[0] & 3u) == (rec[1] & 3u), "pair %d: classes %u and %u", p, rec[0] & 3u, rec[1] & 3u);
    for (int side = 0; side < 2; ++side) {
      const uint32_t d = rec[side];
      uint32_t present = 0;
      for (int k = 1; k <= kt; ++k) present |= (rec[2 * k + side] >> 16);
      const int n = __builtin_popcount(present);
      CHECK(present == (1u << n) - 1u && n <= mc::kFanS, "pair %d side %d: beams 0x%x", p, side, present);
      for (int j = 0; j < n; ++j) {
        Sig s;
        s.v = {(d & mc::FAN_COLS) ? 1 : 0, (d & mc::FAN_NEG) ? 1 : 0, side};
        for (int k = 1; k <= kt; ++k) {
          const uint32_t e = rec[2 * k + side];
          const int lo = (int)(e & 63u) - 32, D = (int)((e >> 6) & 31u);
          s.v.push_back(lo + __builtin_popcount(D & ((1 << j) - 1)));
          s.v.push_back((int)((e >> (16 + j)) & 1u));
        }
        if ((d & mc::FAN_SPECIAL) && (int)((d >> 3) & 7u) == j) {
          const int si = (int)(d >> 8);
          CHECK(si < nspec, "pair %d side %d: special record %d of %d", p, side, si, nspec);
          if (si < nspec) {
            ++spec_refs[si];
            const int b = (int)specs[8 * si];
            CHECK(b >= 0 && b < c.nb && (T.bt[b].axis & 2) && beam_sig(T.bt[b], kt) == s, "special %d: beam %d", si, b);
          }
        }
        slots.push_back(s);
      }
      if (d & mc::FAN_SPECIAL) CHECK((int)((d >> 3) & 7u) < n, "pair %d side %d: special slot past the sector", p, side);
      if (n == 0) CHECK(d == (rec[side ^ 1] & 3u), "pair %d: empty sector's word %x", p, d);
    }
  }
  // every beam's path is in exactly one slot: the two multisets are equal
  int flagged = 0;
  for (const mc::Beam& o : T.bt) {
    beams.push_back(beam_sig(o, kt));
    flagged += (o.axis & 2) != 0;
  }
  std::sort(slots.begin(), slots.end());
  std::sort(beams.begin(), beams.end());
  CHECK(slots == beams, "%zu sector slots do not hold the %zu beams once each", slots.size(), beams.size());
  CHECK(flagged == nspec, "%d flagged beams, %d special records", flagged, nspec);
  for (int si = 0; si < nspec; ++si) {  // one sector each: at most one special beam per sector
    CHECK(spec_refs[si] == 1, "special record %d is named by %d sectors", si, spec_refs[si]);
    const uint32_t* r = specs + 8 * si;
    const int b = (int)r[0];
    if (b < 0 || b >= c.nb) continue;
    const mc::Beam& o = T.bt[b];
    CHECK(r[1] == (((o.axis & 1) ? mc::FAN_COLS : 0u) | (o.sign < 0 ? mc::FAN_NEG : 0u)) && (int)r[2] == o.msign &&
              (int)r[3] == o.K, "special %d: class %u msign %d K %d", si, r[1], (int)r[2], (int)r[3]);
    const int cm = (o.axis & 1) == 0 ? c.Lp : c.Wp, elo = (int)r[4], ehi = (int)r[5];
    for (int c0 = 1; c0 + 1 < cm; ++c0)
      if (diverges(T.bits[(size_t)b * T.cmax + c0], o.bits, c0, cm, o.K, o.msign))
        CHECK(elo <= c0 && c0 <= ehi, "special %d: start %d diverges outside [%d, %d]", si, c0, elo, ehi);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: %s CASES.txt\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::printf("cannot open %s\n", argv[1]);
    return 2;
  }
  int cases = 0;
  Case c;
  while (std::fscanf(f, "%d %la %d %d %d %d %d %d", &c.nb, &c.range, &c.H, &c.Wp, &c.Lp, &c.N, &c.lanes, &c.fan) == 8) {
    c.tab.assign(3 * (size_t)(c.nb > 0 ? c.nb : 0), 0.0);
    c.recs.assign((size_t)(c.nb > 0 ? c.nb : 0), Rec{});
    for (int b = 0; b < c.nb; ++b) {
      Rec& r = c.recs[b];
      if (std::fscanf(f, "%la %la %la %d %d %d %d %u", &c.tab[3 * b], &c.tab[3 * b + 1], &c.tab[3 * b + 2], &r.K, &r.axis,
                      &r.sign, &r.msign, &r.bits) != 8) {
        std::printf("bad beam line in case %d\n", cases);
        std::fclose(f);
        return 2;
      }
    }
    mc::BeamTables T;
    std::string err;
    const bool ok = mc::compile_beams(c.tab.data(), c.nb, c.range, c.H, c.Wp, c.Lp, T, err);
    CHECK(ok, "compile_beams refused %d beams: %s", c.nb, err.c_str());
    if (ok) {
      check_tables(c, T);
      check_fan(c, T);
    }
    ++cases;
  }
  std::fclose(f);
  if (fails || cases == 0) {
    std::printf("%d failures in %d cases\n", fails, cases);
    return 1;
  }
  std::printf("ok %d cases\n", cases);
  return 0;
}
