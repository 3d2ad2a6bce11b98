// mc_beams.h — the beam-table compiler of mc_set_beam_table (mc_capi.hip):
// from the reference's increment table to the beam records, their per-start
// step words, the ray programs of the sparse-beam march and the fan data of
// the dense one.  Host-only and pure (no HIP call, no environment read):
// tests/native/beam_tables_check.cpp and ray_prog_check.cpp include it.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mc_internal.h"
#include "mc_msg.h"

namespace mc {

struct BeamTables {
  std::vector<Beam> bt;
  std::vector<uint64_t> bits;  // [beam][cmax]: the step word of every minor start (Beam's comment)
  int cmax = 0;                // max(Wp, Lp)
  int kmax = 0, kmin = 1 << 30;
  bool common = true;  // every beam has a common pattern (none flagged)
  uint32_t k1 = 0;     // State::beam_k1 of the common patterns
};

// A beam's major axis, signs and K from its (xinc, yinc, distinc) row;
// `minor`: its increment along the minor axis.
inline bool beam_axis_and_k(const double* row, int b, double range, int H, Beam& o, double& minor, std::string& err) {
  const double xi = row[0], yi = row[1], di = row[2];
  // lidar.py:43-45 normalises by max(|xinc|, |yinc|): one of them is +-1
  if (fabs(xi) == 1.0 && fabs(yi) <= 1.0) {
    o.axis = 0; o.sign = xi > 0 ? 1 : -1; minor = yi;
  } else if (fabs(yi) == 1.0 && fabs(xi) <= 1.0) {
    o.axis = 1; o.sign = yi > 0 ? 1 : -1; minor = xi;
  } else {
    return msgf(err, "beam %d is not a normalised lidar.py increment (%g, %g)", b, xi, yi);
  }
  o.msign = minor > 0 ? 1 : (minor < 0 ? -1 : 0);
  o.bits = 0;
  if (!(di >= 1.0)) return msgf(err, "beam %d distinc %g < 1", b, di);
  // currdist = 0; while currdist < range: currdist += distinc  (lidar.py:49-56)
  double dist = 0.0;
  int K = 0;
  while (dist < range && K <= 64) { dist += di; ++K; }
  if (K > H) return msgf(err, "beam %d takes %d steps > window half-width %d", b, K, H);
  o.K = K;
  return true;
}

// The reference's minor-coordinate chain (currx/curry += inc, int() of it)
// from every integer start of the minor axis (cm of them; valid starts are
// the padded-grid interior): row[start] bit k = the minor cell moves at step k.
inline bool beam_start_words(const Beam& o, int b, double minor, int cm, uint64_t* row, std::string& err) {
  for (int c0 = 0; c0 < cm; ++c0) {
    double m = (double)c0;
    int cell = c0;
    uint64_t w = 0;
    for (int k = 0; k < o.K; ++k) {
      m += minor;
      const int next = (int)m;  // trunc toward zero, as Python int()
      const int d = next - cell;
      if (d != 0 && d != o.msign) {
        if (m >= 0.0)  // negative coordinates lie outside the grid: unused
          return msgf(err, "beam %d start %d: minor step %d at k=%d", b, c0, d, k);
      }
      if (d != 0) w |= 1ull << k;
      cell = next;
    }
    row[c0] = w;
  }
  return true;
}

// The first step at which minor start c0, marching with its own word, stands
// on another cell than with the common word, before the first border cell of
// the minor axis (an obstacle: the march ends there and the rest of either
// word is never read); -1: the two paths are one.
inline int beam_leaves_common(uint64_t own, uint64_t common, int c0, int cm, int K, int msign) {
  int a = c0, c = c0;  // cell of the start's own word / of the common word
  for (int k = 0; k < K; ++k) {
    a += ((own >> k) & 1) ? msign : 0;
    c += ((common >> k) & 1) ? msign : 0;
    if (a != c) return k;
    if (a <= 0 || a >= cm - 1) break;  // border reached: the march ends here
  }
  return -1;
}

// The pattern of most starts becomes o.bits; it stands for the beam's table
// when every start a robot can occupy (1 .. cm-2: the border is -1) visits the
// same cells with it (beam_leaves_common).  A beam without such a pattern is
// flagged (axis bit 1) and marches from its per-start table (C4's 360 beams:
// 2 of them, 270 and 315 degrees, whose float64 chains truncate differently
// at starts 1..3).  Returns whether the pattern is common.
inline bool beam_common_pattern(Beam& o, const uint64_t* row, int cm) {
  uint64_t best = row[cm > 2 ? 1 : 0];
  int best_n = 0;
  for (int c0 = 1; c0 + 1 < cm; ++c0) {
    int n = 0;
    for (int c1 = 1; c1 + 1 < cm; ++c1) n += row[c1] == row[c0];
    if (n > best_n) { best_n = n; best = row[c0]; }
    if (2 * n > cm) break;
  }
  o.bits = (uint32_t)best;
  bool bc = true;
  for (int c0 = 1; c0 + 1 < cm && bc; ++c0) bc = beam_leaves_common(row[c0], best, c0, cm, o.K, o.msign) < 0;
  if (!bc) o.axis |= 2;
  return bc;
}

// step-1 cells of the common patterns (lidar.py:52-56: every beam with
// K >= 1 reaches its step-1 cell from the free robot cell)
inline uint32_t beam_k1_mask(const std::vector<Beam>& bt) {
  uint32_t k1 = 1u << 4;  // the robot cell (step 0)
  for (const Beam& o : bt) {
    if (o.K < 1) continue;
    const int mv = (o.bits & 1u) ? o.msign : 0;
    const int dx = (o.axis & 1) == 0 ? o.sign : mv, dy = (o.axis & 1) == 0 ? mv : o.sign;
    k1 |= 1u << (3 * (dx + 1) + (dy + 1));
  }
  return k1;
}

// The tables of `num_beams` (xinc, yinc, distinc) rows for a lidar of `range`
// on a padded Wp x Lp grid of window half-width H; false with the message in `err`.
inline bool compile_beams(const double* table, int num_beams, double range, int H, int Wp, int Lp, BeamTables& out,
                          std::string& err) {
  out = BeamTables{};
  out.cmax = Wp > Lp ? Wp : Lp;
  out.bt.resize(num_beams);
  out.bits.assign((size_t)num_beams * out.cmax, 0);
  for (int b = 0; b < num_beams; ++b) {
    Beam& o = out.bt[b];
    double minor;
    if (!beam_axis_and_k(table + 3 * b, b, range, H, o, minor, err)) return false;
    out.kmax = std::max(out.kmax, o.K);
    out.kmin = std::min(out.kmin, o.K);
    const int cm = o.axis == 0 ? Lp : Wp;
    uint64_t* row = &out.bits[(size_t)b * out.cmax];
    if (!beam_start_words(o, b, minor, cm, row, err)) return false;
    out.common = beam_common_pattern(o, row, cm) && out.common;
  }
  out.k1 = beam_k1_mask(out.bt);
  return true;
}

// Ray program: what ray_init and the read phase's ray_advance chain would
// compute for a lane's rays, built once per beam table and launch geometry
// (with common step bits a ray's cell at step k sits at a fixed offset from
// its agent's cell).  Lane `sub` of a slot marches rays idx = sub * rpl + j
// (j < rpl) of agent idx / nbeams, beam idx % nbeams.  Its row: rpl * km
// int16 offsets T[j * km + k - 1] (k = 1 .. km), two per word, low half
// first -- the ray's packed cell (mc_env_step.h struct Ray) at step k is
// P0(agent) + T; then zero padding to whole 16-byte quads less one word; the
// last word holds a byte per ray: bits 0-4 K + 1 (0: idx >= N * nbeams, a
// dead ray), bits 5-7 the agent.  The table is stored by 16-byte quads, quad
// q of every lane together (word w of lane sub at ray_prog_word): one
// 16-byte load per lane then reads consecutive memory across the slot
// (ray_prog_row_words, ray_prog_word and ray_prog_span: mc_internal.h).
//
// The ray programs of every lane of a slot (lpe rows).  False (out empty)
// when the table cannot hold them: more than one pass of rays, more than 8
// agents, a K that does not fit its field or an offset beyond int16.
inline bool build_ray_prog(const std::vector<Beam>& bt, int N, int lpe, int rpl, int km, int rowbytes,
                           std::vector<uint32_t>& out) {
  out.clear();
  const int nb = (int)bt.size(), total = N * nb;
  if (nb < 1 || N < 1 || N > 8 || km < 1 || km > 30 || rpl < 1 || rpl > 4 || total > lpe * rpl) return false;
  if (ray_prog_span(N, rowbytes, km) > 32767) return false;
  const int rw = ray_prog_row_words(rpl, km);
  const int RB = row_step_words(N, rowbytes) * rowbytes * 64;  // one window row in P units
  out.assign((size_t)lpe * rw, 0u);
  for (int sub = 0; sub < lpe; ++sub) {
    std::vector<uint32_t> row((size_t)rw, 0u);
    for (int j = 0; j < rpl; ++j) {
      const int idx = sub * rpl + j;
      if (idx >= total) continue;  // dead ray: K + 1 = 0, agent 0, offsets 0
      const int a = idx / nb;
      const Beam& bm = bt[idx - a * nb];
      if (bm.K < 0 || bm.K > km) { out.clear(); return false; }
      const bool ax = (bm.axis & 1) == 0;
      // ray_init's d0 / d1, and ray_advance's chain in its 32-bit arithmetic
      const uint32_t d0 = (uint32_t)(ax ? bm.sign * RB : bm.sign);
      const uint32_t d1 = (uint32_t)(ax ? bm.msign : bm.msign * RB);
      uint32_t t = 0;
      for (int k = 1; k <= km; ++k) {
        t += d0 + ((0u - ((bm.bits >> (k - 1)) & 1u)) & d1);
        const int32_t v = (int32_t)t;
        if (v < -32768 || v > 32767) { out.clear(); return false; }
        const int i = j * km + k - 1;
        row[i >> 1] |= (uint32_t)(uint16_t)(int16_t)v << (16 * (i & 1));
      }
      row[rw - 1] |= ((uint32_t)(bm.K + 1) | ((uint32_t)a << 5)) << (8 * j);
    }
    for (int w = 0; w < rw; ++w) out[ray_prog_word(lpe, sub, w)] = row[w];
  }
  return true;
}

using FanSector = std::vector<int>;  // a sector of build_fan: its beams, by minor offset

inline int fan_off(const Beam& o, int k) {  // signed minor offset of step k
  return o.msign * __builtin_popcount(o.bits & ((1u << k) - 1u));
}
inline uint32_t fan_class_bits(const Beam& o) {
  return ((o.axis & 1) ? (uint32_t)FAN_COLS : 0u) | (o.sign < 0 ? (uint32_t)FAN_NEG : 0u);
}

// The beams by octant class ((axis & 1) * 4 + (major sign -) * 2 + (minor
// sign -)), each class ordered by minor offsets and cut greedily into sectors.
inline std::vector<std::vector<FanSector>> fan_sectors(const std::vector<Beam>& bt, int kmax) {
  std::vector<std::vector<int>> cls(8);
  for (int b = 0; b < (int)bt.size(); ++b) {
    const Beam& o = bt[b];
    cls[(o.axis & 1) * 4 + (o.sign < 0 ? 2 : 0) + (o.msign < 0 ? 1 : 0)].push_back(b);
  }
  std::vector<std::vector<FanSector>> secs(8);
  for (int c = 0; c < 8; ++c) {
    std::vector<int>& v = cls[c];
    std::sort(v.begin(), v.end(), [&](int p, int q) {
      for (int k = kmax; k >= 1; --k) {
        const int a = fan_off(bt[p], k), d = fan_off(bt[q], k);
        if (a != d) return a < d;
      }
      return p < q;
    });
    for (int b : v) {
      std::vector<FanSector>& S = secs[c];
      bool join = !S.empty() && (int)S.back().size() < kFanS;
      if (join && (bt[b].axis & 2))
        for (int o : S.back()) join = join && !(bt[o].axis & 2);
      for (int k = 1; join && k <= kmax; ++k) {
        const int d = fan_off(bt[b], k) - fan_off(bt[S.back().back()], k);
        join = d == 0 || d == 1;
      }
      if (join) S.back().push_back(b);
      else S.push_back({b});
    }
  }
  return secs;
}

// spread[D][A] at byte D * 64 + A and expand[D][F] at 2048 + D * 64 + F
inline void fan_lut(uint8_t* lut) {
  for (int D = 0; D < 32; ++D) {
    int r[kFanS] = {0};  // cell of beam i
    for (int i = 1; i < kFanS; ++i) r[i] = r[i - 1] + ((D >> (i - 1)) & 1);
    for (int A = 0; A < 64; ++A) {
      int lit = 0, kill = 0;
      for (int i = 0; i < kFanS; ++i) {
        if ((A >> i) & 1) lit |= 1 << r[i];      // spread: beams A -> their cells
        if ((A >> r[i]) & 1) kill |= 1 << i;     // expand: cells A -> the beams on them
      }
      lut[D * 64 + A] = (uint8_t)lit;
      lut[2048 + D * 64 + A] = (uint8_t)kill;
    }
  }
}

// pair record: [desc+, desc-], then [entry+(k), entry-(k)] per step
inline void fan_pair_record(const std::vector<Beam>& bt, const std::vector<int>& spec, const FanSector& v0,
                            const FanSector& v1, int kmax, std::vector<uint32_t>& out) {
  const uint32_t cls = fan_class_bits(bt[(v0.empty() ? v1 : v0)[0]]);
  // word 0 of a sector: its class bits and special beam; word k: step k's
  // entry (an empty sector: the partner's class bits, entries 0 = no beam)
  auto desc = [&](const FanSector& v) {
    uint32_t w0 = v.empty() ? cls : fan_class_bits(bt[v[0]]);
    for (size_t j = 0; j < v.size(); ++j)
      if (bt[v[j]].axis & 2) {
        const size_t si = std::find(spec.begin(), spec.end(), v[j]) - spec.begin();
        w0 |= FAN_SPECIAL | ((uint32_t)j << 3) | ((uint32_t)si << 8);
      }
    return w0;
  };
  auto entry = [&](const FanSector& v, int k) {
    if (v.empty()) return 0u;
    const int lo = fan_off(bt[v[0]], k);
    uint32_t D = 0, valid = 0;
    for (size_t j = 0; j < v.size(); ++j) {
      if (j + 1 < v.size() && fan_off(bt[v[j + 1]], k) != fan_off(bt[v[j]], k)) D |= 1u << j;
      if (bt[v[j]].K >= k) valid |= 1u << j;
    }
    return (uint32_t)(lo + 32) | (D << 6) | (valid << 16);
  };
  out.push_back(desc(v0));
  out.push_back(desc(v1));
  for (int k = 1; k <= kmax; ++k) {
    out.push_back(entry(v0, k));
    out.push_back(entry(v1, k));
  }
}

// special record of flagged beam b: [elo, ehi] spans the minor starts whose
// own bits leave the common path before the march ends (beam_leaves_common)
inline void fan_special_record(const BeamTables& T, int b, int Wp, int Lp, std::vector<uint32_t>& out) {
  const Beam& o = T.bt[b];
  const int cm = (o.axis & 1) == 0 ? Lp : Wp;
  const uint64_t* row = &T.bits[(size_t)b * T.cmax];
  int elo = 1 << 30, ehi = -1;
  for (int c0 = 1; c0 + 1 < cm; ++c0)
    if (beam_leaves_common(row[c0], o.bits, c0, cm, o.K, o.msign) >= 0) {
      elo = std::min(elo, c0);
      ehi = std::max(ehi, c0);
    }
  const uint32_t rec[8] = {(uint32_t)b, fan_class_bits(o), (uint32_t)o.msign, (uint32_t)o.K,
                           (uint32_t)elo, (uint32_t)ehi, 0u, 0u};
  out.insert(out.end(), rec, rec + 8);
}

// Fan march data of a dense beam set (mc_env_step.h fan_march, layout in
// mc_internal.h State::fan_data).  Beams are grouped by octant class (major
// axis, major sign, minor sign; minor sign 0 counts as +), ordered by their
// minor offsets, and cut greedily into sectors of up to kFanS beams whose
// offsets differ by 0 or 1 between neighbours at every step, at most one
// start-dependent beam (Beam::axis bit 1) per sector.  The two classes of a
// line (same major axis and sign, minor sign + / -) are paired: sector i of
// each, interleaved step by step in one pair record (an empty sector pads the
// shorter class), so one lane reads the line word once for both and marks it
// with one OR; the pairs of the four lines are interleaved, so the pairs of
// one march instruction mark different lines.
// A start-dependent beam marches with its common bits except from the minor
// starts where its own bits differ before the march ends (bits[b][start],
// cm starts); the kernel marches those alone.  Returns false (ray march) for
// sparse sets: fewer than 64 beams (dense_beams), or fewer than two beams per
// sector on average.  N agents on `lanes` lanes of an env slot bound the
// special beams.
inline bool build_fan(const BeamTables& T, int Wp, int Lp, int N, int lanes, std::vector<uint32_t>& out, int& nsec,
                      int& nspec) {
  const std::vector<Beam>& bt = T.bt;
  const int nb = (int)bt.size(), kmax = T.kmax;
  if (nb < 64 || kmax > 27) return false;
  std::vector<int> spec;
  for (int b = 0; b < nb; ++b)
    if (bt[b].axis & 2) spec.push_back(b);
  const std::vector<std::vector<FanSector>> secs = fan_sectors(bt, kmax);
  size_t most = 0;
  for (const auto& S : secs) most = std::max(most, S.size());
  static const FanSector kNone;
  std::vector<std::pair<const FanSector*, const FanSector*>> order;  // (minor +, minor -)
  int real = 0;
  for (size_t i = 0; i < most; ++i)
    for (int m = 0; m < 4; ++m) {
      const bool p = i < secs[2 * m].size(), q = i < secs[2 * m + 1].size();
      if (p || q) order.push_back({p ? &secs[2 * m][i] : &kNone, q ? &secs[2 * m + 1][i] : &kNone});
      real += (int)p + (int)q;
    }
  nsec = 2 * (int)order.size();  // sector slots (pairs x 2, empty ones included)
  nspec = (int)spec.size();
  if (2 * real > nb || N * nspec > lanes || nspec > 255) return false;
  out.assign(kFanLutBytes / 4, 0u);
  fan_lut(reinterpret_cast<uint8_t*>(out.data()));
  for (const auto& pr : order) fan_pair_record(bt, spec, *pr.first, *pr.second, kmax, out);
  for (int b : spec) fan_special_record(T, b, Wp, Lp, out);
  while (out.size() % 4) out.push_back(0u);
  return true;
}

}  // namespace mc
