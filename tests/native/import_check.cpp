// Stand-alone run of mc_import_maps' packing functions (csrc/mc_import.h, the
// code the import kernel runs per tile and per run of the robots plane), for a
// host-only build with sanitizers (tests/test_import_maps_host.py builds and
// runs it; no HIP call).
//
// For maps of 37 x 45, 34 x 48 and 9 x 5 cells (rows narrower than a tile) and
// every base offset 0..15 of the plane inside an exactly-sized heap buffer --
// a read before the plane's first or past its last byte is the sanitizer's to
// find -- with bytes drawn from {0, 1, 2, 255} it checks
//   - import_tile of every tile of the 4 x 4 blocks (the padding tiles
//     included) against a per-cell restatement: bit 8 r + c is set exactly when
//     cell (8 ti + r, 8 tj + c) lies inside the map and its byte is nonzero;
//   - the round trip: export_chunk16 (csrc/mc_export.h) of the packed tiles
//     gives (byte != 0) for every cell;
//   - import_squeeze8 on every pattern of zero / nonzero bytes;
//   - the robots scan: a valid plane is accepted with the right cells, and a
//     value above N, a missing number, a duplicate and a robot on a blocked
//     cell are each rejected.
// Output per map: "map Wp Lp tiles T cells C edge E robots R": tile words
// compared, cells decoded back, words of tiles cut by the map's edge, robots
// planes scanned.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "mc_export.h"
#include "mc_import.h"

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// a plane of `cells` bytes at offset `base` of a heap block of exactly base +
// cells bytes (the block's end is the plane's end)
struct Plane {
  std::unique_ptr<uint8_t[]> block;
  uint8_t* p;
  Plane(int base, uint32_t cells) : block(new uint8_t[base + cells]), p(block.get() + base) {}
};

struct RobotScan {
  std::vector<uint32_t> cnt, cell;
  bool in_range = true;
};

RobotScan scan(const uint8_t* plane, uint32_t cells, int N) {
  RobotScan s;
  s.cnt.assign(64, 0u);
  s.cell.assign(64, 0u);
  const mc::ImportBytes rb{plane};
  for (uint32_t o = 0; o < cells; o += 8u) {
    const int n = cells - o < 8u ? (int)(cells - o) : 8;
    s.in_range &= mc::import_robots_run(n == 8 ? rb.load8(o) : rb.load(o, n), o, N, [&](int i, uint32_t c) {
      ++s.cnt[i];
      s.cell[i] = c;
    });
  }
  return s;
}

int check_map(int Wp, int Lp) {
  const int TR = (Wp + 7) / 8, TC = (Lp + 7) / 8, TRS = (TR + 3) / 4, TCS = (TC + 3) / 4;
  const size_t MT = (size_t)TRS * TCS * 16;
  const uint32_t cells = (uint32_t)Wp * Lp;
  static const uint8_t kValues[4] = {0, 1, 2, 255};
  long tiles = 0, decoded = 0, edge = 0, robots = 0;
  for (int base = 0; base < 16; ++base) {
    Plane pl(base, cells);
    for (uint32_t i = 0; i < cells; ++i) pl.p[i] = kValues[next_u64() & 3u];
    const mc::ImportBytes bytes{pl.p};
    std::vector<uint64_t> words(MT, 0xDEADBEEFDEADBEEFull);
    for (int ti = 0; ti < 4 * TRS; ++ti)
      for (int tj = 0; tj < 4 * TCS; ++tj) {
        uint64_t want = 0ull;
        for (int r = 0; r < 8; ++r)
          for (int c = 0; c < 8; ++c) {
            const int x = 8 * ti + r, y = 8 * tj + c;
            if (x < Wp && y < Lp && pl.p[(size_t)x * Lp + y] != 0) want |= 1ull << (8 * r + c);
          }
        const uint64_t got = mc::import_tile(bytes, Wp, Lp, ti, tj);
        if (got != want) {
          std::printf("FAIL map %d %d base %d: tile %d %d is %016llx, want %016llx\n", Wp, Lp, base, ti, tj,
                      (unsigned long long)got, (unsigned long long)want);
          return 1;
        }
        words[mc::tile_index(TCS, ti, tj)] = got;
        ++tiles;
        if (ti < TR && tj < TC && (8 * ti + 8 > Wp || 8 * tj + 8 > Lp)) ++edge;
      }
    // back through the export's decode
    const auto word = [&](uint32_t i) { return words.at(i); };
    for (uint32_t o = 0; o < cells; o += 16u) {
      uint64_t v[2] = {0xDEADBEEFDEADBEEFull, 0xDEADBEEFDEADBEEFull};
      mc::export_chunk16(word, TCS, Wp, Lp, o, v);
      for (uint32_t k = 0; k < 16u && o + k < cells; ++k) {
        const unsigned got = (unsigned)((v[k >> 3] >> (8 * (k & 7u))) & 0xFFull);
        if (got != (pl.p[o + k] != 0 ? 1u : 0u)) {
          std::printf("FAIL map %d %d base %d: cell %u decodes to %u, byte %u\n", Wp, Lp, base, o + k, got,
                      (unsigned)pl.p[o + k]);
          return 1;
        }
        ++decoded;
      }
    }

    // the robots plane: N robots on distinct free cells; grid < 0 on the border ring and one inner cell
    const int N = 5;
    std::vector<uint64_t> neg(MT, 0ull);
    const auto block = [&](int x, int y) { neg[mc::tile_index(TCS, x >> 3, y >> 3)] |= 1ull << (8 * (x & 7) + (y & 7)); };
    for (int x = 0; x < Wp; ++x)
      for (int y = 0; y < Lp; ++y)
        if (x == 0 || y == 0 || x == Wp - 1 || y == Lp - 1) block(x, y);
    block(Wp / 2, 2);
    const auto negw = [&](uint32_t i) { return neg.at(i); };
    const uint32_t at[N] = {(uint32_t)(1 * Lp + 1), (uint32_t)((Wp - 2) * Lp + Lp - 2), (uint32_t)((Wp / 2) * Lp + 1),
                            (uint32_t)((Wp / 2) * Lp + 3), (uint32_t)(1 * Lp + Lp - 2)};
    Plane rp(base, cells);
    const auto fill = [&]() {
      std::memset(rp.p, 0, cells);
      for (int i = 0; i < N; ++i) rp.p[at[i]] = (uint8_t)(i + 1);
    };
    const auto accepts = [&]() {
      const RobotScan s = scan(rp.p, cells, N);
      ++robots;
      return s.in_range && mc::import_robots_valid(s.cnt.data(), s.cell.data(), N, Lp, TCS, negw);
    };
    fill();
    {
      const RobotScan s = scan(rp.p, cells, N);
      for (int i = 0; i < N; ++i)
        if (s.cnt[i] != 1u || s.cell[i] != at[i]) {
          std::printf("FAIL map %d %d base %d: robot %d seen %u times at %u, want once at %u\n", Wp, Lp, base, i,
                      s.cnt[i], s.cell[i], at[i]);
          return 1;
        }
    }
    bool ok = accepts();
    fill(), rp.p[cells - 1] = (uint8_t)(N + 1);  // a value above N (the plane's last byte)
    ok = ok && !accepts();
    fill(), rp.p[at[2]] = 0;  // a missing number
    ok = ok && !accepts();
    fill(), rp.p[0] = 4;  // a duplicate (the plane's first byte)
    ok = ok && !accepts();
    fill(), rp.p[at[3]] = 0, rp.p[(Wp / 2) * Lp + 2] = 4;  // robot 3 on the blocked inner cell
    ok = ok && !accepts();
    fill(), rp.p[at[0]] = 0, rp.p[Lp - 1] = 1;  // robot 0 on the border ring
    ok = ok && !accepts();
    if (!ok) {
      std::printf("FAIL map %d %d base %d: robots plane validation\n", Wp, Lp, base);
      return 1;
    }
  }
  std::printf("map %d %d tiles %ld cells %ld edge %ld robots %ld\n", Wp, Lp, tiles, decoded, edge, robots);
  return 0;
}

int check_squeeze() {
  static const uint8_t kNonzero[4] = {1, 2, 0x80, 255};
  for (unsigned pat = 0; pat < 256u; ++pat)
    for (int v = 0; v < 4; ++v) {
      uint64_t w = 0ull;
      for (int k = 0; k < 8; ++k)
        if ((pat >> k) & 1u) w |= (uint64_t)kNonzero[(v + k) & 3] << (8 * k);
      if (mc::import_squeeze8(w) != pat) {
        std::printf("FAIL squeeze8 %016llx is %u, want %u\n", (unsigned long long)w, mc::import_squeeze8(w), pat);
        return 1;
      }
    }
  return 0;
}

}  // namespace

int main() {
  const int maps[3][2] = {{37, 45}, {34, 48}, {9, 5}};
  if (check_squeeze()) return 1;
  for (auto& m : maps)
    if (check_map(m[0], m[1])) return 1;
  if (mc::kMapImportable != 112u) {
    std::printf("FAIL kMapImportable\n");
    return 1;
  }
  std::printf("ok 3 maps\n");
  return 0;
}
