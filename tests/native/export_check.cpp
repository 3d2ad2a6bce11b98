// Stand-alone run of mc_export_maps' decode functions (csrc/mc_export.h, the
// code the export kernel runs per 16-byte chunk), for a host-only build with
// sanitizers (tests/test_export_maps_host.py builds and runs it; no HIP call).
//
// For maps of 37 x 45, 34 x 48 and 9 x 5 cells with seeded random tile words
// -- every bit of every word, so edge tiles have bits beyond the map set, as
// grid_neg has -- it checks
//   - export_chunk16 at every offset o of the [Wp][Lp] plane (so every o mod
//     16) against a per-cell restatement: cell (x, y) is bit 8 (x & 7) + (y & 7)
//     of word tile_index(TCS, x >> 3, y >> 3); only bytes inside the plane count;
//   - export_pooled of every tile against a per-cell count over the cells of
//     the tile inside the map, and export_pooled_chunk16 at every offset of the
//     [TR][TC] plane against those counts;
//   - the OR accessor of MC_MAP_OBST_ANY (three maps' words OR-ed);
//   - export_robots_chunk16, dense and pooled, for robots on distinct cells;
//   - export_put at every (offset, length).
// Output per map: "map Wp Lp chunks C rowend R1 rowend2 R2 pooled T": chunks
// checked, those that crossed a row end and those that crossed two, tiles.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mc_export.h"

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

unsigned byte_of(const uint64_t v[2], int k) { return (unsigned)((v[k >> 3] >> (8 * (k & 7))) & 0xFFull); }

// the words of n maps, OR-ed: exact-size heap blocks, an index past one is the
// sanitizer's to find
struct Words {
  std::vector<const std::vector<uint64_t>*> maps;
  uint64_t operator()(uint32_t i) const {
    uint64_t w = 0;
    for (auto* m : maps) w |= m->at(i);
    return w;
  }
};

bool cell(const Words& w, int TCS, int x, int y) {
  return (w(mc::tile_index(TCS, x >> 3, y >> 3)) >> (8 * (x & 7) + (y & 7))) & 1ull;
}

int check_map(int Wp, int Lp) {
  const int TR = (Wp + 7) / 8, TC = (Lp + 7) / 8, TRS = (TR + 3) / 4, TCS = (TC + 3) / 4;
  const size_t MT = (size_t)TRS * TCS * 16;
  std::vector<std::vector<uint64_t>> store(3, std::vector<uint64_t>(MT));
  for (auto& m : store)
    for (auto& w : m) w = next_u64();
  const uint32_t cells = (uint32_t)Wp * Lp;
  long chunks = 0, rowend = 0, rowend2 = 0, pooled = 0;
  for (int pass = 0; pass < 2; ++pass) {  // one map; the OR of three
    Words w;
    w.maps.push_back(&store[0]);
    if (pass) {
      w.maps.push_back(&store[1]);
      w.maps.push_back(&store[2]);
    }
    for (uint32_t o = 0; o < cells; ++o) {
      uint64_t v[2] = {0xDEADBEEFDEADBEEFull, 0xDEADBEEFDEADBEEFull};
      mc::export_chunk16(w, TCS, Wp, Lp, o, v);
      const int n = cells - o < 16u ? (int)(cells - o) : 16;
      for (int k = 0; k < n; ++k) {
        const int x = (int)((o + k) / Lp), y = (int)((o + k) % Lp);
        const unsigned want = cell(w, TCS, x, y) ? 1u : 0u;
        if (byte_of(v, k) != want) {
          std::printf("FAIL map %d %d pass %d: chunk at %u byte %d (cell %d %d) is %u, want %u\n", Wp, Lp, pass, o, k,
                      x, y, byte_of(v, k), want);
          return 1;
        }
      }
      const int rows = (int)((o + n - 1) / Lp) - (int)(o / Lp);
      ++chunks;
      rowend += rows >= 1;
      rowend2 += rows >= 2;
    }
    std::vector<unsigned> counts((size_t)TR * TC);
    for (int ti = 0; ti < TR; ++ti)
      for (int tj = 0; tj < TC; ++tj) {
        unsigned want = 0;
        for (int x = 8 * ti; x < 8 * ti + 8 && x < Wp; ++x)
          for (int y = 8 * tj; y < 8 * tj + 8 && y < Lp; ++y) want += cell(w, TCS, x, y);
        const unsigned got = mc::export_pooled(w(mc::tile_index(TCS, ti, tj)), Wp, Lp, ti, tj);
        if (got != want) {
          std::printf("FAIL map %d %d pass %d: pooled tile %d %d is %u, want %u\n", Wp, Lp, pass, ti, tj, got, want);
          return 1;
        }
        counts[(size_t)ti * TC + tj] = want;
        ++pooled;
      }
    for (uint32_t o = 0; o < (uint32_t)(TR * TC); ++o) {
      uint64_t v[2] = {0xDEADBEEFDEADBEEFull, 0xDEADBEEFDEADBEEFull};
      mc::export_pooled_chunk16(w, TCS, Wp, Lp, o, v);
      for (int k = 0; k < 16 && o + k < (uint32_t)(TR * TC); ++k)
        if (byte_of(v, k) != counts[o + k]) {
          std::printf("FAIL map %d %d pass %d: pooled chunk at %u byte %d is %u, want %u\n", Wp, Lp, pass, o, k,
                      byte_of(v, k), counts[o + k]);
          return 1;
        }
    }
  }
  // robots on distinct cells (robots 1 and 4 share a tile)
  const int N = 5;
  std::vector<int32_t> pos = {0, 0, Wp - 1, Lp - 1, Wp / 2, Lp - 1, Wp / 2 + 1, 0, Wp - 1, Lp - 2};
  for (int dense = 0; dense < 2; ++dense) {
    const int cols = dense ? Lp : TC, rows = dense ? Wp : TR, shift = dense ? 0 : 3;
    std::vector<unsigned> want((size_t)rows * cols, 0u);
    for (int i = 0; i < N; ++i) {
      unsigned& c = want[(size_t)(pos[2 * i] >> shift) * cols + (pos[2 * i + 1] >> shift)];
      c = dense ? (unsigned)(i + 1) : c + 1u;
    }
    for (uint32_t o = 0; o < (uint32_t)(rows * cols); ++o) {
      uint64_t v[2] = {0xDEADBEEFDEADBEEFull, 0xDEADBEEFDEADBEEFull};
      mc::export_robots_chunk16(pos.data(), N, cols, shift, o, v);
      for (int k = 0; k < 16 && o + k < (uint32_t)(rows * cols); ++k)
        if (byte_of(v, k) != want[o + k]) {
          std::printf("FAIL map %d %d: robots (dense %d) chunk at %u byte %d is %u, want %u\n", Wp, Lp, dense, o, k,
                      byte_of(v, k), want[o + k]);
          return 1;
        }
    }
  }
  std::printf("map %d %d chunks %ld rowend %ld rowend2 %ld pooled %ld\n", Wp, Lp, chunks, rowend, rowend2, pooled);
  return 0;
}

int check_put() {
  for (int at = 0; at <= 16; ++at)
    for (int n = 0; at + n <= 16; ++n) {
      const uint64_t b[2] = {next_u64() | 0x0101010101010101ull, next_u64() | 0x0101010101010101ull};
      uint64_t v[2] = {0ull, 0ull};
      mc::export_put(v[0], v[1], at, b[0], b[1], n);
      for (int k = 0; k < 16; ++k) {
        const unsigned want = k >= at && k < at + n ? byte_of(b, k - at) : 0u;
        if (byte_of(v, k) != want) {
          std::printf("FAIL put at %d n %d: byte %d is %u, want %u\n", at, n, k, byte_of(v, k), want);
          return 1;
        }
      }
    }
  return 0;
}

}  // namespace

int main() {
  const int maps[3][2] = {{37, 45}, {34, 48}, {9, 5}};
  for (auto& m : maps)
    if (check_map(m[0], m[1])) return 1;
  if (check_put()) return 1;
  // the plane order of a layer mask
  int kind = -1, agent = -1;
  if (mc::export_planes(127u, 3) != 11 || mc::export_planes(4u | 8u | 16u, 4) != 3 || mc::export_planes(96u, 2) != 4) {
    std::printf("FAIL export_planes\n");
    return 1;
  }
  const int want[11][2] = {{0, 0}, {1, 0}, {2, 0}, {3, 0}, {4, 0}, {5, 0}, {5, 1}, {5, 2}, {6, 0}, {6, 1}, {6, 2}};
  for (int p = 0; p < 11; ++p) {
    mc::export_plane_kind(127u, 3, p, kind, agent);
    if (kind != want[p][0] || agent != want[p][1]) {
      std::printf("FAIL export_plane_kind all %d: %d %d\n", p, kind, agent);
      return 1;
    }
  }
  mc::export_plane_kind(16u | 64u, 3, 2, kind, agent);
  if (kind != 6 || agent != 1) {
    std::printf("FAIL export_plane_kind subset: %d %d\n", kind, agent);
    return 1;
  }
  std::printf("ok 3 maps\n");
  return 0;
}
