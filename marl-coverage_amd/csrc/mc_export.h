// mc_export.h — the decode behind mc_export_maps (mc_export.hip): a map's bit
// tiles as uint8 cells (scale 1) or as one count per 8x8 tile (scale 8).
//
// The output of one plane is a flat byte array -- [Wp][Lp] cells, or
// [TR][TC] tile counts -- and the kernel writes it in 16-byte chunks that
// start at any offset of it, so every function here makes the 16 bytes from
// linear offset `o` of one plane, as two little-endian u64 (out[0]: bytes
// 0..7).  A chunk may run over a row end (several times on a narrow map);
// bytes past the plane's end are don't-care and the caller does not store
// them.  `word(i)` returns tile word i of the map (tile_index order): a
// pointer load, or the OR of the agents' words for MC_MAP_OBST_ANY.
//
// Plain C++ on both sides: the kernel and the host check
// (tests/native/export_check.cpp) run the same code.
#pragma once
#include "mc_internal.h"

namespace mc {

// bits 0..7 of b as 8 bytes of 0 / 1 (bit k -> byte k): a nibble times
// 0x00204081 puts bit k at bit 8k (the four partial products do not overlap)
__host__ __device__ inline uint64_t export_spread8(uint32_t b) {
  const uint32_t lo = ((b & 15u) * 0x00204081u) & 0x01010101u;
  const uint32_t hi = (((b >> 4) & 15u) * 0x00204081u) & 0x01010101u;
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// OR the first n (0..16) bytes of (b0, b1) into the 16-byte value (lo, hi) at
// byte offset at (0..16, at + n <= 16)
__host__ __device__ inline void export_put(uint64_t& lo, uint64_t& hi, int at, uint64_t b0, uint64_t b1, int n) {
  if (n < 8) {
    b0 &= (1ull << (8 * n)) - 1ull;
    b1 = 0ull;
  } else if (n < 16) {
    b1 &= (1ull << (8 * (n - 8))) - 1ull;
  }
  if (at == 0) {
    lo |= b0;
    hi |= b1;
  } else if (at < 8) {
    lo |= b0 << (8 * at);
    hi |= (b1 << (8 * at)) | (b0 >> (64 - 8 * at));
  } else if (at < 16) {
    hi |= b0 << (8 * (at - 8));
  }
}

// K tile words at once: w[k] = word(idx[k]).  The loads do not depend on one
// another, so an accessor whose word() is a chain of loads (the kernel's OR
// over agents) overloads this to keep K of them in flight.
template <int K, class W>
__host__ __device__ inline void export_load(const W& word, const uint32_t (&idx)[K], uint64_t (&w)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = word(idx[k]);
}

// Dense: cells o .. o + 15 (o < Wp * Lp) of the [Wp][Lp] plane, one byte of
// 0 / 1 each.  Cell (x, y) is bit 8 (x & 7) + (y & 7) of tile (x >> 3, y >> 3).
// With Lp >= 16 the chunk is the end of row x from column y (at most 16 bits
// out of three tiles' row bytes) and then the start of row x + 1 (two tiles):
// five words loaded together, no loop and no branch.  Tiles past the row's or
// the map's last are replaced by the last one; their bits are never used.
// Narrower maps take runs of up to 8 cells of one tile row in a loop.
template <class W>
__host__ __device__ inline void export_chunk16(const W& word, int TCS, int Wp, int Lp, uint32_t o, uint64_t out[2]) {
  uint64_t lo = 0ull, hi = 0ull;
  uint32_t x = o / (uint32_t)Lp, y = o - x * (uint32_t)Lp;
  if (Lp >= 16) {
    const uint32_t n1 = (uint32_t)Lp - y < 16u ? (uint32_t)Lp - y : 16u;  // cells of row x
    const int tj = (int)(y >> 3), tmax = (Lp - 1) >> 3;
    const uint32_t x2 = x + 1u < (uint32_t)Wp ? x + 1u : (uint32_t)Wp - 1u;
    const int ti = (int)(x >> 3), ti2 = (int)(x2 >> 3);
    const uint32_t idx[5] = {tile_index(TCS, ti, tj), tile_index(TCS, ti, tj + 1 < tmax ? tj + 1 : tmax),
                             tile_index(TCS, ti, tj + 2 < tmax ? tj + 2 : tmax), tile_index(TCS, ti2, 0),
                             tile_index(TCS, ti2, 1)};  // (tmax >= 1)
    uint64_t w[5];
    export_load<5>(word, idx, w);
    const uint32_t s1 = 8u * (x & 7u), s2 = 8u * (x2 & 7u);
    const uint32_t r1 = ((uint32_t)(w[0] >> s1) & 0xFFu) | (((uint32_t)(w[1] >> s1) & 0xFFu) << 8) |
                        (((uint32_t)(w[2] >> s1) & 0xFFu) << 16);
    const uint32_t r2 = ((uint32_t)(w[3] >> s2) & 0xFFu) | (((uint32_t)(w[4] >> s2) & 0xFFu) << 8);
    const uint32_t bits = ((r1 >> (y & 7u)) & ((1u << n1) - 1u)) | (r2 << n1);
    out[0] = export_spread8(bits & 0xFFu);
    out[1] = export_spread8((bits >> 8) & 0xFFu);
    return;
  }
  int filled = 0;
  while (filled < 16 && x < (uint32_t)Wp) {
    int n = 8 - (int)(y & 7u);
    if (n > Lp - (int)y) n = Lp - (int)y;
    if (n > 16 - filled) n = 16 - filled;
    const uint64_t w = word(tile_index(TCS, (int)(x >> 3), (int)(y >> 3)));
    const uint32_t bits = (uint32_t)(w >> (8u * (x & 7u) + (y & 7u))) & ((1u << n) - 1u);
    export_put(lo, hi, filled, export_spread8(bits), 0ull, n);
    filled += n;
    y += (uint32_t)n;
    if (y == (uint32_t)Lp) {
      y = 0u;
      ++x;
    }
  }
  out[0] = lo;
  out[1] = hi;
}

// Pooled: the set bits of tile (ti, tj)'s word w that are cells of
// [0, Wp) x [0, Lp) (an edge tile of grid_neg has bits beyond the grid)
__host__ __device__ inline uint32_t export_pooled(uint64_t w, int Wp, int Lp, int ti, int tj) {
  const int nr = Wp - 8 * ti, nc = Lp - 8 * tj;
  if (nr <= 0 || nc <= 0) return 0u;
  uint64_t m = ~0ull;
  if (nc < 8) m = ((1ull << nc) - 1ull) * 0x0101010101010101ull;
  if (nr < 8) m &= (1ull << (8 * nr)) - 1ull;
  w &= m;
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(w);
#else
  return (uint32_t)__builtin_popcountll(w);
#endif
}

// Pooled: counts o .. o + 15 of the [TR][TC] plane (TR = ceil(Wp / 8), TC =
// ceil(Lp / 8)), one byte of 0..64 each; pooled cell (i, j) is tile (i, j)
template <class W>
__host__ __device__ inline void export_pooled_chunk16(const W& word, int TCS, int Wp, int Lp, uint32_t o,
                                                      uint64_t out[2]) {
  const uint32_t TR = (uint32_t)(Wp + 7) >> 3, TC = (uint32_t)(Lp + 7) >> 3;
  const uint32_t t0 = o / TC;
  // eight words loaded together per output half (tiles past the plane's end:
  // a tile of the last row, not counted)
  uint32_t ti = t0, tj = o - t0 * TC;
  for (int h = 0; h < 2; ++h) {
    uint32_t idx[8];
    uint64_t w[8];
    uint32_t ui = ti, uj = tj;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      idx[k] = tile_index(TCS, (int)(ui < TR ? ui : TR - 1u), (int)uj);
      if (++uj == TC) {
        uj = 0u;
        ++ui;
      }
    }
    export_load<8>(word, idx, w);
    uint64_t v = 0ull;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint64_t c = ti < TR ? export_pooled(w[k], Wp, Lp, (int)ti, (int)tj) : 0u;
      v |= c << (8 * k);
      if (++tj == TC) {
        tj = 0u;
        ++ti;
      }
    }
    out[h] = v;
  }
}

// The robots plane.  pos: (x, y) of the env's n robots.  Dense (shift 0, cols
// = Lp): i + 1 at robot i's cell.  Pooled (shift 3, cols = TC): the number of
// robots in each tile.  Robots never share a cell.
__host__ __device__ inline void export_robots_chunk16(const int32_t* pos, int n, int cols, int shift, uint32_t o,
                                                      uint64_t out[2]) {
  uint64_t v[2] = {0ull, 0ull};
  for (int i = 0; i < n; ++i) {
    const uint32_t x = (uint32_t)pos[2 * i] >> shift, y = (uint32_t)pos[2 * i + 1] >> shift;
    const uint32_t d = x * (uint32_t)cols + y - o;
    if (d >= 16u || y >= (uint32_t)cols) continue;
    const int sh = 8 * (int)(d & 7u);
    if (shift == 0) v[d >> 3] = (v[d >> 3] & ~(0xFFull << sh)) | ((uint64_t)(i + 1) << sh);
    else v[d >> 3] += 1ull << sh;
  }
  out[0] = v[0];
  out[1] = v[1];
}

// The planes a layer mask selects, in output order: the set bits of
// layers & 31 (one plane each, ascending), then FREE's and then OBST's N
// agent planes.  kind: the layer's bit index (0..6); agent: the plane's agent.
constexpr uint32_t kMapAll = 127u, kMapSingles = 31u, kMapFreeBit = 5u, kMapObstBit = 6u;

__host__ __device__ inline int export_planes(uint32_t layers, int N) {
  int p = 0;
  for (uint32_t b = 0; b < 5u; ++b) p += (int)((layers >> b) & 1u);
  return p + (int)((layers >> kMapFreeBit) & 1u) * N + (int)((layers >> kMapObstBit) & 1u) * N;
}

__host__ __device__ inline void export_plane_kind(uint32_t layers, int N, int p, int& kind, int& agent) {
  agent = 0;
  for (int b = 0; b < 5; ++b)
    if ((layers >> b) & 1u) {
      if (p == 0) {
        kind = b;
        return;
      }
      --p;
    }
  if (((layers >> kMapFreeBit) & 1u) && p < N) {
    kind = (int)kMapFreeBit;
    agent = p;
    return;
  }
  if ((layers >> kMapFreeBit) & 1u) p -= N;
  kind = (int)kMapObstBit;
  agent = p;
}

}  // namespace mc
