// mc_import.h — the packing behind mc_import_maps (mc_import.hip), the inverse
// of mc_export.h: a dense uint8 plane [Wp][Lp] (nonzero = set) as 8x8-cell bit
// tiles, and the scan of a robots plane (i + 1 at robot i's cell).
//
// A plane starts at any byte address (Wp * Lp is generally odd), so the input
// is read through a byte accessor: `bytes.load8(o)` returns the 8 bytes from
// offset o of the plane as a little-endian u64, `bytes.load(o, n)` the n (1..8)
// bytes from there, the other bytes zero; each reads nothing but those bytes.
// Nothing here asks for a byte past a row's end or past the plane.
//
// Plain C++ on both sides: the kernel and the host check
// (tests/native/import_check.cpp) run the same code.
#pragma once
#include <string.h>

#include "mc_internal.h"

namespace mc {

// the layers mc_import_maps takes (MC_MAP_ROBOTS | MC_MAP_FREE | MC_MAP_OBST)
constexpr uint32_t kMapImportable = 16u | 32u | 64u;

// The accessor over memory.  Eight bytes are one load at any alignment (gfx950
// takes unaligned global loads; the host a memcpy); a shorter run (a map
// narrower than a tile, the last bytes of a robots plane) goes byte by byte.
struct ImportBytes {
  const uint8_t* p;
  __host__ __device__ inline uint64_t load8(uint32_t o) const {
    uint64_t v;
    memcpy(&v, p + o, 8);
    return v;
  }
  __host__ __device__ inline uint64_t load(uint32_t o, int n) const {
    uint64_t v = 0ull;
    for (int k = 0; k < n; ++k) v |= (uint64_t)p[o + k] << (8 * k);
    return v;
  }
};

// 8 bytes -> 8 bits: bit k = (byte k != 0).  The first line leaves 0x80 in
// every nonzero byte; the product moves bit 8k of the 0 / 1 bytes to bit
// 56 + k (the partial products 7j + 8k are distinct: no carries).
__host__ __device__ inline uint32_t import_squeeze8(uint64_t v) {
  const uint64_t m = 0x7F7F7F7F7F7F7F7Full;
  const uint64_t nz = (((v & m) + m) | v) & ~m;
  return (uint32_t)(((nz >> 7) * 0x0102040810204080ull) >> 56);
}

// Tile word (ti, tj) of the plane: bit 8 r + c = cell (8 ti + r, 8 tj + c) is
// nonzero; rows and columns of the tile beyond [0, Wp) x [0, Lp) are clear
// (a tile wholly outside, a padding tile of the last blocks, is 0).
//
// On a map of 8 or more columns (import_tile_wide; 8 ti < Wp and 8 tj < Lp, the
// tile has cells of the map) every tile is eight 8-byte loads that do not
// depend on one another, with no branch between them, so the loads of several
// planes' tiles can be on their way together.  A tile that the grid's right
// edge cuts (nc < 8 columns) loads the 8 bytes that end at the row's end and
// shifts the columns before the tile out; one that the bottom edge cuts (nr <
// 8 rows) loads its last row again and masks the rows out.  A narrower map has
// one column of tiles, read in runs of Lp bytes (import_tile_narrow).
template <class A>
__host__ __device__ inline uint64_t import_tile_wide(const A& bytes, int Wp, int Lp, int ti, int tj) {
  const int nr = Wp - 8 * ti < 8 ? Wp - 8 * ti : 8, nc = Lp - 8 * tj < 8 ? Lp - 8 * tj : 8;
  const int back = 8 - nc;
  const uint32_t o = (uint32_t)(8 * ti) * (uint32_t)Lp + (uint32_t)(8 * tj - back);
  uint64_t v[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = bytes.load8(o + (uint32_t)(r < nr ? r : nr - 1) * (uint32_t)Lp);
  uint64_t w = 0ull;
#pragma unroll
  for (int r = 0; r < 8; ++r) w |= (uint64_t)import_squeeze8(v[r] >> (8 * back)) << (8 * r);
  return nr < 8 ? w & ((1ull << (8 * nr)) - 1ull) : w;
}

template <class A>
__host__ __device__ inline uint64_t import_tile_narrow(const A& bytes, int Wp, int Lp, int ti) {
  uint64_t w = 0ull;
  for (int r = 0; r < 8 && 8 * ti + r < Wp; ++r)
    w |= (uint64_t)import_squeeze8(bytes.load((uint32_t)(8 * ti + r) * (uint32_t)Lp, Lp)) << (8 * r);
  return w;
}

template <class A>
__host__ __device__ inline uint64_t import_tile(const A& bytes, int Wp, int Lp, int ti, int tj) {
  if (8 * ti >= Wp || 8 * tj >= Lp) return 0ull;
  return Lp >= 8 ? import_tile_wide(bytes, Wp, Lp, ti, tj) : import_tile_narrow(bytes, Wp, Lp, ti);
}

// The robots plane: v holds the bytes of cells o, o + 1, .. of its flat
// [Wp * Lp] bytes (`bytes.load8(o)`, or `load(o, n)` at the plane's end); seen(i, cell) for every byte i + 1 in
// 1..N; returns false when a byte is above N.
template <class S>
__host__ __device__ inline bool import_robots_run(uint64_t v, uint32_t o, int N, S&& seen) {
  bool ok = true;
  for (int k = 0; v != 0ull; ++k, v >>= 8) {
    const int b = (int)(v & 0xFFull);
    if (b == 0) continue;
    if (b > N) ok = false;
    else seen(b - 1, o + (uint32_t)k);
  }
  return ok;
}

// After the scan: a robot was seen cnt times, last at cell (x * Lp + y).  Valid
// when it was seen exactly once, on a cell that is not blocked; neg(i): tile
// word i of the env's grid < 0 map.
template <class G>
__host__ __device__ inline bool import_robot_valid(uint32_t cnt, uint32_t cell, int Lp, int TCS, const G& neg) {
  if (cnt != 1u) return false;
  const uint32_t x = cell / (uint32_t)Lp, y = cell - x * (uint32_t)Lp;
  return ((neg(tile_index(TCS, (int)(x >> 3), (int)(y >> 3))) >> (8u * (x & 7u) + (y & 7u))) & 1ull) == 0ull;
}

// ... for all N robots of the plane
template <class G>
__host__ __device__ inline bool import_robots_valid(const uint32_t* cnt, const uint32_t* cell, int N, int Lp, int TCS,
                                                    const G& neg) {
  for (int i = 0; i < N; ++i)
    if (!import_robot_valid(cnt[i], cell[i], Lp, TCS, neg)) return false;
  return true;
}

}  // namespace mc
