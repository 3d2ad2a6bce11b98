// mc_vistab.h — the lidar's marks as a table: one record per (pool grid, cell).
//
// The cells a lidar at cell (x, y) of grid g marks are a function of the grid,
// the cell and the beam table only, and pool grids are static between
// mc_set_grids / mc_generate_grids calls.  A record is what the march leaves
// in the env kernel's mark-row plane, relative to the robot: word r (0 <= r <=
// 2H) is the row x - H + r, its bit c the cell (x - H + r, y - H + c) -- the
// robot's own cell, the free cells every beam passes up to its first obstacle,
// and that obstacle (cells outside the map are obstacles: isInBounds).  The
// split into free and obstacle marks stays with the grid tiles (gather_marks).
// 2H + 1 <= kVisRows rows of 2H + 1 <= 21 bits, padded to one 128-byte line;
// the step kernel shifts a row by up to 11 bits into a 32-bit window row.
//
// vis_record is plain C++ on both sides: the build kernel (mc_vistab.hip) and
// the host check (tests/native/vis_table_check.cpp) run the same code.
#pragma once
#include "mc_internal.h"

namespace mc {

constexpr int kVisRows = 21;      // rows (and bits per row) a record can hold: H <= 10
// the record's form.  Unsplit is the measured choice (profiles/r14/vis_tiles/)
#ifndef MC_VIS_SPLIT
#define MC_VIS_SPLIT 0
#endif
constexpr bool kVisSplit = MC_VIS_SPLIT != 0;
constexpr int kVisTiles = 16;                          // tiles of one plane of a record: 4 x 4
constexpr int kVisRecWords = kVisSplit ? 64 : 32;      // u32 words per record: one or two 128-byte lines

// whether a State's lidar fits a record
__host__ __device__ constexpr bool vis_fits(int H) { return H >= 1 && 2 * H + 1 <= kVisRows; }

// bytes of the table of a pool: G grids of Wp x Lp cells
__host__ __device__ inline size_t vis_table_bytes(int G, int Wp, int Lp) {
  return (size_t)G * Wp * Lp * kVisRecWords * 4;
}

// record index of cell (x, y) of pool grid g
__host__ __device__ inline uint32_t vis_index(int Wp, int Lp, int g, int x, int y) {
  return ((uint32_t)g * (uint32_t)Wp + (uint32_t)x) * (uint32_t)Lp + (uint32_t)y;
}

// Byte offset, in the table of a pool of G grids of Wp x Lp cells, of map tile
// (gi, gj)'s tile of the record of cell (x, y) of grid g (H: the lidar's
// range; the record's origin tile is ((x - H) >> 3, (y - H) >> 3)).  on: the
// tile is one of the record's 4 x 4 (and the item is `live`); without it the
// record's first tile is addressed.  Clamped to the table whatever the
// arguments hold: the step kernel loads through it unpredicated, and a step
// ahead for a predicted cell (mc_env_step.h vis_items_load, vis_prefetch).
__host__ __device__ inline size_t vis_item_offset(int G, int Wp, int Lp, int H, int g, int gi, int gj, int x, int y,
                                                  bool live, bool* on) {
  const uint32_t last = (uint32_t)G * (uint32_t)Wp * (uint32_t)Lp - 1u;  // never past the table
  const uint32_t ri = (uint32_t)(gi - ((x - H) >> 3)), rj = (uint32_t)(gj - ((y - H) >> 3));
  *on = live & (ri < 4u) & (rj < 4u);
  const uint32_t idx = vis_index(Wp, Lp, g, x, y);
  const uint32_t rec = idx < last ? idx : last;
  return (size_t)rec * (kVisRecWords * 4) + (*on ? (ri * 4u + rj) * 8u : 0u);
}

// isInBounds + grid < 0 of one grid's tiles (neg: its MT tiles in tile_index order)
__host__ __device__ inline bool vis_blocked(const uint64_t* neg, int TCS, int Wp, int Lp, int x, int y) {
  if (x < 0 || y < 0 || x >= Wp || y >= Lp) return true;
  return (neg[tile_index(TCS, x >> 3, y >> 3)] >> (((x & 7) << 3) | (y & 7))) & 1ull;
}

// The record of cell (x, y): the generic march of mc_env_step.h (ray_init,
// ray_advance, ray_mark and sense()'s premarks) run for every beam from that
// cell.  beam_bits / bcmax / beam_common / beam_k1 as in State.  rec:
// kVisRecWords words, all written.
__host__ __device__ inline void vis_record(const uint64_t* neg, int TCS, int Wp, int Lp, int H, const Beam* beams,
                                           int nbeams, const uint64_t* beam_bits, int bcmax, int beam_common,
                                           uint32_t beam_k1, int x, int y, uint32_t* rec) {
  for (int r = 0; r < kVisRecWords; ++r) rec[r] = 0u;
  if (vis_blocked(neg, TCS, Wp, Lp, x, y)) {  // no robot stands here; the reference's beams would all end at once
    rec[H] = 1u << H;
    return;
  }
  // step 0 of every beam is the robot's own cell; with common patterns the
  // step-1 cells are marked once per agent (State::beam_k1, a 3 x 3 mask)
  rec[H] |= 1u << H;
  for (int dx = -1; dx <= 1; ++dx)
    for (int dy = -1; dy <= 1; ++dy)
      if ((beam_k1 >> (3 * (dx + 1) + (dy + 1))) & 1u) rec[H + dx] |= 1u << (H + dy);
  for (int b = 0; b < nbeams; ++b) {
    const Beam bm = beams[b];
    const bool ax = (bm.axis & 1) == 0;  // major axis x (rows)
    const uint32_t bits =
        (beam_common || !(bm.axis & 2)) ? bm.bits : (uint32_t)beam_bits[(size_t)b * bcmax + (ax ? y : x)];
    int cx = x, cy = y;
    for (int k = 1; k <= bm.K; ++k) {
      // ray_advance with step k - 1's bit: one cell along the major axis,
      // and along the minor one where the float64 chain's cell moves
      const int mv = ((bits >> (k - 1)) & 1u) ? bm.msign : 0;
      cx += ax ? bm.sign : mv;
      cy += ax ? mv : bm.sign;
      const int r = cx - x + H, c = cy - y + H;
      if (r < 0 || r > 2 * H || c < 0 || c > 2 * H) break;  // (cannot happen: K <= H)
      rec[r] |= 1u << c;
      if (vis_blocked(neg, TCS, Wp, Lp, cx, cy)) break;  // oc[int(cx), int(cy)] < 0: the beam ends here
    }
  }
}

// The table's record of cell (x, y) from vis_record's rows: the marks as map
// tiles (see the head of this file).  SPLIT: 16 free-mark tiles, then 16
// obstacle-mark tiles -- a mark is an obstacle mark where vis_blocked, which
// for whole tiles is the grid tile itself (cells of an edge tile beyond the map
// are set in it: pack_grids_kernel) or all ones outside the map's tiles.
// out: 16 (SPLIT: 32) tiles, all written.
template <bool SPLIT>
__host__ __device__ inline void vis_tiles_as(const uint32_t* rows, const uint64_t* neg, int TCS, int Wp, int Lp, int H,
                                             int x, int y, uint64_t* out) {
  const int ox = (x - H) >> 3, oy = (y - H) >> 3;  // arithmetic shifts: floor
  const int rx = (x - H) - 8 * ox, ry = (y - H) - 8 * oy;  // 0 .. 7
  for (int t = 0; t < (SPLIT ? 2 : 1) * kVisTiles; ++t) out[t] = 0ull;
  for (int r = 0; r <= 2 * H; ++r) {
    const uint32_t w = rows[r] << ry;  // the window row from its first tile's column 0: 7 + 21 bits
    const int lx = rx + r;
    for (int j = 0; j < 4; ++j) out[4 * (lx >> 3) + j] |= (uint64_t)((w >> (8 * j)) & 0xFFu) << (8 * (lx & 7));
  }
  if (SPLIT) {
    const int TR = (Wp + 7) >> 3, TC = (Lp + 7) >> 3;
    for (int t = 0; t < kVisTiles; ++t) {
      const int gi = ox + (t >> 2), gj = oy + (t & 3);
      const uint64_t n = (gi >= 0 && gj >= 0 && gi < TR && gj < TC) ? neg[tile_index(TCS, gi, gj)] : ~0ull;
      const uint64_t m = out[t];
      out[t] = m & ~n;
      out[kVisTiles + t] = m & n;
    }
  }
}
__host__ __device__ inline void vis_tiles(const uint32_t* rows, const uint64_t* neg, int TCS, int Wp, int Lp, int H,
                                          int x, int y, uint64_t* out) {
  vis_tiles_as<kVisSplit>(rows, neg, TCS, Wp, Lp, H, x, y, out);
}

// the build kernel's launcher (mc_vistab.hip): every record of the pool's
// table from the State's grids and beam table, on `stream`
hipError_t launch_vis_build(const State& s, uint32_t* table, hipStream_t stream);

}  // namespace mc
