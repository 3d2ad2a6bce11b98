// mc_dijkstra.hip — the dijkstra_input observation layer.
//
// Reference: Environments/dijkstra.py:112-187 dijkstra_path_map, called from
// Environments/dec_grid_rl.py:354-358 as
//   dijkstra_path_map(free_pad[i] - obst_pad[i], x + pad, y + pad)
// and cropped E x E around the robot into obs layer 3.  On the map
// g = free - obst (1 explored, 0 unexplored, -1 obstacle; the pad ring is 0)
// a PriorityQueue of (cost, (x, y)) pops cells in BFS order, ties by (x, y);
// the first popped 0-cell is the end point; the path is then walked back from
// it, at each cell taking the first neighbour in the order +x, -x, +y, -y whose
// cost is one less.
//
// GPU form, two kernels.  The window kernel runs one wave per (env, agent)
// on the 64 x 64 cells (8 x 8 tiles) around the robot, one window row per
// lane in registers: a BFS layer is two cross-lane shifts and a few bit
// operations, no LDS and no barrier.  Every cell of BFS layer j lies within
// L1 distance j of the start, and the robot sits at least 24 cells inside
// the window on every side, so layers 1..24 (and the walk back, which stays
// on cells of cost < d*) are exact in the window; an (env, agent) whose
// nearest unexplored cell is farther is appended to a device list that the
// full kernel (below) then solves on the whole map.
//
// Full kernel: one workgroup per listed (env, agent).  The map is held in LDS
// as row bitboards (one bit per cell, 64 columns per word) over the
// pad-extended grid.  BFS layer j is dilate(layer j-1) & ~reached & ~obstacle: a whole
// layer per step of bit operations.  The pop order inside a layer only
// matters for the end point, which is the (x, y)-smallest 0-cell of the first
// layer that holds one — a workgroup min.  For the walk back only cost mod 3
// is kept (two bitboards): a neighbour of a cost-j cell has cost j-1, j or
// j+1, and mod 3 tells them apart.  Four lanes test the four neighbours of
// the walk in parallel; the first valid one in reference order wins.
//
// Big kernel (dijkstra_big_kernel): the full kernel's role on maps whose
// seven bitboards do not fit one workgroup's LDS (about 360 x 360 cells and
// up).  Same BFS, same end point, same walk back; the planes sit in a
// library-owned HBM scratch, one slot per workgroup of a fixed grid, and the
// agent's tiles are read from the state directly.  Layer j only holds cells
// within L1 distance j of the start, so its sweep covers the band of rows
// sx - j .. sx + j and the words of columns sy - j .. sy + j: the work grows
// with d*^2, not with the map, and a plane word is initialised by the sweep
// that first meets it.
//
// Every kernel's body is a template over a compile-time sink for its result:
// the obs layer's crop (dijkstra_*_kernel) or the move of mc_frontier_actions
// (frontier_*_kernel: action byte, d* and goal per item; mc_frontier.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>

#include "mc_bitboard.h"
#include "mc_frontier.h"

namespace mc {

namespace {

constexpr int kDjThreads = 256;
constexpr unsigned kDjFullGrid = 256;  // workgroups of the full-map kernel over the listed items

struct DjLds {
  uint64_t *ob, *tg, *bl, *f0, *f1, *m0, *m1;
  uint64_t *tf, *to;  // the agent's free / obstacle tiles
};

// What a solve leaves behind (a compile-time choice of every kernel below; the
// BFS and the end point are shared).  The crop sink records the path cells
// inside the E x E crop: obs layer `layer` of obs_out.  The move sink keeps
// only the walk's last step, the cell reached at j = 1, and one lane stores the
// action byte, d* and the goal (mc_frontier_actions; dist / goal may be null).
struct DjCropSink {
  static constexpr bool kCrop = true;
  int layer, Lc;
  uint8_t* __restrict__ obs_out;
};

struct DjMoveSink {
  static constexpr bool kCrop = false;
  uint8_t* __restrict__ act;   // [B][N]
  int32_t* __restrict__ dist;  // [B][N] or null
  int32_t* __restrict__ goal;  // [B][N][2] or null
  // item ea: d*, the start and the cost-1 cell (extended coordinates; any cell
  // when d* < 1), the end point's extended cell index (when d* >= 0)
  __device__ __forceinline__ void put(uint32_t ea, int dstar, int sx, int sy, int c1x, int c1y, int end,
                                      int RY, int pad) const {
    act[ea] = (uint8_t)(dstar >= 1 ? frontier_action(c1x - sx, c1y - sy) : kActStay);
    if (dist) dist[ea] = dstar;
    if (goal) {
      int32_t gx, gy;
      frontier_cell_xy(dstar >= 0 ? end : sx * RY + sy, RY, pad, &gx, &gy);
      goal[2 * (size_t)ea] = gx;
      goal[2 * (size_t)ea + 1] = gy;
    }
  }
};

}  // namespace

// one (env, agent) on the whole map; every thread of the workgroup calls it
template <class Sink>
__device__ __forceinline__ void dijkstra_full(const State& s, int pad, const Sink& out, int e, int a,
                                              char* smem) {
  __shared__ int s_end[3], s_any[3];  // per BFS layer j: slot j % 3
  __shared__ uint32_t s_crop[32];
  const int tid = threadIdx.x;
  const int RX = s.Wp + 2 * pad, RY = s.Lp + 2 * pad, RW = (RY + 63) >> 6, NW = RX * RW;
  const int mt = s.MT;
  DjLds L;
  uint64_t* p = reinterpret_cast<uint64_t*>(smem);
  L.ob = p;
  L.tg = p + NW;
  L.bl = p + 2 * NW;
  L.f0 = p + 3 * NW;
  L.f1 = p + 4 * NW;
  L.m0 = p + 5 * NW;
  L.m1 = p + 6 * NW;
  L.tf = p + 7 * NW;
  L.to = L.tf + mt;

  // the agent's maps (tiles) and start cell
  const size_t fb = ((size_t)e * s.N + a) * mt;
  for (int i = tid; i < mt; i += kDjThreads) {
    L.tf[i] = s.freem[fb + i];
    L.to[i] = s.obstm[fb + i];
  }
  const int sx = s.pos[((size_t)e * s.N + a) * 2] + pad;
  const int sy = s.pos[((size_t)e * s.N + a) * 2 + 1] + pad;
  if constexpr (Sink::kCrop) {
    if (tid < 32) s_crop[tid] = 0;
  }
  if (tid < 3) {
    s_end[tid] = INT32_MAX;
    s_any[tid] = 0;
  }
  __syncthreads();
  // g = free - obst: obstacle where only obst is set, target (0) where both or
  // neither are; columns past the extended grid are neither
  const uint64_t last = (RY & 63) ? low_mask(RY & 63) : ~0ull;
  for (int i = tid; i < NW; i += kDjThreads) {
    const int u = i / RW, w = i - u * RW;
    uint64_t f, o;
    f = row_word(s, L.tf, pad, u, w);
    o = row_word(s, L.to, pad, u, w);
    const uint64_t in = (w == RW - 1) ? last : ~0ull;
    L.ob[i] = o & ~f & in;
    L.tg[i] = ~(f ^ o) & in;
    const int si = sx * RW + (sy >> 6);
    const uint64_t sb = (i == si) ? (1ull << (sy & 63)) : 0ull;
    L.bl[i] = sb;
    L.f0[i] = sb;
    L.m0[i] = 0;
    L.m1[i] = 0;
  }
  __syncthreads();

  // ---- BFS by layers ------------------------------------------------------
  int dstar = -1, end = -1;
  if ((L.tg[sx * RW + (sy >> 6)] >> (sy & 63)) & 1ull) {
    dstar = 0;  // the start cell itself is unexplored
    end = sx * RY + sy;
  } else {
    uint64_t* cur = L.f0;
    uint64_t* nxt = L.f1;
    for (int j = 1; j <= RX * RY; ++j) {
      // slot j % 3 collects layer j; slot (j+1) % 3 is reset for the next
      // layer: every thread has read slot (j-2) % 3 before this layer began
      const int par = j % 3, nxt_slot = (j + 1) % 3;
      if (tid == 0) {
        s_end[nxt_slot] = INT32_MAX;
        s_any[nxt_slot] = 0;
      }
      int any = 0, best = INT32_MAX;
      for (int i = tid; i < NW; i += kDjThreads) {
        const int u = i / RW, w = i - u * RW;
        const uint64_t c = cur[i];
        uint64_t d = c | (c << 1) | (c >> 1);
        if (w > 0) d |= cur[i - 1] >> 63;
        if (w < RW - 1) d |= cur[i + 1] << 63;
        if (u > 0) d |= cur[i - RW];
        if (u < RX - 1) d |= cur[i + RW];
        const uint64_t in = (w == RW - 1) ? last : ~0ull;
        const uint64_t nf = d & ~L.bl[i] & ~L.ob[i] & in;
        nxt[i] = nf;
        if (nf) {
          L.bl[i] |= nf;
          const int m = j % 3;
          if (m == 1) L.m0[i] |= nf;
          if (m == 2) L.m1[i] |= nf;
          any = 1;
          const uint64_t hit = nf & L.tg[i];
          if (hit) best = min(best, u * RY + 64 * w + __ffsll((unsigned long long)hit) - 1);
        }
      }
      if (any) atomicOr(&s_any[par], 1);
      if (best != INT32_MAX) atomicMin(&s_end[par], best);
      __syncthreads();
      if (s_end[par] != INT32_MAX) {
        dstar = j;
        end = s_end[par];
        break;
      }
      if (!s_any[par]) break;  // no reachable unexplored cell: empty path
      uint64_t* t = cur;
      cur = nxt;
      nxt = t;
    }
  }

  // ---- walk back from the end point (first wave, lanes 0..3) --------------
  const int E = s.E, ego = s.ego;
  const int cx0 = sx - ego, cy0 = sy - ego;  // crop origin (dgrid coordinates)
  int c1u = sx, c1v = sy;                    // move sink: the path's cost-1 cell
  if (dstar >= 0 && tid < 64) {
    int cu = end / RY, cv = end - (end / RY) * RY;
    int j = dstar;
    const int du = tid == 0 ? 1 : (tid == 1 ? -1 : 0);
    const int dv = tid == 2 ? 1 : (tid == 3 ? -1 : 0);
    for (;;) {
      if constexpr (Sink::kCrop) {
        if (tid == 0) {
          const int r = cu - cx0, c = cv - cy0;
          if (r >= 0 && r < E && c >= 0 && c < E) s_crop[r] |= 1u << c;
        }
      } else if (j == 1) {
        c1u = cu;
        c1v = cv;
      }
      if (j == 0) break;
      const int nu = cu + du, nv = cv + dv;
      bool ok = false;
      if (tid < 4 && nu >= 0 && nu < RX && nv >= 0 && nv < RY) {
        const int i = nu * RW + (nv >> 6), b = nv & 63;
        const int m = (int)((L.m0[i] >> b) & 1ull) + 2 * (int)((L.m1[i] >> b) & 1ull);
        ok = ((L.bl[i] >> b) & 1ull) && m == (j - 1) % 3;
      }
      const uint64_t v = __ballot(ok) & 0xFull;
      if (!v) {  // cannot happen: a cost-j cell has a cost-(j-1) neighbour
        if (tid == 0) atomicOr(s.err, ERR_WINDOW);
        break;
      }
      const int q = __ffsll((unsigned long long)v) - 1;
      cu = __shfl(nu, q);
      cv = __shfl(nv, q);
      --j;
    }
  }
  if constexpr (Sink::kCrop) {
    __syncthreads();
    // ---- obs layer `layer` of agent a: the path cells inside the crop ----------
    uint8_t* dst = out.obs_out + (((size_t)e * s.N + a) * out.Lc + out.layer) * E * E;
    for (int i = tid; i < E * E; i += kDjThreads) {
      const int r = i / E, c = i - r * E;
      dst[i] = (uint8_t)((s_crop[r] >> c) & 1u);
    }
  } else {
    // ---- the move: lane 0 of the walk's wave holds the cost-1 cell ---------------
    if (tid == 0) out.put((uint32_t)e * (uint32_t)s.N + (uint32_t)a, dstar, sx, sy, c1u, c1v, end, RY, pad);
  }
}

// Full-map solve of the listed (env, agent) items: a fixed grid strides over
// the *count entries (the count is uniform, so every wave reaches the end).
// list == nullptr: every (env, agent), one workgroup each.
// count[0] = entries, count[1] = workgroups done: the last workgroup to
// finish zeroes both for the next step's window kernel (every workgroup has
// read the entry count before it counts itself done) and keeps the entry
// count in count[2] (MC_FIELD_DJ_LISTED for the obs layer's list; the frontier
// call brings count words and a list of its own).
template <class Sink>
__device__ __forceinline__ void dijkstra_items(const State& s, int pad, const Sink& out,
                                               const uint32_t* __restrict__ list,
                                               uint32_t* __restrict__ count, char* smem) {
  const uint32_t n_items = list ? __atomic_load_n(count, __ATOMIC_RELAXED) : (uint32_t)gridDim.x;
  for (uint32_t it = blockIdx.x; it < n_items; it += (list ? gridDim.x : n_items)) {
    __syncthreads();  // the previous item's LDS reads are done
    const uint32_t ea = list ? list[it] : it;
    dijkstra_full(s, pad, out, (int)(ea / (uint32_t)s.N), (int)(ea % (uint32_t)s.N), smem);
  }
  if (list && threadIdx.x == 0) {
    if (n_items == 0) {  // nothing listed: nothing to reset (every workgroup read 0)
      if (blockIdx.x == 0) count[2] = 0;
    } else {
      __threadfence();
      if (atomicAdd(count + 1, 1u) == gridDim.x - 1) {
        atomicExch(count + 2, atomicExch(count, 0u));
        atomicExch(count + 1, 0u);
      }
    }
  }
}

__global__ __launch_bounds__(kDjThreads) void dijkstra_kernel(State s, int pad, int layer, int Lc,
                                                              uint8_t* __restrict__ obs_out,
                                                              const uint32_t* __restrict__ list,
                                                              uint32_t* __restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  dijkstra_items(s, pad, DjCropSink{layer, Lc, obs_out}, list, count, smem);
}

// ... with the move sink, over the frontier call's own list (mc_frontier_actions)
__global__ __launch_bounds__(kDjThreads) void frontier_kernel(State s, int pad, DjMoveSink out,
                                                              const uint32_t* __restrict__ list,
                                                              uint32_t* __restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  dijkstra_items(s, pad, out, list, count, smem);
}

// ---- window kernel ---------------------------------------------------------
constexpr int kDjWinDepth = 24;  // BFS layers the 64 x 64 window holds exactly (a multiple of 3)

// whole-wave lane shifts of a 64-bit row (DPP wave_shr:1 / wave_shl:1; the
// lane past the end reads 0): row r - 1 / row r + 1 of the window at lane r
__device__ __forceinline__ uint64_t row_above(uint64_t v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x138, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x138, 0xF, 0xF, true);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ uint64_t row_below(uint64_t v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x130, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x130, 0xF, 0xF, true);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

__device__ __forceinline__ uint64_t bits_between(int lo, int hi) {  // bits [lo, hi), 0 <= lo, hi <= 64
  if (hi <= lo) return 0;
  const uint64_t h = hi >= 64 ? ~0ull : ((1ull << hi) - 1);
  return h & ~((1ull << lo) - 1);
}

// bit c of lane `lane`'s row v (lane and c uniform)
__device__ __forceinline__ uint32_t lane_bit(uint64_t v, int lane, int c) {
  const uint32_t w = (uint32_t)(v >> (c & 32));
  return ((uint32_t)__builtin_amdgcn_readlane((int)w, lane) >> (c & 31)) & 1u;
}

// cells whose neighbour at shift S has cost one less (cost mod 3 classes
// K0, K1, K2; the predecessor of class k is class k + 2 mod 3)
__device__ __forceinline__ uint64_t pred(uint64_t k0, uint64_t k1, uint64_t k2, uint64_t s0,
                                         uint64_t s1, uint64_t s2) {
  return (k0 & s2) | (k1 & s0) | (k2 & s1);
}

// grid = B * N workgroups of one wave; lane r holds window row r.  The window
// is tiles [tx - 4, tx + 4) x [ty - 4, ty + 4) of the robot's tile (tx, ty),
// i.e. map rows X0 = 8 (tx - 4) .. X0 + 63 and columns Y0 .. Y0 + 63; bit c of
// a row word is column Y0 + c.  depth: the exact layers (kDjWinDepth).
template <class Sink>
__device__ __forceinline__ void dijkstra_window(const State& s, int pad, const Sink& out,
                                                uint32_t* __restrict__ list,
                                                uint32_t* __restrict__ count, int depth) {
  __shared__ uint8_t s_rows[2][64 * 8];  // free / obstacle window rows (tile transpose)
  const uint32_t ea = blockIdx.x;
  const int r = threadIdx.x;
  const int px = s.pos[2 * ea], py = s.pos[2 * ea + 1];  // padded-grid cell of the robot
  const int tx0 = (px >> 3) - 4, ty0 = (py >> 3) - 4;
  const int X0 = 8 * tx0, Y0 = 8 * ty0;
  const int X = X0 + r;
  const int rs = px - X0, cs = py - Y0;  // the robot in window coordinates (32..39)

  // ---- the agent's maps: lane l loads tile (tx0 + l / 8, ty0 + l % 8) of each
  // plane; byte k of it (tile row k) goes to window row 8 (l / 8) + k, byte l % 8
  {
    const int ti = tx0 + (r >> 3), tj = ty0 + (r & 7);
    uint64_t f = 0, o = 0;
    if (ti >= 0 && ti < s.TR && tj >= 0 && tj < s.TC) {
      const size_t i = (size_t)ea * s.MT + tile_index(s.TCS, ti, tj);
      f = s.freem[i];
      o = s.obstm[i];
    }
    uint8_t* df = s_rows[0] + (r >> 3) * 64 + (r & 7);
    uint8_t* dob = s_rows[1] + (r >> 3) * 64 + (r & 7);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      df[8 * k] = (uint8_t)(f >> (8 * k));
      dob[8 * k] = (uint8_t)(o >> (8 * k));
    }
  }
  __syncthreads();
  const uint64_t f = reinterpret_cast<const uint64_t*>(s_rows[0])[r];
  const uint64_t o = reinterpret_cast<const uint64_t*>(s_rows[1])[r];
  // cells of the extended grid (the pad ring is unexplored: a target)
  const uint64_t valid = (X >= -pad && X < s.Wp + pad)
                             ? bits_between(max(-pad - Y0, 0), min(s.Lp + pad - Y0, 64))
                             : 0ull;
  const uint64_t ob = o & ~f & valid;    // g = -1
  const uint64_t tg = ~(f ^ o) & valid;  // g = 0

  // ---- BFS by layers in registers ---------------------------------------------
  // avail: cells not reached yet; m0 / m1: layers j = 1 / 2 (mod 3).  Three
  // layers per trip (each one's mod-3 plane is static) and one target test
  // per trip: a trip with a hit then finds its first layer that has one.
  // Layers past d* (at most two) join the planes too; that is harmless: a
  // neighbour of a cost-j cell has cost j-1, j or j+1, so the walk back's
  // mod-3 test only ever meets those.  A frontier that dies out ends the
  // search at the trip's end (the layers after an empty one are empty).
  // depth is a multiple of 3 (launch_dijkstra).
  int dstar = -1, er = rs, ec = cs;
  bool full = false;
  uint64_t cur = r == rs ? (1ull << cs) : 0ull;
  uint64_t avail = ~ob & valid & ~cur, m0 = 0, m1 = 0;
  if (lane_bit(tg, rs, cs)) {
    dstar = 0;  // the start cell itself is unexplored
  } else {
    for (int j = 0;; j += 3) {
      if (j >= depth) {
        full = true;
        break;
      }
      uint64_t nf[3];
      nf[0] = (cur | (cur << 1) | (cur >> 1) | row_above(cur) | row_below(cur)) & avail;
      avail ^= nf[0];
      m0 |= nf[0];
      nf[1] = (nf[0] | (nf[0] << 1) | (nf[0] >> 1) | row_above(nf[0]) | row_below(nf[0])) & avail;
      avail ^= nf[1];
      m1 |= nf[1];
      nf[2] = (nf[1] | (nf[1] << 1) | (nf[1] >> 1) | row_above(nf[1]) | row_below(nf[1])) & avail;
      avail ^= nf[2];
      cur = nf[2];
      if (__ballot(((nf[0] | nf[1] | nf[2]) & tg) != 0)) {
        // the first layer of the trip with a target; its (x, y)-smallest one:
        // lowest row, then column
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const uint64_t hit = nf[q] & tg;
          const uint64_t hr = __ballot(hit != 0);
          if (hr) {
            er = __ffsll((unsigned long long)hr) - 1;
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)hit, er);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(hit >> 32), er);
            ec = lo ? __ffs(lo) - 1 : 32 + __ffs(hi) - 1;
            dstar = j + 1 + q;
            break;
          }
        }
        break;
      }
      if (!__ballot(cur != 0)) break;  // no reachable unexplored cell: empty path
    }
  }
  if (full) {  // farther than the window holds: the full kernel solves it
    if (r == 0) list[atomicAdd(count, 1u)] = ea;
    return;
  }

  // ---- walk back (dijkstra.py:166-185): from each cell the first neighbour in
  // the order +x, -x, +y, -y whose cost is one less.  The choice of every
  // reached cell at once, as two direction planes q = 2 d1 + d0 (a reached
  // cell of cost >= 1 always has such a neighbour: its BFS parent); then the
  // walk reads one bit pair per step (readlane, scalar).  Only crop cells are
  // recorded: lane k keeps crop row k.
  const int E = s.E, ego = s.ego;
  const int cr0 = rs - ego, cc0 = cs - ego;  // crop origin (window coordinates)
  uint32_t crop = 0;
  int c1r = rs, c1c = cs;  // move sink: the path's cost-1 cell (window coordinates)
  if (dstar >= 0) {
    const uint64_t k1 = m0, k2 = m1, k0 = ~ob & valid & ~avail & ~m0 & ~m1;  // reached, cost = 0 mod 3
    const uint64_t px_ = pred(k0, k1, k2, row_below(k0), row_below(k1), row_below(k2));
    const uint64_t mx_ = pred(k0, k1, k2, row_above(k0), row_above(k1), row_above(k2));
    const uint64_t py_ = pred(k0, k1, k2, k0 >> 1, k1 >> 1, k2 >> 1);
    const uint64_t d1 = ~px_ & ~mx_;
    const uint64_t d0 = (~px_ & mx_) | (d1 & ~py_);
    int cu = er, cv = ec;
    for (int j = dstar;; --j) {
      if constexpr (Sink::kCrop) {
        const int kr = cu - cr0, kc = cv - cc0;
        if ((unsigned)kr < (unsigned)E && (unsigned)kc < (unsigned)E && r == kr) crop |= 1u << kc;
      } else if (j == 1) {
        c1r = cu;
        c1c = cv;
      }
      if (j == 0) break;
      const int q = (int)(2 * lane_bit(d1, cu, cv) + lane_bit(d0, cu, cv));
      cu += q == 0 ? 1 : (q == 1 ? -1 : 0);
      cv += q == 2 ? 1 : (q == 3 ? -1 : 0);
    }
  }
  if constexpr (Sink::kCrop) {
    // ---- obs layer `layer`: crop row k = window row rs - ego + k ------------------
    if (r < E) {
      uint8_t* dst = out.obs_out + ((size_t)ea * out.Lc + out.layer) * E * E + (size_t)r * E;
      for (int c = 0; c < E; ++c) dst[c] = (uint8_t)((crop >> c) & 1u);
    }
  } else {
    // ---- the move: the walk is wave-uniform, lane 0 stores it (extended
    // coordinates: window cell (k, c) is padded-grid cell (X0 + k, Y0 + c))
    const int RY = s.Lp + 2 * pad;
    if (r == 0)
      out.put(ea, dstar, px + pad, py + pad, X0 + c1r + pad, Y0 + c1c + pad,
              frontier_cell_index(X0 + er, Y0 + ec, RY, pad), RY, pad);
  }
}

__global__ __launch_bounds__(64) void dijkstra_window_kernel(State s, int pad, int layer, int Lc,
                                                             uint8_t* __restrict__ obs_out,
                                                             uint32_t* __restrict__ list,
                                                             uint32_t* __restrict__ count,
                                                             int depth) {
  dijkstra_window(s, pad, DjCropSink{layer, Lc, obs_out}, list, count, depth);
}

__global__ __launch_bounds__(64) void frontier_window_kernel(State s, int pad, DjMoveSink out,
                                                             uint32_t* __restrict__ list,
                                                             uint32_t* __restrict__ count,
                                                             int depth) {
  dijkstra_window(s, pad, out, list, count, depth);
}

// ---- big kernel: the planes in HBM -----------------------------------------
namespace {

// workgroups (= scratch slots) of the big kernel: one per CU (256 depth-120
// items on bg2_1073x1073 took 3.19 / 1.68 / 1.02 ms at 64 / 128 / 256,
// profiles/r7/dj_big)
constexpr unsigned kDjBigGrid = 256;
constexpr size_t kDjBigBudget = 256ull << 20;   // bytes of scratch the slots may take together
constexpr int kDjBigPlanes = 7;                 // ob, tg, bl, m0, m1, f0, f1

// the words BFS layer j can touch: rows ulo..uhi, words wlo..whi of each
struct DjBand {
  int ulo, uhi, wlo, whi;
  __device__ __forceinline__ bool rows(int u) const { return u >= ulo && u <= uhi; }
  __device__ __forceinline__ bool words(int w) const { return w >= wlo && w <= whi; }
};

__device__ __forceinline__ DjBand dj_band(int sx, int sy, int j, int RX, int RY) {
  const int r = min(j, RX + RY);  // every cell is within L1 distance RX + RY
  return {max(sx - r, 0), min(sx + r, RX - 1), max(sy - r, 0) >> 6, min(sy + r, RY - 1) >> 6};
}

}  // namespace

// One (env, agent) on the whole map, planes in this workgroup's scratch slot;
// every thread of the workgroup calls it.  The slot still holds the last
// solve's words, so nothing is read that this solve has not written: the
// bands are nested, a word outside band j - 1 counts as empty (no reached
// cell can lie there), and the sweep of layer j writes every plane of a word
// that enters the band with it.  The frontier planes need no such care past
// band 0: layer j writes nxt over all of band j, which is all that layer
// j + 1 reads of it.  Threads hand words to each other only across the
// __syncthreads() that ends a layer (one workgroup owns the slot).
template <class Sink>
__device__ __forceinline__ void dijkstra_big(const State& s, int pad, const Sink& out, int e, int a,
                                             uint64_t* planes) {
  __shared__ int s_end[3], s_any[3], s_tg0;  // per BFS layer j: slot j % 3; the start cell's target bit
  __shared__ uint32_t s_crop[32];
  const int tid = threadIdx.x;
  const int RX = s.Wp + 2 * pad, RY = s.Lp + 2 * pad, RW = (RY + 63) >> 6;
  const size_t NW = (size_t)RX * RW;
  uint64_t* const ob = planes;
  uint64_t* const tg = planes + NW;
  uint64_t* const bl = planes + 2 * NW;
  uint64_t* const m0 = planes + 3 * NW;
  uint64_t* const m1 = planes + 4 * NW;
  uint64_t* const f0 = planes + 5 * NW;
  uint64_t* const f1 = planes + 6 * NW;
  // the agent's maps (tiles) and start cell
  const uint64_t* tf = s.freem + ((size_t)e * s.N + a) * s.MT;
  const uint64_t* to = s.obstm + ((size_t)e * s.N + a) * s.MT;
  const int sx = s.pos[((size_t)e * s.N + a) * 2] + pad;
  const int sy = s.pos[((size_t)e * s.N + a) * 2 + 1] + pad;
  const uint64_t last = (RY & 63) ? low_mask(RY & 63) : ~0ull;
  if constexpr (Sink::kCrop) {
    if (tid < 32) s_crop[tid] = 0;
  }
  if (tid < 3) {
    s_end[tid] = INT32_MAX;
    s_any[tid] = 0;
  }
  if (tid == 0) {  // band 0: the start cell's word
    const int w = sy >> 6;
    const size_t i = (size_t)sx * RW + w;
    const uint64_t f = row_word(s, tf, pad, sx, w), o = row_word(s, to, pad, sx, w);
    const uint64_t in = (w == RW - 1) ? last : ~0ull;
    const uint64_t t = ~(f ^ o) & in, sb = 1ull << (sy & 63);
    ob[i] = o & ~f & in;
    tg[i] = t;
    bl[i] = sb;
    f0[i] = sb;
    m0[i] = 0;
    m1[i] = 0;
    s_tg0 = (int)((t >> (sy & 63)) & 1ull);
  }
  __syncthreads();

  // ---- BFS by layers ------------------------------------------------------
  int dstar = -1, end = -1;
  DjBand fb = dj_band(sx, sy, 0, RX, RY);  // the band of the last layer swept
  if (s_tg0) {
    dstar = 0;  // the start cell itself is unexplored
    end = sx * RY + sy;
  } else {
    uint64_t* cur = f0;
    uint64_t* nxt = f1;
    for (int j = 1; j <= RX * RY; ++j) {
      // slot j % 3 collects layer j; slot (j+1) % 3 is reset for the next
      // layer: every thread has read slot (j-2) % 3 before this layer began
      const int par = j % 3, nxt_slot = (j + 1) % 3;
      if (tid == 0) {
        s_end[nxt_slot] = INT32_MAX;
        s_any[nxt_slot] = 0;
      }
      const DjBand pb = fb;  // band j - 1: the words written so far
      fb = dj_band(sx, sy, j, RX, RY);
      const int bw = fb.whi - fb.wlo + 1, n = (fb.uhi - fb.ulo + 1) * bw;
      int any = 0, best = INT32_MAX;
      for (int k = tid; k < n; k += kDjThreads) {
        const int ur = k / bw, u = fb.ulo + ur, w = fb.wlo + (k - ur * bw);
        const size_t i = (size_t)u * RW + w;
        const bool old = pb.rows(u) && pb.words(w);
        uint64_t d = 0;
        if (pb.rows(u)) {
          if (old) {
            const uint64_t c = cur[i];
            d = c | (c << 1) | (c >> 1);
          }
          if (pb.words(w - 1)) d |= cur[i - 1] >> 63;
          if (pb.words(w + 1)) d |= cur[i + 1] << 63;
        }
        if (pb.words(w)) {
          if (pb.rows(u - 1)) d |= cur[i - RW];
          if (pb.rows(u + 1)) d |= cur[i + RW];
        }
        const uint64_t in = (w == RW - 1) ? last : ~0ull;
        uint64_t o, r, t = 0;
        if (old) {
          o = ob[i];
          r = bl[i];
        } else {  // the word enters the band: g = free - obst, as dijkstra_full
          const uint64_t f = row_word(s, tf, pad, u, w);
          o = row_word(s, to, pad, u, w);
          t = ~(f ^ o) & in;
          o = o & ~f & in;
          r = 0;
          ob[i] = o;
          tg[i] = t;
        }
        const uint64_t nf = d & ~r & ~o & in;
        const int m = j % 3;
        nxt[i] = nf;
        if (!old) {
          bl[i] = nf;
          m0[i] = m == 1 ? nf : 0ull;
          m1[i] = m == 2 ? nf : 0ull;
        } else if (nf) {
          bl[i] = r | nf;
          if (m == 1) m0[i] |= nf;
          if (m == 2) m1[i] |= nf;
        }
        if (nf) {
          any = 1;
          const uint64_t hit = nf & (old ? tg[i] : t);
          if (hit) best = min(best, u * RY + 64 * w + __ffsll((unsigned long long)hit) - 1);
        }
      }
      if (any) atomicOr(&s_any[par], 1);
      if (best != INT32_MAX) atomicMin(&s_end[par], best);
      __syncthreads();
      if (s_end[par] != INT32_MAX) {
        dstar = j;
        end = s_end[par];
        break;
      }
      if (!s_any[par]) break;  // no reachable unexplored cell: empty path
      uint64_t* t = cur;
      cur = nxt;
      nxt = t;
    }
  }

  // ---- walk back from the end point (first wave, lanes 0..3): the planes of
  // the four neighbours from HBM, one dependent load per path cell; a
  // neighbour outside the last band was never reached
  const int E = s.E, ego = s.ego;
  const int cx0 = sx - ego, cy0 = sy - ego;  // crop origin (dgrid coordinates)
  int c1u = sx, c1v = sy;                    // move sink: the path's cost-1 cell
  if (dstar >= 0 && tid < 64) {
    int cu = end / RY, cv = end - (end / RY) * RY;
    int j = dstar;
    const int du = tid == 0 ? 1 : (tid == 1 ? -1 : 0);
    const int dv = tid == 2 ? 1 : (tid == 3 ? -1 : 0);
    for (;;) {
      if constexpr (Sink::kCrop) {
        if (tid == 0) {
          const int r = cu - cx0, c = cv - cy0;
          if (r >= 0 && r < E && c >= 0 && c < E) s_crop[r] |= 1u << c;
        }
      } else if (j == 1) {
        c1u = cu;
        c1v = cv;
      }
      if (j == 0) break;
      const int nu = cu + du, nv = cv + dv;
      bool ok = false;
      if (tid < 4 && nv >= 0 && nv < RY && fb.rows(nu) && fb.words(nv >> 6)) {
        const size_t i = (size_t)nu * RW + (nv >> 6);
        const int b = nv & 63;
        const int m = (int)((m0[i] >> b) & 1ull) + 2 * (int)((m1[i] >> b) & 1ull);
        ok = ((bl[i] >> b) & 1ull) && m == (j - 1) % 3;
      }
      const uint64_t v = __ballot(ok) & 0xFull;
      if (!v) {  // cannot happen: a cost-j cell has a cost-(j-1) neighbour
        if (tid == 0) atomicOr(s.err, ERR_WINDOW);
        break;
      }
      const int q = __ffsll((unsigned long long)v) - 1;
      cu = __shfl(nu, q);
      cv = __shfl(nv, q);
      --j;
    }
  }
  if constexpr (Sink::kCrop) {
    __syncthreads();
    // ---- obs layer `layer` of agent a: the path cells inside the crop ----------
    uint8_t* dst = out.obs_out + (((size_t)e * s.N + a) * out.Lc + out.layer) * E * E;
    for (int i = tid; i < E * E; i += kDjThreads) {
      const int r = i / E, c = i - r * E;
      dst[i] = (uint8_t)((s_crop[r] >> c) & 1u);
    }
  } else {
    // ---- the move: lane 0 of the walk's wave holds the cost-1 cell ---------------
    if (tid == 0) out.put((uint32_t)e * (uint32_t)s.N + (uint32_t)a, dstar, sx, sy, c1u, c1v, end, RY, pad);
  }
}

// dijkstra_kernel's role and list protocol (count[0..2] as there) with the
// planes in HBM: workgroup blockIdx.x owns scratch slot blockIdx.x and strides
// over the listed items (list == nullptr: over all n_all (env, agent) items).
template <class Sink>
__device__ __forceinline__ void dijkstra_big_items(const State& s, int pad, const Sink& out,
                                                   const uint32_t* __restrict__ list,
                                                   uint32_t* __restrict__ count, uint32_t n_all,
                                                   uint64_t* scratch, size_t slot_words) {
  uint64_t* planes = scratch + (size_t)blockIdx.x * slot_words;
  const uint32_t n_items = list ? __atomic_load_n(count, __ATOMIC_RELAXED) : n_all;
  for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    __syncthreads();  // the previous item's reads (LDS and slot) are done
    const uint32_t ea = list ? list[it] : it;
    dijkstra_big(s, pad, out, (int)(ea / (uint32_t)s.N), (int)(ea % (uint32_t)s.N), planes);
  }
  if (list && threadIdx.x == 0) {
    if (n_items == 0) {  // nothing listed: nothing to reset (every workgroup read 0)
      if (blockIdx.x == 0) count[2] = 0;
    } else {
      __threadfence();
      if (atomicAdd(count + 1, 1u) == gridDim.x - 1) {
        atomicExch(count + 2, atomicExch(count, 0u));
        atomicExch(count + 1, 0u);
      }
    }
  }
}

__global__ __launch_bounds__(kDjThreads) void dijkstra_big_kernel(State s, int pad, int layer, int Lc,
                                                                  uint8_t* __restrict__ obs_out,
                                                                  const uint32_t* __restrict__ list,
                                                                  uint32_t* __restrict__ count,
                                                                  uint32_t n_all, uint64_t* scratch,
                                                                  size_t slot_words) {
  dijkstra_big_items(s, pad, DjCropSink{layer, Lc, obs_out}, list, count, n_all, scratch, slot_words);
}

__global__ __launch_bounds__(kDjThreads) void frontier_big_kernel(State s, int pad, DjMoveSink out,
                                                                  const uint32_t* __restrict__ list,
                                                                  uint32_t* __restrict__ count,
                                                                  uint32_t n_all, uint64_t* scratch,
                                                                  size_t slot_words) {
  dijkstra_big_items(s, pad, out, list, count, n_all, scratch, slot_words);
}

size_t dijkstra_lds_bytes(const State& s, int pad) {
  const size_t RX = s.Wp + 2 * pad, RW = (s.Lp + 2 * pad + 63) / 64;
  return (7 * RX * RW + 2 * (size_t)s.MT) * 8;
}

// bytes of one scratch slot of the big kernel: its seven planes
size_t dijkstra_big_slot_bytes(const State& s, int pad) {
  const size_t RX = s.Wp + 2 * pad, RW = (s.Lp + 2 * pad + 63) / 64;
  return kDjBigPlanes * RX * RW * 8;
}

// slots (= workgroups) of the big kernel: one per item up to the fixed grid
// (MARLCOV_DJ_BIG_GRID: tests make many items share few slots) and to what
// the scratch budget holds, at least one
unsigned dijkstra_big_slots(const State& s, int pad) {
  const char* v = getenv("MARLCOV_DJ_BIG_GRID");
  const int g = v ? atoi(v) : 0;
  size_t n = g > 0 && g <= 4096 ? (size_t)g : kDjBigGrid;
  n = std::min(n, (size_t)s.B * s.N);
  n = std::min(n, kDjBigBudget / dijkstra_big_slot_bytes(s, pad));
  return (unsigned)std::max<size_t>(n, 1);
}

// list: u32 [3 + B*N] (entry count, workgroups done, last entry count, then
// the entries),
// library-owned, zero between steps.  window = false: every (env, agent) on
// the full map (the parity tests' second mode).  big: the big kernel's scratch
// of big_slots slots (mc_create: the LDS bitboards do not fit, or
// MARLCOV_DJ_BIG=1) -- it then takes the full kernel's place; nullptr: the
// full kernel.  (launch_solve below, for either sink.)
namespace {

// the three kernels of each sink (list == nullptr: every item, no protocol)
void run_window(const DjCropSink& o, unsigned items, hipStream_t st, const State& s, int pad, uint32_t* list,
                int depth) {
  hipLaunchKernelGGL(dijkstra_window_kernel, dim3(items), dim3(64), 0, st, s, pad, o.layer, o.Lc, o.obs_out,
                     list + 3, list, depth);
}
void run_window(const DjMoveSink& o, unsigned items, hipStream_t st, const State& s, int pad, uint32_t* list,
                int depth) {
  hipLaunchKernelGGL(frontier_window_kernel, dim3(items), dim3(64), 0, st, s, pad, o, list + 3, list, depth);
}
void run_full(const DjCropSink& o, unsigned grid, size_t lds, hipStream_t st, const State& s, int pad,
              uint32_t* list) {
  hipLaunchKernelGGL(dijkstra_kernel, dim3(grid), dim3(kDjThreads), lds, st, s, pad, o.layer, o.Lc, o.obs_out,
                     (const uint32_t*)(list ? list + 3 : nullptr), list);
}
void run_full(const DjMoveSink& o, unsigned grid, size_t lds, hipStream_t st, const State& s, int pad,
              uint32_t* list) {
  hipLaunchKernelGGL(frontier_kernel, dim3(grid), dim3(kDjThreads), lds, st, s, pad, o,
                     (const uint32_t*)(list ? list + 3 : nullptr), list);
}
void run_big(const DjCropSink& o, unsigned slots, hipStream_t st, const State& s, int pad, uint32_t* list,
             unsigned items, uint64_t* big, size_t slot_words) {
  hipLaunchKernelGGL(dijkstra_big_kernel, dim3(slots), dim3(kDjThreads), 0, st, s, pad, o.layer, o.Lc, o.obs_out,
                     (const uint32_t*)(list ? list + 3 : nullptr), list, items, big, slot_words);
}
void run_big(const DjMoveSink& o, unsigned slots, hipStream_t st, const State& s, int pad, uint32_t* list,
             unsigned items, uint64_t* big, size_t slot_words) {
  hipLaunchKernelGGL(frontier_big_kernel, dim3(slots), dim3(kDjThreads), 0, st, s, pad, o,
                     (const uint32_t*)(list ? list + 3 : nullptr), list, items, big, slot_words);
}

template <class Sink>
hipError_t launch_solve(const State& s, int pad, const Sink& out, uint32_t* list, bool window, uint64_t* big,
                        unsigned big_slots, hipStream_t stream) {
  const unsigned items = (unsigned)((size_t)s.B * s.N);
  // dynamic LDS of the full kernel / words of a scratch slot of the big kernel
  const size_t lds = big ? 0 : dijkstra_lds_bytes(s, pad);
  const size_t slot_words = big ? dijkstra_big_slot_bytes(s, pad) / 8 : 0;
  if (!window) {
    if (big)  // a fixed grid over every item: a slot per workgroup
      run_big(out, big_slots, stream, s, pad, nullptr, items, big, slot_words);
    else
      run_full(out, items, lds, stream, s, pad, nullptr);
    return hipGetLastError();
  }
  static const int depth = [] {  // MARLCOV_DJ_DEPTH: fewer exact layers (diagnostics, A/B)
    const char* v = getenv("MARLCOV_DJ_DEPTH");
    const int d = v ? atoi(v) : kDjWinDepth;
    return d >= 0 && d < kDjWinDepth ? d - d % 3 : kDjWinDepth;  // whole trips of 3 layers
  }();
  run_window(out, items, stream, s, pad, list, depth);
  if (big) {  // the listed items: the big kernel's fixed grid strides over the count
    run_big(out, big_slots, stream, s, pad, list, items, big, slot_words);
    return hipGetLastError();
  }
  // the listed items: a fixed grid (hipGraph capture) strides over the count
  static const unsigned full_grid = [] {  // MARLCOV_DJ_FULL_GRID: A/B of the fixed grid
    const char* v = getenv("MARLCOV_DJ_FULL_GRID");
    const int g = v ? atoi(v) : 0;
    return g > 0 && g <= 4096 ? (unsigned)g : kDjFullGrid;
  }();
  run_full(out, items < full_grid ? items : full_grid, lds, stream, s, pad, list);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_dijkstra(const State& s, int pad, int layer, int Lc, uint8_t* obs,
                           uint32_t* list, bool window, uint64_t* big, unsigned big_slots,
                           hipStream_t stream) {
  return launch_solve(s, pad, DjCropSink{layer, Lc, obs}, list, window, big, big_slots, stream);
}

// mc_frontier_actions: the same launches with the move sink, over the frontier
// call's own list (same layout); dist / goal may be null
hipError_t launch_frontier(const State& s, int pad, uint8_t* act, int32_t* dist, int32_t* goal,
                           uint32_t* list, bool window, uint64_t* big, unsigned big_slots,
                           hipStream_t stream) {
  return launch_solve(s, pad, DjMoveSink{act, dist, goal}, list, window, big, big_slots, stream);
}

// mc_frontier_setup: the full kernel's dynamic LDS past 64 KiB needs the
// attribute once (mc_capi.hip sets it on dijkstra_kernel at every step)
hipError_t frontier_allow_lds(size_t lds) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&frontier_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

}  // namespace mc
