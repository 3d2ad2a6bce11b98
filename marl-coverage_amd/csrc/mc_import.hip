// mc_import.hip — the kernel of mc_import_maps (include/marlcov.h), the inverse
// of mc_export.hip: dense uint8 planes [count][P][Wp][Lp] (robots, free0..,
// obst0..; nonzero = set) become the tiled bit maps, the union map, the two
// counters and the positions of chosen envs, in one launch.
//
// One workgroup per slot.  The kernel is load-bound (8 input bytes per output
// bit-row), so the work is laid out by the input: a lane takes tile t = ti *
// TC + tj, consecutive lanes consecutive tj, so the wave's loads of one cell
// row are one contiguous run of the plane (8 bytes per lane, at any alignment:
// a plane is Wp * Lp bytes, generally odd; mc_import.h).  For its tile a lane
// packs the N free words, stores them, ORs them into the union word and counts
// both, then packs and stores the N obstacle words; the counts are reduced
// over the workgroup and written to the env record.  The lanes wait on memory
// round trips, not on arithmetic, so a lane keeps two agents' tiles (16 loads)
// on their way together, and the robots scan four runs.  A map larger than
// the workgroup is walked in passes (one workgroup per slot also for a 1,075
// x 1,075 map: DESIGN.md §7).  Maps narrower than 8 cells, which have no
// whole 8-byte row, are a second instantiation that reads runs of Lp bytes.
//
// Checked before any store to the slot's env: dev_envs[k] outside [0, B), and
// with a robots plane a byte above N, a robot number absent or present twice,
// an env whose pool grid index is outside [0, G), a robot on a cell with grid
// < 0.  Such a slot leaves its env untouched and sets ERR_IMPORT; every other
// slot of the call is applied.  The entries of dev_envs must be distinct.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "mc_import.h"

namespace mc {

constexpr int kImportMaxThreads = 512;
constexpr int kImportScan = 4;  // 8-byte runs of the robots plane a lane loads together

// kWide: maps of 8 or more columns (mc_import.h)
template <bool kWide>
__device__ __forceinline__ uint64_t tile_word(const ImportBytes& bytes, int Wp, int Lp, int ti, int tj) {
  if constexpr (kWide) return import_tile_wide(bytes, Wp, Lp, ti, tj);
  else return import_tile_narrow(bytes, Wp, Lp, ti);
}

template <bool kWide>
__global__ __launch_bounds__(kImportMaxThreads) void import_kernel(State s, uint32_t layers, int P,
                                                                   uint32_t plane_bytes,
                                                                   const int32_t* __restrict__ dev_envs,
                                                                   const uint8_t* __restrict__ in) {
  __shared__ uint32_t sh_cnt[64], sh_cell[64];  // per robot: times seen, its cell (N <= 64: mc_create)
  __shared__ uint32_t sh_bad, sh_sum[2];
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const uint32_t k = blockIdx.x;
  const int e = dev_envs ? dev_envs[k] : (int)k;
  if (e < 0 || e >= s.B) {  // (uniform over the workgroup)
    if (tid == 0) atomicOr(s.err, (uint32_t)ERR_IMPORT);
    return;
  }
  const uint8_t* __restrict__ plane = in + (size_t)k * (size_t)P * plane_bytes;
  if (tid < 64) {
    sh_cnt[tid] = 0u;
    sh_cell[tid] = 0u;
  }
  if (tid == 0) {
    sh_bad = 0u;
    sh_sum[0] = 0u;
    sh_sum[1] = 0u;
  }
  __syncthreads();

  if (layers & 16u) {  // MC_MAP_ROBOTS: scan, validate, then store
    const int g = s.rec[e].env_grid;
    const ImportBytes rb{plane};
    const auto seen = [&](int i, uint32_t c) {
      atomicAdd(&sh_cnt[i], 1u);
      sh_cell[i] = c;
    };
    const uint32_t runs = plane_bytes >> 3, stride = (uint32_t)nt;  // whole 8-byte runs; a lane's step in runs
    bool ok = true;
    for (uint32_t i0 = (uint32_t)tid; i0 < runs; i0 += kImportScan * stride) {
      uint64_t v[kImportScan];  // kImportScan runs a lane, loaded together
#pragma unroll
      for (int j = 0; j < kImportScan; ++j) {
        const uint32_t i = i0 + (uint32_t)j * stride;
        v[j] = i < runs ? rb.load8(8u * i) : 0ull;
      }
#pragma unroll
      for (int j = 0; j < kImportScan; ++j) ok &= import_robots_run(v[j], 8u * (i0 + (uint32_t)j * stride), s.N, seen);
    }
    if (tid == 0 && (plane_bytes & 7u))  // the plane's last, short run
      ok &= import_robots_run(rb.load(8u * runs, (int)(plane_bytes & 7u)), 8u * runs, s.N, seen);
    if (!ok) sh_bad = 1u;
    __syncthreads();
    if (tid < s.N) {  // robot tid: seen once, on a cell of its env's grid that is not blocked
      bool valid = g >= 0 && g < s.G;
      if (valid) {
        const uint64_t* __restrict__ neg = s.grid_neg + (size_t)g * s.MT;
        valid = import_robot_valid(sh_cnt[tid], sh_cell[tid], s.Lp, s.TCS, [&](uint32_t i) { return neg[i]; });
      }
      if (!valid) sh_bad = 1u;
    }
    __syncthreads();
    if (sh_bad) {
      if (tid == 0) atomicOr(s.err, (uint32_t)ERR_IMPORT);
      return;
    }
    if (tid < s.N) {
      const uint32_t c = sh_cell[tid], x = c / (uint32_t)s.Lp;
      *reinterpret_cast<int2*>(s.pos + ((size_t)e * s.N + tid) * 2) = make_int2((int)x, (int)(c - x * (uint32_t)s.Lp));
    }
    plane += plane_bytes;
  }

  const bool has_free = (layers & 32u) != 0u, has_obst = (layers & 64u) != 0u;
  if (has_free || has_obst) {
    const uint8_t* __restrict__ fplane = plane;
    const uint8_t* __restrict__ oplane = plane + (has_free ? (size_t)s.N * plane_bytes : 0);
    const size_t mt = (size_t)s.MT;
    uint64_t* __restrict__ fm = s.freem + (size_t)e * s.N * mt;
    uint64_t* __restrict__ om = s.obstm + (size_t)e * s.N * mt;
    const int T = s.TR * s.TC;
    uint32_t fc = 0u, vc = 0u;
    for (int t = tid; t < T; t += nt) {
      const int ti = t / s.TC, tj = t - ti * s.TC;
      const uint32_t idx = tile_index(s.TCS, ti, tj);
      // two agents' tiles at a time: 16 loads on their way together
      if (has_free) {
        uint64_t u = 0ull;
        for (int a = 0; a < s.N; a += 2) {
          const int b = a + 1 < s.N ? a + 1 : a;  // (an odd N's last agent twice)
          const uint64_t w0 = tile_word<kWide>(ImportBytes{fplane + (size_t)a * plane_bytes}, s.Wp, s.Lp, ti, tj);
          const uint64_t w1 = tile_word<kWide>(ImportBytes{fplane + (size_t)b * plane_bytes}, s.Wp, s.Lp, ti, tj);
          fm[(size_t)a * mt + idx] = w0;
          fm[(size_t)b * mt + idx] = w1;
          u |= w0 | w1;
          fc += (uint32_t)__popcll(w0) + (b != a ? (uint32_t)__popcll(w1) : 0u);
        }
        s.vis[(size_t)e * mt + idx] = u;
        vc += (uint32_t)__popcll(u);
      }
      if (has_obst)
        for (int a = 0; a < s.N; a += 2) {
          const int b = a + 1 < s.N ? a + 1 : a;
          const uint64_t w0 = tile_word<kWide>(ImportBytes{oplane + (size_t)a * plane_bytes}, s.Wp, s.Lp, ti, tj);
          const uint64_t w1 = tile_word<kWide>(ImportBytes{oplane + (size_t)b * plane_bytes}, s.Wp, s.Lp, ti, tj);
          om[(size_t)a * mt + idx] = w0;
          om[(size_t)b * mt + idx] = w1;
        }
    }
    if (has_free) {  // FREE_COUNT / VISITED_COUNT: wave sums, then one LDS add per wave
      for (int d = 32; d >= 1; d >>= 1) {
        fc += __shfl_xor(fc, d, 64);
        vc += __shfl_xor(vc, d, 64);
      }
      if ((tid & 63) == 0) {
        atomicAdd(&sh_sum[0], fc);
        atomicAdd(&sh_sum[1], vc);
      }
      __syncthreads();
      if (tid == 0) {
        s.rec[e].free_cnt = sh_sum[0];
        s.rec[e].vis_cnt = sh_sum[1];
      }
    }
  }

  // dist_reward: max(d) of the env's maps is unknown and their top-cell caches are void
  if (tid < s.N) {
    if (s.dist_mw) *reinterpret_cast<int2*>(s.dist_mw + ((size_t)e * s.N + tid) * 2) = make_int2(-1, -1);
    if (s.dist_ch) {
      int4* h = reinterpret_cast<int4*>(s.dist_ch + ((size_t)e * s.N + tid) * 8);
      h[0] = make_int4(-1, -1, -1, -1);
      h[1] = make_int4(-1, -1, -1, -1);
    }
  }
}

hipError_t launch_import(const State& s, uint32_t layers, const int32_t* dev_envs, int count, const uint8_t* dev_in,
                         hipStream_t stream) {
  int P = 0;
  if (layers & 16u) P += 1;
  if (layers & 32u) P += s.N;
  if (layers & 64u) P += s.N;
  const uint64_t plane = (uint64_t)s.Wp * s.Lp;
  if (count < 1 || P < 1 || plane < 1) return hipSuccess;
  if (plane * (uint64_t)P >= 0x7FFFFFFFull) return hipErrorInvalidValue;
  int nt = (s.TR * s.TC + 63) & ~63;
  if (nt < 64) nt = 64;  // (at least N lanes: N <= 64)
  if (nt > kImportMaxThreads) nt = kImportMaxThreads;
  if (s.Lp >= 8)
    hipLaunchKernelGGL(import_kernel<true>, dim3((unsigned)count), dim3((unsigned)nt), 0, stream, s, layers, P,
                       (uint32_t)plane, dev_envs, dev_in);
  else
    hipLaunchKernelGGL(import_kernel<false>, dim3((unsigned)count), dim3((unsigned)nt), 0, stream, s, layers, P,
                       (uint32_t)plane, dev_envs, dev_in);
  return hipGetLastError();
}

}  // namespace mc
