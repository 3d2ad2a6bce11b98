// mc_export.hip — the kernel of mc_export_maps (include/marlcov.h): the tiled
// bit maps of chosen envs as dense uint8 planes (scale 1) or as one count per
// 8x8 tile (scale 8), uint8 [count][P][rows][cols], in one launch.
//
// The kernel is store-bound (8 output bytes per input bit-word row), so the
// work is laid out by the output.  All slots' planes are one flat byte array;
// lane l of the grid makes the 16-byte-aligned chunk l of it and writes it
// with one 16-byte store, consecutive lanes taking consecutive chunks (1 KiB
// per wave store, whatever alignment a plane or slot starts at: Wp * Lp is
// generally no multiple of 16).  A chunk that runs over a plane or slot end is
// put together from the pieces of both sides (mc_export.h).  Narrower (byte)
// stores are used only for the tail of the whole array and next to a slot
// that is skipped for a bad index.  A workgroup's 4 KiB span lies in one slot
// or two and reads a few dozen tile words, which the lanes of a wave share
// (five words per dense chunk, loaded together; the same ones in neighbouring
// lanes), so the words come from the L1 / L2, not once per lane from HBM.
//
// Checked before any load through the index: dev_envs[k] outside [0, B) (or,
// when a grid plane is asked for, an env whose pool grid index is outside
// [0, G)) leaves slot k untouched and sets ERR_EXPORT; the lane that holds the
// slot's first byte reports it.
// Reads state only.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "mc_export.h"

namespace mc {

constexpr int kExportThreads = 256;

// tile word i of a plane's map: the OR of n maps `stride` words apart
struct ExportWords {
  const uint64_t* p;
  int n;
  uint32_t stride;
  __device__ __forceinline__ uint64_t operator()(uint32_t i) const {
    uint64_t w = p[i];
    for (int a = 1; a < n; ++a) w |= p[(size_t)a * stride + i];
    return w;
  }
};

// export_load of the accessor.  The kernel waits on memory round trips, not on
// arithmetic, so the K words of U maps are loaded together: the OR over N
// agents costs ceil(N / U) round trips, not K * N (a map past the last is
// replaced by the group's first: OR-ing it again changes nothing).
template <int K>
__device__ __forceinline__ void export_load(const ExportWords& word, const uint32_t (&idx)[K], uint64_t (&w)[K]) {
  if (word.n == 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = word.p[idx[k]];
    return;
  }
  constexpr int U = K <= 5 ? 4 : 2;
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = 0ull;
  for (int a = 0; a < word.n; a += U) {
    uint64_t t[U][K];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t* __restrict__ q = word.p + (size_t)(a + u < word.n ? a + u : a) * word.stride;
#pragma unroll
      for (int k = 0; k < K; ++k) t[u][k] = q[idx[k]];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < K; ++k) w[k] |= t[u][k];
  }
}

// plane_bytes: bytes of one plane (Wp * Lp, or TR * TC pooled); slot_bytes = P
// * plane_bytes (< 2^31: launch_export); total = count * slot_bytes.  The two
// scales are two kernels: the pooled decode holds more words in registers.
template <bool pooled>
__global__ __launch_bounds__(kExportThreads) void export_kernel(State s, uint32_t layers, int P,
                                                                uint32_t plane_bytes, uint32_t slot_bytes,
                                                                uint64_t total, const int32_t* __restrict__ dev_envs,
                                                                uint8_t* __restrict__ out) {
  // the workgroup's first chunk: slot and offset in it (uniform), then the lane's
  const uint64_t f0 = (uint64_t)blockIdx.x * (kExportThreads * 16);
  const uint64_t k0 = f0 / slot_bytes;
  const uint64_t f = f0 + (uint64_t)threadIdx.x * 16;
  if (f >= total) return;
  const uint64_t t = (f0 - k0 * slot_bytes) + (uint64_t)threadIdx.x * 16;  // < 2^31 + 4096
  const uint32_t dk = (uint32_t)t / slot_bytes;
  uint64_t k = k0 + dk;
  const uint32_t r = (uint32_t)t - dk * slot_bytes;
  int p = (int)(r / plane_bytes);
  uint32_t o = r - (uint32_t)p * plane_bytes;
  const int nvalid = total - f < 16 ? (int)(total - f) : 16;

  uint64_t lo = 0ull, hi = 0ull;
  uint32_t keep = 0u;  // bit j: byte j of the chunk is written
  int filled = 0;
  while (filled < nvalid) {
    const int e = dev_envs ? dev_envs[k] : (int)k;
    bool bad = e < 0 || e >= s.B;
    int g = 0;
    if (!bad && (layers & 3u)) {  // the grid planes: the env's pool grid
      g = s.rec[e].env_grid;
      bad = g < 0 || g >= s.G;
    }
    int n = nvalid - filled;
    if ((uint32_t)n > plane_bytes - o) n = (int)(plane_bytes - o);
    if (bad) {
      if (p == 0 && o == 0u) atomicOr(s.err, (uint32_t)ERR_EXPORT);
    } else {
      int kind, agent;
      export_plane_kind(layers, s.N, p, kind, agent);
      uint64_t v[2];
      if (kind == 4) {  // MC_MAP_ROBOTS
        export_robots_chunk16(s.pos + (size_t)e * s.N * 2, s.N, pooled ? s.TC : s.Lp, pooled ? 3 : 0, o, v);
      } else {
        const size_t mt = (size_t)s.MT;
        ExportWords w{nullptr, 1, (uint32_t)s.MT};
        if (kind == 0) w.p = s.grid_neg + (size_t)g * mt;
        else if (kind == 1) w.p = s.grid_pos + (size_t)g * mt;
        else if (kind == 2) w.p = s.vis + (size_t)e * mt;
        else if (kind == 3) {  // MC_MAP_OBST_ANY
          w.p = s.obstm + (size_t)e * s.N * mt;
          w.n = s.N;
        } else if (kind == 5) w.p = s.freem + ((size_t)e * s.N + agent) * mt;
        else w.p = s.obstm + ((size_t)e * s.N + agent) * mt;
        if (pooled) export_pooled_chunk16(w, s.TCS, s.Wp, s.Lp, o, v);
        else export_chunk16(w, s.TCS, s.Wp, s.Lp, o, v);
      }
      export_put(lo, hi, filled, v[0], v[1], n);
      keep |= ((1u << n) - 1u) << filled;
    }
    filled += n;
    o += (uint32_t)n;
    if (o == plane_bytes) {
      o = 0u;
      if (++p == P) {
        p = 0;
        ++k;
      }
    }
  }
  if (keep == 0xFFFFu) {
    *reinterpret_cast<uint4*>(out + f) =
        make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
  } else {
    for (int j = 0; j < 16; ++j)
      if ((keep >> j) & 1u) out[f + j] = (uint8_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xFFull);
  }
}

hipError_t launch_export(const State& s, uint32_t layers, int scale, const int32_t* dev_envs, int count,
                         uint8_t* dev_out, hipStream_t stream) {
  const int P = export_planes(layers, s.N);
  const uint64_t plane = scale == 8 ? (uint64_t)s.TR * s.TC : (uint64_t)s.Wp * s.Lp;
  const uint64_t slot = plane * (uint64_t)P;
  if (count < 1 || P < 1 || plane < 1) return hipSuccess;
  if (slot >= 0x7FFFFFFFull) return hipErrorInvalidValue;
  const uint64_t total = slot * (uint64_t)count;
  const uint64_t blocks = (total + kExportThreads * 16 - 1) / (kExportThreads * 16);
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (scale == 8)
    hipLaunchKernelGGL(export_kernel<true>, dim3((unsigned)blocks), dim3(kExportThreads), 0, stream, s, layers, P,
                       (uint32_t)plane, (uint32_t)slot, total, dev_envs, dev_out);
  else
    hipLaunchKernelGGL(export_kernel<false>, dim3((unsigned)blocks), dim3(kExportThreads), 0, stream, s, layers, P,
                       (uint32_t)plane, (uint32_t)slot, total, dev_envs, dev_out);
  return hipGetLastError();
}

}  // namespace mc
