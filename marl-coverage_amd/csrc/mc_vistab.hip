// mc_vistab.hip — builds the lidar's visibility table (mc_vistab.h): one
// record per (pool grid, cell), whenever the pool or the beam table changes.
//
// A thread marches one cell's beams (vis_record, the code the host check
// runs) into its own row of an LDS staging area -- the record's words are
// indexed by the ray's row, which registers cannot be -- and the workgroup
// then writes its kVisBlock records, consecutive in the table, as whole
// 16-byte quads (coalesced: one record per 8 lanes).
#include "mc_vistab.h"

namespace mc {

constexpr int kVisBlock = 256;                  // records (threads) per workgroup round
constexpr int kVisStage = kVisRecWords + 1;     // odd row stride: the threads' rows fall on different banks

__global__ __launch_bounds__(kVisBlock) void vis_build_kernel(State s, uint32_t* __restrict__ table, uint32_t total) {
  __shared__ uint32_t stage[kVisBlock * kVisStage];
  const uint32_t cells = (uint32_t)s.Wp * (uint32_t)s.Lp;
  for (uint32_t i0 = blockIdx.x * kVisBlock; i0 < total; i0 += gridDim.x * kVisBlock) {  // uniform trip count
    const uint32_t i = i0 + threadIdx.x;
    if (i < total) {
      const uint32_t g = i / cells, c = i - g * cells;
      const int x = (int)(c / (uint32_t)s.Lp), y = (int)(c - (uint32_t)x * (uint32_t)s.Lp);
      vis_record(s.grid_neg + (size_t)g * s.MT, s.TCS, s.Wp, s.Lp, s.H, s.beams, s.nbeams, s.beam_bits, s.bcmax,
                 s.beam_common, s.beam_k1, x, y, stage + threadIdx.x * kVisStage);
    }
    __syncthreads();
    // quad q of the round: record q / 8, words 4 (q % 8) ..
    for (uint32_t q = threadIdx.x; q < kVisBlock * (kVisRecWords / 4); q += kVisBlock) {
      const uint32_t r = q >> 3, w = (q & 7u) * 4;
      if (i0 + r < total) {
        const uint32_t* src = stage + r * kVisStage + w;
        *reinterpret_cast<uint4*>(table + (size_t)(i0 + r) * kVisRecWords + w) = make_uint4(src[0], src[1], src[2], src[3]);
      }
    }
    __syncthreads();
  }
}

hipError_t launch_vis_build(const State& s, uint32_t* table, hipStream_t stream) {
  const uint64_t total = (uint64_t)s.G * s.Wp * s.Lp;  // (the caller keeps it below 2^32)
  const uint64_t rounds = (total + kVisBlock - 1) / kVisBlock;
  const unsigned blocks = (unsigned)(rounds < (1u << 20) ? rounds : (1u << 20));
  hipLaunchKernelGGL(vis_build_kernel, dim3(blocks), dim3(kVisBlock), 0, stream, s, table, (uint32_t)total);
  return hipGetLastError();
}

}  // namespace mc
