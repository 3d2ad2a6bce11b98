// mc_vistab.hip — builds the lidar's visibility table (mc_vistab.h): one
// record per (pool grid, cell), whenever the pool or the beam table changes.
//
// A thread marches one cell's beams (vis_record, the code the host check
// runs) into its own row of an LDS staging area -- the record's words are
// indexed by the ray's row, which registers cannot be -- converts those rows
// into the record's tiles (vis_tiles, likewise indexed by the row) in a second
// staging area, and the workgroup then writes its kVisBlock records,
// consecutive in the table, as whole 16-byte quads (coalesced: one 128-byte
// line per 8 lanes).
#include "mc_vistab.h"

namespace mc {

constexpr int kVisBlock = kVisSplit ? 64 : 128;  // records (threads) per workgroup round: both stages within 64 KB
constexpr int kVisStage = kVisRecWords + 1;      // odd row stride: the threads' rows fall on different banks
constexpr int kVisTileStage = kVisRecWords + 2;  // words between the threads' tiles (8-byte aligned; 2 mod 4 banks)

__global__ __launch_bounds__(kVisBlock) void vis_build_kernel(State s, uint32_t* __restrict__ table, uint32_t total) {
  __shared__ uint32_t stage[kVisBlock * kVisStage];
  __shared__ uint64_t tiles[kVisBlock * kVisTileStage / 2];
  const uint32_t cells = (uint32_t)s.Wp * (uint32_t)s.Lp;
  for (uint32_t i0 = blockIdx.x * kVisBlock; i0 < total; i0 += gridDim.x * kVisBlock) {  // uniform trip count
    const uint32_t i = i0 + threadIdx.x;
    if (i < total) {
      const uint32_t g = i / cells, c = i - g * cells;
      const int x = (int)(c / (uint32_t)s.Lp), y = (int)(c - (uint32_t)x * (uint32_t)s.Lp);
      const uint64_t* neg = s.grid_neg + (size_t)g * s.MT;
      uint32_t* rows = stage + threadIdx.x * kVisStage;
      vis_record(neg, s.TCS, s.Wp, s.Lp, s.H, s.beams, s.nbeams, s.beam_bits, s.bcmax, s.beam_common, s.beam_k1, x, y,
                 rows);
      vis_tiles(rows, neg, s.TCS, s.Wp, s.Lp, s.H, x, y, tiles + threadIdx.x * (kVisTileStage / 2));
    }
    __syncthreads();
    // quad q of the round: record q / (kVisRecWords / 4), its words 4 (q % ..) ..
    constexpr uint32_t QR = kVisRecWords / 4;
    const uint32_t* tw = reinterpret_cast<const uint32_t*>(tiles);
    for (uint32_t q = threadIdx.x; q < kVisBlock * QR; q += kVisBlock) {
      const uint32_t r = q / QR, w = (q % QR) * 4;
      if (i0 + r < total) {
        const uint32_t* src = tw + r * kVisTileStage + w;
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
