// mc_fork.hip — fork / restore env state on the device: the gather kernel of
// mc_copy_envs and mc_sg_copy_envs (include/marlcov.h).
//
// Env e of the destination handle takes every per-env array slice of env
// dev_src[e] of the source handle (-1: env e stays as it is).  The callers
// (mc_capi.hip, mc_super.hip) list their handles' arrays in a ForkTable
// (mc_fork.h), passed by value; the kernel knows nothing of either env type.
//
// Launch: `chunks` workgroups of kForkThreads lanes per destination env,
// workgroup w serving env w / chunks.  Every workgroup of an env reads the
// same index and makes the same checks, so the "-1" and the error exits are
// uniform over them; chunk 0 reports the error.  The checks come before any
// load through the index:
//   - the index is in [-1, src_envs);
//   - within one handle, a source env s named by another env keeps itself
//     (dev_src[s] is -1 or s), so the call reads only envs it does not write
//     and needs no ordering between its workgroups.
// A field is moved with its table width (16-, 8-, 4- or 1-byte accesses),
// lane-contiguous, kForkUnroll loads in flight per lane before the stores.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "mc_fork.h"

namespace mc {

constexpr int kForkThreads = 256;
constexpr int kForkUnroll = 4;

template <class T>
__device__ __forceinline__ void fork_copy(const char* __restrict__ src, char* __restrict__ dst, uint64_t bytes,
                                          uint32_t first, uint32_t stride) {
  const T* __restrict__ s = reinterpret_cast<const T*>(src);
  T* __restrict__ d = reinterpret_cast<T*>(dst);
  const uint64_t units = bytes / sizeof(T);
  // (a load past the slice's end re-reads unit i instead, so a round's loads
  // are issued together and unconditionally; only the stores are predicated)
  for (uint64_t i = first; i < units; i += (uint64_t)kForkUnroll * stride) {
    T v[kForkUnroll];
#pragma unroll
    for (int k = 0; k < kForkUnroll; ++k) {
      const uint64_t j = i + (uint64_t)k * stride;
      v[k] = s[j < units ? j : i];
    }
#pragma unroll
    for (int k = 0; k < kForkUnroll; ++k) {
      const uint64_t j = i + (uint64_t)k * stride;
      if (j < units) d[j] = v[k];
    }
  }
}

__global__ __launch_bounds__(kForkThreads) void fork_kernel(ForkTable t, const int32_t* __restrict__ dev_src,
                                                            int src_envs, int dst_envs, int same, uint32_t chunks,
                                                            uint32_t* err, uint32_t err_bit) {
  const uint32_t e = blockIdx.x / chunks, c = blockIdx.x - e * chunks;
  if (e >= (uint32_t)dst_envs) return;
  const int sidx = dev_src[e];
  if (sidx == -1 || (same && sidx == (int)e)) return;
  bool bad = sidx < -1 || sidx >= src_envs;
  if (!bad && same) {  // (src_envs == dst_envs: dev_src[sidx] is in bounds)
    const int keep = dev_src[sidx];
    bad = keep != -1 && keep != sidx;
  }
  if (bad) {
    if (c == 0 && threadIdx.x == 0) atomicOr(err, err_bit);
    return;
  }
  const uint32_t first = c * kForkThreads + threadIdx.x, stride = chunks * kForkThreads;
  for (int k = 0; k < t.nf; ++k) {
    const ForkField f = t.f[k];
    const char* src = f.src + (uint64_t)sidx * f.bytes;
    char* dst = f.dst + (uint64_t)e * f.bytes;
    if (f.width == 16) fork_copy<uint4>(src, dst, f.bytes, first, stride);
    else if (f.width == 8) fork_copy<uint2>(src, dst, f.bytes, first, stride);
    else if (f.width == 4) fork_copy<uint32_t>(src, dst, f.bytes, first, stride);
    else fork_copy<uint8_t>(src, dst, f.bytes, first, stride);
  }
}

hipError_t launch_fork(const ForkTable& t, const int32_t* dev_src, int src_envs, int dst_envs, bool same,
                       uint32_t* err, uint32_t err_bit, hipStream_t stream) {
  if (dst_envs < 1 || t.nf < 1) return hipSuccess;
  // workgroups per env: enough to fill the device at small batches (about
  // 2048 workgroups), but at least 4 KiB of state each and at most 64
  const size_t per_env = t.bytes_per_env();
  size_t chunks = (2048 + (size_t)dst_envs - 1) / (size_t)dst_envs;
  const size_t by_bytes = (per_env + 4095) / 4096;
  if (chunks > by_bytes) chunks = by_bytes;
  if (chunks > 64) chunks = 64;
  if (chunks < 1) chunks = 1;
  const size_t blocks = (size_t)dst_envs * chunks;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fork_kernel, dim3((unsigned)blocks), dim3(kForkThreads), 0, stream, t, dev_src, src_envs,
                     dst_envs, same ? 1 : 0, (uint32_t)chunks, err, err_bit);
  return hipGetLastError();
}

}  // namespace mc
