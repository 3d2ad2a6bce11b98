// mc_fork.h — the per-env state gather behind mc_copy_envs / mc_sg_copy_envs
// (mc_fork.hip): the two C-ABI callers describe their handles' per-env arrays
// by one table and share one kernel.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mc {

constexpr int kForkMaxFields = 16;

// One per-env array of the two handles: env e's slice is the `bytes` bytes at
// base + e * bytes.  `width` is the access size the kernel uses for it (16,
// 8, 4 or 1): the largest that divides both bases and `bytes`.
struct ForkField {
  const char* src;
  char* dst;
  uint64_t bytes;
  uint32_t width;
  uint32_t pad_;
};

struct ForkTable {
  ForkField f[kForkMaxFields];
  int nf = 0;
  // add a field (null on either side: the handles have no such array)
  void add(const void* src, void* dst, size_t bytes) {
    if (!src || !dst || bytes == 0 || nf >= kForkMaxFields) return;
    const uintptr_t m = (uintptr_t)src | (uintptr_t)dst | (uintptr_t)bytes;
    const uint32_t w = (m & 15) == 0 ? 16u : (m & 7) == 0 ? 8u : (m & 3) == 0 ? 4u : 1u;
    f[nf++] = ForkField{static_cast<const char*>(src), static_cast<char*>(dst), (uint64_t)bytes, w, 0u};
  }
  size_t bytes_per_env() const {
    size_t t = 0;
    for (int i = 0; i < nf; ++i) t += f[i].bytes;
    return t;
  }
};

// Env e of the destination (dst_envs of them) takes the table's slices of env
// dev_src[e] of the source (src_envs); `same`: one handle is both.  An index
// outside [-1, src_envs), or within one handle a source env that the call
// also overwrites, leaves env e untouched and ORs `err_bit` (the handle
// type's ERR_FORK) into *err.  One launch.
hipError_t launch_fork(const ForkTable& t, const int32_t* dev_src, int src_envs, int dst_envs, bool same,
                       uint32_t* err, uint32_t err_bit, hipStream_t stream);

}  // namespace mc
