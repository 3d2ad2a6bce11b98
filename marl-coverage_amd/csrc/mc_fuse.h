// mc_fuse.h — the chunks of a fused mc_step_many call (mc_capi.hip): K steps
// run as ceil(K / S) env-kernel launches of at most S steps each, S from
// MARLCOV_FUSE_STEPS.  Host arithmetic only (tests/native/fuse_chunks_check.cpp
// runs it under sanitizers).  Not part of the public ABI.  mc_sg_step_many
// (mc_super.hip) chunks its step-kernel launches with the same arithmetic: its
// quotients take the FUSE_OBS slot, and FUSE_ADJ stays at stride 0.
#pragma once
#include <stdint.h>

namespace mc {

constexpr int kFuseStepsDefault = 64, kFuseStepsMax = 1024;

// the five per-step buffers of mc_step_many, in this order everywhere
enum { FUSE_ACTIONS = 0, FUSE_REWARD, FUSE_DONE, FUSE_OBS, FUSE_ADJ, FUSE_BUFS };

// MARLCOV_FUSE_STEPS as given (null: unset) -> steps per launch, 1..kFuseStepsMax
// (0 and 1: one launch per step)
inline int fuse_steps_from_env(const char* v) {
  if (!v || !*v) return kFuseStepsDefault;
  long n = 0;
  for (const char* p = v; *p >= '0' && *p <= '9' && n <= kFuseStepsMax; ++p) n = n * 10 + (*p - '0');
  return n < 1 ? 1 : (n > kFuseStepsMax ? kFuseStepsMax : (int)n);
}

inline int64_t fuse_chunk_count(int64_t K, int S) { return K <= 0 ? 0 : (K + S - 1) / S; }

struct FuseChunk {
  int64_t first;           // the chunk's first step
  int32_t count;           // its steps, 1..S
  int64_t off[FUSE_BUFS];  // first * stride: byte offset of step `first` in each buffer
};

// every k * stride of a call of K steps fits int64 (strides >= 0): tested on
// the largest, (K - 1) * stride, before anything is enqueued
inline bool fuse_offsets_fit(int64_t K, const int64_t (&stride)[FUSE_BUFS]) {
  if (K <= 1) return true;
  for (int b = 0; b < FUSE_BUFS; ++b)
    if (stride[b] < 0 || (stride[b] > 0 && K - 1 > INT64_MAX / stride[b])) return false;
  return true;
}

// chunk i (0 <= i < fuse_chunk_count(K, S)) of K steps at S per launch; false
// (nothing written) for an index outside the call or an offset past int64
inline bool fuse_chunk(int64_t K, int S, int64_t i, const int64_t (&stride)[FUSE_BUFS], FuseChunk* c) {
  if (S < 1 || i < 0 || i >= fuse_chunk_count(K, S) || !fuse_offsets_fit(K, stride)) return false;
  c->first = i * S;  // < K
  const int64_t left = K - c->first;
  c->count = (int32_t)(left < S ? left : S);
  for (int b = 0; b < FUSE_BUFS; ++b) c->off[b] = c->first * stride[b];
  return true;
}

// The step whose action row step k of a launch of num_steps steps (0 <= k <
// num_steps) prefetches while it runs (the env kernel's carried head,
// mc_env_step.h): the next one, and at the launch's last step its own row
// again -- the caller's buffer may end with the launch's last row, so no
// address past it is formed.  The kernel adds (this - k) * stride to step k's
// row.  (constexpr: host and device alike)
constexpr int fuse_prefetch_step(int k, int num_steps) { return (int64_t)k + 1 < num_steps ? k + 1 : k; }

// The cell (x | y << 16) the carried head predicts for a robot after the next
// step, from its cell before it, its action byte and whether the byte's target
// cell is blocked (out of bounds, or grid < 0): moves_front's rule for one
// robot alone.  Other robots are not looked at: a robot held back by one, or
// let through by one that left, is a misprediction, which the step that uses
// the prefetched visibility record finds by comparing with the cell the moves
// gave, and then loads the record as a step without the prefetch does.
constexpr uint32_t fuse_target_cell(uint32_t xy, uint32_t act) {
  return (uint32_t)((int)(xy & 0xFFFFu) + ((act == 0) - (act == 2))) |
         ((uint32_t)((int)(xy >> 16) + ((act == 1) - (act == 3))) << 16);
}
constexpr uint32_t fuse_predict_cell(uint32_t xy, uint32_t act, bool blocked) {
  return (act <= 3 && !blocked) ? fuse_target_cell(xy, act) : xy;
}

}  // namespace mc
