// Host check of the fused loop's action prefetch (csrc/mc_fuse.h
// fuse_prefetch_step), built host-only with AddressSanitizer and UBSan by
// tests/test_fuse_prefetch_host.py.  A call of K steps at S per launch is
// walked chunk by chunk the way mc_step_many launches it, over a heap buffer
// of exactly K action rows: in every step of every launch the prefetched row
// is read through the kernel's own address expression, so a row past the
// launch's last step (or past the buffer) is an ASan report.  The prefetched
// step must be the next one, and the launch's last step its own.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mc_fuse.h"

using namespace mc;

static int fails = 0;
#define EXPECT(c)                                              \
  do {                                                         \
    if (!(c)) {                                                \
      printf("FAIL line %d: %s\n", __LINE__, #c);              \
      ++fails;                                                 \
    }                                                          \
  } while (0)

// row: bytes of one step's actions; stride: bytes between two steps' rows (>= row, or 0: every step reads one row)
static void walk(int64_t K, int S, int64_t row, int64_t stride) {
  const int64_t st[FUSE_BUFS] = {stride, 0, 0, 0, 0};
  // exactly the caller's bytes: K - 1 strides and one row (heap: ASan guards both ends)
  std::vector<uint8_t> buf((size_t)(K > 0 ? (K - 1) * stride + row : 0));
  for (int64_t k = 0; k < K; ++k)
    for (int64_t i = 0; i < row; ++i) buf[(size_t)(k * stride + i)] = (uint8_t)(stride ? k : 0);
  int64_t reads = 0;
  for (int64_t c = 0; c < fuse_chunk_count(K, S); ++c) {
    FuseChunk ch;
    EXPECT(fuse_chunk(K, S, c, st, &ch));
    const uint8_t* actions = buf.data() + ch.off[FUSE_ACTIONS];  // the launch's io.actions
    const int num_steps = ch.count;
    for (int k = 0; k < num_steps; ++k) {
      const uint8_t* cur = actions + (int64_t)k * stride;  // io_at_step
      const int p = fuse_prefetch_step(k, num_steps);
      EXPECT(p == (k == num_steps - 1 ? k : k + 1));
      EXPECT(p >= 0 && p < num_steps);
      const uint8_t* an = cur + (int64_t)(p - k) * stride;  // the kernel's expression
      EXPECT(an >= buf.data() && an + row <= buf.data() + buf.size());
      if (an + row <= buf.data() + buf.size()) {
        EXPECT(an[0] == (uint8_t)(stride ? ch.first + p : 0));  // the row of the launch's step p
        EXPECT(an[row - 1] == an[0]);
        ++reads;
      }
    }
  }
  EXPECT(reads == K);
  printf("K %lld S %d stride %lld: %lld prefetches inside the buffer\n", (long long)K, S, (long long)stride,
         (long long)reads);
}

int main() {
  for (int S : {1, 2, 3, 64})
    for (int64_t K : {1, 2, 3, 7, 63, 64, 65, 200}) {
      walk(K, S, 8, 8);    // rows back to back: the buffer ends with the last row
      walk(K, S, 8, 24);   // padded rows: the buffer still ends with the last row
      walk(K, S, 8, 0);    // stride 0: one row for every step
    }
  walk(0, 64, 8, 8);
  // the ends of the domain
  EXPECT(fuse_prefetch_step(0, 1) == 0);
  EXPECT(fuse_prefetch_step(0, 2) == 1);
  EXPECT(fuse_prefetch_step(1, 2) == 1);
  EXPECT(fuse_prefetch_step(kFuseStepsMax - 2, kFuseStepsMax) == kFuseStepsMax - 1);
  EXPECT(fuse_prefetch_step(kFuseStepsMax - 1, kFuseStepsMax) == kFuseStepsMax - 1);
  EXPECT(fuse_prefetch_step(INT32_MAX - 1, INT32_MAX) == INT32_MAX - 1);  // no int overflow in k + 1
  static_assert(fuse_prefetch_step(5, 6) == 5 && fuse_prefetch_step(4, 6) == 5, "usable at compile time");
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
