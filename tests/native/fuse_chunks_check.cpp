// Host check of the fused mc_step_many chunk arithmetic (csrc/mc_fuse.h),
// built host-only with AddressSanitizer and UBSan by
// tests/test_fuse_chunks_host.py.  For every case the chunks must tile
// 0 .. K-1 in order with at most S steps each, and every offset must equal
// first * stride; an overflowing k * stride must be refused.
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

static void tiles(int64_t K, int S, const int64_t (&st)[FUSE_BUFS]) {
  const int64_t n = fuse_chunk_count(K, S);
  EXPECT(n == (K + S - 1) / S);
  std::vector<FuseChunk> cs((size_t)n);  // heap: an index past the end is an ASan report
  int64_t next = 0;
  for (int64_t i = 0; i < n; ++i) {
    EXPECT(fuse_chunk(K, S, i, st, &cs[(size_t)i]));
    const FuseChunk& c = cs[(size_t)i];
    EXPECT(c.first == next);
    EXPECT(c.count >= 1 && c.count <= S);
    EXPECT(i == n - 1 || c.count == S);
    for (int b = 0; b < FUSE_BUFS; ++b) EXPECT(c.off[b] == c.first * st[b]);
    next += c.count;
  }
  EXPECT(next == K);
  FuseChunk x;
  x.count = -7;
  EXPECT(!fuse_chunk(K, S, n, st, &x) && x.count == -7);   // past the last chunk: refused, nothing written
  EXPECT(!fuse_chunk(K, S, -1, st, &x) && x.count == -7);
  printf("K %lld S %d -> %lld launches\n", (long long)K, S, (long long)n);
}

int main() {
  const int64_t zero[FUSE_BUFS] = {0, 0, 0, 0, 0};
  const int64_t some[FUSE_BUFS] = {20, 40, 5, 1500, 80};
  const int64_t mixed[FUSE_BUFS] = {16, 0, 0, 300, 0};
  const int S = 64;
  for (int64_t K : {0, 1, S - 1, S, S + 1, 200}) {
    tiles(K, S, zero);
    tiles(K, S, some);
    tiles(K, S, mixed);
  }
  tiles(40, 16, some);
  tiles(40, 1, some);   // S = 1: one launch per step
  tiles(1, 1, zero);
  tiles(3000, kFuseStepsMax, some);
  EXPECT(fuse_chunk_count(200, 64) == 4);
  EXPECT(fuse_chunk_count(40, 16) == 3);
  EXPECT(fuse_chunk_count(40, 1) == 40);
  EXPECT(fuse_chunk_count(0, 64) == 0);

  // an overflowing k * stride: refused for every chunk, nothing written
  const int64_t huge[FUSE_BUFS] = {4, 8, 1, INT64_MAX / 100, 0};
  EXPECT(fuse_offsets_fit(101, huge));   // 100 * (INT64_MAX / 100) fits
  EXPECT(!fuse_offsets_fit(102, huge));  // 101 * ... does not
  FuseChunk x;
  x.first = -3;
  EXPECT(fuse_chunk(101, S, 1, huge, &x) && x.off[FUSE_OBS] == 64 * (INT64_MAX / 100));
  x.first = -3;
  EXPECT(!fuse_chunk(102, S, 0, huge, &x) && x.first == -3);
  EXPECT(!fuse_chunk(102, S, 1, huge, &x) && x.first == -3);
  const int64_t neg[FUSE_BUFS] = {4, -8, 1, 0, 0};
  EXPECT(!fuse_offsets_fit(2, neg));
  EXPECT(fuse_offsets_fit(INT32_MAX, some));
  const int64_t top[FUSE_BUFS] = {INT64_MAX, 0, 0, 0, 0};
  EXPECT(fuse_offsets_fit(2, top) && !fuse_offsets_fit(3, top));

  // the knob: default 64, clamped to 1 .. 1024, 0 and 1 mean one launch per step
  EXPECT(fuse_steps_from_env(nullptr) == 64);
  EXPECT(fuse_steps_from_env("") == 64);
  EXPECT(fuse_steps_from_env("0") == 1);
  EXPECT(fuse_steps_from_env("1") == 1);
  EXPECT(fuse_steps_from_env("16") == 16);
  EXPECT(fuse_steps_from_env("1024") == 1024);
  EXPECT(fuse_steps_from_env("1025") == 1024);
  EXPECT(fuse_steps_from_env("99999999999999999999999") == 1024);
  EXPECT(fuse_steps_from_env("-5") == 1);
  EXPECT(fuse_steps_from_env("x") == 1);
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
