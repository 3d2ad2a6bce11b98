// Stand-alone check of the host-built ray programs (csrc/mc_internal.h
// build_ray_prog), for a host-only build with sanitizers
// (tests/test_ray_program_host.py builds and runs it; no HIP call).
//
// Input (a text file): per case one line "N lpe rpl km rowbytes nbeams", then
// per beam "K axis sign msign bits".  For every lane, ray and step the
// program's offset must equal a direct replay of the march's chain
// (mc_env_step.h ray_init / ray_advance), fit int16, and the ray's K and
// agent must be the mapping's (K = -1 for rays past N * nbeams).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mc_beams.h"

static int fails = 0;
#define CHECK(c, ...)                 \
  do {                                \
    if (!(c)) {                       \
      if (++fails <= 20) {            \
        std::printf("FAIL " __VA_ARGS__); \
        std::printf("\n");            \
      }                               \
    }                                 \
  } while (0)

static void check_case(int N, int lpe, int rpl, int km, int rowbytes, const std::vector<mc::Beam>& bt) {
  const int nb = (int)bt.size(), total = N * nb;
  std::vector<uint32_t> prog;
  const bool ok = mc::build_ray_prog(bt, N, lpe, rpl, km, rowbytes, prog);
  CHECK(ok, "build_ray_prog refused N=%d lpe=%d rpl=%d km=%d nb=%d", N, lpe, rpl, km, nb);
  if (!ok) return;
  const int rw = mc::ray_prog_row_words(rpl, km);
  CHECK(rw % 4 == 0 && 2 * (rw - 1) >= rpl * km, "row words %d", rw);
  CHECK(prog.size() == (size_t)lpe * rw, "size %zu != %d rows of %d", prog.size(), lpe, rw);
  const int RB = (rowbytes == 4 ? (N | 1) : 1) * rowbytes * 64;  // one window row in P units
  for (int sub = 0; sub < lpe; ++sub) {
    std::vector<uint32_t> row((size_t)rw);  // the lane's words, stored by quads across the lanes
    for (int w = 0; w < rw; ++w) row[w] = prog[mc::ray_prog_word(lpe, sub, w)];
    for (int j = 0; j < rpl; ++j) {
      const int idx = sub * rpl + j;
      const uint32_t mb = (row[rw - 1] >> (8 * j)) & 0xFFu;
      const int K = (int)(mb & 31u) - 1, a = (int)(mb >> 5);
      if (idx >= total) {
        CHECK(K == -1, "lane %d ray %d: dead ray has K %d", sub, j, K);
        continue;
      }
      const mc::Beam& bm = bt[idx % nb];
      CHECK(K == bm.K && a == idx / nb, "lane %d ray %d: K %d a %d, want %d %d", sub, j, K, a, bm.K, idx / nb);
      // the march's own chain from an arbitrary start cell
      const bool ax = (bm.axis & 1) == 0;
      const uint32_t d0 = (uint32_t)(ax ? bm.sign * RB : bm.sign);
      const uint32_t d1 = (uint32_t)(ax ? bm.msign : bm.msign * RB);
      const uint32_t P0 = (0x2345u << 6) | 17u;
      uint32_t P = P0;
      for (int k = 1; k <= km; ++k) {
        P += d0 + ((0u - ((bm.bits >> (k - 1)) & 1u)) & d1);  // ray_advance(R, k - 1)
        const int i = j * km + k - 1;
        const int32_t T = (int32_t)(int16_t)(uint16_t)(row[i >> 1] >> (16 * (i & 1)));
        const int32_t want = (int32_t)(P - P0);
        CHECK(want >= -32768 && want <= 32767, "lane %d ray %d step %d: offset %d beyond int16", sub, j, k, want);
        CHECK(T == want, "lane %d ray %d step %d: T %d, replay %d", sub, j, k, T, want);
        CHECK(P0 + (uint32_t)T == P, "lane %d ray %d step %d: P0 + T != P", sub, j, k);
      }
    }
    // the padding between the offsets and the meta word is zero
    for (int w = (rpl * km + 1) / 2; w < rw - 1; ++w) CHECK(row[w] == 0u, "lane %d pad word %d", sub, w);
  }
  // a geometry the table cannot hold is refused and leaves no table
  std::vector<uint32_t> none(3, 7u);
  CHECK(!mc::build_ray_prog(bt, N, (total + rpl - 1) / rpl - 1, rpl, km, rowbytes, none) && none.empty(),
        "one lane too few was accepted");
  CHECK(!mc::build_ray_prog(bt, 9, 64 * nb, rpl, km, rowbytes, none) && none.empty(), "9 agents were accepted");
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: %s CASES.txt\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::printf("cannot open %s\n", argv[1]);
    return 2;
  }
  int cases = 0, N, lpe, rpl, km, rowbytes, nb;
  while (std::fscanf(f, "%d %d %d %d %d %d", &N, &lpe, &rpl, &km, &rowbytes, &nb) == 6) {
    std::vector<mc::Beam> bt((size_t)(nb > 0 ? nb : 0));
    for (auto& b : bt) {
      int K, axis, sign, msign;
      unsigned bits;
      if (std::fscanf(f, "%d %d %d %d %u", &K, &axis, &sign, &msign, &bits) != 5) {
        std::printf("bad beam line in case %d\n", cases);
        std::fclose(f);
        return 2;
      }
      b.K = K;
      b.axis = (int16_t)axis;
      b.sign = (int16_t)sign;
      b.msign = msign;
      b.bits = bits;
    }
    check_case(N, lpe, rpl, km, rowbytes, bt);
    ++cases;
  }
  std::fclose(f);
  if (fails || cases == 0) {
    std::printf("%d failures in %d cases\n", fails, cases);
    return 1;
  }
  std::printf("ok %d cases\n", cases);
  return 0;
}
