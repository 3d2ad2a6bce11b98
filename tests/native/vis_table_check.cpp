// Stand-alone run of the visibility table's record function (csrc/mc_vistab.h
// vis_record, the code the build kernel runs), for a host-only build with
// sanitizers (tests/test_vis_table_host.py builds and runs it; no HIP call).
//
// Input (a text file), per case:
//   "Wp Lp H nbeams beam_common beam_k1 bcmax"
//   nbeams lines "K axis sign msign bits"
//   nbeams * bcmax per-start words (hex), beam-major
//   Wp lines of Lp characters, '#' = grid < 0
// Output, per case: "case Wp Lp H", then per cell "x y" and its 2H + 1 row
// words (hex).  The words past row 2H must be zero.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mc_vistab.h"

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
  int cases = 0, Wp, Lp, H, nb, common, bcmax;
  unsigned k1;
  while (std::fscanf(f, "%d %d %d %d %d %u %d", &Wp, &Lp, &H, &nb, &common, &k1, &bcmax) == 7) {
    if (Wp < 1 || Lp < 1 || nb < 1 || bcmax < (Wp > Lp ? Wp : Lp) || !mc::vis_fits(H)) {
      std::printf("bad case header %d\n", cases);
      return 2;
    }
    std::vector<mc::Beam> bt((size_t)nb);
    for (auto& b : bt) {
      int K, axis, sign, msign;
      unsigned bits;
      if (std::fscanf(f, "%d %d %d %d %u", &K, &axis, &sign, &msign, &bits) != 5) return 2;
      b.K = K;
      b.axis = (int16_t)axis;
      b.sign = (int16_t)sign;
      b.msign = msign;
      b.bits = bits;
    }
    std::vector<uint64_t> bb((size_t)nb * bcmax);
    for (auto& w : bb) {
      unsigned long long v;
      if (std::fscanf(f, "%llx", &v) != 1) return 2;
      w = v;
    }
    // the grid's tiles as pack_grids_kernel leaves them: cells of an edge
    // tile beyond the grid, and the padding tiles of the last blocks, blocked
    const int TR = (Wp + 7) / 8, TC = (Lp + 7) / 8, TRS = (TR + 3) / 4, TCS = (TC + 3) / 4;
    std::vector<uint64_t> neg((size_t)TRS * TCS * 16, ~0ull);
    for (int x = 0; x < Wp; ++x) {
      char line[4096];
      if (Lp >= (int)sizeof(line) || std::fscanf(f, "%4095s", line) != 1) return 2;
      for (int y = 0; y < Lp; ++y) {
        if (line[y] == 0) return 2;
        if (line[y] != '#') neg[mc::tile_index(TCS, x >> 3, y >> 3)] &= ~(1ull << (((x & 7) << 3) | (y & 7)));
      }
    }
    std::printf("case %d %d %d\n", Wp, Lp, H);
    for (int x = 0; x < Wp; ++x)
      for (int y = 0; y < Lp; ++y) {
        // an exact-size heap block per record: a write past it is the sanitizer's to find
        std::vector<uint32_t> rec((size_t)mc::kVisRecWords, 0xDEADBEEFu);
        mc::vis_record(neg.data(), TCS, Wp, Lp, H, bt.data(), nb, bb.data(), bcmax, common, k1, x, y, rec.data());
        std::printf("%d %d", x, y);
        for (int r = 0; r <= 2 * H; ++r) std::printf(" %x", rec[r]);
        std::printf("\n");
        for (int r = 2 * H + 1; r < mc::kVisRecWords; ++r)
          if (rec[r] != 0u) {
            std::printf("FAIL cell %d %d: word %d past the record's rows is %x\n", x, y, r, rec[r]);
            return 1;
          }
      }
    ++cases;
  }
  std::fclose(f);
  std::printf("ok %d cases\n", cases);
  return cases ? 0 : 1;
}
