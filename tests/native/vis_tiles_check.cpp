// Stand-alone run of the visibility table's tile-form record (csrc/mc_vistab.h
// vis_tiles_as, the code the build kernel runs after vis_record), for a
// host-only build with sanitizers (tests/test_vis_tiles_host.py builds and runs
// it; no HIP call).  Both forms are checked whatever kVisSplit the library is
// built with.
//
// Input: the format of vis_table_check.cpp.  For every cell of every case the
// unsplit and the split record are compared, bit by bit, with a per-cell
// restatement from vis_record's rows and vis_blocked:
//   bit (r << 3) | c of tile (i, j) is the cell (8 (ox + i) + r, 8 (oy + j) + c),
//   (ox, oy) = (floor((x - H) / 8), floor((y - H) / 8));
//   it is set iff the cell lies in the window [x - H, x + H] x [y - H, y + H]
//   and its row word has the cell's bit; split: in the free tiles iff also not
//   vis_blocked, in the obstacle tiles iff vis_blocked (outside the map too).
// Also: every bit outside the window is zero, the split tiles are disjoint and
// their OR is the unsplit record.  Output per case: "case Wp Lp H", the
// residues (x - H) & 7 x (y - H) & 7 seen as a 64-bit mask, and the window
// sides that left the map (bit 0 x < 0, 1 x >= Wp, 2 y < 0, 3 y >= Lp).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mc_vistab.h"

static int floordiv8(int v) { return v >= 0 ? v / 8 : -((-v + 7) / 8); }

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
    uint64_t residues = 0;
    unsigned sides = 0;
    long marks = 0;
    for (int x = 0; x < Wp; ++x)
      for (int y = 0; y < Lp; ++y) {
        // exact-size heap blocks: a write past one is the sanitizer's to find
        std::vector<uint32_t> rec((size_t)mc::kVisRecWords, 0xDEADBEEFu);
        mc::vis_record(neg.data(), TCS, Wp, Lp, H, bt.data(), nb, bb.data(), bcmax, common, k1, x, y, rec.data());
        std::vector<uint64_t> un((size_t)mc::kVisTiles, 0xDEADBEEFDEADBEEFull);
        std::vector<uint64_t> sp((size_t)2 * mc::kVisTiles, 0xDEADBEEFDEADBEEFull);
        mc::vis_tiles_as<false>(rec.data(), neg.data(), TCS, Wp, Lp, H, x, y, un.data());
        mc::vis_tiles_as<true>(rec.data(), neg.data(), TCS, Wp, Lp, H, x, y, sp.data());
        const int ox = floordiv8(x - H), oy = floordiv8(y - H);
        residues |= 1ull << ((((x - H) & 7) << 3) | ((y - H) & 7));
        sides |= (x - H < 0 ? 1u : 0u) | (x + H >= Wp ? 2u : 0u) | (y - H < 0 ? 4u : 0u) | (y + H >= Lp ? 8u : 0u);
        long seen = 0, want_seen = 0;
        for (int r = 0; r <= 2 * H; ++r) want_seen += __builtin_popcount(rec[r]);
        for (int t = 0; t < mc::kVisTiles; ++t) {
          const int i = t >> 2, j = t & 3;
          for (int b = 0; b < 64; ++b) {
            const int cx = 8 * (ox + i) + (b >> 3), cy = 8 * (oy + j) + (b & 7);
            const int dr = cx - (x - H), dc = cy - (y - H);
            const bool inwin = dr >= 0 && dr <= 2 * H && dc >= 0 && dc <= 2 * H;
            const bool mark = inwin && ((rec[dr] >> dc) & 1u);
            const bool blocked = mc::vis_blocked(neg.data(), TCS, Wp, Lp, cx, cy);
            const bool gu = (un[t] >> b) & 1ull, gf = (sp[t] >> b) & 1ull, go = (sp[mc::kVisTiles + t] >> b) & 1ull;
            if (!inwin && (gu || gf || go)) {
              std::printf("FAIL cell %d %d: tile %d bit %d outside the window is set\n", x, y, t, b);
              return 1;
            }
            if (gu != mark || gf != (mark && !blocked) || go != (mark && blocked)) {
              std::printf("FAIL cell %d %d H %d: tile %d bit %d (cell %d %d) unsplit %d free %d obstacle %d, want mark %d blocked %d\n",
                          x, y, H, t, b, cx, cy, (int)gu, (int)gf, (int)go, (int)mark, (int)blocked);
              return 1;
            }
            seen += gu;
          }
          if ((sp[t] & sp[mc::kVisTiles + t]) != 0ull || (sp[t] | sp[mc::kVisTiles + t]) != un[t]) {
            std::printf("FAIL cell %d %d: split tiles %d overlap or do not add up to the unsplit tile\n", x, y, t);
            return 1;
          }
        }
        if (seen != want_seen) {  // every mark of the rows has a place in the 4 x 4 tiles
          std::printf("FAIL cell %d %d: %ld marks in the tiles, %ld in the rows\n", x, y, seen, want_seen);
          return 1;
        }
        marks += seen;
      }
    std::printf("case %d %d %d residues %llx sides %x marks %ld\n", Wp, Lp, H, (unsigned long long)residues, sides, marks);
    ++cases;
  }
  std::fclose(f);
  std::printf("ok %d cases\n", cases);
  return cases ? 0 : 1;
}
