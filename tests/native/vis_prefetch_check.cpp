// Host check of the fused loop's record prefetch (csrc/mc_fuse.h
// fuse_predict_cell; csrc/mc_vistab.h vis_item_offset), built host-only with
// AddressSanitizer and UBSan by tests/test_vis_prefetch_host.py.
//
// 1. The predictor against a literal restatement of moves_front's rule for one
//    robot alone (mc_env_step.h): every action byte, every cell of a 20 x 26
//    map with its four borders, blocked and free targets.
// 2. The address expression the step and the prefetch share, walked the way
//    vis_prefetch walks it (block origins from the cell before the step, the
//    record of the predicted cell) over a heap buffer of exactly
//    vis_table_bytes(G, Wp, Lp) bytes: every 8-byte read must land inside it
//    (an ASan report otherwise), for real cells and for garbage ones.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mc_fuse.h"
#include "mc_vistab.h"

using namespace mc;

static int fails = 0;
#define EXPECT(c)                                 \
  do {                                            \
    if (!(c)) {                                   \
      if (fails < 20) printf("FAIL line %d: %s\n", __LINE__, #c); \
      ++fails;                                    \
    }                                             \
  } while (0)

constexpr int Wp = 20, Lp = 26, H = 10;  // the C2 lidar's range

// moves_front for robot i with no other robot in the way: the target is the
// cell one step along the byte's direction; the robot takes it when the byte
// is 0..3 and the target is neither out of bounds nor grid < 0
static void restated(int x, int y, int act, bool grid_neg_at_target, int* ox, int* oy, bool* blocked) {
  int tx = x, ty = y;
  if (act == 0) tx = x + 1;
  if (act == 1) ty = y + 1;
  if (act == 2) tx = x - 1;
  if (act == 3) ty = y - 1;
  const bool inb = tx >= 0 && tx < Wp && ty >= 0 && ty < Lp;
  *blocked = !inb || grid_neg_at_target;
  const bool acts = act >= 0 && act <= 3;
  const bool ok = acts && !*blocked;
  *ox = ok ? tx : x;
  *oy = ok ? ty : y;
}

static long check_predictor() {
  long n = 0;
  for (int x = 0; x < Wp; ++x)
    for (int y = 0; y < Lp; ++y)
      for (int act = 0; act < 256; ++act)
        for (int neg = 0; neg < 2; ++neg) {
          int wx, wy;
          bool blocked;
          restated(x, y, act, neg != 0, &wx, &wy, &blocked);
          const uint32_t xy = (uint32_t)x | ((uint32_t)y << 16);
          const uint32_t got = fuse_predict_cell(xy, (uint32_t)act, blocked);
          EXPECT(got == ((uint32_t)wx | ((uint32_t)wy << 16)));
          EXPECT((got & 0xFFFFu) < (uint32_t)Wp && (got >> 16) < (uint32_t)Lp);  // a cell of the map
          if (act <= 3 && !blocked) EXPECT(got == fuse_target_cell(xy, (uint32_t)act));
          ++n;
        }
  static_assert(fuse_predict_cell(5u | (7u << 16), 0, false) == (6u | (7u << 16)), "usable at compile time");
  static_assert(fuse_predict_cell(5u | (7u << 16), 3, true) == (5u | (7u << 16)), "a blocked target: stays");
  static_assert(fuse_predict_cell(5u | (7u << 16), 200, false) == (5u | (7u << 16)), "no act: stays");
  return n;
}

// one prefetch of an item the way vis_prefetch forms it: (x, y) the robot's
// cell before the step (the block origin), (px, py) the predicted cell
static void prefetch_item(const std::vector<uint8_t>& tab, int G, int g, int x, int y, int px, int py, int ti, int tj,
                          bool live, long* reads, long* ons) {
  const int bx = (x - H - 1) >> 3, by = (y - H - 1) >> 3;
  bool on = false;
  const size_t off = vis_item_offset(G, Wp, Lp, H, g, bx + ti, by + tj, px, py, live, &on);
  EXPECT(off % 8 == 0 && off + 8 <= tab.size());
  uint64_t v;
  memcpy(&v, tab.data() + off, 8);  // the load: inside the heap buffer or an ASan report
  const size_t rec = off / (kVisRecWords * 4);
  EXPECT(v == (uint64_t)rec);
  const bool real = px >= 0 && px < Wp && py >= 0 && py < Lp && g >= 0 && g < G;
  if (real) EXPECT(rec == vis_index(Wp, Lp, g, px, py));  // the predicted cell's record
  if (on) {
    EXPECT(live);
    const int ri = bx + ti - ((px - H) >> 3), rj = by + tj - ((py - H) >> 3);
    EXPECT(ri >= 0 && ri < 4 && rj >= 0 && rj < 4);
    EXPECT(off % (kVisRecWords * 4) == (size_t)(ri * 4 + rj) * 8);
    ++*ons;
  } else {
    EXPECT(off % (kVisRecWords * 4) == 0);
  }
  ++*reads;
}

static void walk_table(int G) {
  // exactly the table's bytes (heap: ASan guards both ends); every tile of record r holds r
  std::vector<uint8_t> tab(vis_table_bytes(G, Wp, Lp));
  for (size_t r = 0; r < tab.size() / (kVisRecWords * 4); ++r)
    for (int t = 0; t < kVisRecWords / 2; ++t) {
      const uint64_t v = r;
      memcpy(tab.data() + r * (kVisRecWords * 4) + (size_t)t * 8, &v, 8);
    }
  long reads = 0, ons = 0;
  const int TW = 4;  // tiles a side of a robot's block (the C2 shapes)
  for (int g = 0; g < G; ++g)
    for (int x = 0; x < Wp; ++x)
      for (int y = 0; y < Lp; ++y)
        for (int act = 0; act < 256; ++act) {
          for (int neg = 0; neg < 2; ++neg) {
            const int tx = x + ((act == 0) - (act == 2)), ty = y + ((act == 1) - (act == 3));
            const bool blocked = neg || tx < 0 || tx >= Wp || ty < 0 || ty >= Lp;
            const uint32_t pc = fuse_predict_cell((uint32_t)x | ((uint32_t)y << 16), (uint32_t)act, blocked);
            for (int ti = 0; ti < TW; ++ti)
              for (int tj = 0; tj < TW; ++tj)
                prefetch_item(tab, G, g, x, y, (int)(pc & 0xFFFFu), (int)(pc >> 16), ti, tj, true, &reads, &ons);
            prefetch_item(tab, G, g, x, y, (int)(pc & 0xFFFFu), (int)(pc >> 16), 0, 0, false, &reads, &ons);
          }
        }
  // garbage: cells and grids no step produces still read inside the table
  const int junk[] = {-1, -8, -1000000, INT32_MIN / 2, 0xFFFF, 0x7FFF, Wp, Lp, 1 << 20};
  for (int g : {0, G - 1, G, -1, 1 << 20})
    for (int x : junk)
      for (int y : junk)
        for (int px : junk)
          for (int py : junk)
            for (int t = 0; t < TW * TW; ++t) prefetch_item(tab, G, g, x, y, px, py, t / TW, t % TW, true, &reads, &ons);
  EXPECT(ons > 0 && ons < reads);
  printf("G %d: %ld prefetch reads inside the table of %zu bytes\n", G, reads, tab.size());
}

int main() {
  printf("predictor: %ld cases\n", check_predictor());
  walk_table(1);
  walk_table(3);
  if (fails) {
    printf("%d failures\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
