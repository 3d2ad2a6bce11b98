// Stand-alone run of mc_frontier_actions' plain-C++ parts (csrc/mc_frontier.h:
// what the move sink of the BFS kernels and the C ABI run), for a host-only
// build with sanitizers (tests/test_frontier_host.py builds and runs it; no HIP
// call).  The extended grid is mc_bitboard.h's: RX = Wp + 2 pad rows of RY =
// Lp + 2 pad cells, extended cell (u, v) = padded-grid cell (u - pad, v - pad).
//
// It checks
//   - the four step codes (+x 0, +y 1, -x 2, -y 3) and that every other step of
//     [-2, 2]^2 is the stay code;
//   - the cell index -> (x, y) conversion for pad 0, 2 and 5 on a 37 x 45 map at
//     the four corners of the extended grid (ring cells: negative coordinates
//     and ones past the grid), and its round trip over every cell;
//   - every argument check: its code and the argument its message names.
// Output: "steps S", "pad P corners 4 cells C" per pad, "checks K", "ok".
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "mc_bitboard.h"
#include "mc_frontier.h"

namespace {

int g_bad = 0, g_checked = 0;

#define EXPECT(cond)                                              \
  do {                                                            \
    ++g_checked;                                                  \
    if (!(cond)) {                                                \
      std::printf("line %d: %s is false\n", __LINE__, #cond);     \
      ++g_bad;                                                    \
    }                                                             \
  } while (0)

bool names(const mc::FrontierCheck& c, int rc, const char* who, const char* what) {
  return c.rc == rc && std::strstr(c.msg, who) && std::strstr(c.msg, what);
}

}  // namespace

int main() {
  // ---- step codes
  int steps = 0;
  for (int dx = -2; dx <= 2; ++dx)
    for (int dy = -2; dy <= 2; ++dy, ++steps) {
      int want = mc::kActStay;
      if (dx == 1 && dy == 0) want = 0;
      if (dx == 0 && dy == 1) want = 1;
      if (dx == -1 && dy == 0) want = 2;
      if (dx == 0 && dy == -1) want = 3;
      EXPECT(mc::frontier_action(dx, dy) == want);
    }
  EXPECT(mc::kActStay == 4);
  std::printf("steps %d\n", steps);

  // ---- cell index -> padded-grid (x, y)
  const int Wp = 37, Lp = 45;
  const int pads[3] = {0, 2, 5};
  for (int pad : pads) {
    const int RX = Wp + 2 * pad, RY = Lp + 2 * pad;
    const int cu[4] = {0, 0, RX - 1, RX - 1}, cv[4] = {0, RY - 1, 0, RY - 1};
    const int wx[4] = {-pad, -pad, Wp + pad - 1, Wp + pad - 1}, wy[4] = {-pad, Lp + pad - 1, -pad, Lp + pad - 1};
    for (int k = 0; k < 4; ++k) {
      int32_t x = 1 << 20, y = 1 << 20;
      mc::frontier_cell_xy(cu[k] * RY + cv[k], RY, pad, &x, &y);
      EXPECT(x == wx[k] && y == wy[k]);
    }
    int cells = 0;
    for (int u = 0; u < RX; ++u)
      for (int v = 0; v < RY; ++v, ++cells) {
        int32_t x, y;
        mc::frontier_cell_xy(u * RY + v, RY, pad, &x, &y);
        EXPECT(x == u - pad && y == v - pad);
        EXPECT(mc::frontier_cell_index(x, y, RY, pad) == u * RY + v);
      }
    std::printf("pad %d corners 4 cells %d\n", pad, cells);
  }

  // ---- argument checks
  const int before = g_checked;
  int env = 0, act = 0;  // any non-null addresses
  EXPECT(names(mc::frontier_check_setup(nullptr, Wp, Lp, 2), mc::kFrontierEinval, "mc_frontier_setup", "null env"));
  EXPECT(names(mc::frontier_check_setup(&env, 46341, 46341, 0), mc::kFrontierEinval, "mc_frontier_setup", "32-bit"));
  EXPECT(mc::frontier_check_setup(&env, 46340, 46340, 0).rc == 0);
  EXPECT(names(mc::frontier_check_setup(&env, 46338, 46338, 2), mc::kFrontierEinval, "mc_frontier_setup", "32-bit"));
  EXPECT(mc::frontier_check_setup(&env, Wp, Lp, 5).rc == 0);
  EXPECT(mc::frontier_cells_fit(46340, 46340, 0) && !mc::frontier_cells_fit(46341, 46341, 0));
  EXPECT(names(mc::frontier_check_variant(nullptr), mc::kFrontierEinval, "mc_frontier_variant", "null env"));
  EXPECT(mc::frontier_check_variant(&env).rc == 0);
  EXPECT(names(mc::frontier_check_actions(nullptr, &act, true), mc::kFrontierEinval, "mc_frontier_actions", "null env"));
  EXPECT(names(mc::frontier_check_actions(&env, nullptr, true), mc::kFrontierEinval, "mc_frontier_actions", "null dev_actions"));
  // (the arguments come before the state: a null dev_actions before setup is still MC_EINVAL)
  EXPECT(names(mc::frontier_check_actions(&env, nullptr, false), mc::kFrontierEinval, "mc_frontier_actions", "null dev_actions"));
  EXPECT(names(mc::frontier_check_actions(&env, &act, false), mc::kFrontierEstate, "mc_frontier_actions", "mc_frontier_setup"));
  EXPECT(mc::frontier_check_actions(&env, &act, true).rc == 0);
  EXPECT(mc::kFrontierEinval == -1 && mc::kFrontierEstate == -3);
  std::printf("checks %d\n", g_checked - before);

  if (g_bad) {
    std::printf("%d failed\n", g_bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
