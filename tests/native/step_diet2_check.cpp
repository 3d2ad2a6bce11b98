// Host check of what the carried step kernels compute in a shorter form
// (csrc/mc_internal.h edge_clip; csrc/mc_env_select.h ItemGeo), built
// host-only with AddressSanitizer and UBSan by tests/test_step_diet2_host.py.
//
// 1. edge_clip (two masks, two compares) equals tile_in_grid (mc_device.h,
//    restated here, and the definition cell by cell) for every tile of every
//    Wp, Lp in 8..40.
// 2. ItemGeo's agent, tile and liveness equal stage_load's two divisions for
//    every lane and item of the carried kernels' slots (32 and 64 lanes), and
//    the dedup rounds merge builds from it are every (item, lower agent) pair
//    some lane has.
// 3. shape_matches refuses a State whose TW is not window_tiles(H): the
//    geometry is derived from H alone.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mc_env_select.h"
#include "mc_vistab.h"

using namespace mc;

static long fails = 0;
#define EXPECT(c)                                 \
  do {                                            \
    if (!(c)) {                                   \
      if (fails < 20) printf("FAIL line %d: %s\n", __LINE__, #c); \
      ++fails;                                    \
    }                                             \
  } while (0)

constexpr int H = 10, TW = window_tiles(H);

// tile_in_grid (mc_device.h) with the map's sides as arguments
static uint64_t low_mask_ref(int w) { return w >= 64 ? ~0ull : ((1ull << w) - 1ull); }
static uint64_t tile_in_grid_ref(int Wp, int Lp, int ti, int tj) {
  const int rv = Wp - 8 * ti, cv = Lp - 8 * tj;
  if (rv >= 8 && cv >= 8) return ~0ull;
  if (rv <= 0 || cv <= 0) return 0ull;
  const uint64_t cols = (cv >= 8 ? 0xFFull : ((1ull << cv) - 1ull)) * 0x0101010101010101ull;
  return cols & low_mask_ref(8 * (rv >= 8 ? 8 : rv));
}

static long check_clip() {
  long n = 0;
  for (int Wp = 8; Wp <= 40; ++Wp)
    for (int Lp = 8; Lp <= 40; ++Lp) {
      const int TR = (Wp + 7) >> 3, TC = (Lp + 7) >> 3;
      const uint64_t rowm = edge_row_mask(Wp), colm = edge_col_mask(Lp);
      for (int gi = 0; gi < TR; ++gi)
        for (int gj = 0; gj < TC; ++gj) {
          const uint64_t got = edge_clip(rowm, colm, TR, TC, gi, gj);
          EXPECT(got == tile_in_grid_ref(Wp, Lp, gi, gj));
          uint64_t def = 0;
          for (int r = 0; r < 8; ++r)
            for (int c = 0; c < 8; ++c)
              if (8 * gi + r < Wp && 8 * gj + c < Lp) def |= 1ull << (8 * r + c);
          EXPECT(got == def);
          ++n;
        }
    }
  static_assert(edge_clip(edge_row_mask(130), edge_col_mask(130), 17, 17, 16, 3) == 0xFFFFull, "the bench map's last row");
  static_assert(edge_clip(edge_row_mask(130), edge_col_mask(130), 17, 17, 3, 16) == 0x0303030303030303ull, "... column");
  static_assert(edge_clip(edge_row_mask(128), edge_col_mask(128), 16, 16, 15, 15) == ~0ull, "no cell beyond the map");
  return n;
}

static uint32_t udiv_ref(uint32_t n, uint32_t magic) { return magic ? (uint32_t)(((uint64_t)n * magic) >> 32) : n; }

template <int LPE, int N>
static long check_geo() {
  using G = ItemGeo<LPE, N, TW>;
  static_assert(G::ok, "the carried kernels' geometry");
  const int TW2 = TW * TW, items = N * TW2;
  const uint32_t mg_TW = magic_div(TW), mg_TW2 = magic_div(TW2);
  long n = 0;
  for (int sub = 0; sub < LPE; ++sub)
    for (int k = 0; k < kMaxItemsPerLane; ++k) {
      // stage_load's general form
      const int idx = sub + k * LPE;
      const bool it = idx < items;
      const int a = it ? (int)udiv_ref(idx, mg_TW2) : 0;
      const int rem = idx - a * TW2;
      const int ti = (int)udiv_ref(rem, mg_TW), tj = rem - ti * TW;
      EXPECT(G::live(k) == it);
      EXPECT(G::agent(sub, k) == a);
      if (it) {
        EXPECT(G::ti(sub) == ti && G::tj(sub) == tj);
        EXPECT(a >= G::first(k) && a < G::first(k) + G::AG && a < N);
      }
      ++n;
    }
  // merge's rounds: (k, b) is built iff b < first(k) + AG - 1 (and b < N - 1); it is
  // needed iff some lane's item k is live with an agent above b
  for (int k = 0; k < kMaxItemsPerLane; ++k)
    for (int b = 0; b < N - 1; ++b) {
      bool needed = false;
      for (int sub = 0; sub < LPE; ++sub) needed |= sub + k * LPE < items && b < (sub + k * LPE) / TW2;
      const bool built = G::live(k) && b < G::first(k) + G::AG - 1;
      EXPECT(built == needed);
      // b < first(k): lower in every lane with the item
      if (built && b < G::first(k))
        for (int sub = 0; sub < LPE; ++sub) EXPECT(b < G::agent(sub, k));
    }
  return n;
}

static void check_tw_refused() {
  State s = {};
  s.N = 4;
  s.H = 10;
  s.TW = window_tiles(10);
  s.sensor = 0;
  s.nbeams = 21;
  s.ego = 2;
  s.Lc = 3;
  s.beam_kmax = 10;
  s.beam_kmin = 8;
  EXPECT(shape_matches<ShapeC2V>(s));
  s.TW = window_tiles(10) + 1;
  EXPECT(!shape_matches<ShapeC2V>(s));
  s.TW = 0;
  EXPECT(!shape_matches<ShapeC2V>(s));
}

int main() {
  check_tw_refused();
  printf("clip: %ld tiles\n", check_clip());
  printf("geometry: %ld items\n", check_geo<32, 4>() + check_geo<64, 4>());
  if (fails) {
    printf("%ld failures\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
