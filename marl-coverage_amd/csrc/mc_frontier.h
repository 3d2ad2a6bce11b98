// mc_frontier.h — the plain-C++ parts of mc_frontier_actions (mc_dijkstra.hip's
// move sink, mc_capi.hip): the action code of a step, the padded-grid
// coordinates of an extended cell index, and the argument checks.
//
// Plain C++ on both sides: the kernels, the C ABI and the host check
// (tests/native/frontier_check.cpp) run the same code.
#pragma once
#include <stdint.h>

namespace mc {

constexpr int kActStay = 4;  // MC_ACT_STAY

// The MC_ACT_* code of the unit step (dx, dy): +x 0, +y 1, -x 2, -y 3
// (dec_grid_rl.py:131-145); any other step (the agent stays) is kActStay.
__host__ __device__ inline int frontier_action(int dx, int dy) {
  if (dy == 0) return dx == 1 ? 0 : (dx == -1 ? 2 : kActStay);
  if (dx == 0) return dy == 1 ? 1 : (dy == -1 ? 3 : kActStay);
  return kActStay;
}

// Extended cell index u * RY + v (RY = Lp + 2 pad columns) -> padded-grid
// (x, y) = (u - pad, v - pad): a ring cell has a negative coordinate or one
// past the grid.
__host__ __device__ inline void frontier_cell_xy(int32_t cell, int RY, int pad, int32_t* x, int32_t* y) {
  const int32_t u = cell / RY;
  *x = u - pad;
  *y = cell - u * RY - pad;
}

// ... and back (the window kernel names its end point by padded coordinates)
__host__ __device__ inline int32_t frontier_cell_index(int32_t x, int32_t y, int RY, int pad) {
  return (x + pad) * RY + (y + pad);
}

// the extended grid's cells are int32 indices (mc_create's rule for dijkstra_input)
inline bool frontier_cells_fit(int Wp, int Lp, int pad) {
  return ((int64_t)Wp + 2 * pad) * ((int64_t)Lp + 2 * pad) <= INT32_MAX;
}

// The argument checks of the three entry points, in the order they are made:
// the return code (0, kFrontierEinval = MC_EINVAL, kFrontierEstate = MC_ESTATE)
// and the message, which names the argument.
constexpr int kFrontierEinval = -1, kFrontierEstate = -3;

struct FrontierCheck {
  int rc;
  const char* msg;
};

inline FrontierCheck frontier_check_setup(const void* env, int Wp, int Lp, int pad) {
  if (!env) return {kFrontierEinval, "mc_frontier_setup: null env"};
  if (!frontier_cells_fit(Wp, Lp, pad))
    return {kFrontierEinval, "mc_frontier_setup: the grid's extended cells exceed a 32-bit index"};
  return {0, ""};
}

inline FrontierCheck frontier_check_variant(const void* env) {
  if (!env) return {kFrontierEinval, "mc_frontier_variant: null env"};
  return {0, ""};
}

inline FrontierCheck frontier_check_actions(const void* env, const void* dev_actions, bool is_setup) {
  if (!env) return {kFrontierEinval, "mc_frontier_actions: null env"};
  if (!dev_actions) return {kFrontierEinval, "mc_frontier_actions: null dev_actions"};
  if (!is_setup) return {kFrontierEstate, "mc_frontier_actions: call mc_frontier_setup on this handle first"};
  return {0, ""};
}

}  // namespace mc
