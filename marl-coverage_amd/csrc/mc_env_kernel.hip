// mc_env_kernel.hip — the env kernel's dispatch: the row of mc_env_select.h
// for a State, its public name and its launch.  The kernels themselves
// (mc_env_step.h) are instantiated by the mc_env_inst_*.hip files; this file
// instantiates none.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "mc_env_select.h"

namespace mc {

// the launchers, row for row with kEnvRows
#define MC_ENV_EXTERN(T, P, W, SH, NAME) extern template EnvLauncher launch_one<T, P, W, SH>;
#define MC_ENV_LAUNCHER(T, P, W, SH, NAME) &launch_one<T, P, W, SH>,
MC_ENV_ROWS(MC_ENV_EXTERN)
static EnvLauncher* const kEnvLaunchers[] = {MC_ENV_ROWS(MC_ENV_LAUNCHER)};
#undef MC_ENV_EXTERN
#undef MC_ENV_LAUNCHER

// MARLCOV_SPECIALIZE=0 forces the generic (runtime-shape) kernels (A/B tests)
static bool getenv_spec() {
  static const bool on = [] {
    const char* v = getenv("MARLCOV_SPECIALIZE");
    return !(v && v[0] == '0');
  }();
  return on;
}

static int select_env(const State& s, int nt, int epw) { return select_env_row(s, nt, epw, getenv_spec()); }

const char* env_variant(const State& s, int nt, int epw) {
  const int i = select_env(s, nt, epw);
  return i < 0 ? "none" : kEnvRows[i].name;
}

const char* env_label(const State& s, int nt, int epw) {
  const int i = select_env(s, nt, epw);
  return i < 0 ? "none" : kEnvRows[i].label;
}

bool env_takes_vis_table(const State& s, int nt, int epw) { return env_takes_vis_table(s, nt, epw, getenv_spec()); }

hipError_t launch_env(const State& s, int mode, const uint8_t* actions, const uint8_t* env_mask,
                      const int32_t* inj_pos, double* reward, uint8_t* done, uint8_t* obs,
                      uint8_t* adj, int num_steps, const EnvStrides& strides, int nt, int epw,
                      hipStream_t stream) {
  if (num_steps < 1 || (mode != MODE_STEP && num_steps != 1)) return hipErrorInvalidValue;  // a reset is one pass
  const int i = select_env(s, nt, epw);
  if (i < 0) return hipErrorInvalidValue;  // (no mc_create geometry gets here: env_geometry)
  kEnvLaunchers[i](s, mode, actions, env_mask, inj_pos, reward, done, obs, adj, num_steps, strides, stream);
  return hipGetLastError();
}

}  // namespace mc
