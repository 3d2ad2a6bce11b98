// mc_env_inst_gen64.hip — the env kernels of runtime shape with 64-bit window rows
// (mc_env_select.h MC_ENV_ROWS_GEN64), compiled in a file of their own.
#include "mc_env_step.h"

namespace mc {
MC_ENV_ROWS_GEN64(MC_ENV_INSTANTIATE)
}  // namespace mc
