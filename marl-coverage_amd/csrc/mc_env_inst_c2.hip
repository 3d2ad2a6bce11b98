// mc_env_inst_c2.hip — the env kernels of the compiled C2 shapes
// (mc_env_select.h MC_ENV_ROWS_C2), compiled in a file of their own.
#include "mc_env_step.h"

namespace mc {
MC_ENV_ROWS_C2(MC_ENV_INSTANTIATE)
}  // namespace mc
