// mc_env_inst_c45.hip — the env kernels of the compiled C4 and C5 shapes
// (mc_env_select.h MC_ENV_ROWS_C45), compiled in a file of their own.
#include "mc_env_step.h"

namespace mc {
MC_ENV_ROWS_C45(MC_ENV_INSTANTIATE)
}  // namespace mc
