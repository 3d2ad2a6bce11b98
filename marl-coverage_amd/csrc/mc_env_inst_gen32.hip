// mc_env_inst_gen32.hip — the env kernels of runtime shape with 32-bit window rows
// (mc_env_select.h MC_ENV_ROWS_GEN32), compiled in a file of their own.
#include "mc_env_step.h"

namespace mc {
MC_ENV_ROWS_GEN32(MC_ENV_INSTANTIATE)
}  // namespace mc
