// mw_step_plan's K1, the wave-per-env form: the same source as mw_setup.hip around the sub-step loop with one action per sub-step
// (mw_setup_common.h: step_env_repeat with PLAN, MW_K1_PLAN).
#define MW_K1_PLAN 1
#define MW_SETUP_KERNEL_NAME mw_step_plan_kernel
#include "mw_setup.hip"
