// mw_step_plan_trace's K1, the wave-per-env form: mw_step_plan's (mw_setup_plan.hip) with each sub-step's row of the caller's trace
// stored beside the env's state (mw_setup_common.h: step_env_repeat with PLAN and TRACE, MW_K1_TRACE).
#define MW_K1_PLAN 1
#define MW_K1_TRACE 1
#define MW_SETUP_KERNEL_NAME mw_step_trace_kernel
#include "mw_setup.hip"
