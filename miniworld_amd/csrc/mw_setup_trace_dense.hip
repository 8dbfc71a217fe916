// mw_step_plan_trace's K1, the dense form: mw_step_plan's (mw_setup_plan_dense.hip) with each sub-step's row of the caller's trace
// stored beside the env's state (mw_setup_common.h: step_env_repeat with PLAN and TRACE, MW_K1_TRACE).
#define MW_K1_PLAN 1
#define MW_K1_TRACE 1
#define MW_DENSE_KERNEL_NAME mw_step_trace_dense_kernel
#include "mw_setup_dense.hip"
