// mw_step_plan_trace's dense K1 compiled for the MW_RNG_PCG64 stream (mw_rng.h).
#define MW_RNG_KIND 1
#define MW_K1_PLAN 1
#define MW_K1_TRACE 1
#define MW_DENSE_KERNEL_NAME mw_step_trace_dense_pcg_kernel
#include "mw_setup_dense.hip"
