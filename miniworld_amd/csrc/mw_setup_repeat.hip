// mw_step_repeat's K1, the wave-per-env form: the same source as mw_setup.hip around the sub-step loop
// (mw_setup_common.h: step_env_repeat, MW_K1_REPEAT).
#define MW_K1_REPEAT 1
#define MW_SETUP_KERNEL_NAME mw_step_repeat_kernel
#include "mw_setup.hip"
