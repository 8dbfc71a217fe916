// mw_step_repeat's K1, the dense form: the same source as mw_setup_dense.hip around the sub-step loop
// (mw_setup_common.h: step_env_repeat, MW_K1_REPEAT).
#define MW_K1_REPEAT 1
#define MW_DENSE_KERNEL_NAME mw_step_repeat_dense_kernel
#include "mw_setup_dense.hip"
