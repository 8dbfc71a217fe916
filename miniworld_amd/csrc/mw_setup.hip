// K1 — per-env step, the wave-per-env form (small scenes use the dense form, mw_setup_dense.hip).  Both run step_env
// (mw_setup_common.h, which see for the reference file:line map).
//
// Lanes cooperate: collision segments and entities are tested one per lane (ballot).
// All double-precision dynamics follow numpy's evaluation order.
#include "mw_setup_common.h"
#include "mw_kernels.h"

#ifndef MW_K1_OCC
#define MW_K1_OCC 3      // waves per SIMD the register allocation aims at
#endif

// (lanes_per_env: the dense form's argument, 0 and unused here: one env per workgroup)
extern "C" __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(MW_K1_OCC, 4))) void MW_K1_NAME()(
    MW_K1_PARAMS)
{
    __shared__ int s_claim;
    __shared__ unsigned char gen_ws[MW_GEN_WS_BYTES];
    // spare mode: blocks appended to the grid regenerate the spare worlds consumed in earlier steps, beside the step
    // itself (measured both ways: at the head of the grid they delay the env blocks more than they hide)
    if ((int)blockIdx.x >= a.N) {
        mw::refill_spares(a, (int)blockIdx.x - a.N, (int)threadIdx.x, gen_ws);
        return;
    }
    const int lane = threadIdx.x & 63;
    MW_K1_STEP(false, a.env_base + (int)blockIdx.x, lane, lane == 0, gen_ws, &s_claim);
}
