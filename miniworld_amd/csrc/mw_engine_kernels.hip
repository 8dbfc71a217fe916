// The host runtime's own small kernels: mw_get_info's gather and the list and row copy of a same-step step with final observations
// (mw_engine.hip, mw_engine_frame.hip).
#include "mw_kernels.h"

// mw_get_info: what the envs' step() returns in `info` beside the observation (collecthealth.py:100, tmaze.py:89, ymaze.py:125)
extern "C" __global__ void mw_info_kernel(int N, int E, const int32_t *health, const double *epos, int slot, int32_t *out_health, double *out_pos)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (out_health) out_health[i] = health[i];
    if (out_pos)
        for (int c = 0; c < 3; ++c) out_pos[(size_t)i * 3 + c] = epos[((size_t)c * E + slot) * N + i];
}

// Same-step auto-reset with final observations (mw_set_final_obs), behind the first pass's step kernel: the envs whose episode
// ended with this step — reset_pending, set by the step kernel run as the next-step mode's terminal step — in ascending order, as
// list[0] = count, list[1 + i] = env.  One workgroup, ballot compaction, deterministic.  The finished worlds' pending removals go:
// the same-step install drops them (a picked object's world is replaced; CollectHealth's consumed kit does not respawn).
extern "C" __global__ __launch_bounds__(1024) void mw_final_list_kernel(int N, const uint8_t *__restrict__ pending, int32_t *__restrict__ pending_remove,
                                                                       int32_t *__restrict__ list)
{
    __shared__ int s_wave[16];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int i0 = 0; i0 < N; i0 += 1024) {
        const int i = i0 + tid;
        const bool p = i < N && pending[i] != 0;
        const unsigned long long m = __ballot(p);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = base, total = 0;
        for (int w = 0; w < 16; ++w) {
            const int c = s_wave[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (p) {
            list[1 + before + __popcll(m & ((1ull << lane) - 1ull))] = i;
            pending_remove[i] = -1;
        }
        base += total;
        __syncthreads();        // (s_wave is rewritten by the next round)
    }
    if (tid == 0) list[0] = base;
}

// ... behind the first pass's frame: the listed envs' rows of the observation (and depth) into the final buffers.  Grid N, one
// workgroup per list slot.
extern "C" __global__ __launch_bounds__(256) void mw_final_copy_kernel(const int32_t *__restrict__ list, const uint8_t *__restrict__ obs,
                                                                      uint8_t *__restrict__ final_obs, unsigned long long row_bytes,
                                                                      const float *__restrict__ depth, float *__restrict__ final_depth, int depth_row)
{
    if ((int)blockIdx.x >= list[0]) return;
    const size_t env = (size_t)list[1 + blockIdx.x];
    const uint8_t *src = obs + env * row_bytes;
    uint8_t *dst = final_obs + env * row_bytes;
    if ((((uintptr_t)obs | (uintptr_t)final_obs | (uintptr_t)row_bytes) & 15u) == 0) {
        for (size_t k = threadIdx.x; k < row_bytes / 16; k += blockDim.x)
            reinterpret_cast<uint4 *>(dst)[k] = reinterpret_cast<const uint4 *>(src)[k];
    } else {
        for (size_t k = threadIdx.x; k < row_bytes; k += blockDim.x) dst[k] = src[k];
    }
    if (depth && final_depth)
        for (int k = threadIdx.x; k < depth_row; k += blockDim.x) final_depth[env * depth_row + k] = depth[env * depth_row + k];
}
