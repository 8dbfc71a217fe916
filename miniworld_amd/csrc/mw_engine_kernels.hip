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

// The frame plan of a plain whole-batch step through the quad kernel (mw_policy.h: frame_plans; mw_frame_plan.h: the decision and the
// plan block), behind the geometry kernel: per env the source byte (mw_get_frame_source) and, unless the env is left alone, an entry in
// the draw list or the copy list.  A lane per env, MW_PLAN_ENVS = 64 envs per wavefront: the lane loads the clean byte, the key K1
// stored for this frame, the header and the keys of all MW_FC_MAX_SLOTS slots — the slots the cache does not have re-read its last one
// and do not count — and, for an ordered plan, the length of its display list, every load issued before the first comparison: one
// round trip to memory.  The appends are aggregated per wavefront: ballots, then ONE atomic instruction per wavefront — lane 0 adds
// to the two counts as one 64-bit word, and in an ordered plan lanes 1 and 2 add the wavefront's eight class counts, four 16-bit
// fields to a word, each word on a line of its own (one line takes ~88 atomics/us: an atomic per env, or two per eight envs, cost more
// than the rest of the kernel — 14.6 us measured at 4096 envs against 5.4 with one per wavefront).  No LDS; grid ceil(N /
// MW_PLAN_ENVS) wavefronts.
// reuse: MW_RASTER_REUSE applies; meta: the cache's key table, null without a cache (slots 0); nvis: the display lists' lengths for an
// ordered plan (frame_plan_ordered), null for one unordered draw list; next: the engine's other plan block, whose counters this
// launch zeroes for the frame after this one.
extern "C" __global__ __launch_bounds__(64) void mw_frame_plan_kernel(int N, int reuse, const uint8_t *__restrict__ frame_clean, const uint64_t *__restrict__ key,
                                                                     const uint64_t *__restrict__ meta, int slots, const int32_t *__restrict__ nvis,
                                                                     uint8_t *__restrict__ frame_source, uint32_t *__restrict__ plan, uint32_t *__restrict__ next)
{
    const int lane = (int)threadIdx.x, env = (int)blockIdx.x * MW_PLAN_ENVS + lane;
    const bool ordered = nvis != nullptr;
    if (blockIdx.x == 0) {
        if (lane < 2) next[lane] = 0u;
        else if (lane < 4) next[MW_PLAN_CLS_LO + lane - 2] = 0u;
        else if (lane < 6) next[MW_PLAN_CLS_HI + lane - 4] = 0u;
        else if (lane == 6) plan[2] = ordered ? (uint32_t)MW_PLAN_CLASSES : 0u;
    }
    const bool on = env < N;
    uint32_t v = MW_SRC_CLEAN;          // (a lane without an env appends nothing)
    uint32_t cls = 0u;
    if (on) {
        const bool clean = frame_clean[env] != 0;
        const int32_t len = ordered ? nvis[env] : 0;
        uint32_t match = 0u, header = 0u;
        if (meta) {
            const uint64_t *row = static_cast<const uint64_t *>(__builtin_assume_aligned(meta + (size_t)env * MW_FC_META_WORDS(slots), 16));
            const uint64_t *cur = static_cast<const uint64_t *>(__builtin_assume_aligned(key + (size_t)env * MW_FC_KEY_WORDS, 16));
            header = (uint32_t)row[0];
#pragma unroll
            for (int j = 0; j < MW_FC_MAX_SLOTS; ++j) {
                const int jj = j < slots ? j : slots - 1;
                match |= mw_fc_key_equal(static_cast<const uint64_t *>(__builtin_assume_aligned(row + 2 + MW_FC_KEY_WORDS * jj, 16)), cur) && j < slots ? 1u << j : 0u;
            }
        }
        v = mw_frame_verdict(clean, reuse != 0, match, header, meta ? slots : 0);
        frame_source[env] = (uint8_t)v;
        cls = mw_plan_cost_class(len);
    }
    const uint32_t src = v & 0xFFu;
    const bool draw = on && src == MW_SRC_DRAWN, copy = on && src >= (uint32_t)MW_SRC_SLOT(0);
    const uint64_t md = __builtin_amdgcn_ballot_w64(draw), mc = __builtin_amdgcn_ballot_w64(copy), below = (1ull << lane) - 1ull;
    // (plan[0] and plan[1] as one 64-bit word: draw entries in the low half, copy entries in the high half; neither can carry — nor
    // can a 16-bit class count: the counters start at zero and an ordered plan has at most MW_PLAN_ORDERED_MAX_N envs)
    unsigned long long add = (unsigned long long)__popcll(md) | (unsigned long long)__popcll(mc) << 32, add_lo = 0ull, add_hi = 0ull;
    uint64_t mine = md;                 // the drawn lanes this lane shares a list with
    if (ordered) {
#pragma unroll
        for (uint32_t c = 0; c < MW_PLAN_CLASSES; ++c) {
            const uint64_t m = __builtin_amdgcn_ballot_w64(draw && cls == c);
            (c < 4u ? add_lo : add_hi) |= (unsigned long long)__popcll(m) << (16u * (c & 3u));
            mine = cls == c ? m : mine;
        }
    }
    unsigned long long old = 0ull;
    if (lane < 3) {
        const unsigned long long a = lane == 0 ? add : lane == 1 ? add_lo : add_hi;
        uint32_t *at = plan + (lane == 0 ? 0 : lane == 1 ? MW_PLAN_CLS_LO : MW_PLAN_CLS_HI);
        if (a) old = atomicAdd(reinterpret_cast<unsigned long long *>(at), a);
    }
    const uint32_t old_lo = (uint32_t)old, old_hi = (uint32_t)(old >> 32);
    const uint32_t bd = (uint32_t)__builtin_amdgcn_readlane((int)old_lo, 0), bc = (uint32_t)__builtin_amdgcn_readlane((int)old_hi, 0);
    const uint64_t base_lo = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)old_lo, 1) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)old_hi, 1) << 32;
    const uint64_t base_hi = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)old_lo, 2) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)old_hi, 2) << 32;
    const uint32_t entry = (uint32_t)env | (v >> 8) << MW_PLAN_ENV_BITS;
    // (the counts start at zero, so a list never outgrows its N entries; the tests keep a stray count from writing past them)
    const uint32_t id = (ordered ? mw_plan_class_count(base_lo, base_hi, cls) : bd) + (uint32_t)__popcll(mine & below), ic = bc + (uint32_t)__popcll(mc & below);
    if (draw && id < (uint32_t)N) plan[MW_PLAN_DRAW(N, ordered ? cls : 0u) + id] = entry;
    if (copy && ic < (uint32_t)N) plan[MW_PLAN_COPY(N) + ic] = entry;
}
