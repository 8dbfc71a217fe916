// Frame stacking (mw_set_frame_stack): the last K returned frames of every env, oldest first, kept on the device.
//
// Storage: the caller's ring, [N][2K - 1][frame].  Push number j of the engine (0, 1, ...; phase p = j mod K) writes the env's frame
// to slot p + K - 1 and, when p >= 1, to slot p - 1 as well: every frame exists twice, K slots apart, so the window of the last K
// frames is always K CONSECUTIVE slots — those from p on — and nothing is ever shifted or gathered.  The caller reads the window as a
// strided view of the ring.
//
// A rebuild (the first frame of an episode, mw_stack_refresh) writes all 2K - 1 slots of the env as if its last K pushes had been
// K - 1 pad frames and then the frame: the frame goes to the two slots a push of phase p writes, the pad — the frame again
// (MW_STACK_PAD_RESET) or zeros (MW_STACK_PAD_ZERO) — to every other slot, so the windows of the next K - 1 pushes show the pad
// leaving on the old side one frame at a time.
//
// Workgroups are over (env, chunk of the frame).  What happens to an env — an ordinary push, a rebuild, a final-stack row — is
// decided from per-env bytes and is the same for all of its workgroups.  A lane owns the same units of every slot: it reads its units
// of the old window for the final-stack row before it overwrites them, so the chunks of an env cannot race and no barrier is needed.
// The flag bytes are double-buffered for the same reason: every workgroup of an env reads flags_in, one of them writes flags_out.
#include <hip/hip_runtime.h>

#include "mw_kernels.h"

namespace {

template <typename T> __device__ __forceinline__ T zero_unit();
template <> __device__ __forceinline__ uint4 zero_unit<uint4>() { return make_uint4(0u, 0u, 0u, 0u); }
template <> __device__ __forceinline__ uint8_t zero_unit<uint8_t>() { return 0; }

// T: uint4 when every base and the frame size are multiples of 16 bytes (80 x 60 x 3, 84 x 84 x 3, every grey frame), else bytes.
// phase: the push's own (PUSH), or the last push's (refresh: the rebuilt window is the current one).
template <typename T, bool PUSH>
__device__ __forceinline__ void stack_env_chunk(int depth, int pad, int phase, unsigned long long frame_bytes, const uint8_t *__restrict__ obs, uint8_t *ring,
                                                const uint8_t *__restrict__ flags_in, uint8_t *__restrict__ flags_out, const uint8_t *__restrict__ term,
                                                const uint8_t *__restrict__ trunc, const uint8_t *__restrict__ pending, const uint8_t *__restrict__ final_obs,
                                                uint8_t *__restrict__ final_stack)
{
    const size_t env = blockIdx.x;
    const uint8_t fl = flags_in[env];
    // the call installed a world for the env: same-step auto-reset with a generator (the host passes the flags only then)
    const bool ended = PUSH && term && (term[env] | trunc[env]) != 0;
    const bool rebuild = PUSH ? (fl != 0 || ended) : (fl & MW_STACK_FRESH) != 0;
    if (blockIdx.y == 0 && threadIdx.x == 0)
        flags_out[env] = PUSH ? (uint8_t)(pending && pending[env] ? MW_STACK_PENDING : 0) : (uint8_t)(fl & ~MW_STACK_FRESH);
    if (!PUSH && !rebuild) return;
    const bool fin = PUSH && final_stack && ended;
    const size_t units = (size_t)(frame_bytes / sizeof(T)), slots = 2 * (size_t)depth - 1;
    const T *src = reinterpret_cast<const T *>(obs + env * frame_bytes);
    T *ring_env = reinterpret_cast<T *>(ring + env * slots * frame_bytes);
    const size_t first = (size_t)blockIdx.y * (MW_STACK_THREADS * MW_STACK_UNROLL) + threadIdx.x;
    // the env's row of the final stack: its K - 1 newest frames from before this push — the old window without its oldest slot; the
    // pad where the env has no valid stack (reset or never pushed, and not refreshed) —, then the terminal frame
    const T *term_frame = fin ? reinterpret_cast<const T *>(final_obs + env * frame_bytes) : nullptr;
    T *row = fin ? reinterpret_cast<T *>(final_stack + env * (size_t)depth * frame_bytes) : nullptr;
    const size_t old_first = (size_t)((phase + depth - 1) % depth) + 1;
    const size_t hi = (size_t)(phase + depth - 1);      // the two slots of the frame: hi and hi - depth (none at phase 0)
#pragma unroll
    for (int i = 0; i < MW_STACK_UNROLL; ++i) {
        const size_t u = first + (size_t)i * MW_STACK_THREADS;
        if (u >= units) break;
        const T f = src[u];
        if (fin) {
            const T t = term_frame[u];
            // (branches, not selects between 16-byte values: the compiler turns those into an indexed pair in scratch)
            if (!(fl & MW_STACK_FRESH))
                for (int k = 0; k < depth - 1; ++k) row[(size_t)k * units + u] = ring_env[(old_first + k) * units + u];
            else if (pad == MW_STACK_PAD_ZERO)
                for (int k = 0; k < depth - 1; ++k) row[(size_t)k * units + u] = zero_unit<T>();
            else
                for (int k = 0; k < depth - 1; ++k) row[(size_t)k * units + u] = t;
            row[(size_t)(depth - 1) * units + u] = t;
        }
        if (rebuild && pad == MW_STACK_PAD_ZERO) {
            for (size_t s = 0; s < slots; ++s)
                if (s != hi && s + depth != hi) ring_env[s * units + u] = zero_unit<T>();
        } else if (rebuild) {
            for (size_t s = 0; s < slots; ++s)
                if (s != hi && s + depth != hi) ring_env[s * units + u] = f;
        }
        ring_env[hi * units + u] = f;
        if (phase >= 1) ring_env[(hi - depth) * units + u] = f;
    }
}

}  // namespace

// One push, behind the last raster kernel of an mw_step / mw_step_repeat.  Grid (N, chunks), MW_STACK_THREADS lanes.
//   flags_in / flags_out  the env's "rebuild on the next push" byte, this push's and the next one's (MW_STACK_*)
//   term, trunc           the call's flags when an env that finished was given its next world in this call, else null
//   pending               reset_pending when the env's next call installs a world (next-step auto-reset), else null
//   final_obs, final_stack  the terminal frames of this call and the final-stack rows they complete, or null
extern "C" __global__ __launch_bounds__(MW_STACK_THREADS) void mw_stack_push_kernel(MW_STACK_ARGS, const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc,
                                                                                   const uint8_t *__restrict__ pending, const uint8_t *__restrict__ final_obs,
                                                                                   uint8_t *__restrict__ final_stack)
{
    if (wide) stack_env_chunk<uint4, true>(depth, pad, phase, frame_bytes, obs, ring, flags_in, flags_out, term, trunc, pending, final_obs, final_stack);
    else stack_env_chunk<uint8_t, true>(depth, pad, phase, frame_bytes, obs, ring, flags_in, flags_out, term, trunc, pending, final_obs, final_stack);
}

// mw_stack_refresh: the same body for the envs marked MW_STACK_FRESH alone, no push — the ring position stays.
extern "C" __global__ __launch_bounds__(MW_STACK_THREADS) void mw_stack_refresh_kernel(MW_STACK_ARGS)
{
    if (wide) stack_env_chunk<uint4, false>(depth, pad, phase, frame_bytes, obs, ring, flags_in, flags_out, nullptr, nullptr, nullptr, nullptr, nullptr);
    else stack_env_chunk<uint8_t, false>(depth, pad, phase, frame_bytes, obs, ring, flags_in, flags_out, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// mw_reset: the envs it writes start a new episode — their stacks are rebuilt by mw_stack_refresh or by their next push; a rebuild
// that a pending next-step auto-reset would have caused goes with the pending reset itself.
extern "C" __global__ void mw_stack_mark_kernel(int N, const uint8_t *__restrict__ mask, int force_all, uint8_t *__restrict__ flags)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N && (force_all || mask[i])) flags[i] = MW_STACK_FRESH;
}

// A frameless mw_step_plan: no push, but episodes begin and end inside the call.  The env's next push rebuilds its stack iff the env
// began an episode since its last push: MW_STACK_FRESH where the call installed a world — same-step: it set term | trunc; next-step:
// the env entered with reset_pending, which its flag byte says (MW_STACK_PENDING: the push, the snapshot loads and this kernel keep
// it in step with reset_pending) —, MW_STACK_PENDING where the call left reset_pending set.  In place: one thread reads and writes
// an env's byte.
extern "C" __global__ void mw_stack_plan_kernel(int N, const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc,
                                                const uint8_t *__restrict__ pending, uint8_t *__restrict__ flags)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    uint8_t fl = flags[i];
    if (term && (term[i] | trunc[i]) != 0) fl = MW_STACK_FRESH;
    if (pending) {
        if (fl & MW_STACK_PENDING) fl = MW_STACK_FRESH;
        if (pending[i]) fl |= MW_STACK_PENDING;
    }
    flags[i] = fl;
}
