// mw_reset_kernel — batched MiniWorldEnv.reset (miniworld.py:544-604): one thread per env, or one wavefront per
// env for the Maze generator (its 127 rooms are emitted one per lane; grid = N blocks then).
#include "mw_gen.h"
#include "mw_kernels.h"

extern "C" __global__ __launch_bounds__(64) void MW_KERNEL_NAME(mw_reset)(MwArgs a, const uint8_t *__restrict__ mask, int force_all, int mark_refill)
{
    __shared__ unsigned char ws[64][MW_GEN_WS_BYTES];
    const bool wave_per_env = a.generator == MW_GEN_MAZE;
    const int env = wave_per_env ? (int)blockIdx.x : (int)(blockIdx.x * 64 + threadIdx.x);
    if (env >= a.N) return;
    if (!force_all && !mask[env]) return;
    mw::generate_world(*a.gen_live, env, wave_per_env ? ws[0] : ws[threadIdx.x], wave_per_env ? (int)threadIdx.x : 0);
    if (!wave_per_env || threadIdx.x == 0) {
        if (mark_refill) a.refill_mask[env] = 1u;      // spare mode: its spare is stale now
        a.reset_pending[env] = 0;       // the new world replaces a pending next-step auto-reset
        a.pending_remove[env] = -1;     // ... and nothing has "just left" its entity list (the old episode's last pickup, K1's frame_clean)
        a.fc_epoch[env] += 1u;          // ... and no cached frame of the old one shows it (MwArgs::fc_epoch)
    }
}

// spare mode: regenerate every consumed spare now (mw_reset needs them current); grid like K1's refill blocks
extern "C" __global__ __launch_bounds__(64) void MW_KERNEL_NAME(mw_refill)(MwArgs a)
{
    __shared__ unsigned char refill_ws[MW_GEN_WS_BYTES];
    mw::refill_spares(a, (int)blockIdx.x, (int)threadIdx.x, refill_ws);
}

// CollectHealth: the kit consumed by this step respawns after its frame was set up (collecthealth.py:86-90), with
// place_entity's draws from the env's stream; one thread per env, launched behind the geometry kernel
extern "C" __global__ __launch_bounds__(64) void MW_KERNEL_NAME(mw_collect_respawn)(MwArgs a)
{
    const int env = (int)(blockIdx.x * 64 + threadIdx.x);
    if (env >= a.N) return;
    const int rs = a.pending_remove[env];
    if (rs < 0) return;
    mw::collect_respawn(a, env, a.shared_geom ? 0 : env, rs, a.ax[env], a.az[env]);
    a.pending_remove[env] = -1;
}

// Same-step auto-reset with final observations, between the two passes of the step (mw_engine_frame.hip): the listed envs (int32
// [0] count, [1 + i] env: the ones whose episode ended with this step, whose terminal frame was drawn) install their next world
// through the same install code as the step kernel's, and leave nothing of the finished episode behind: no pending removal (a
// picked object, CollectHealth's consumed kit), no pending next-step reset, no frame_clean byte.  One wavefront per list slot; grid N.
extern "C" __global__ __launch_bounds__(64) void MW_KERNEL_NAME(mw_final_install)(MwArgs a, const int32_t *__restrict__ list)
{
    __shared__ unsigned char gen_ws[MW_GEN_WS_BYTES];
    __shared__ int s_claim;
    if ((int)blockIdx.x >= list[0]) return;
    const int env = list[1 + blockIdx.x], lane = (int)threadIdx.x;
    mw::install_next_world<false>(a, env, lane, gen_ws, &s_claim);
    if (lane == 0) {
        a.pending_remove[env] = -1;
        a.reset_pending[env] = 0;
        a.frame_clean[env] = 0;         // (K1 ran as a terminal step and may have found the finished episode's last frame unchanged)
        a.fc_epoch[env] += 1u;          // (a world installed: MwArgs::fc_epoch)
    }
}

// mw_reset_where: mw_reset(mask, seeds) with both arrays on the device — every masked env's stream becomes the stream of its seed
// (mw_rng.h: the host's own seeding arithmetic) and its live world is generated from it, as by mw_reset_kernel with mark_refill; the
// grid is that kernel's.  seeds[env] is not read under a zero mask byte.  MW_GEN_NONE: the stream alone.
extern "C" __global__ __launch_bounds__(64) void MW_KERNEL_NAME(mw_reset_where)(MwArgs a, const uint8_t *__restrict__ mask, const uint64_t *__restrict__ seeds)
{
    __shared__ unsigned char ws[64][MW_GEN_WS_BYTES];
    const bool wave_per_env = a.generator == MW_GEN_MAZE;
    const int env = wave_per_env ? (int)blockIdx.x : (int)(blockIdx.x * 64 + threadIdx.x);
    if (env >= a.N || !mask[env]) return;
    if (!wave_per_env || threadIdx.x == 0) mw::rng_seed_store(a.rng, a.N, env, seeds[env]);
    if (a.generator == MW_GEN_NONE) return;
    if (wave_per_env) {         // (the env's 64 lanes all load the stream lane 0 stored; the whole workgroup is here)
        __threadfence_block();
        __syncthreads();
    }
    mw::generate_world(*a.gen_live, env, wave_per_env ? ws[0] : ws[threadIdx.x], wave_per_env ? (int)threadIdx.x : 0);
    if (!wave_per_env || threadIdx.x == 0) {
        if (a.refill_mask) a.refill_mask[env] = 1u;     // spare mode: its spare is stale now
        a.reset_pending[env] = 0;
        a.pending_remove[env] = -1;     // (as mw_reset_kernel: the old episode's removal is not the new world's)
        a.fc_epoch[env] += 1u;
    }
}

// Same-step auto-reset from chosen seeds (mw_set_reset_seeds), between the two passes of the step in mw_final_install_kernel's place:
// the listed envs — and no other: next_seed[env] is read for them alone — start the episode of their seed, and leave behind what that
// kernel leaves behind.  (fc_source: the list pass draws the env's row, whatever the first pass did with it.)
extern "C" __global__ __launch_bounds__(64) void MW_KERNEL_NAME(mw_seed_install)(MwArgs a, const int32_t *__restrict__ list, const uint64_t *__restrict__ next_seed)
{
    __shared__ unsigned char gen_ws[MW_GEN_WS_BYTES];
    if ((int)blockIdx.x >= list[0]) return;
    const int env = list[1 + blockIdx.x], lane = (int)threadIdx.x;
    mw::install_seeded_world(a, env, lane, gen_ws, next_seed[env]);
    if (lane == 0) {
        a.pending_remove[env] = -1;
        a.reset_pending[env] = 0;
        a.frame_clean[env] = 0;
        a.fc_epoch[env] += 1u;
        a.fc_source[env] = 0;
    }
}

#if MW_RNG_KIND == 0
// mw_reset without seeds in spare mode: the masked envs take their pre-generated world (one wavefront per env)
extern "C" __global__ __launch_bounds__(64) void mw_take_spare_kernel(MwArgs a, const uint8_t *__restrict__ mask, int force_all)
{
    const int env = blockIdx.x;
    if (env >= a.N) return;
    if (!force_all && !mask[env]) return;
    mw::take_spare(a, env, (int)threadIdx.x);
    if (threadIdx.x == 0) { a.refill_mask[env] = 1u; a.reset_pending[env] = 0; a.pending_remove[env] = -1; a.fc_epoch[env] += 1u; }
}
#endif
