// State views on the device: mw_get_state_device's gather of the envs' state into the caller's rows and mw_set_state_where's masked
// scatter of rows into the engine (mw_engine.hip; the index arithmetic: mw_state_view.h).  One wavefront per env, MW_SV_THREADS lanes
// per workgroup: the lanes stride over the elements of each of the env's rows, so the caller's side is contiguous per env; the
// engine's side is strided by N, where the neighbouring envs of the workgroup and of the next ones share sectors.  No LDS, no scratch.
#include "mw_kernels.h"

// mw_get_state_device: rows `item` = env - first_env of every non-null field := the env's live state.  Reads only.
extern "C" __global__ __launch_bounds__(MW_SV_THREADS) void mw_state_get_kernel(MwStateArrays a, mw_state_view v, int N, int E, int first_env, int count)
{
    const int lane = (int)threadIdx.x & 63;
    const int item = (int)blockIdx.x * MW_SV_ENVS + ((int)threadIdx.x >> 6);
    if (item >= count) return;
    mwsv::gather_env(a, v, E, (size_t)N, (size_t)first_env + (size_t)item, (size_t)item, lane, 64);
}

// mw_set_state_where: for every env under the mask, row `env` of every non-null field into the engine's state, then what the env is
// owed (mw_engine.hip).  Nothing of an unmasked env's rows is read.  A masked env whose carried slot or one of whose entity kinds is
// out of range is skipped whole — the test comes before the first store, a ballot makes it the wavefront's — and sets MW_ST_STATE_BAD.
extern "C" __global__ __launch_bounds__(MW_SV_THREADS) void mw_state_set_where_kernel(MwStateArrays a, mw_state_view v, const uint8_t *__restrict__ mask,
                                                                                      int N, int E, uint32_t *__restrict__ status,
                                                                                      uint8_t *__restrict__ reset_pending, uint8_t *__restrict__ frame_clean,
                                                                                      uint32_t *__restrict__ fc_epoch, uint8_t *__restrict__ stack_flags)
{
    const int lane = (int)threadIdx.x & 63;
    const int env = (int)blockIdx.x * MW_SV_ENVS + ((int)threadIdx.x >> 6);
    if (env >= N) return;
    if (!mask[env]) return;
    bool bad = false;
    if (v.ent_kind && lane < E) bad = !mwsv::kind_ok(v.ent_kind[(size_t)env * (size_t)E + (size_t)lane]);       // (E <= 64: a lane per slot)
    if (v.carrying && lane == 0) bad = bad || !mwsv::carrying_ok(v.carrying[env], E);
    if (__ballot(bad) != 0ull) {
        if (lane == 0) atomicOr(status, MW_ST_STATE_BAD);
        return;
    }
    mwsv::scatter_env(a, v, E, (size_t)N, (size_t)env, (size_t)env, lane, 64);
    if (lane == 0) {
        // a state written from outside replaces whatever a pending next-step reset would have installed, and with it the rebuild of
        // the env's frame stack that reset would have caused (mw_set_state's rule); the env's frame is no longer the one in d_obs,
        // and no cached frame of it may match again (the epoch is part of a frame's key, MwArgs::fc_epoch)
        reset_pending[env] = 0;
        frame_clean[env] = 0;
        fc_epoch[env] += 1u;
        if (stack_flags) stack_flags[env] = (uint8_t)(stack_flags[env] & ~MW_STACK_PENDING);
    }
}
