// Grid rollouts on the device (mw_grid_plan, mw_engine_gridplan.hip; the rule, the plane and the plan's loop: mw_gridplan.h; the launch:
// mwpolicy::gridplan_launch).
//
// mw_gridplan_kernel, a plan per lane: a workgroup of min(256, P rounded up to 64) lanes per (env, block of plans) — 32 plans are one
//   wavefront per env, 4096 are 16 workgroups of an env, which share its planes through L2.  A masked-off env's workgroups leave before
//   any barrier.  Dynamic LDS: the env's obstacle plane as a bit per cell inside its ring (mwgplan::plane_bytes, at most 12.3 KiB),
//   zeroed, then staged from the bytes — 4 at a time where the row's alignment allows, an LDS atomic or per opaque byte — between two
//   barriers; an env the grid does not cover stages nothing (the env's, so the workgroup's: every lane meets the barriers or none).
//   Then each lane runs its plan (mwgplan::run) with no further barrier: MW_GPLAN_AHEAD actions are loaded into registers before the
//   first of them is executed — lane p reads d_plans[k][env][p], so a wavefront's load is one row of 64 consecutive elements, a quarter
//   of the bytes in the uint8 form —, the sine and cosine are evaluated only by a lane whose heading changed since its last move, the
//   refusal test reads LDS alone and does float arithmetic only for set bits, and the field and the cost plane are read in global
//   memory, once per accepted move (a turn stays in its cell).  A lane whose plan stopped leaves the loop unless it has trace rows to
//   repeat.  The lanes past P of the last block stage and then leave.
// Indices: p < P, so plans are read below T * N * P, pose_out written below N * P * 3, stats below N * P * 5, trace below T * N * P * 3;
// pose and step are read at env * 3 .. + 2.  A flat cell index is built only from floors compared, as doubles, against 0 and gx, gz: it
// lies in 0 .. cells - 1 of the env's own row of field / extra / opaque, tensors the caller sized [N][gz][gx].  A bit index is
// mwgplan::bit_of of a row in -1 .. gz and a column in -1 .. gx, below (gx + 2) * (gz + 2), and the word behind it is the spare one.
#include "mw_kernels.h"

extern "C" __global__ __launch_bounds__(MW_GPLAN_THREADS) void mw_gridplan_kernel(MwRayArgs a, mw_nav_params p, mwgplan::Call q,
                                                                                  const uint8_t *__restrict__ mask, const uint8_t *__restrict__ opaque,
                                                                                  const void *__restrict__ plans, const double *__restrict__ pose,
                                                                                  const double *__restrict__ step, const uint16_t *__restrict__ field,
                                                                                  const uint8_t *__restrict__ extra, double *__restrict__ pose_out,
                                                                                  int32_t *__restrict__ stats, double *__restrict__ trace)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t gridplan_bits[];
    const int threads = (int)blockDim.x, lane = (int)threadIdx.x;
    const unsigned per_env = ((unsigned)q.P + (unsigned)threads - 1u) / (unsigned)threads;
    const size_t env = blockIdx.x / per_env;
    const size_t plan = (size_t)(blockIdx.x % per_env) * (size_t)threads + (size_t)lane;
    if (mask && !mask[env]) return;
    const mwgplan::Env e = mwgplan::env_of(a.w, p, q, step, env);
    const size_t cells = (size_t)e.g.gx * (size_t)e.g.gz;
    if (!e.covered) {
        if (lane == 0) atomicOr(a.w.status, MW_ST_DEPTH_BAD);
    } else {
        mwgplan::zero_plane(gridplan_bits, e.g.gx, e.g.gz, lane, threads);
        __syncthreads();
        mwgplan::stage_plane(opaque + env * cells, gridplan_bits, e.g.gx, e.g.gz, e.outside, lane, threads, [](uint32_t *word, uint32_t bit) { atomicOr(word, bit); });
        __syncthreads();
    }
    if (plan >= (size_t)q.P) return;
    const double x = pose ? pose[env * 3] : a.w.ax[env], z = pose ? pose[env * 3 + 1] : a.w.az[env], dir = pose ? pose[env * 3 + 2] : a.adir[env];
    mwgplan::run(e, q, (size_t)a.w.N, gridplan_bits, plans, env, plan, x, z, dir, field ? field + env * cells : nullptr, extra ? extra + env * cells : nullptr,
                 pose_out, stats, trace);
}
