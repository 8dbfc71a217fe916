// Navigation fields on the device (mw_nav_build / mw_nav_query, mw_engine_nav.hip; the arithmetic and every phase: mw_nav.h).
//
// mw_nav_build_kernel: one workgroup of MW_NAV_THREADS lanes per env, the env's cost grid in dynamic LDS (2 bytes per cell, at most
// 64 KiB: two workgroups per CU).  A masked-off env's workgroup leaves at once.  Phases, a barrier between each:
//   1. every cell unreached, or blocked beyond the extent
//   2. occupancy: a wavefront per wall, its lanes over the cells of the wall's inflated bounding box only; then a wavefront per
//      blocking entity.  Plain same-value stores, idempotent in any order.
//   3. sources
//   4. relaxation in LDS until a whole round changes nothing.  Updates only lower a cell, so lanes read each other's newest values.
//      A round is the four directional sweeps at once — lanes 0-127 the rows forward, 128-255 the rows back, 256-383 the columns
//      forward, 384-511 the columns back, each lane carrying its line's cost in a register — or, with MW_NAV_JACOBI, one whole-grid
//      pass of all lanes.  The round count has a hard bound (mwnav::max_passes); reaching it refuses the env.
//   5. the fixed point is tested for a cost that did not fit, then the grid is copied to the caller's row, consecutive lanes
//      consecutive cells.
// Every index into the grid is below gx * gz <= MW_NAV_MAX_CELLS (checked before the launch, with the bytes of LDS): boxes are clamped
// to the grid (mwnav::axis_range), neighbours are tested against it (mwnav::at), sweeps run over whole lines.
#include "mw_kernels.h"

extern "C" __global__ __launch_bounds__(MW_NAV_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void mw_nav_build_kernel(MwNavArgs a, mw_nav_params p, const uint8_t *__restrict__ mask,
                                                                                 const double *__restrict__ d_target, uint16_t *__restrict__ field,
                                                                                 int32_t *__restrict__ passes)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t f[];
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (mask && !mask[env]) return;
    const mwnav::Grid g = mwnav::grid_of(a, p, env);
    const int cells = g.gx * g.gz;
    uint16_t *row = field + env * (size_t)cells;
    if (!mwnav::covers(g)) {
        for (int c = lane; c < cells; c += MW_NAV_THREADS) row[c] = (uint16_t)MW_NAV_BLOCKED;
        if (lane == 0) atomicOr(a.status, MW_ST_NAV_BAD);
        return;
    }
    mwnav::init_cells(g, f, false, lane, MW_NAV_THREADS);
    __syncthreads();
    {
        const int wave = lane >> 6, wl = lane & 63;
        const double *segs = mwnav::segs_of(a, env);
        const int ns = mwnav::nsegs_of(a, env);
        for (int s = wave; s < ns; s += MW_NAV_THREADS / 64) mwnav::block_seg(g, f, segs + (size_t)s * 4, a.agent_radius + p.margin, wl, 64);
        for (int s = wave; s < a.E; s += MW_NAV_THREADS / 64)
            if (mwnav::slot_blocks(a, p, d_target == nullptr, env, s))
                mwnav::block_ent(g, f, mwnav::ent_pos(a, env, s, 0), mwnav::ent_pos(a, env, s, 2), a.agent_radius + mwnav::ent_radius(a, env, s) + p.margin, wl, 64);
    }
    __syncthreads();
    mwnav::mark_sources(g, f, mwnav::target_of(a, p, d_target, env), lane, MW_NAV_THREADS);
    __syncthreads();
    const int bound = mwnav::max_passes(g.gx, g.gz);
    const bool jacobi = (p.flags & MW_NAV_JACOBI) != 0;
    int n = 0;
    bool settled = false;
    while (!settled && n < bound) {     // (n and settled are the workgroup's: every lane sees the same barrier results)
        const bool changed = jacobi ? mwnav::jacobi_pass(f, g.gx, g.gz, lane, MW_NAV_THREADS)
                                    : mwnav::sweep(f, g.gx, g.gz, lane / (MW_NAV_THREADS / 4), lane % (MW_NAV_THREADS / 4), MW_NAV_THREADS / 4);
        ++n;
        settled = __syncthreads_or(changed) == 0;
    }
    const bool far = __syncthreads_or(mwnav::too_far(f, g.gx, g.gz, lane, MW_NAV_THREADS)) != 0;
    const bool bad = !settled || far;
    for (int c = lane; c < cells; c += MW_NAV_THREADS) row[c] = bad ? (uint16_t)MW_NAV_BLOCKED : f[c];
    if (lane == 0) {
        if (bad) atomicOr(a.status, MW_ST_NAV_BAD);
        if (passes) passes[env] = n;
    }
}

// mw_nav_query: a lane per env; reads the field, the extent, the target (not with MW_NAV_GRID) and the position, writes the three outputs that are asked for
extern "C" __global__ __launch_bounds__(MW_NAV_QUERY_THREADS) void mw_nav_query_kernel(MwNavArgs a, mw_nav_params p, const double *__restrict__ d_target,
                                                                                       const uint16_t *__restrict__ field, const double *__restrict__ pos,
                                                                                       int32_t *__restrict__ cost, int32_t *__restrict__ next,
                                                                                       double *__restrict__ waypoint)
{
    const size_t env = (size_t)blockIdx.x * MW_NAV_QUERY_THREADS + threadIdx.x;
    if (env >= (size_t)a.N) return;
    const mwnav::Grid g = mwnav::grid_of(a, p, env);
    const double x = pos ? pos[env * 3] : a.ax[env], z = pos ? pos[env * 3 + 2] : a.az[env];
    const uint16_t *f = field + env * (size_t)(g.gx * g.gz);
    // (a grid field, mw_nav_build_grid's, has no target to read: at cost 0 the cell's own centre)
    const mwnav::Answer r = (p.flags & MW_NAV_GRID) ? mwnav::query_grid(g, f, x, z) : mwnav::query(g, f, mwnav::target_of(a, p, d_target, env), x, z);
    if (cost) cost[env] = r.cost;
    if (next) next[env] = r.next;
    if (waypoint) { waypoint[env * 2] = r.wx; waypoint[env * 2 + 1] = r.wz; }
}
