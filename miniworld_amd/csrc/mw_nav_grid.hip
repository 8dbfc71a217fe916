// Grid navigation fields on the device (mw_nav_build_grid, mw_engine_nav.hip; the arithmetic and every phase: mw_nav_grid.h, mw_nav.h).
//
// mw_nav_grid_kernel: mw_nav_build_kernel's shape — one workgroup of MW_NAV_THREADS lanes per env, the env's cost grid in dynamic LDS,
// 2 bytes per cell — with the occupancy, the sources and the cell costs read from the caller's rows.  With extra costs a byte per
// cell follows the grid in LDS (at most 64 + 32 KiB: one workgroup per CU at the largest grids), staged once so that a sweep's loads of
// it are LDS reads ahead of the carried cost like those of the lines beside; read from global memory in the sweep instead, the build
// with extra costs was no faster (4 to 8 % slower, in a variant whose build without them was 1 to 4 % slower: profiles/r38).  A
// masked-off env's workgroup leaves at once.  Phases, a barrier between each:
//   1. stage the env's row of d_blocked (and of d_extra): consecutive lanes consecutive bytes, aligned words with a peeled head and
//      tail (the row starts at byte env * gx * gz)
//   2. inflate, with R > 0: every wavefront walks its share of the cells 64 at a time, and for each raw cell among them — found by a
//      ballot, so the loop is the wavefront's — its lanes share the (2R + 1)^2 offsets of the stencil (mwnav::inflate_from).  The
//      inflated cells carry a reserved value (mw_nav_grid.h says why), which a pass over the grid then folds into 0xFFFF.
//      Scattered, not gathered: a gather reads up to (2R + 1)^2 - 1 cells for every free cell, whatever the density — 48 LDS reads per
//      cell at the default clearance —, the scatter one stencil per raw cell, a few per cent of that on a sensed map.  Measured on
//      depth maps (profiles/r38): with the gather the whole build took 17 to 35 % longer.
//   3. sources: the mask's, then those of the env's point
//   4. relaxation, as mw_nav_build_kernel's: the four sweeps at once over a quarter of the lanes each, or whole-grid passes — the
//      functions of mw_nav.h without extra costs, those of mw_nav_grid.h with
//   5. the fixed point is tested for a cost that did not fit, the grid copied to the caller's row
// Every index into the grid is below gx * gz <= MW_NAV_MAX_CELLS (checked before the launch, with the bytes of LDS): the staging runs
// over 0 .. cells - 1 of rows the caller sized [N][gz][gx], inflate_from tests each neighbour against the grid, mark_sources clamps
// its box, neighbours are tested (mwnav::at), sweeps run over whole lines.
#include "mw_kernels.h"

static_assert(MW_NAV_GRID_THREADS == MW_NAV_THREADS, "mwpolicy::nav_grid_launch states the workgroup this kernel is launched with");

extern "C" __global__ __launch_bounds__(MW_NAV_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void mw_nav_grid_kernel(
    MwNavArgs a, mw_nav_params p, int R, const uint8_t *__restrict__ mask, const uint8_t *__restrict__ blocked, const uint8_t *__restrict__ sources,
    const double *__restrict__ d_target, const uint8_t *__restrict__ extra, uint16_t *__restrict__ field, int32_t *__restrict__ passes)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t f[];
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (mask && !mask[env]) return;
    const int gx = p.gx, gz = p.gz, cells = gx * gz;
    uint8_t *x = (uint8_t *)f + mwnav::grid_field_bytes(cells);
    uint16_t *row = field + env * (size_t)cells;
    mwnav::stage_blocked(blocked + env * (size_t)cells, f, cells, lane, MW_NAV_THREADS);
    if (extra) mwnav::stage_extra(extra + env * (size_t)cells, x, cells, lane, MW_NAV_THREADS);
    __syncthreads();
    if (R > 0) {
        const int wave = lane >> 6, wl = lane & 63;
        for (int base = wave * 64; base < cells; base += MW_NAV_THREADS) {
            const int c = base + wl;
            unsigned long long raw = __ballot(c < cells && f[c] == MW_NAV_BLOCKED);
            while (raw) {
                const int o = base + (int)__builtin_ctzll(raw);
                raw &= raw - 1;
                mwnav::inflate_from(f, gx, gz, o / gx, o % gx, R, p.cell, p.margin, wl, 64);
            }
        }
        __syncthreads();
        mwnav::fold(f, cells, lane, MW_NAV_THREADS);
        __syncthreads();
    }
    if (sources) mwnav::mark_mask_sources(sources + env * (size_t)cells, f, cells, lane, MW_NAV_THREADS);
    if (d_target) mwnav::mark_sources(mwnav::grid_build_grid(a, p, d_target, env), f, mwnav::target_of(a, p, d_target, env), lane, MW_NAV_THREADS);
    __syncthreads();
    const int bound = mwnav::max_passes(gx, gz);
    const bool jacobi = (p.flags & MW_NAV_JACOBI) != 0;
    const int dir = lane / (MW_NAV_THREADS / 4), dl = lane % (MW_NAV_THREADS / 4);
    int n = 0;
    bool settled = false;
    while (!settled && n < bound) {     // (n and settled are the workgroup's: every lane sees the same barrier results)
        bool changed;
        if (extra) changed = jacobi ? mwnav::jacobi_pass_x(f, x, gx, gz, lane, MW_NAV_THREADS) : mwnav::sweep_x(f, x, gx, gz, dir, dl, MW_NAV_THREADS / 4);
        else changed = jacobi ? mwnav::jacobi_pass(f, gx, gz, lane, MW_NAV_THREADS) : mwnav::sweep(f, gx, gz, dir, dl, MW_NAV_THREADS / 4);
        ++n;
        settled = __syncthreads_or(changed) == 0;
    }
    const bool far = __syncthreads_or(mwnav::too_far(f, gx, gz, lane, MW_NAV_THREADS)) != 0;
    const bool bad = !settled || far;
    for (int c = lane; c < cells; c += MW_NAV_THREADS) row[c] = bad ? (uint16_t)MW_NAV_BLOCKED : f[c];
    if (lane == 0) {
        if (bad) atomicOr(a.status, MW_ST_NAV_BAD);
        if (passes) passes[env] = n;
    }
}
