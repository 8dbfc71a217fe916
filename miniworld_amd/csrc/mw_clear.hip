// Grid clearance on the device (mw_grid_clearance, mw_engine_clear.hip; the rule, the array and every phase: mw_clear.h).
//
// mw_clear_kernel: one workgroup of MW_CLEAR_THREADS lanes per env; a masked-off env's leaves before any barrier.  Dynamic LDS
// (mwpolicy::clear_launch), sized by the env's cell count: one int16 per cell and nothing else — 64 KiB at MW_NAV_MAX_CELLS, 21 KiB for
// the Maze's 103 x 103 cells, so that seven of its workgroups share a CU's 160 KiB.  Phases, a barrier between each:
//   1. stage the env's row with mwnav::each_byte (aligned words, peeled ends: the row starts at byte env * gx * gz): 0 on a marked cell,
//      kNoOff elsewhere.  The barrier is __syncthreads_or of "I saw a marked cell": an env without one writes its sentinels and is done.
//   2. the column pass, a lane per column: one walk down, one up, leave each cell's signed row offset to the nearest marked cell of its
//      own column, the upper one at a tie.  Consecutive lanes touch consecutive int16s: two lanes per bank, the least a 16-bit array has.
//   3. the row pass, a cell per lane, consecutive lanes consecutive cells: from its own column's offset outwards over the offsets of
//      its row, d = 1, 2, ..., the least d^2 + dj^2 and at equal values the lowest index, until d^2 > best, the row's ends or the
//      limit.  No stack, no scratch; neighbouring lanes read neighbouring addresses; with walls about the scan is a few cells long.
//      The lane writes dist2, nearest and the band's cost byte — the bands are in the argument struct, compared as integers —
//      straight to the caller's rows.
// All of it is integer and every cell's result is a minimum the rule defines: nothing depends on the schedule.
// Indices: every LDS index is j * gx + i' with 0 <= j < gz and 0 <= i' < gx (the scan tests i - d >= 0 and i + d < gx), below cells =
// gx * gz <= MW_NAV_MAX_CELLS (checked before the launch, with the bytes of LDS); the staging and the outputs run over 0 .. cells - 1 of
// rows the caller sized [N][gz][gx]; |dj| < gz <= 32768 fits an int16 beside kNoOff = -32768; d < gx, so d^2 + dj^2 < 2^31; a nearest
// index (j + dj) * gx + i' names a marked cell of the grid; limit * limit < 2^30 (mwclear::bounded_limit, at the entry point).
#include "mw_kernels.h"

extern "C" __global__ __launch_bounds__(MW_CLEAR_THREADS) void mw_clear_kernel(MwNavArgs a, int gx, int gz, int limit, MwClearBands bands,
                                                                              const uint8_t *__restrict__ mask, const uint8_t *__restrict__ marked,
                                                                              int32_t *__restrict__ dist2, int32_t *__restrict__ nearest,
                                                                              uint8_t *__restrict__ cost)
{
    extern __shared__ __attribute__((aligned(16))) int16_t clear_lds[];
    constexpr int T = MW_CLEAR_THREADS;
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (mask && !mask[env]) return;
    const int cells = gx * gz;
    const size_t row = env * (size_t)cells;
    int32_t *near_row = nearest ? nearest + row : nullptr;
    uint8_t *cost_row = cost ? cost + row : nullptr;

    const bool mine = mwclear::stage(marked + row, clear_lds, cells, lane, T);
    if (!__syncthreads_or(mine)) {          // (the workgroup's: every lane sees the same barrier result)
        mwclear::write_none(cells, dist2 + row, near_row, cost_row, lane, T);
        return;
    }
    mwclear::column_pass(clear_lds, gx, gz, lane, T);
    __syncthreads();
    mwclear::row_pass(clear_lds, gx, gz, limit, bands, dist2 + row, near_row, cost_row, lane, T);
}
