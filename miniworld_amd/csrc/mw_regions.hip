// Grid regions on the device (mw_grid_regions, mw_engine_regions.hip; the rule, the arrays and every phase: mw_regions.h).
//
// mw_regions_kernel: one workgroup of MW_REGIONS_THREADS lanes per env; a masked-off env's leaves before any barrier.  Dynamic LDS
// (mwpolicy::regions_launch), sized by the env's cell count: a uint16 label per cell, a uint16 size per cell, an Entry of 24 bytes per
// listed region, a word per lane — 64 + 64 + 6 + 1 KiB at MW_NAV_MAX_CELLS and MW_REGION_MAX, 48 KiB for the Maze's 103 x 103 cells, so
// that three of its workgroups share a CU.  Phases, a barrier between each:
//   1. stage the env's row with mwnav::each_byte (aligned words, peeled ends: the row starts at byte env * gx * gz): a member cell's
//      label is its own index; the sizes and the table start empty
//   2. label: rounds of — a hook pass, a cell per lane: the lowest label among a cell's neighbours goes to the cell its own label
//      names; then passes that take every cell to the label its label names until none moves — until a round changes nothing
//      (__syncthreads_or), at most cells + 1 of them.  Every lane is busy in every pass and a region of any shape settles in a few
//      rounds.  Measured against it and not kept (profiles/r41, tools/experiments/README.md): every row and every column forth and
//      back with a carried label, mw_nav.h's sweeps, with and without the jumps — a lane per line is busy, and a thin diagonal region
//      takes a round per cell: 1.4 to 4.5 times the time on frontier masks and on the cells a field reaches.
//      Every store lowers a label to another of its region (mw_regions.h), so the fixed point does not depend on the schedule.
//   3. sizes at the roots: a stretch of equal labels among kRun consecutive cells is one LDS atomic add into the 32-bit word two sizes
//      share (a size is at most 32768: no carry crosses)
//   4. rank the qualified roots in scan order: every lane counts those among its own consecutive cells, reads the lanes' counts for its
//      first rank and the total, and files its roots — the listed ones into the table, every root's code in place of its size
//   5. the listed regions' sums of rows and columns: a stretch of one region is one atomic add each
//   6. their least distance to size * centroid: a 64-bit LDS atomic minimum per stretch, skipped when a plain read already shows less
//   7. the lowest cell at that distance: a 32-bit atomic minimum from the few cells that are
//   8. the table goes to the caller's rows, every cell's code to its label row
// All of it is integer, minima and sums: nothing depends on the order the atomics arrive in.
// Indices: a cell index is below cells = gx * gz <= MW_NAV_MAX_CELLS (checked before the launch, with the bytes of LDS): the staging and
// every pass run over 0 .. cells - 1 of rows the caller sized [N][gz][gx], a sweep over whole lines with its side lines tested, a label
// is kNone — tested before it is used as an index — or the index of a cell; a region index is below K <= MW_REGION_MAX, the size of a
// row of size, cell and sum; the sizes' last word may reach one element past an odd cell count, inside the rounded allocation.
#include "mw_kernels.h"

extern "C" __global__ __launch_bounds__(MW_REGIONS_THREADS) void mw_regions_kernel(MwNavArgs a, int gx, int gz, int diag, int min_cells, int K,
                                                                                  const uint8_t *__restrict__ mask, const uint8_t *__restrict__ member,
                                                                                  int32_t *__restrict__ count, int32_t *__restrict__ size,
                                                                                  int32_t *__restrict__ cell, int32_t *__restrict__ sum,
                                                                                  int16_t *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t regions_lds[];
    constexpr int T = MW_REGIONS_THREADS;
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (mask && !mask[env]) return;
    const int cells = gx * gz;
    uint8_t *base = reinterpret_cast<uint8_t *>(regions_lds);
    uint16_t *label = regions_lds;
    uint16_t *sizes = reinterpret_cast<uint16_t *>(base + mwregions::label_bytes(cells));
    mwregions::Entry *tab = reinterpret_cast<mwregions::Entry *>(base + 2 * mwregions::label_bytes(cells));
    int32_t *scan = reinterpret_cast<int32_t *>(base + 2 * mwregions::label_bytes(cells) + mwregions::table_bytes(K));

    mwregions::stage(member + env * (size_t)cells, label, sizes, cells, lane, T);
    mwregions::clear_table(tab, K, lane, T);
    __syncthreads();

    const int bound = mwregions::max_rounds(cells);
    int n = 0;
    bool settled = false;
    while (!settled && n < bound) {     // (n and settled are the workgroup's: every lane sees the same barrier results)
        bool changed = mwregions::hook_pass(label, gx, gz, diag != 0, lane, T);
        __syncthreads();
        for (bool moved = true; moved;) {       // (moved is the workgroup's; a pass that moves anything shortens every chain it touches)
            const bool mine = mwregions::jump_pass(label, cells, lane, T);
            changed = changed || mine;
            moved = __syncthreads_or(mine) != 0;
        }
        ++n;
        settled = __syncthreads_or(changed) == 0;
    }

    mwregions::count_sizes(label, sizes, cells, lane, T, [](uint16_t *s, int root, int k) {
        atomicAdd(reinterpret_cast<uint32_t *>(s + (root & ~1)), (uint32_t)k << (16 * (root & 1)));
    });
    __syncthreads();

    scan[lane] = mwregions::count_qualified(label, sizes, cells, min_cells, lane, T);
    __syncthreads();
    int rank = 0, total = 0;
    for (int l = 0; l < T; ++l) {
        const int c = scan[l];
        rank += l < lane ? c : 0;
        total += c;
    }
    mwregions::file_roots(label, sizes, tab, cells, min_cells, K, rank, lane, T);
    __syncthreads();

    mwregions::sum_cells(label, sizes, tab, cells, gx, lane, T, [](int32_t *w, int32_t v) { atomicAdd(w, v); });
    __syncthreads();
    mwregions::least_distance(label, sizes, tab, cells, gx, lane, T, [](unsigned long long *w, unsigned long long d) { atomicMin(w, d); });
    __syncthreads();
    mwregions::lowest_cell(label, sizes, tab, cells, gx, lane, T, [](int32_t *w, int32_t c) { atomicMin(w, c); });
    __syncthreads();

    if (lane == 0) count[env] = total;
    mwregions::write_list(tab, K, size + env * (size_t)K, cell + env * (size_t)K, sum ? sum + env * (size_t)K * 2 : nullptr, lane, T);
    if (out) mwregions::write_labels(label, sizes, out + env * (size_t)cells, cells, lane, T);
}
