// Scan maps on the device (mw_scan_project, mw_engine_scan.hip; the rule, the arrays and every phase: mw_scan.h).
//
// mw_scan_kernel: one workgroup of MW_SCAN_THREADS lanes per env; a masked-off env's leaves before any barrier.  Dynamic LDS
// (mwpolicy::scan_launch), sized by the env's cell count and the beams: the free and the obstacle plane, a bit per cell (4 KiB each at
// MW_NAV_MAX_CELLS), then R + 1 prefix words (16 KiB at MW_RAY_MAX) and mwscan::kTailWords more.  Phases, a barrier between each:
//   0. zero the planes and the tail
//   1. a beam per lane: validate, count its tasks 1 + nx + nz into pre[b], OR the obstacle bit of its end cell (an LDS atomic)
//   2. the exclusive prefix sums of pre in place: every lane adds up a run of ceil(R / lanes) consecutive counts, the runs' sums are
//      scanned over each wavefront by shuffles and over the wavefronts through a tail word each, then every lane writes its run back
//   3. the tasks, dealt flat: lane l takes tasks l, l + lanes, ...; a binary search in pre gives the task's beam, the beam is made
//      again from its t and dir (neighbouring lanes mostly share it: the loads coalesce to one line), the closed form gives the task's
//      one cell, an LDS atomic ORs its free bit.  No lane walks a beam: a 0.3 m beam and a 10 m beam cost what they contribute.
//   4. the merge: both planes into the env's bytes by aligned words, free & ~obstacle on the way; the new cells are summed over each
//      wavefront by a butterfly and over the workgroup by an LDS atomic add into the tail; lane 0 writes `newly` and carries `count`
// An env whose extent the grid does not cover gets its rows zeroed, its counts 0 and MW_ST_DEPTH_BAD (mw_depth_project's own bit:
// mw_check's message names the condition).
// Indices: a beam index is below R, so t is read below N * R and dir below N * R * 2; origin at env * 3 and + 2; a cell index comes out
// of mwscan::inside, 0 .. cells - 1, its word below plane_words(cells); pre is indexed 0 .. R; a task k is below pre[R] <=
// R * (gx + gz + 3) < 2^28; a map byte is below (env + 1) * 2 * cells of a tensor the caller sized [N][2][gz][gx].
#include "mw_kernels.h"

namespace {

// pre[0 .. R) counts -> exclusive prefix sums, pre[R] the total; wave_sum: MW_SCAN_THREADS / 64 words.  Every lane of the workgroup calls it.
__device__ inline void prefix_sums(int32_t *pre, int32_t *wave_sum, int R, int lane)
{
    constexpr int T = MW_SCAN_THREADS;
    const int run = (R + T - 1) / T;
    const int b0 = lane * run < R ? lane * run : R, b1 = b0 + run < R ? b0 + run : R;
    int32_t sum = 0;
    for (int b = b0; b < b1; ++b) sum += pre[b];
    int32_t inc = sum;
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t v = __shfl_up(inc, d);
        if ((lane & 63) >= d) inc += v;
    }
    if ((lane & 63) == 63) wave_sum[lane >> 6] = inc;
    __syncthreads();
    int32_t base = inc - sum;
    for (int w = 0; w < (lane >> 6); ++w) base += wave_sum[w];
    for (int b = b0; b < b1; ++b) {
        const int32_t v = pre[b];
        pre[b] = base;
        base += v;
    }
    if (lane == T - 1) pre[R] = base;       // (the last lane's run ends the beams, or is empty behind them)
}

}  // namespace

extern "C" __global__ __launch_bounds__(MW_SCAN_THREADS) void mw_scan_kernel(MwNavArgs a, mw_nav_params p, double max_range, int R,
                                                                             const double *__restrict__ t, const double *__restrict__ dir,
                                                                             const double *__restrict__ origin, const uint8_t *__restrict__ mask,
                                                                             const uint8_t *__restrict__ clear, uint8_t *__restrict__ map,
                                                                             int32_t *__restrict__ count, int32_t *__restrict__ newly)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t scan_lds[];
    constexpr int T = MW_SCAN_THREADS;
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (mask && !mask[env]) return;
    const mwnav::Grid g = mwnav::grid_of(a, p, env);
    const int n = g.gx * g.gz;
    uint8_t *rows = map + env * 2 * (size_t)n;
    if (!mwnav::covers(g)) {
        mwscan::zero_rows(rows, n, lane, T);
        if (lane == 0) {
            count[env * 2] = count[env * 2 + 1] = 0;
            if (newly) newly[env * 2] = newly[env * 2 + 1] = 0;
            atomicOr(a.status, MW_ST_DEPTH_BAD);
        }
        return;
    }
    const int words = (int)(mwscan::plane_bytes(n) / 4);
    uint32_t *free_bits = scan_lds, *obstacle = scan_lds + words;
    int32_t *pre = reinterpret_cast<int32_t *>(scan_lds + 2 * words);
    uint32_t *tail = scan_lds + 2 * words + (R + 1);        // [0], [1]: the new cells; [2 ..]: the wavefronts' sums of the prefix
    const mwscan::Scan s{g, origin ? origin[env * 3] : a.ax[env], origin ? origin[env * 3 + 2] : a.az[env], max_range,
                         t + env * (size_t)R, dir + env * (size_t)R * 2, R};

    mwscan::zero_words(scan_lds, 2 * words, lane, T);
    mwscan::zero_words(tail, mwscan::kTailWords, lane, T);
    __syncthreads();
    mwscan::count_beams(s, obstacle, pre, lane, T);
    __syncthreads();
    prefix_sums(pre, reinterpret_cast<int32_t *>(tail + 2), R, lane);
    __syncthreads();
    mwscan::deal_tasks(s, free_bits, pre, lane, T);
    __syncthreads();
    const bool cleared = clear && clear[env];
    int nf = 0, no = 0;
    mwscan::merge_plane(free_bits, obstacle, n, cleared, rows, nf, lane, T);
    mwscan::merge_plane(obstacle, nullptr, n, cleared, rows + n, no, lane, T);
    for (int m = 32; m >= 1; m >>= 1) {
        nf += __shfl_xor(nf, m);
        no += __shfl_xor(no, m);
    }
    if ((lane & 63) == 0) {
        atomicAdd(tail, (uint32_t)nf);
        atomicAdd(tail + 1, (uint32_t)no);
    }
    __syncthreads();
    if (lane == 0) {
        const int tf = (int)tail[0], to = (int)tail[1];
        count[env * 2] = (cleared ? 0 : count[env * 2]) + tf;
        count[env * 2 + 1] = (cleared ? 0 : count[env * 2 + 1]) + to;
        if (newly) {
            newly[env * 2] = tf;
            newly[env * 2 + 1] = to;
        }
    }
}
