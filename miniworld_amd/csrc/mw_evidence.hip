// Scan evidence on the device (mw_scan_evidence, mw_engine_evidence.hip; the rule, the arrays and every phase: mw_evidence.h).
//
// mw_evidence_kernel: one workgroup of MW_EVIDENCE_THREADS lanes per env; a masked-off env's leaves before any barrier.  Dynamic LDS
// (mwpolicy::evidence_launch), sized by the env's cell count and the beams: the counting plane, a 32-bit word per cell (128 KiB at
// MW_NAV_MAX_CELLS), then R + 1 prefix words (16 KiB at MW_RAY_MAX) and mwevid::kTailWords more.  Phases, a barrier between each:
//   0. zero the plane and the tail
//   1. a beam per lane: validate, count its tasks nx + nz into pre[b], add a hit to its end cell's word (an LDS atomic); the lanes' kept
//      beams are summed over each wavefront by a butterfly and over the workgroup by an LDS atomic into the tail
//   2. the exclusive prefix sums of pre in place, as mw_scan.hip makes them (the same function on this workgroup's width)
//   3. lane 0 adds the kept beams to the start cell's word, once; the tasks, dealt flat: lane l takes tasks l, l + lanes, ...; a binary
//      search in pre gives the task's beam, the closed form its one cell, a z task drops itself where the x task of its column names the
//      same cell, an LDS atomic adds the pass.  (MW_EVIDENCE_FORM 2: the lanes of a wavefront that hold the same cell elect one that adds
//      their number — a ballot per distinct cell; measured and not the default: profiles/r48.)
//   4. the resolve: the counts and the env's evidence bytes, by aligned words of four cells, into the new evidence bytes — and each
//      cell's ev' into its LDS word; the four sums over each wavefront by a butterfly and over the workgroup by an LDS atomic each
//   5. the emits, where asked for: the free, the obstacle and the score plane from the LDS words, each along its own 4-byte boundaries;
//      lane 0 writes `count` and `changed`
// An env whose extent the grid does not cover gets its rows zeroed, its counts 0 and MW_ST_DEPTH_BAD, as in mw_scan_kernel.
// Indices: a beam index is below R, so t is read below N * R and dir below N * R * 2; origin at env * 3 and + 2; a cell index comes out
// of mwscan::inside, 0 .. cells - 1, and names one word of the plane; pre is indexed 0 .. R; a task k is below pre[R] <= R * (gx + gz + 3)
// < 2^28; an evidence or score byte is below (env + 1) * cells, a map byte below (env + 1) * 2 * cells of tensors the caller sized
// [N][gz][gx] and [N][2][gz][gx].
#include "mw_kernels.h"

namespace {

// pre[0 .. R) counts -> exclusive prefix sums, pre[R] the total; wave_sum: T / 64 words.  Every lane of the workgroup calls it.
// (mw_scan.hip's, which is written on MW_SCAN_THREADS and stays as it is.)
template <int T>
__device__ inline void prefix_sums(int32_t *pre, int32_t *wave_sum, int R, int lane)
{
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

__device__ inline int wave_sum_of(int v)
{
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

}  // namespace

extern "C" __global__ __launch_bounds__(MW_EVIDENCE_THREADS) void mw_evidence_kernel(MwNavArgs a, mw_nav_params p, double max_range, int R, mwevid::Rule rule,
                                                                                     const double *__restrict__ t, const double *__restrict__ dir,
                                                                                     const double *__restrict__ origin, const uint8_t *__restrict__ mask,
                                                                                     const uint8_t *__restrict__ clear, int8_t *__restrict__ ev,
                                                                                     uint8_t *__restrict__ map, uint8_t *__restrict__ score,
                                                                                     int32_t *__restrict__ count, int32_t *__restrict__ changed)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t evidence_lds[];
    constexpr int T = MW_EVIDENCE_THREADS, first = MW_EVIDENCE_FORM == 1 ? 0 : 1;
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (mask && !mask[env]) return;
    const mwnav::Grid g = mwnav::grid_of(a, p, env);
    const int n = g.gx * g.gz;
    int8_t *ev_row = ev + env * (size_t)n;
    uint8_t *map_rows = map ? map + env * 2 * (size_t)n : nullptr, *score_row = score ? score + env * (size_t)n : nullptr;
    if (!mwnav::covers(g)) {
        mwevid::zero_rows(ev_row, map_rows, score_row, n, lane, T);
        if (lane == 0) {
            count[env * 2] = count[env * 2 + 1] = 0;
            if (changed) changed[env * 2] = changed[env * 2 + 1] = 0;
            atomicOr(a.status, MW_ST_DEPTH_BAD);
        }
        return;
    }
    const int words = (int)(mwevid::count_bytes(n) / 4);
    uint32_t *cnt = evidence_lds;
    int32_t *pre = reinterpret_cast<int32_t *>(evidence_lds + words);
    uint32_t *tail = evidence_lds + words + (R + 1);        // [0 .. 3]: the sums; [4]: the kept beams; [5 ..]: the wavefronts' sums of the prefix
    const mwscan::Scan s{g, origin ? origin[env * 3] : a.ax[env], origin ? origin[env * 3 + 2] : a.az[env], max_range,
                         t + env * (size_t)R, dir + env * (size_t)R * 2, R};

    mwscan::zero_words(cnt, n, lane, T);
    mwscan::zero_words(tail, mwevid::kTailWords, lane, T);
    __syncthreads();
    const int kept = wave_sum_of(mwevid::count_beams(s, cnt, pre, first, lane, T));
    if ((lane & 63) == 0 && kept) atomicAdd(tail + mwevid::kSums, (uint32_t)kept);
    __syncthreads();
    prefix_sums<T>(pre, reinterpret_cast<int32_t *>(tail + mwevid::kSums + 1), R, lane);
    __syncthreads();
    if (lane == 0) mwevid::fold_start(s, cnt, first, (int)tail[mwevid::kSums]);
#if MW_EVIDENCE_FORM == 2
    // every lane of a wavefront arrives here in every round (mwevid::deal_tasks): the lanes with a cell elect, cell by cell, the lowest
    // lane that holds it, and that lane adds how many hold it
    mwevid::deal_tasks(s, pre, first, lane, T, [cnt, lane](int c) {
        unsigned long long todo = __ballot(c >= 0);
        while (todo) {
            const int leader = __ffsll(todo) - 1;
            const int lc = __shfl(c, leader);
            const unsigned long long same = __ballot(c == lc);
            if ((lane & 63) == leader) atomicAdd(cnt + lc, (uint32_t)__popcll(same));
            todo &= ~same;
        }
    });
#else
    mwevid::deal_tasks(s, pre, first, lane, T, [cnt](int c) { if (c >= 0) mwevid::add_count(cnt, c, 1u); });
#endif
    __syncthreads();
    const bool cleared = clear && clear[env];
    mwevid::Sums sums{0, 0, 0, 0};
    mwevid::resolve_plane(cnt, n, cleared, rule, ev_row, sums, lane, T);
    const int nf = wave_sum_of(sums.free), no = wave_sum_of(sums.obstacle), cf = wave_sum_of(sums.changed_free), co = wave_sum_of(sums.changed_obstacle);
    if ((lane & 63) == 0) {
        atomicAdd(tail, (uint32_t)nf);
        atomicAdd(tail + 1, (uint32_t)no);
        atomicAdd(tail + 2, (uint32_t)cf);
        atomicAdd(tail + 3, (uint32_t)co);
    }
    __syncthreads();
    mwevid::emit_planes(cnt, n, rule, map_rows, score_row, lane, T);
    if (lane == 0) {
        count[env * 2] = (int32_t)tail[0];
        count[env * 2 + 1] = (int32_t)tail[1];
        if (changed) {
            changed[env * 2] = (int32_t)tail[2];
            changed[env * 2 + 1] = (int32_t)tail[3];
        }
    }
}
