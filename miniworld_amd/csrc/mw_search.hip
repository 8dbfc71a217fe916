// Scan search on the device (mw_scan_search, mw_engine_search.hip; the rule, the arrays, the key and every phase: mw_search.h).
//
// mw_search_kernel: one workgroup of MW_SEARCH_THREADS lanes, four wavefronts, per env; a masked-off env's leaves before any barrier, and so
// does one of an env the grid does not cover: both conditions are the env's, uniform over its workgroup.  Dynamic LDS
// (mwpolicy::search_launch): the score plane, a byte per cell; the bound plane, (gz + 7) x (gx + 7) bytes; `batch` end-cell lists of R
// words; a bound word per block of the batch; a fill word per rotation; the tail (ticket, refined count, best key, first key).  Phases:
//   0. stage the plane by aligned words of the caller's row, zero the fill words and the tail; barrier
//   1. the bound plane: the 8-maximum along the rows, an element per lane; barrier; down the columns in place, a column per lane
//   r0. per batch of rotations r0 .. r0 + nb - 1, three barriers:
//      a. lane 0 clears the ticket and the first key; every lane lists the batch's end cells, a beam per lane per rotation, compacted
//         through the LDS counters fill[r]; barrier (it also ends phase 1, and the previous batch's refinement)
//      b. the bounds, a block per lane: one sum over the rotation's list of bytes of the bound plane — a list entry is one LDS word the
//         lanes read together, the bytes of adjacent blocks lie 8 apart —; each lane's greatest goes into the first key by one LDS
//         atomicMax; barrier
//      c. the refinement, a block per wavefront: tickets from the LDS counter, the block of the greatest bound first; a block whose
//         bound lies below the best score (the high bits of the best key, read where it stands) is skipped, the others are scored, a
//         translation per lane — the 64 bytes of an end cell are eight runs of eight —, folded by a butterfly max and one 64-bit LDS
//         atomicMax per block; barrier
//   K. lane 0 decodes best and score and writes the stats: the blocks refined, K * blocks.
// An env whose extent the grid does not cover gets zeros and MW_ST_DEPTH_BAD (mw_scan_match's own bit there).
// Indices: t, dir, origin, the score row and the staged plane as in mw_match.hip.  The bound plane is written at (y + 7) * (gx + 7) + x + 7
// with y < gz and x < gx, below (gz + 7) * (gx + 7), and read in bound_blocks only after both unsigned compares (mw_search.h).  List g starts
// at g * R < batch * R words and holds at most R entries at fill[r]'s old value, r < K <= MW_MATCH_MAX_ROT fill words; a task k is below
// nb * blocks <= batch * blocks bound words: ticket 0 and ticket `first` swap, and first < nb * blocks because it is the index of a task
// bound_blocks visited (task 0 always exists).  A lookup's row * gx + col is formed only after 0 <= row < gz and 0 <= col < gx.  best at
// env * 3 + 0 .. 2, best_score at env, stats at env * 2 + 0 .. 1.
#include "mw_kernels.h"

extern "C" __global__ __launch_bounds__(MW_SEARCH_THREADS) void mw_search_kernel(MwNavArgs a, mw_nav_params p, double max_range, int R, MwMatchRot rot, int W, int batch,
                                                                                 int prune, const uint8_t *__restrict__ score, const double *__restrict__ t,
                                                                                 const double *__restrict__ dir, const double *__restrict__ origin,
                                                                                 const uint8_t *__restrict__ mask, int32_t *__restrict__ best,
                                                                                 int32_t *__restrict__ best_score, int32_t *__restrict__ stats)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t search_lds[];
    constexpr int T = MW_SEARCH_THREADS;
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (mask && !mask[env]) return;
    const mwnav::Grid g = mwnav::grid_of(a, p, env);
    const int n = g.gx * g.gz, K = rot.n;
    int32_t *st = stats ? stats + env * 2 : nullptr;
    if (!mwnav::covers(g)) {
        mwsearch::write_none(best + env * 3, best_score + env, st, lane);
        if (lane == 0) atomicOr(a.status, MW_ST_DEPTH_BAD);
        return;
    }
    uint8_t *plane = search_lds, *M = plane + mwsearch::plane_bytes(n);
    uint32_t *ends = reinterpret_cast<uint32_t *>(M + mwsearch::bound_bytes(g.gz, g.gx));
    uint32_t *words = ends + mwsearch::ends_bytes(R, batch) / 4;
    uint32_t *fill = words + mwsearch::words_bytes(W, batch) / 4;
    uint32_t *work = fill + MW_MATCH_MAX_ROT;
    unsigned long long *top = reinterpret_cast<unsigned long long *>(work + 2), *first = top + 1;
    const mwmatch::Match m{g, origin ? origin[env * 3] : a.ax[env], origin ? origin[env * 3 + 2] : a.az[env], max_range,
                           t + env * (size_t)R, dir + env * (size_t)R * 2, R, W};

    mwmatch::stage(score + env * (size_t)n, plane, n, false, lane, T);
    for (int k = lane; k < MW_MATCH_MAX_ROT + mwsearch::kTailBytes / 4; k += T) fill[k] = 0u;
    __syncthreads();
    mwsearch::bound_rows(plane, g.gx, g.gz, M, lane, T);
    __syncthreads();
    mwsearch::bound_cols(M, g.gx, g.gz, lane, T);
    for (int r0 = 0; r0 < K; r0 += batch) {
        const int nb = K - r0 < batch ? K - r0 : batch;
        if (lane == 0) {
            work[0] = 0u;
            *first = 0ull;
        }
        for (int i = 0; i < nb; ++i) mwmatch::list_ends(m, rot.cs[r0 + i][0], rot.cs[r0 + i][1], ends + (size_t)i * R, fill + r0 + i, lane, T);
        __syncthreads();
        const uint64_t mine = mwsearch::bound_blocks(M, g.gx, g.gz, W, r0, nb, ends, R, fill, words, lane, T);
        if (mine) atomicMax(first, (unsigned long long)mine);
        __syncthreads();
        mwsearch::refine(plane, g.gx, g.gz, W, r0, nb, ends, R, fill, words, 0xFFFFFFFFu - (uint32_t)*first, work, top, prune != 0, lane);
        __syncthreads();
    }
    if (lane == 0) {
        mwsearch::decode((uint64_t)*top, W, best + env * 3, best_score + env);
        if (st) {
            st[0] = (int32_t)work[1];
            st[1] = K * mwsearch::blocks(W);
        }
    }
}
