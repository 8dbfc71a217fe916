// Scan search (mw_scan_search, include/mwengine.h; kernel: mw_search.hip): mw_scan_match's answer over a window of up to
// MW_SEARCH_MAX_WINDOW cells either way, by branch and bound — Olson's multi-resolution search with one coarse level, Cartographer's
// branch and bound cut to depth one.  The translations of a rotation are cut into blocks of 8 x 8; a block's BOUND, one sum over the
// rotation's end cells of an 8 x 8 maximum of the plane, is at least every score in the block, and a block whose bound lies below the
// best score found so far holds no winner and is skipped.  Plain C++ like mw_match.h: the kernel calls these functions with (lane, stride)
// of a workgroup, tests/hostcheck/grid_search.cpp calls search_one on the host, which runs the same phases with (0, 1).
//
// The rule is mw_scan_match's (mw_match.h states it; mwmatch::end_of and list_ends are used as they are): the same end cells, the same
// counting test, the same sums, the same order of ties.  Only the key is wider, because the window is.
//
// The arrays (LDS in the kernel, the caller's on the host):
//   plane   the env's score bytes as they are, a byte per cell, unpadded (mwmatch::stage's byte form)
//   M       the bound plane, (gz + 7) x (gx + 7) bytes: M[y][x] for y in -7 .. gz - 1, x in -7 .. gx - 1, stored at [(y + 7)][(x + 7)], is the
//           maximum of plane0[y .. y + 7][x .. x + 7] with plane0 zero outside the grid.  Built by two passes: along the rows into the
//           rows 7 .. gz + 6 of M itself, then down the columns in place (bound_cols says why that is safe).
//   ends    `batch` lists of R words, the end cells of the batch's rotations as mwmatch::list_ends packs them: (row + W) << 16 | (col + W)
//   fill    a word per rotation: how many entries its list holds
//   words   a word per block of the batch: its bound
//   work    two words: the next ticket of the batch's task list; the blocks refined so far in the call
//   top     one 64-bit word: the best candidate so far
//   first   one 64-bit word: the batch's block of the highest bound, bound << 32 | ~task — it is refined first, so that the best rises early
// A block: anchor (b0, a0) = (-W + 8 j, -W + 8 i), i, j in 0 .. ceil((2 W + 1) / 8) - 1; its translations are b0 .. b0 + 7 x a0 .. a0 + 7
// cut at W (the last row and column of blocks are partial unless 2 W + 1 is a multiple of 8).  Its bound is the sum over the list of
// M[row + b0][col + a0], 0 where that lies outside M: M covers the cells row + b0 .. + 7, col + a0 .. + 7 that every translation of the block —
// a partial one's too — reads, so the bound is at least each of its scores.  It is at most 4096 * 255 < 2^20.
// A candidate's key: score << 39 | ~((a^2 + b^2) << 23 | flat) in the low 39 bits, flat = (r * side + b + W) * side + a + W with side =
// 2 W + 1.  flat < 64 * 257 * 257 < 2^23, a^2 + b^2 <= 32768 < 2^16, score < 2^20: the fields do not meet, the key is below 2^59, and the
// greatest key is the rule's best, as mw_match.h's is.  No candidate's key is 0.
// Why the schedule does not matter: the best score only grows.  A block is skipped iff its bound < the best score read at that moment,
// which is at most the final best score: every score in the block is below the final one, so the block holds no candidate the final
// maximum could be — not even a tie.  A bound equal to the best is refined: the tie rank may be better.  A stale read of `top` is a
// lower one: it prunes less, never more.  So best and score are the brute-force ones for any order of blocks and any number of workers;
// only work[1], the count of refined blocks, depends on the schedule.
#pragma once
#include "mw_match.h"

#ifndef MW_SEARCH_THREADS
#define MW_SEARCH_THREADS 256           // lanes of mw_search_kernel's workgroup, a multiple of 64
#endif

namespace mwsearch {

constexpr int kBlock = 8;               // a block's side; a wavefront of 64 lanes refines one
constexpr int kTailBytes = 32;          // behind the fill words: work[2], then top and first, 8-aligned
constexpr int kBoundWords = 2048;       // the most bound words a batch holds, unless one rotation alone has more

MW_HD int blocks_side(int W) { return (2 * W + 1 + kBlock - 1) / kBlock; }
MW_HD int blocks(int W) { return blocks_side(W) * blocks_side(W); }
// the bytes of the staged plane, of the bound plane, of the batch's lists, of its bound words and of the fill words with the tail, each rounded up to 16
MW_HD size_t plane_bytes(long long cells) { return mwmatch::plane_bytes(cells, false); }
MW_HD size_t bound_bytes(int gz, int gx) { return ((size_t)(gz + kBlock - 1) * (size_t)(gx + kBlock - 1) + 15) / 16 * 16; }
MW_HD size_t ends_bytes(int rays, int batch) { return ((size_t)batch * (size_t)rays * 4 + 15) / 16 * 16; }
MW_HD size_t words_bytes(int W, int batch) { return ((size_t)batch * (size_t)blocks(W) * 4 + 15) / 16 * 16; }
MW_HD size_t fill_bytes() { return (size_t)MW_MATCH_MAX_ROT * 4 + kTailBytes; }

MW_HD uint64_t key_of(int32_t score, int r, int b, int a, int W)
{
    const int side = 2 * W + 1;
    const uint64_t rank = (uint64_t)(a * a + b * b) << 23 | (uint64_t)((r * side + b + W) * side + a + W);
    return (uint64_t)score << 39 | (~rank & 0x7FFFFFFFFFull);
}
// best[3] = (r, a, b) and the score of a key
MW_HD void decode(uint64_t key, int W, int32_t *best, int32_t *best_score)
{
    const int side = 2 * W + 1, flat = (int)(~key & 0x7FFFFFull);
    best[0] = flat / (side * side);
    best[1] = flat % side - W;
    best[2] = flat / side % side - W;
    *best_score = (int32_t)(key >> 39);
}

// ---- the bound plane ---------------------------------------------------------------------------------------------------------------------
// pass 1, an element per worker: the maximum along the row, H[y][x] = max plane[y][x .. x + 7] cut to the grid, for y in 0 .. gz - 1 and
// x in -7 .. gx - 1, into M's row y + 7.  Reads plane at y * gx + c with 0 <= c < gx; writes M at (y + 7) * (gx + 7) + x + 7 < (gz + 7) * (gx + 7).
MW_HD void bound_rows(const uint8_t *plane, int gx, int gz, uint8_t *M, int lane, int stride)
{
    const int mx = gx + kBlock - 1;
    for (int k = lane; k < gz * mx; k += stride) {
        const int y = k / mx, x = k % mx - (kBlock - 1);
        const int x0 = x < 0 ? 0 : x, x1 = x + kBlock - 1 < gx - 1 ? x + kBlock - 1 : gx - 1;
        uint8_t m = 0;
        for (int c = x0; c <= x1; ++c) m = plane[y * gx + c] > m ? plane[y * gx + c] : m;
        M[(y + kBlock - 1) * mx + x + kBlock - 1] = m;
    }
}
// pass 2, a column per worker, y ascending from -7: M[y][x] = max H[y .. y + 7][x] cut to the grid's rows, in place.  H[j] lies in M's row
// j + 7, M[y] goes to row y + 7: step y reads the rows max(y, 0) + 7 .. min(y + 7, gz - 1) + 7 and then writes row y + 7, which no later
// step of the column reads (they read from row y + 8 on), and no other worker touches the column.  The rows 0 .. 6, never written by
// pass 1, are written here before anything reads them: they are read by nobody in this pass.
MW_HD void bound_cols(uint8_t *M, int gx, int gz, int lane, int stride)
{
    const int mx = gx + kBlock - 1;
    for (int x = lane; x < mx; x += stride)
        for (int y = -(kBlock - 1); y < gz; ++y) {
            const int y0 = y < 0 ? 0 : y, y1 = y + kBlock - 1 < gz - 1 ? y + kBlock - 1 : gz - 1;
            uint8_t m = 0;
            for (int j = y0; j <= y1; ++j) m = M[(j + kBlock - 1) * mx + x] > m ? M[(j + kBlock - 1) * mx + x] : m;
            M[(y + kBlock - 1) * mx + x] = m;
        }
}

// ---- a batch of rotations r0 .. r0 + nb - 1: task k = g * blocks + q is block q of rotation r0 + g ------------------------------------------
// the bounds, a task per worker: words[k], and the worker's greatest bound << 32 | ~k (0 for a worker without a task).  An entry's
// (row + W) + (b0 - W) + 7 = row + b0 + 7 is M's stored row; one unsigned compare tests -7 <= row + b0 < gz.
MW_HD uint64_t bound_blocks(const uint8_t *M, int gx, int gz, int W, int r0, int nb, const uint32_t *ends, int R, const uint32_t *fill, uint32_t *words, int lane,
                            int stride)
{
    const int ns = blocks_side(W), nblk = ns * ns, mx = gx + kBlock - 1, mz = gz + kBlock - 1;
    uint64_t mine = 0;
    for (int k = lane; k < nb * nblk; k += stride) {
        const int g = k / nblk, q = k % nblk, n = (int)fill[r0 + g];
        const int db = kBlock * (q / ns) - 2 * W + kBlock - 1, da = kBlock * (q % ns) - 2 * W + kBlock - 1;
        const uint32_t *list = ends + (size_t)g * R;
        uint32_t sum = 0;
        for (int e = 0; e < n; ++e) {
            const uint32_t v = list[e];
            const int y = (int)(v >> 16) + db, x = (int)(v & 0xFFFFu) + da;
            if ((unsigned)y < (unsigned)mz && (unsigned)x < (unsigned)mx) sum += M[y * mx + x];
        }
        words[k] = sum;
        const uint64_t key = (uint64_t)sum << 32 | (0xFFFFFFFFu - (uint32_t)k);
        mine = key > mine ? key : mine;
    }
    return mine;
}
// the score of one translation: mwmatch::correlate's sum
MW_HD int32_t score_at(const uint8_t *plane, int gx, int gz, int W, const uint32_t *list, int n, int b, int a)
{
    int32_t sum = 0;
    for (int e = 0; e < n; ++e) {
        const uint32_t v = list[e];
        const int row = (int)(v >> 16) + (b - W), col = (int)(v & 0xFFFFu) + (a - W);
        if ((unsigned)row < (unsigned)gz && (unsigned)col < (unsigned)gx) sum += plane[row * gx + col];
    }
    return sum;
}
// the next ticket: a wavefront takes one through its first lane; the host's one worker counts plainly.  Every lane issues the atomic, the
// first lane adding 1 and the others 0, and so does refine's fold at its end: no branch on the lane stands between an atomic and the
// cross-lane read in this loop.  The form with `if (lane 0)` around the atomics hung on the device; this one is kept because it is safe.
MW_HD uint32_t take(uint32_t *ticket, int lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t k = atomicAdd(ticket, (lane & 63) == 0 ? 1u : 0u);
    return (uint32_t)__shfl((int)k, 0);
#else
    return (*ticket)++;
#endif
}
// the best score so far, one value for the whole wavefront
MW_HD uint32_t best_so_far(const unsigned long long *top)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__shfl((int)(uint32_t)(*(const volatile unsigned long long *)top >> 39), 0);
#else
    return (uint32_t)(*top >> 39);
#endif
}
// the refinement, a block per wavefront (the host: per worker, the 64 translations in turn): tickets from work[0] until the batch's
// tasks are out; ticket 0 is the block `first`, ticket `first` block 0.  A block whose bound < the best score is skipped; a refined one
// scores its translations — lane (db, da) = (lane / 8 % 8, lane % 8) its one, lanes beyond W sit out —, folds them into `top` by
// mw_match_kernel's fold (a butterfly max of the keys, an LDS atomicMax) and counts in work[1].  Every lane of a wavefront takes the
// same path: the ticket, the bound and the best score read are the wavefront's.
MW_HD void refine(const uint8_t *plane, int gx, int gz, int W, int r0, int nb, const uint32_t *ends, int R, const uint32_t *fill, const uint32_t *words, uint32_t first,
                  uint32_t *work, unsigned long long *top, bool prune, int lane)
{
    const int ns = blocks_side(W), nblk = ns * ns;
    const uint32_t tasks = (uint32_t)(nb * nblk);
    for (;;) {
        uint32_t k = take(work, lane);
        if (k >= tasks) break;
        k = k == 0 ? first : k == first ? 0 : k;
        if (prune && words[k] < best_so_far(top)) continue;
        const int g = (int)k / nblk, q = (int)k % nblk, r = r0 + g, n = (int)fill[r];
        const int b0 = kBlock * (q / ns) - W, a0 = kBlock * (q % ns) - W;
        const uint32_t *list = ends + (size_t)g * R;
#if defined(__HIP_DEVICE_COMPILE__)
        const int sub = lane & 63, b = b0 + (sub >> 3), a = a0 + (sub & 7);
        uint64_t key = 0;
        if (b <= W && a <= W) key = key_of(score_at(plane, gx, gz, W, list, n, b, a), r, b, a, W);
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), d);
            const uint64_t other = (uint64_t)hi << 32 | lo;
            key = other > key ? other : key;
        }
        atomicMax(top, (unsigned long long)key);        // (the butterfly left the block's greatest key in every lane)
        atomicAdd(work + 1, sub == 0 ? 1u : 0u);
#else
        for (int sub = 0; sub < kBlock * kBlock; ++sub) {
            const int b = b0 + (sub >> 3), a = a0 + (sub & 7);
            if (b > W || a > W) continue;
            const uint64_t key = key_of(score_at(plane, gx, gz, W, list, n, b, a), r, b, a, W);
            *top = key > *top ? key : *top;
        }
        ++work[1];
#endif
    }
}
// an env whose extent the grid does not cover: zeros, the stats too
MW_HD void write_none(int32_t *best, int32_t *best_score, int32_t *stats, int lane)
{
    if (lane != 0) return;
    best[0] = best[1] = best[2] = 0;
    *best_score = 0;
    if (stats) stats[0] = stats[1] = 0;
}

// ---- a whole call for one env by one worker: the host's path (tests/hostcheck/grid_search.cpp); the kernel runs the same phases ---------
// origin, t, dir, score: as for mwmatch::match_one; plane: plane_bytes(cells) bytes; M: bound_bytes(gz, gx); ends: R words and words:
// blocks(W) (a batch of one); best: the env's [3]; stats: its [2] or null.  false for an env whose extent the grid does not cover
inline bool search_one(const MwNavArgs &a, const mw_nav_params &p, double max_range, int R, const MwMatchRot &rot, int W, bool prune, size_t env, const double *origin,
                       const double *t, const double *dir, const uint8_t *score, uint8_t *plane, uint8_t *M, uint32_t *ends, uint32_t *words, int32_t *best,
                       int32_t *best_score, int32_t *stats)
{
    const mwnav::Grid g = mwnav::grid_of(a, p, env);
    if (!mwnav::covers(g)) {
        write_none(best, best_score, stats, 0);
        return false;
    }
    const mwmatch::Match m{g, origin ? origin[0] : a.ax[env], origin ? origin[2] : a.az[env], max_range, t, dir, R, W};
    mwmatch::stage(score, plane, g.gx * g.gz, false, 0, 1);
    bound_rows(plane, g.gx, g.gz, M, 0, 1);
    bound_cols(M, g.gx, g.gz, 0, 1);
    unsigned long long top = 0;
    uint32_t fill[MW_MATCH_MAX_ROT] = {}, work[2] = {0, 0};
    for (int r = 0; r < rot.n; ++r) {
        work[0] = 0;
        mwmatch::list_ends(m, rot.cs[r][0], rot.cs[r][1], ends, fill + r, 0, 1);
        const uint64_t first = bound_blocks(M, g.gx, g.gz, W, r, 1, ends, R, fill, words, 0, 1);
        refine(plane, g.gx, g.gz, W, r, 1, ends, R, fill, words, 0xFFFFFFFFu - (uint32_t)first, work, &top, prune, 0);
    }
    decode((uint64_t)top, W, best, best_score);
    if (stats) {
        stats[0] = (int32_t)work[1];
        stats[1] = rot.n * blocks(W);
    }
    return true;
}

}  // namespace mwsearch
