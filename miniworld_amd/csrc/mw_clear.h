// Grid clearance (mw_grid_clearance, include/mwengine.h; kernel: mw_clear.hip): for every cell of a nav grid the squared distance, in
// cells, to the nearest marked cell of a byte mask — an obstacle plane's inflation layer, the distance to the nearest frontier or seen
// cell —, that cell's index, and a cost byte from bands of the distance.  Plain C++ like mw_regions.h and mw_nav_grid.h: the kernel
// calls these functions with (lane, stride) of a workgroup, tests/hostcheck/grid_clearance.cpp calls clear_one on the host, which runs
// the same phases with (0, 1).
//
// The rule (the header states it in full): dist2 = the least (j - j')^2 + (i - i')^2 over the marked cells (j', i') of the env, nearest
// = the lowest flat index j' * gx + i' at it; kNone / -1 in an env without a marked cell; with a limit L > 0 kFar / -1 beyond L^2; the
// cost is that of the first band (thr, cost) with dist2 <= thr, 0 with none.
//
// The one array:
//   off     int16 per cell: the signed row offset dj = j' - j to the nearest marked cell (j', i) of the cell's OWN column, the upper one
//           (dj < 0) at equal distance, 0 on a marked cell, kNoOff for a column without one.  |dj| < gz <= MW_NAV_MAX_CELLS = 32768, so
//           every offset lies in -32767 .. 32767 and kNoOff = -32768 is none of them.
// Why one array is enough: a marked cell (j', i') that is not its column's nearest to row j is strictly farther from (j, i) than the
// column's nearest — the same (i - i')^2, a larger (j - j')^2 — or equally far with a higher index (the lower one of a tie: its row is
// higher), so the minimum over the marked cells, ties to the lowest index, is the minimum over the columns' nearest cells.  The row pass
// takes it cell by cell, outwards: a column d away contributes at least d^2, so once d^2 > best nothing further can win or tie.
// Sizes: d < gx, |dj| < gz and gx * gz <= 32768 give d^2 + dj^2 < 2^30 + 1 < 2^31; an index (j + dj) * gx + i' is below gx * gz.
#pragma once
#include "mw_nav_grid.h"

#ifndef MW_CLEAR_THREADS
#define MW_CLEAR_THREADS 256            // lanes of mw_clear_kernel's workgroup, a multiple of 64 (512 measured: profiles/r42)
#endif

// the cost bands, by value in the kernel's arguments: n pairs, thr strictly ascending
struct MwClearBands { int32_t n; int32_t thr[MW_CLEAR_MAX_BANDS]; int32_t cost[MW_CLEAR_MAX_BANDS]; };

namespace mwclear {

constexpr int kNoOff = -32768;
constexpr int32_t kNone = MW_CLEAR_NONE, kFar = MW_CLEAR_FAR;

// the bytes of dynamic LDS: the offsets, rounded up to 16
MW_HD size_t off_bytes(long long cells) { return ((size_t)cells * sizeof(int16_t) + 15) / 16 * 16; }

// null, or the text of what is wrong with n bands of (thr, cost) pairs
MW_HD const char *bands_error(const int32_t *pairs, int n)
{
    if (n < 0 || n > MW_CLEAR_MAX_BANDS) return "a band count outside 0 .. MW_CLEAR_MAX_BANDS";
    for (int b = 0; b < n; ++b) {
        if (pairs[2 * b] < 0) return "a negative threshold";
        if (b > 0 && pairs[2 * b] <= pairs[2 * b - 2]) return "thresholds that do not ascend";
        if (pairs[2 * b + 1] < 0 || pairs[2 * b + 1] > 255) return "a cost outside 0 .. 255";
    }
    return nullptr;
}
MW_HD MwClearBands make_bands(const int32_t *pairs, int n)
{
    MwClearBands k{};
    k.n = n;
    for (int b = 0; b < n; ++b) { k.thr[b] = pairs[2 * b]; k.cost[b] = pairs[2 * b + 1]; }
    return k;
}
// the cost of the first band that holds d2; the sentinels are above every threshold
MW_HD uint8_t band_cost(const MwClearBands &k, int32_t d2)
{
    for (int b = 0; b < k.n; ++b)
        if (d2 <= k.thr[b]) return (uint8_t)k.cost[b];
    return 0;
}

// the limit the passes see: no real dist2 reaches 32768^2 = 2^30, so a limit from there on is none, and limit * limit stays an int32
MW_HD int bounded_limit(int32_t limit) { return limit >= 32768 ? 0 : (int)limit; }

// ---- staging: 0 on a marked cell, kNoOff elsewhere; whether this worker saw a marked cell
MW_HD bool stage(const uint8_t *row, int16_t *off, int cells, int lane, int stride)
{
    bool any = false;
    mwnav::each_byte(row, cells, lane, stride, [off, &any](int c, uint8_t b) { off[c] = (int16_t)(b ? 0 : kNoOff); any = any || b != 0; });
    return any;
}

// ---- the column pass, a column per worker: down with the last marked row above, then up with the next one below, which takes the
// cell only where it is strictly nearer (a tie stays with the upper one, the lower index).  A marked cell is the one that holds 0.
MW_HD void column_pass(int16_t *off, int gx, int gz, int lane, int stride)
{
    for (int i = lane; i < gx; i += stride) {
        int seen = -1;
        for (int j = 0; j < gz; ++j) {
            int16_t &o = off[j * gx + i];
            if (o == 0) seen = j;
            else if (seen >= 0) o = (int16_t)(seen - j);
        }
        seen = -1;
        for (int j = gz - 1; j >= 0; --j) {
            int16_t &o = off[j * gx + i];
            if (o == 0) seen = j;
            else if (seen >= 0 && (o == kNoOff || seen - j < -(int)o)) o = (int16_t)(seen - j);
        }
    }
}

// ---- the row pass and the outputs, a cell per worker: from the cell's own column outwards, d = 1, 2, ..., the columns i - d and i + d
// of its row, until d^2 > best (strict: a tie at d^2 == best is still looked at), d > limit, or both columns are off the row.
struct Best { int32_t d2, cell; };
MW_HD void take(Best &b, int o, int d, int j, int col, int gx)
{
    if (o == kNoOff) return;
    const int32_t v = d * d + o * o, c = (j + o) * gx + col;
    if (v < b.d2 || (v == b.d2 && c < b.cell)) b = Best{v, c};
}
MW_HD Best nearest_of(const int16_t *off, int gx, int j, int i, int limit)
{
    const int16_t *row = off + j * gx;
    Best b{kNone, -1};
    take(b, row[i], 0, j, i, gx);
    const int reach = limit > 0 && limit < gx ? limit : gx - 1;
    for (int d = 1; d <= reach && d * d <= b.d2; ++d) {
        const bool l = i - d >= 0, r = i + d < gx;
        if (!l && !r) break;
        if (l) take(b, row[i - d], d, j, i - d, gx);
        if (r) take(b, row[i + d], d, j, i + d, gx);
    }
    if (limit > 0 && b.d2 > limit * limit) b = Best{kFar, -1};      // (limit <= 32767, bounded_limit: the product is below 2^30)
    return b;
}
MW_HD void row_pass(const int16_t *off, int gx, int gz, int limit, const MwClearBands &bands, int32_t *dist2, int32_t *nearest, uint8_t *cost,
                    int lane, int stride)
{
    for (int c = lane; c < gx * gz; c += stride) {
        const Best b = nearest_of(off, gx, c / gx, c % gx, limit);
        dist2[c] = b.d2;
        if (nearest) nearest[c] = b.cell;
        if (cost) cost[c] = band_cost(bands, b.d2);
    }
}
// an env without a marked cell: nothing is staged further
MW_HD void write_none(int cells, int32_t *dist2, int32_t *nearest, uint8_t *cost, int lane, int stride)
{
    for (int c = lane; c < cells; c += stride) {
        dist2[c] = kNone;
        if (nearest) nearest[c] = -1;
        if (cost) cost[c] = 0;
    }
}

// ---- a whole call for one env by one worker: the host's path (tests/hostcheck/grid_clearance.cpp); the kernel runs the same phases -----
// off: cells elements of the caller's; marked, dist2, nearest, cost: the env's own rows (nearest, cost may be null)
inline void clear_one(int gx, int gz, int limit, const MwClearBands &bands, const uint8_t *marked, int16_t *off, int32_t *dist2, int32_t *nearest,
                      uint8_t *cost)
{
    const int cells = gx * gz;
    limit = bounded_limit(limit);
    if (!stage(marked, off, cells, 0, 1)) { write_none(cells, dist2, nearest, cost, 0, 1); return; }
    column_pass(off, gx, gz, 0, 1);
    row_pass(off, gx, gz, limit, bands, dist2, nearest, cost, 0, 1);
}

}  // namespace mwclear
