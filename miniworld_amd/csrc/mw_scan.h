// Scan maps (mw_scan_project, include/mwengine.h; kernel: mw_scan.hip): the beams of a range scan traced into an occupancy map — the
// cells a beam passes through are free, the cell it ends in is an obstacle.  Plain C++ like mw_clear.h and mw_depth.h: the kernel calls
// these functions with (lane, stride) of a workgroup, tests/hostcheck/grid_scan.cpp calls scan_one on the host, which runs the same
// phases with (0, 1).
//
// The rule (the header states it in full), float64, only + - * / and floor, no contraction, in this order:
//   u0 = (ox - min_x) / cell; w0 = (oz - min_z) / cell; gu = dx / cell; gw = dz / cell
//   e = t < max_range ? t : max_range; hit = t < max_range; u1 = u0 + e * gu; w1 = w0 + e * gw
//   kept iff t >= 0 and u0, w0, u1, w1 are all strictly inside -2^30 .. 2^30 (a NaN or an infinity fails)
//   a kept beam's cells: the start cell (floor(w0), floor(u0)); per x line L it crosses — gu > 0: floor(u0) + 1 .. floor(u1), gu < 0:
//   floor(u1) + 1 .. floor(u0), clipped to 0 .. gx — column gu > 0 ? L : L - 1 and row floor(w0 + ((double)L - u0) / gu * gw); the
//   mirrored cells per z line; each only if row and column are inside the grid, compared as doubles
//   obstacle set: the end cells (floor(w1), floor(u1)) of the kept beams with hit; free set: the kept beams' cells outside it
// A kept beam has finite gu and gw: an infinite one makes e * g infinite or NaN and the beam is dropped.  Its four coordinates are
// below 2^30 in magnitude, so their floors are ints and the line counts are int arithmetic; a crossing's other coordinate may be
// anything (a huge quotient, a NaN from inf * 0) and is tested as a double before it becomes an index.
//
// The arrays (LDS in the kernel, the caller's on the host):
//   bits    two bit planes, a bit per cell in 32-bit words: free, then obstacle
//   pre     R + 1 int32: a beam's task count 1 + nx + nz (0: dropped), then the exclusive prefix sums, pre[R] the total
// A task (beam, c) is one cell of the beam: c = 0 the start cell, 1 .. nx the x lines in ascending L, then the z lines.  Tasks are
// numbered through all beams; task k belongs to the last beam b with pre[b] <= k.  Both sets are unions of bits, so nothing depends on
// who sets which or when.
#pragma once
#include "mw_nav_grid.h"

#ifndef MW_SCAN_THREADS
#define MW_SCAN_THREADS 256             // lanes of mw_scan_kernel's workgroup, a multiple of 64
#endif

namespace mwscan {

constexpr double kBound = 1073741824.0;                         // 2^30
constexpr int kTailWords = 2 + MW_SCAN_THREADS / 64;            // behind pre: the two new-cell sums, a word per wavefront for the prefix

// the bytes of one bit plane and of the prefix with its tail, either rounded up to 16
MW_HD size_t plane_words(long long cells) { return ((size_t)cells + 31) / 32; }
MW_HD size_t plane_bytes(long long cells) { return (plane_words(cells) * 4 + 15) / 16 * 16; }
MW_HD size_t prefix_bytes(int rays) { return (((size_t)rays + 1 + kTailWords) * 4 + 15) / 16 * 16; }

struct Beam {
    double u0, w0, gu, gw, u1, w1;
    int xl, nx, zl, nz;         // the first (lowest) clipped line per axis and how many
    bool keep, hit;
};

MW_HD bool bounded(double v) { return v > -kBound && v < kBound; }

// the lines strictly between a0 and a1 in the direction of g, clipped to 0 .. n: the lowest and the count
MW_HD void lines_of(double a0, double a1, double g, int n, int &first, int &count)
{
    const int f0 = (int)floor(a0), f1 = (int)floor(a1);
    int lo = 1, hi = 0;
    if (g > 0.0) { lo = f0 + 1; hi = f1; }
    if (g < 0.0) { lo = f1 + 1; hi = f0; }
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    first = lo;
    count = hi >= lo ? hi - lo + 1 : 0;
}

MW_HD Beam beam_of(const mwnav::Grid &g, double ox, double oz, double t, double dx, double dz, double max_range)
{
    Beam b{};
    b.u0 = (ox - g.min_x) / g.cell;
    b.w0 = (oz - g.min_z) / g.cell;
    b.gu = dx / g.cell;
    b.gw = dz / g.cell;
    b.hit = t < max_range;
    const double e = b.hit ? t : max_range;
    b.u1 = b.u0 + e * b.gu;
    b.w1 = b.w0 + e * b.gw;
    b.keep = t >= 0.0 && bounded(b.u0) && bounded(b.w0) && bounded(b.u1) && bounded(b.w1);
    if (b.keep) {
        lines_of(b.u0, b.u1, b.gu, g.gx, b.xl, b.nx);
        lines_of(b.w0, b.w1, b.gw, g.gz, b.zl, b.nz);
    }
    return b;
}
MW_HD int tasks_of(const Beam &b) { return b.keep ? 1 + b.nx + b.nz : 0; }

// the flat index of (row, col), -1 outside the grid: compared as doubles before any conversion, so that a NaN fails
MW_HD int inside(double row, double col, int gx, int gz)
{
    if (!(row >= 0.0 && row < (double)gz && col >= 0.0 && col < (double)gx)) return -1;
    return (int)row * gx + (int)col;
}
// the cell of task c of a kept beam, 0 <= c < tasks_of(b)
MW_HD int task_cell(const Beam &b, int gx, int gz, int c)
{
    if (c == 0) return inside(floor(b.w0), floor(b.u0), gx, gz);
    if (c <= b.nx) {
        const double L = (double)(b.xl + (c - 1));
        return inside(floor(b.w0 + (L - b.u0) / b.gu * b.gw), b.gu > 0.0 ? L : L - 1.0, gx, gz);
    }
    const double L = (double)(b.zl + (c - 1 - b.nx));
    return inside(b.gw > 0.0 ? L : L - 1.0, floor(b.u0 + (L - b.w0) / b.gw * b.gu), gx, gz);
}
MW_HD int end_cell(const Beam &b, int gx, int gz) { return inside(floor(b.w1), floor(b.u1), gx, gz); }

// a bit of a plane: the workgroup's lanes share the words, the host's one worker does not
MW_HD void set_bit(uint32_t *plane, int c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(plane + (c >> 5), 1u << (c & 31));
#else
    plane[c >> 5] |= 1u << (c & 31);
#endif
}
MW_HD uint32_t bit_at(const uint32_t *plane, int c) { return (plane[c >> 5] >> (c & 31)) & 1u; }

// what a call reads of one env, by value
struct Scan {
    mwnav::Grid g;
    double ox, oz, max_range;
    const double *t, *dir;      // the env's rows [R], [R][2]
    int R;
};
MW_HD Beam beam(const Scan &s, int b) { return beam_of(s.g, s.ox, s.oz, s.t[b], s.dir[2 * b], s.dir[2 * b + 1], s.max_range); }

// ---- the phases of a call; `lane` of `stride` workers share each ------------------------------------------------------------------

MW_HD void zero_words(uint32_t *w, int n, int lane, int stride)
{
    for (int k = lane; k < n; k += stride) w[k] = 0u;
}
// phase 1, a beam per worker: its task count, and the obstacle bit of its end cell
MW_HD void count_beams(const Scan &s, uint32_t *obstacle, int32_t *pre, int lane, int stride)
{
    for (int b = lane; b < s.R; b += stride) {
        const Beam m = beam(s, b);
        pre[b] = tasks_of(m);
        if (m.keep && m.hit) {
            const int c = end_cell(m, s.g.gx, s.g.gz);
            if (c >= 0) set_bit(obstacle, c);
        }
    }
}
// the beam of task k: the last b with pre[b] <= k (pre[0] = 0 <= k < pre[R])
MW_HD int beam_of_task(const int32_t *pre, int R, int k)
{
    int lo = 0, hi = R;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
}
// phase 2, a task per worker: its one cell's free bit
MW_HD void deal_tasks(const Scan &s, uint32_t *free_bits, const int32_t *pre, int lane, int stride)
{
    const int total = pre[s.R];
    for (int k = lane; k < total; k += stride) {
        const int b = beam_of_task(pre, s.R, k);
        const int c = task_cell(beam(s, b), s.g.gx, s.g.gz, k - pre[b]);
        if (c >= 0) set_bit(free_bits, c);
    }
}

// phase 3: a plane's bits into the env's row of bytes.  A byte that is 0 becomes 1 where the bit `want & ~minus` is set; a cleared row
// is rewritten whole.  The row starts at any byte: up to 3 head bytes singly, then aligned 32-bit words of four cells, then the tail
// (mwnav::each_byte's split).  `added` grows by the bytes that went 0 -> 1, a popcount per word.
MW_HD uint32_t wanted(const uint32_t *want, const uint32_t *minus, int c) { return bit_at(want, c) & ~(minus ? bit_at(minus, c) : 0u); }
MW_HD int merge_byte(uint8_t *row, int c, bool hit, bool cleared)
{
    if (cleared) {
        row[c] = hit ? 1 : 0;
        return hit ? 1 : 0;
    }
    if (!hit || row[c] != 0) return 0;
    row[c] = 1;
    return 1;
}
MW_HD void merge_plane(const uint32_t *want, const uint32_t *minus, int n, bool cleared, uint8_t *row, int &added, int lane, int stride)
{
    int head = (int)((4 - ((uintptr_t)row & 3)) & 3);
    head = head < n ? head : n;
    const int words = (n - head) / 4, tail = head + words * 4;
    for (int c = lane; c < head; c += stride) added += merge_byte(row, c, wanted(want, minus, c) != 0u, cleared);
    for (int w = lane; w < words; w += stride) {
        const int c0 = head + 4 * w;
        uint32_t on = 0u;               // a byte of 0 / 1 per cell (little-endian, like every target here)
        for (int k = 0; k < 4; ++k) on |= wanted(want, minus, c0 + k) << (8 * k);
        void *p = __builtin_assume_aligned(row + c0, 4);
        uint32_t v = 0u;
        if (!cleared) {
            if (!on) continue;
            __builtin_memcpy(&v, p, 4);
            const uint32_t set = ((((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) >> 7) & 0x01010101u;      // 1 per byte != 0: no carry leaves a byte
            on &= ~set;
            if (!on) continue;
        }
        v |= on;
        __builtin_memcpy(p, &v, 4);
        added += __builtin_popcount(on);
    }
    for (int c = tail + lane; c < n; c += stride) added += merge_byte(row, c, wanted(want, minus, c) != 0u, cleared);
}
MW_HD void zero_rows(uint8_t *rows, int n, int lane, int stride)
{
    for (int k = lane; k < 2 * n; k += stride) rows[k] = 0;
}

// ---- a whole call for one env by one worker: the host's path (tests/hostcheck/grid_scan.cpp); the kernel runs the same phases ---------
// origin: the env's [3] or null = the agent; t, dir: the env's rows; bits: 2 * plane_words(cells) words; pre: R + 1 entries; rows: the env's
// [2][gz][gx]; count, newly: its [2] (newly may be null).  false for an env whose extent the grid does not cover
inline bool scan_one(const MwNavArgs &a, const mw_nav_params &p, double max_range, int R, size_t env, const double *origin, const double *t, const double *dir,
                     bool clear, uint32_t *bits, int32_t *pre, uint8_t *rows, int32_t *count, int32_t *newly)
{
    const mwnav::Grid g = mwnav::grid_of(a, p, env);
    const int n = g.gx * g.gz, words = (int)plane_words(n);
    if (!mwnav::covers(g)) {
        zero_rows(rows, n, 0, 1);
        count[0] = count[1] = 0;
        if (newly) newly[0] = newly[1] = 0;
        return false;
    }
    const Scan s{g, origin ? origin[0] : a.ax[env], origin ? origin[2] : a.az[env], max_range, t, dir, R};
    uint32_t *free_bits = bits, *obstacle = bits + words;
    zero_words(bits, 2 * words, 0, 1);
    count_beams(s, obstacle, pre, 0, 1);
    int32_t sum = 0;
    for (int b = 0; b < R; ++b) { const int32_t v = pre[b]; pre[b] = sum; sum += v; }
    pre[R] = sum;
    deal_tasks(s, free_bits, pre, 0, 1);
    int nf = 0, no = 0;
    merge_plane(free_bits, obstacle, n, clear, rows, nf, 0, 1);
    merge_plane(obstacle, nullptr, n, clear, rows + n, no, 0, 1);
    count[0] = (clear ? 0 : count[0]) + nf;
    count[1] = (clear ? 0 : count[1]) + no;
    if (newly) { newly[0] = nf; newly[1] = no; }
    return true;
}

}  // namespace mwscan
