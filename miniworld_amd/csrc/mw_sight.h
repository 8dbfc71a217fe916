// Grid sight (mw_grid_sight, include/mwengine.h; kernel: mw_sight.hip): what a viewpoint cell would see on the caller's own uint8 grid —
// line of sight from cell centre to cell centre over opaque cells, a range and a cone, summed against a weight plane per viewpoint and
// marked in a seen plane.  Plain C++ like mw_nav_grid.h and mw_seen.h: the kernel calls these functions with (lane, stride) of a
// wavefront, tests/hostcheck/grid_sight.cpp calls sight_one on the host, which runs the same phases with (0, 1).
//
// The rule (the header states it in full): with A = (ja, ia), B = (jb, ib), dx = ib - ia, dz = jb - ja, the cell Q = (j, i) hides B
// from A iff it is opaque, is neither A nor B, lies in their bounding box and
//     2 * |dx * (j - ja) - dz * (i - ia)| <= |dx| + |dz|                                                        (integers, closed)
// The walk: along the major axis — M = max(|dx|, |dz|) steps, m the signed extent of the other axis — step k looks at the cells at
// minor offset u with 2 * |M * u - m * k| <= |dx| + |dz|.  They lie within one cell of the real m * k / M, so they are among
// f - 1, f, f + 1 with f = floor(m * k / M): at most 3 probes per step, the exact test applied to each, and the walk stops at the first
// opaque one.  M and |m| are extents along different axes of a grid of at most MW_NAV_MAX_CELLS cells: every product here is far
// below 2^31.
// Range and cone are mwseen::in_cone's float64 tests on v = ((double)dx * cell, (double)dz * cell): the grid's origin does not enter.
// Gains are integer sums and the seen plane gets same-value stores, so nothing depends on how targets are spread over lanes.
#pragma once
#include "mw_nav_grid.h"
#include "mw_seen.h"

#define MW_SIGHT_THREADS 256            // lanes of mw_sight_kernel's workgroup, a multiple of 64

namespace mwsight {

// a viewpoint: its cell and heading; ok == false: no viewpoint (gain 0, nothing marked)
struct Eye { int j, i; double hx, hz; bool ok; };

// the bytes of dynamic LDS: a bit per cell of the opaque row in 32-bit words, with weights a byte per cell, a gain word per viewpoint;
// each rounded up to 16
MW_HD size_t bits_bytes(long long cells) { return (((size_t)cells + 31) / 32 * 4 + 15) / 16 * 16; }
MW_HD size_t weight_bytes(long long cells, bool weighted) { return weighted ? ((size_t)cells + 15) / 16 * 16 : 0; }
MW_HD size_t gain_bytes(int views) { return ((size_t)views * 4 + 15) / 16 * 16; }

// the cells a range spans along an axis, with one to spare (the exact test decides; this bounds the work): 1 .. limit, limit >= 1.
// The clamp comes before the conversion, as in mwnav::axis_range.
MW_HD int reach_cells(double cell, double range, int limit)
{
    double r = floor(range / cell) + 1.0;
    r = r < (double)limit ? r : (double)limit;
    r = r > 1.0 ? r : 1.0;
    return (int)r;
}
// the 64-cell chunks of the largest box an eye can have: (2R + 1)^2 cells, clamped to the grid
MW_HD int chunks_of(int R, int gx, int gz)
{
    const int w = 2 * R + 1 < gx ? 2 * R + 1 : gx, h = 2 * R + 1 < gz ? 2 * R + 1 : gz;
    return (w * h + 63) / 64;
}
// the cells within R of the eye, clamped to the grid
MW_HD mwnav::Box box_of(const Eye &e, int R, int gx, int gz)
{
    return {e.i - R > 0 ? e.i - R : 0, e.i + R < gx - 1 ? e.i + R : gx - 1, e.j - R > 0 ? e.j - R : 0, e.j + R < gz - 1 ? e.j + R : gz - 1};
}

// ---- the opaque row as bits: bit c & 31 of word c >> 5.  `set` ors a bit into a word other workers set bits of too (the kernel: an
// LDS atomic; the host: |=); only the opaque bytes reach it.
MW_HD void zero_bits(uint32_t *bits, int cells, int lane, int stride)
{
    for (int w = lane; w < (cells + 31) / 32; w += stride) bits[w] = 0u;
}
template <typename Set>
MW_HD void stage_bits(const uint8_t *row, uint32_t *bits, int cells, int lane, int stride, Set set)
{
    mwnav::each_byte(row, cells, lane, stride, [bits, set](int c, uint8_t b) { if (b) set(bits + (c >> 5), 1u << (c & 31)); });
}
MW_HD bool opaque_at(const uint32_t *bits, int c) { return (bits[c >> 5] >> (c & 31)) & 1u; }

// ---- the predicate, as the header writes it (the walk applies it to its candidates; the tests apply it to every cell of the box)
MW_HD int iabs(int v) { return v < 0 ? -v : v; }
MW_HD bool meets(int dx, int dz, int qj, int qi) { return 2 * iabs(dx * qj - dz * qi) <= iabs(dx) + iabs(dz); }       // (qj, qi): Q - A

// does an opaque cell hide B from A: the walk along the major axis.  f and rem are carried from step to step, m * k = f * M + rem with
// 0 <= rem < M (|m| <= M: one correction per step, no division), so that M * u - m * k = M * (u - f) - rem.
MW_HD bool hidden(const uint32_t *bits, int gx, int ja, int ia, int jb, int ib)
{
    const int dx = ib - ia, dz = jb - ja;
    const bool xmajor = iabs(dx) >= iabs(dz);
    const int M = xmajor ? iabs(dx) : iabs(dz), m = xmajor ? dz : dx, sgn = (xmajor ? dx : dz) < 0 ? -1 : 1;
    if (M == 0) return false;
    const int lo = m < 0 ? m : 0, hi = m < 0 ? 0 : m, S = M + iabs(m);
    int f = 0, rem = 0;
    for (int k = 0; k <= M; ++k) {
        for (int d = -1; d <= 1; ++d) {
            const int u = f + d;
            if (u < lo || u > hi || 2 * iabs(M * d - rem) > S) continue;
            if ((k == 0 && u == 0) || (k == M && u == m)) continue;     // A and B themselves
            const int j = xmajor ? ja + u : ja + sgn * k, i = xmajor ? ia + sgn * k : ia + u;
            if (opaque_at(bits, j * gx + i)) return true;
        }
        rem += m;
        if (rem >= M) { rem -= M; ++f; } else if (rem < 0) { rem += M; --f; }
    }
    return false;
}

// is B seen from the eye: range and cone (mwseen::in_cone on the offset between the centres), then the walk
MW_HD bool sees(const uint32_t *bits, int gx, double cell, const mwseen::Sight &s, const Eye &e, int jb, int ib)
{
    const mwseen::View v{0.0, 0.0, e.hx, e.hz};
    const mwray::Ray r{0.0, 0.0, (double)(ib - e.i) * cell, (double)(jb - e.j) * cell};
    return mwseen::in_cone(v, s, r) && !hidden(bits, gx, e.j, e.i, jb, ib);
}

// ---- the viewpoints
// the heading mw_ray_cast's fan forms for an angle at offset 0 (mwseen::view_of on a one-env view of that angle)
MW_HD void heading_of(double ang, const mwseen::Sight &s, double &hx, double &hz)
{
    MwRayArgs one{};
    one.w.ax = one.w.az = one.adir = &ang;
    const mwseen::View v = mwseen::view_of(one, s, 0);
    hx = v.hx;
    hz = v.hz;
}
// viewpoint v of env `env` from the caller's rows: a cell outside 0 .. cells - 1 is none; without dirs the heading is never read (the
// cone is all round: the entry point refuses anything else)
MW_HD Eye eye_of_cell(const mwseen::Sight &s, int gx, int gz, const int32_t *cells, const double *dirs, size_t at)
{
    const int32_t c = cells[at];
    Eye e{0, 0, 0.0, 0.0, c >= 0 && c < gx * gz};
    if (!e.ok) return e;
    e.j = c / gx;
    e.i = c % gx;
    if (dirs) heading_of(dirs[at], s, e.hx, e.hz);
    return e;
}
// the agent's own cell (mwnav::cell_of on the env's grid) and heading; a NaN position is no viewpoint
MW_HD Eye eye_of_agent(const MwRayArgs &a, const mwnav::Grid &g, const mwseen::Sight &s, size_t env)
{
    const mwseen::View v = mwseen::view_of(a, s, env);
    if (v.ox != v.ox || v.oz != v.oz) return {0, 0, 0.0, 0.0, false};
    return {mwnav::cell_of(v.oz, g.min_z, g.cell, g.gz), mwnav::cell_of(v.ox, g.min_x, g.cell, g.gx), v.hx, v.hz, true};
}

// ---- the targets of one eye: cells k = first + lane, first + lane + stride, ... below `last` of its box b (row-major); the sum of
// the seen cells' weights (w null: their count), each marked in `seen` where there is one
MW_HD int32_t look(const uint32_t *bits, const uint8_t *w, int gx, double cell, const mwseen::Sight &s, const Eye &e, const mwnav::Box &b, int first, int last,
                   uint8_t *seen, int lane, int stride)
{
    const int bw = mwnav::box_w(b);
    int32_t sum = 0;
    for (int k = first + lane; k < last; k += stride) {
        const int j = b.j0 + k / bw, i = b.i0 + k % bw;
        if (!sees(bits, gx, cell, s, e, j, i)) continue;
        const int c = j * gx + i;
        sum += w ? (int32_t)w[c] : 1;
        if (seen) seen[c] = 1;
    }
    return sum;
}

// ---- a whole call for one env by one worker: the host's path (tests/hostcheck/grid_sight.cpp); the kernel runs the same phases -------
// bits: (cells + 31) / 32 words of the caller's; opaque, weight, seen: the env's own rows (weight, seen may be null); cells, dirs:
// the env's `views` entries, or cells null for the agent of `a` (views = 1).  Returns false for an env whose extent the grid does not
// cover (agent mode only): gain 0, nothing marked.
inline bool sight_one(const MwRayArgs &a, const mw_nav_params &p, const mwseen::Sight &s, size_t env, int views, const uint8_t *opaque, const uint8_t *weight,
                      const int32_t *cells, const double *dirs, uint32_t *bits, int32_t *gain, uint8_t *seen)
{
    const int gx = p.gx, gz = p.gz, n = gx * gz;
    for (int v = 0; v < views; ++v) gain[v] = 0;
    mwnav::Grid g{0.0, 0.0, 0.0, 0.0, p.cell, gx, gz};
    if (!cells) {
        g = mwnav::grid_of(a.w, p, env);
        if (!mwnav::covers(g)) return false;
    }
    zero_bits(bits, n, 0, 1);
    stage_bits(opaque, bits, n, 0, 1, [](uint32_t *word, uint32_t bit) { *word |= bit; });
    const int R = reach_cells(p.cell, s.range, gx > gz ? gx : gz);
    for (int v = 0; v < views; ++v) {
        const Eye e = cells ? eye_of_cell(s, gx, gz, cells, dirs, (size_t)v) : eye_of_agent(a, g, s, env);
        if (!e.ok) continue;
        const mwnav::Box b = box_of(e, R, gx, gz);
        gain[v] = look(bits, weight, gx, p.cell, s, e, b, 0, mwnav::box_cells(b), seen, 0, 1);
    }
    return true;
}

}  // namespace mwsight
