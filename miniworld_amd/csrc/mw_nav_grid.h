// Grid navigation fields (mw_nav_build_grid, include/mwengine.h; kernel: mw_nav_grid.hip): a nav field whose occupancy, sources and cell
// costs are the caller's own tensors — the inflation of the raw obstacle cells, the sources of a mask, the relaxation with an extra
// cost per cell, and the query's waypoint on such a field.  Plain C++ like mw_nav.h, whose grid, sources of a point, unweighted
// relaxation, too_far, max_passes and query it reuses: the kernel calls these functions with (lane, stride) of a workgroup or of a
// wavefront, tests/hostcheck/nav_grid.cpp calls the same functions with (0, 1) on the host.
//
// Arithmetic (float64, no contraction):
//   inflated by o        sqrt((double)(di*di + dj*dj)) * cell < margin, (dj, di) != (0, 0) the offset from the raw obstacle cell o
//   radius R             the smallest integer with R * cell >= margin: no offset beyond |di|, |dj| <= R can pass the test
//   cost of a cell       extra + min over the admissible neighbours of cost + 5 / + 7; a source: 0
// While the occupancy is built a cell holds MW_NAV_BLOCKED where the caller's byte says so (a RAW cell: its final value already),
// kInflated where only the inflation blocks it, MW_NAV_UNREACHED else.  Inflating stores kInflated, and only over cells that are not
// raw, so the test "is it raw" reads the same answer whatever other lanes have stored meanwhile; fold() then makes kInflated
// MW_NAV_BLOCKED.  The other way — a bit per raw cell in 4 KiB more LDS — would add a read-modify-write of a shared word per staged
// cell (an LDS atomic, or a pass per 32 cells) and a second array to index in the scatter; the reserved value needs neither, and
// 0xFFFD is no cost a field can hold at that point (every cell is 0xFFFF or 0xFFFE before the sources are marked).
#pragma once
#include "mw_nav.h"

#define MW_NAV_GRID_THREADS 512         // lanes of mw_nav_grid_kernel's workgroup (= MW_NAV_THREADS, mw_kernels.h)

namespace mwnav {

constexpr int kInflated = 0xFFFD;

// the bytes of dynamic LDS of a build: the uint16 cost grid, and behind it — with extra costs — a byte per cell; either rounded up to 16
MW_HD size_t grid_field_bytes(long long cells) { return ((size_t)cells * sizeof(uint16_t) + 15) / 16 * 16; }
MW_HD size_t grid_extra_bytes(long long cells, bool weighted) { return weighted ? ((size_t)cells + 15) / 16 * 16 : 0; }

// R of the header; -1 for a margin the call refuses (R > MW_NAV_MAX_INFLATE, a NaN, a negative)
MW_HD int inflate_radius(double cell, double margin)
{
    if (!(margin >= 0.0) || !(cell > 0.0)) return -1;
    for (int r = 0; r <= MW_NAV_MAX_INFLATE; ++r)
        if ((double)r * cell >= margin) return r;
    return -1;
}

// ---- staging: a row of the caller's bytes into LDS, consecutive workers consecutive bytes.  An env's row starts at byte env * cells,
// which is no multiple of 4 for an odd cell count: up to 3 head bytes singly, then aligned 32-bit words, then the tail singly.
template <typename Put>
MW_HD void each_byte(const uint8_t *src, int n, int lane, int stride, Put put)
{
    int head = (int)((4 - ((uintptr_t)src & 3)) & 3);
    head = head < n ? head : n;
    const int words = (n - head) / 4, tail = head + words * 4;
    for (int c = lane; c < head; c += stride) put(c, src[c]);
    for (int w = lane; w < words; w += stride) {
        uint32_t v;
        __builtin_memcpy(&v, __builtin_assume_aligned(src + head + 4 * w, 4), 4);
        for (int k = 0; k < 4; ++k) put(head + 4 * w + k, (uint8_t)(v >> (8 * k)));     // (little-endian, like every target here)
    }
    for (int c = tail + lane; c < n; c += stride) put(c, src[c]);
}
// the raw occupancy: != 0 blocked
MW_HD void stage_blocked(const uint8_t *row, uint16_t *f, int cells, int lane, int stride)
{
    each_byte(row, cells, lane, stride, [f](int c, uint8_t b) { f[c] = (uint16_t)(b ? MW_NAV_BLOCKED : MW_NAV_UNREACHED); });
}
// the extra costs, as they are (row null: zeros)
MW_HD void stage_extra(const uint8_t *row, uint8_t *x, int cells, int lane, int stride)
{
    each_byte(row, cells, lane, stride, [x](int c, uint8_t b) { x[c] = b; });
}

// ---- inflation: scattered from one raw cell (j, i), its (2R + 1)^2 offsets dealt over the workers, as block_ent deals an entity's box
MW_HD void inflate_from(uint16_t *f, int gx, int gz, int j, int i, int R, double cell, double margin, int lane, int stride)
{
    const int w = 2 * R + 1;
    for (int k = lane; k < w * w; k += stride) {
        const int dj = k / w - R, di = k % w - R;
        const int nj = j + dj, ni = i + di;
        if ((dj == 0 && di == 0) || (unsigned)nj >= (unsigned)gz || (unsigned)ni >= (unsigned)gx) continue;
        if (sqrt((double)(di * di + dj * dj)) * cell < margin && f[nj * gx + ni] != MW_NAV_BLOCKED) f[nj * gx + ni] = (uint16_t)kInflated;
    }
}
MW_HD void fold(uint16_t *f, int cells, int lane, int stride)
{
    for (int c = lane; c < cells; c += stride)
        if (f[c] == kInflated) f[c] = (uint16_t)MW_NAV_BLOCKED;
}

// ---- sources of a mask: behind the occupancy, which they read
MW_HD void mark_mask_sources(const uint8_t *row, uint16_t *f, int cells, int lane, int stride)
{
    each_byte(row, cells, lane, stride, [f](int c, uint8_t b) { if (b && f[c] != MW_NAV_BLOCKED) f[c] = 0; });
}
// the grid of a build: the env's own origin with point sources, none read without (mark_sources alone looks at min_x, min_z)
MW_HD Grid grid_build_grid(const MwNavArgs &a, const mw_nav_params &p, const double *d_target, size_t env)
{
    return d_target ? grid_of(a, p, env) : Grid{0.0, 0.0, 0.0, 0.0, p.cell, p.gx, p.gz};
}

// ---- relaxation with an extra cost per cell: jacobi_pass and sweep_line of mw_nav.h with x[c] added to the cheapest way in.  A
// source stays 0 (every way in costs 5 or more); a way in is at most 0xFFFD + 7, so the sum with a byte fits an int with room.
MW_HD bool jacobi_pass_x(uint16_t *f, const uint8_t *x, int gx, int gz, int lane, int stride)
{
    bool changed = false;
    for (int c = lane; c < gx * gz; c += stride) {
        const int v = f[c];
        if (v == MW_NAV_BLOCKED || v == 0) continue;
        int b = best_via(f, gx, gz, c / gx, c % gx);
        if (b == kNone) continue;
        b += (int)x[c];
        if (b < v && b < MW_NAV_UNREACHED) { f[c] = (uint16_t)b; changed = true; }
    }
    return changed;
}
MW_HD bool sweep_line_x(uint16_t *f, const uint8_t *x, int n, int nlines, int line, int sk, int sl, bool rev)
{
    bool changed = false;
    int prev = MW_NAV_BLOCKED, pu = MW_NAV_BLOCKED, pd = MW_NAV_BLOCKED;
    const bool hu = line > 0, hd = line < nlines - 1;
    for (int t = 0; t < n; ++t) {
        const int c = line * sl + (rev ? n - 1 - t : t) * sk;
        int v = f[c];
        const int e = (int)x[c];        // (with u and d: read ahead of the carried `prev`)
        const int u = hu ? (int)f[c - sl] : MW_NAV_BLOCKED, d = hd ? (int)f[c + sl] : MW_NAV_BLOCKED;
        if (v != MW_NAV_BLOCKED) {
            int b = lower(via(prev, 5), lower(via(u, 5), via(d, 5)));
            if (prev != MW_NAV_BLOCKED && u != MW_NAV_BLOCKED) b = lower(b, via(pu, 7));
            if (prev != MW_NAV_BLOCKED && d != MW_NAV_BLOCKED) b = lower(b, via(pd, 7));
            if (b != kNone) {
                b += e;
                if (b < v && b < MW_NAV_UNREACHED) { f[c] = (uint16_t)b; v = b; changed = true; }
            }
        }
        prev = v; pu = u; pd = d;
    }
    return changed;
}
MW_HD bool sweep_x(uint16_t *f, const uint8_t *x, int gx, int gz, int dir, int lane, int stride)
{
    const bool rows = dir < 2;
    const int nlines = rows ? gz : gx, n = rows ? gx : gz, sk = rows ? 1 : gx, sl = rows ? gx : 1;
    bool changed = false;
    for (int line = lane; line < nlines; line += stride) changed = sweep_line_x(f, x, n, nlines, line, sk, sl, (dir & 1) != 0) || changed;
    return changed;
}
// (too_far serves as it is: an unreached cell with a reached neighbour is one whose cost, extra included, did not fit)

// ---- the query on a grid field: at cost 0 the waypoint is the centre of the cell itself; no target is read
MW_HD Answer query_grid(const Grid &g, const uint16_t *f, double x, double z)
{
    Answer r = query(g, f, Target{0.0, 0.0, 0.0}, x, z);
    if (r.cost == 0) { r.wx = centre(g.min_x, r.next % g.gx, g.cell); r.wz = centre(g.min_z, r.next / g.gx, g.cell); }
    return r;
}

// ---- a whole build by one worker: the host's path (tests/hostcheck/nav_grid.cpp); the kernel runs the same phases -------------------
// `x`: cells bytes of the caller's to stage the extra costs in, read only with `extra`.  Returns false, and a row of 0xFFFF, for an
// env the kernel would refuse.
inline bool build_grid_one(const MwNavArgs &a, const mw_nav_params &p, const uint8_t *blocked, const uint8_t *sources, const double *d_target,
                           const uint8_t *extra, size_t env, uint16_t *f, uint8_t *x, int sweeps, int *passes)
{
    const int gx = p.gx, gz = p.gz, cells = gx * gz, R = inflate_radius(p.cell, p.margin);
    if (passes) *passes = 0;
    stage_blocked(blocked + env * (size_t)cells, f, cells, 0, 1);
    if (R > 0) {
        for (int c = 0; c < cells; ++c)
            if (f[c] == MW_NAV_BLOCKED) inflate_from(f, gx, gz, c / gx, c % gx, R, p.cell, p.margin, 0, 1);
        fold(f, cells, 0, 1);
    }
    if (sources) mark_mask_sources(sources + env * (size_t)cells, f, cells, 0, 1);
    if (d_target) mark_sources(grid_build_grid(a, p, d_target, env), f, target_of(a, p, d_target, env), 0, 1);
    if (extra) stage_extra(extra + env * (size_t)cells, x, cells, 0, 1);
    int n = 0;
    bool settled = false;
    while (!settled && n < max_passes(gx, gz)) {
        bool changed = false;
        if (sweeps)
            for (int dir = 0; dir < 4; ++dir) changed = (extra ? sweep_x(f, x, gx, gz, dir, 0, 1) : sweep(f, gx, gz, dir, 0, 1)) || changed;
        else changed = extra ? jacobi_pass_x(f, x, gx, gz, 0, 1) : jacobi_pass(f, gx, gz, 0, 1);
        ++n;
        settled = !changed;
    }
    if (passes) *passes = n;
    const bool ok = settled && !too_far(f, gx, gz, 0, 1);
    if (!ok)
        for (int c = 0; c < cells; ++c) f[c] = (uint16_t)MW_NAV_BLOCKED;
    return ok;
}

}  // namespace mwnav
