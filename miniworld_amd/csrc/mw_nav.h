// Navigation fields (mw_nav_build / mw_nav_query, include/mwengine.h; kernels: mw_nav.hip): the grid over an env's floor plan, which
// of its cells the walls and entities block, the cells a target is reached from, the relaxation of the 5 / 7 move costs to their fixed
// point, and the query.  Plain C++: the kernels call these functions with (lane, stride) of a workgroup, tests/hostcheck/nav_field.cpp
// calls the same functions with (0, 1) on the host.
//
// Arithmetic, all float64, no contraction (the build's -ffp-contract=off; a plain host compiler has no fused operations to use):
//   centre(lo, i)        lo + ((double)i + 0.5) * cell
//   wall distance        the closest-point distance of intersect_wave (mw_setup_common.h; math.py:30-62), restated below in the
//                        same order of operations — the step kernels' code is not shared, their code objects stay as they are
//   blocked by a wall    distance < agent_radius + margin
//   blocked by a slot    sqrt(dx*dx + dz*dz) < (agent_radius + radius) + margin, dx = pos - centre
//   source               sqrt(dx*dx + dz*dz) < reach, dx = target - centre; a slot's reach is near()'s threshold (near_agent)
// The field's fixed point is unique (costs only fall, from one start), so the order in which cells are relaxed never shows.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mwengine.h"
#include "mw_hd.h"

// what the kernels need of the engine (MwArgs' members of the same names), by value
struct MwNavArgs {
    const double *segs;         // [sets][max_segs][4]
    const int32_t *nsegs;       // [sets]
    const double *extent;       // [4][N]
    const int32_t *ekind;       // [E][N]
    const double *epos;         // [3][E][N]
    const double *egeom;        // [9][E][N]
    const int32_t *carry;       // [N]
    const double *ax, *az;      // [N]
    uint32_t *status;
    int32_t N, E, max_segs, shared_geom;
    double agent_radius, max_forward_step;
};

namespace mwnav {

constexpr int kNone = 0x7FFFFFFF;       // "no path this way"

struct Grid {
    double min_x, max_x, min_z, max_z, cell;
    int gx, gz;
};
struct Target {
    double x, z, reach;
};
struct Box {        // cells i0 .. i1 x j0 .. j1, empty when a first exceeds a last
    int i0, i1, j0, j1;
};
struct Answer {
    int32_t cost, next;
    double wx, wz;
};

MW_HD Grid grid_of(const MwNavArgs &a, const mw_nav_params &p, size_t env)
{
    const size_t N = (size_t)a.N;
    return {a.extent[env], a.extent[N + env], a.extent[2 * N + env], a.extent[3 * N + env], p.cell, p.gx, p.gz};
}
MW_HD const double *segs_of(const MwNavArgs &a, size_t env) { return a.segs + (a.shared_geom ? 0 : env) * (size_t)a.max_segs * 4; }
MW_HD int nsegs_of(const MwNavArgs &a, size_t env)
{
    const int n = a.nsegs[a.shared_geom ? 0 : env];
    return n < 0 ? 0 : (n > a.max_segs ? a.max_segs : n);
}
MW_HD double ent_pos(const MwNavArgs &a, size_t env, int slot, int k) { return a.epos[((size_t)k * (size_t)a.E + (size_t)slot) * (size_t)a.N + env]; }
MW_HD double ent_radius(const MwNavArgs &a, size_t env, int slot) { return a.egeom[((size_t)7 * (size_t)a.E + (size_t)slot) * (size_t)a.N + env]; }
MW_HD int ent_kind(const MwNavArgs &a, size_t env, int slot) { return a.ekind[(size_t)slot * (size_t)a.N + env]; }

MW_HD double centre(double lo, int i, double cell) { return lo + ((double)i + 0.5) * cell; }
// the grid reaches past the extent on both axes: the first cell beyond it would be blocked anyway
MW_HD bool covers(const Grid &g) { return centre(g.min_x, g.gx, g.cell) > g.max_x && centre(g.min_z, g.gz, g.cell) > g.max_z; }
MW_HD bool beyond(const Grid &g, int j, int i) { return centre(g.min_x, i, g.cell) > g.max_x || centre(g.min_z, j, g.cell) > g.max_z; }

// closest-point distance from (x, z) to the segment s = (ax, az, bx, bz): intersect_wave's lines
MW_HD double seg_dist(const double *s, double x, double z)
{
    const double sax = s[0], saz = s[1], sbx = s[2], sbz = s[3];
    const double abx = sbx - sax, abz = sbz - saz;
    const double apx = x - sax, apz = z - saz;
    const double dap = apx * abx + apz * abz;
    const double dab = abx * abx + abz * abz;
    double t = dap / dab;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double cx = sax + t * abx, cz = saz + t * abz;
    const double dx = cx - x, dz = cz - z;
    return sqrt(dx * dx + dz * dz);
}

// near()'s threshold for a slot (near_agent, mw_setup_common.h): radius + agent_radius + 1.1 * max_forward_step, in float32 — left to
// right, the product rounded first — for a mesh entity
MW_HD double slot_reach(double radius, double agent_radius, double max_forward_step, bool mesh)
{
    const double more = 1.1 * max_forward_step;
    return mesh ? (double)(((float)radius + (float)agent_radius) + (float)more) : radius + agent_radius + more;
}
// the target of env `env`: its row of the caller's points, or the slot
MW_HD Target target_of(const MwNavArgs &a, const mw_nav_params &p, const double *d_target, size_t env)
{
    if (d_target) return {d_target[env * 3], d_target[env * 3 + 2], p.reach};
    const int s = p.target_slot;
    return {ent_pos(a, env, s, 0), ent_pos(a, env, s, 2), slot_reach(ent_radius(a, env, s), a.agent_radius, a.max_forward_step, ent_kind(a, env, s) == MW_ENT_MESH)};
}
// does slot `slot` block cells at all
MW_HD bool slot_blocks(const MwNavArgs &a, const mw_nav_params &p, bool slot_target, size_t env, int slot)
{
    return (p.flags & MW_NAV_ENTITIES) && ent_kind(a, env, slot) != MW_ENT_NONE && slot != a.carry[env] && !(slot_target && slot == p.target_slot);
}

// The cells whose centre can lie within r of the box lo .. hi of one axis, with a cell to spare on either side (the exact test
// decides; this only bounds the work), clamped to 0 .. n - 1.  The clamps come before the conversion: a NaN or a huge value becomes a
// bound of the grid, never an int out of range.
MW_HD void axis_range(double lo, double hi, double r, double org, double cell, int n, int &first, int &last)
{
    double a = floor((lo - r - org) / cell) - 1.0, b = floor((hi + r - org) / cell) + 1.0;
    a = a > 0.0 ? a : 0.0;
    a = a < (double)n ? a : (double)n;
    b = b < (double)(n - 1) ? b : (double)(n - 1);
    b = b > -1.0 ? b : -1.0;
    first = (int)a;
    last = (int)b;
}
MW_HD Box box_of(const Grid &g, double lox, double hix, double loz, double hiz, double r)
{
    Box b;
    axis_range(lox, hix, r, g.min_x, g.cell, g.gx, b.i0, b.i1);
    axis_range(loz, hiz, r, g.min_z, g.cell, g.gz, b.j0, b.j1);
    return b;
}
MW_HD int box_w(const Box &b) { return b.i1 >= b.i0 ? b.i1 - b.i0 + 1 : 0; }
MW_HD int box_cells(const Box &b) { return b.j1 >= b.j0 ? box_w(b) * (b.j1 - b.j0 + 1) : 0; }

// ---- the phases of a build; `lane` of `stride` workers share each ----------------------------------------------------------------

// every cell unreached, or blocked where its centre lies beyond the extent (or everywhere: the row of an env that is refused)
MW_HD void init_cells(const Grid &g, uint16_t *f, bool all_blocked, int lane, int stride)
{
    for (int c = lane; c < g.gx * g.gz; c += stride)
        f[c] = (uint16_t)(all_blocked || beyond(g, c / g.gx, c % g.gx) ? MW_NAV_BLOCKED : MW_NAV_UNREACHED);
}
// one wall: the cells of its inflated bounding box whose centre is closer than r (plain same-value stores: idempotent, any order)
MW_HD void block_seg(const Grid &g, uint16_t *f, const double *s, double r, int lane, int stride)
{
    const Box b = box_of(g, s[0] < s[2] ? s[0] : s[2], s[0] < s[2] ? s[2] : s[0], s[1] < s[3] ? s[1] : s[3], s[1] < s[3] ? s[3] : s[1], r);
    const int w = box_w(b), n = box_cells(b);
    for (int k = lane; k < n; k += stride) {
        const int j = b.j0 + k / w, i = b.i0 + k % w;
        if (seg_dist(s, centre(g.min_x, i, g.cell), centre(g.min_z, j, g.cell)) < r) f[j * g.gx + i] = (uint16_t)MW_NAV_BLOCKED;
    }
}
// one entity at (ex, ez)
MW_HD void block_ent(const Grid &g, uint16_t *f, double ex, double ez, double r, int lane, int stride)
{
    const Box b = box_of(g, ex, ex, ez, ez, r);
    const int w = box_w(b), n = box_cells(b);
    for (int k = lane; k < n; k += stride) {
        const int j = b.j0 + k / w, i = b.i0 + k % w;
        const double dx = ex - centre(g.min_x, i, g.cell), dz = ez - centre(g.min_z, j, g.cell);
        if (sqrt(dx * dx + dz * dz) < r) f[j * g.gx + i] = (uint16_t)MW_NAV_BLOCKED;
    }
}
// the sources: behind the occupancy, which they read
MW_HD void mark_sources(const Grid &g, uint16_t *f, const Target &t, int lane, int stride)
{
    const Box b = box_of(g, t.x, t.x, t.z, t.z, t.reach);
    const int w = box_w(b), n = box_cells(b);
    for (int k = lane; k < n; k += stride) {
        const int j = b.j0 + k / w, i = b.i0 + k % w;
        const double dx = t.x - centre(g.min_x, i, g.cell), dz = t.z - centre(g.min_z, j, g.cell);
        if (sqrt(dx * dx + dz * dz) < t.reach && f[j * g.gx + i] != MW_NAV_BLOCKED) f[j * g.gx + i] = 0;
    }
}

// ---- relaxation ------------------------------------------------------------------------------------------------------------------

MW_HD int at(const uint16_t *f, int gx, int gz, int j, int i) { return ((unsigned)j < (unsigned)gz && (unsigned)i < (unsigned)gx) ? (int)f[j * gx + i] : MW_NAV_BLOCKED; }
MW_HD int via(int nb, int step) { return nb < MW_NAV_UNREACHED ? nb + step : kNone; }
MW_HD int lower(int a, int b) { return a < b ? a : b; }
// the cheapest way into (j, i) through its 8 neighbours as they stand: kNone when none of them is reached
MW_HD int best_via(const uint16_t *f, int gx, int gz, int j, int i)
{
    const int u = at(f, gx, gz, j - 1, i), d = at(f, gx, gz, j + 1, i), l = at(f, gx, gz, j, i - 1), r = at(f, gx, gz, j, i + 1);
    int b = lower(lower(via(u, 5), via(d, 5)), lower(via(l, 5), via(r, 5)));
    if (u != MW_NAV_BLOCKED && l != MW_NAV_BLOCKED) b = lower(b, via(at(f, gx, gz, j - 1, i - 1), 7));
    if (u != MW_NAV_BLOCKED && r != MW_NAV_BLOCKED) b = lower(b, via(at(f, gx, gz, j - 1, i + 1), 7));
    if (d != MW_NAV_BLOCKED && l != MW_NAV_BLOCKED) b = lower(b, via(at(f, gx, gz, j + 1, i - 1), 7));
    if (d != MW_NAV_BLOCKED && r != MW_NAV_BLOCKED) b = lower(b, via(at(f, gx, gz, j + 1, i + 1), 7));
    return b;
}
// A whole-grid pass: every unblocked cell takes the cheapest way in when that lowers it.  A cost of 0xFFFE or more is never stored
// (it would read as "unreached"); too_far finds such cells at the fixed point.  Workers may read each other's newest values.
MW_HD bool jacobi_pass(uint16_t *f, int gx, int gz, int lane, int stride)
{
    bool changed = false;
    for (int c = lane; c < gx * gz; c += stride) {
        const int v = f[c];
        if (v == MW_NAV_BLOCKED) continue;
        const int b = best_via(f, gx, gz, c / gx, c % gx);
        if (b < v && b < MW_NAV_UNREACHED) { f[c] = (uint16_t)b; changed = true; }
    }
    return changed;
}
// A directional sweep of one line, the cost carried in a register: line `line` of `nlines`, n cells long; a step along the line moves
// `sk` cells in the array, a step to the next line `sl` (rows: 1, gx; columns: gx, 1); rev = from the far end.  Cell k takes the
// cheapest of: the cell before it (5), its two neighbours in the lines beside (5), and the two cells diagonally behind (7, both cells
// between free) — the side values of the step before serve as the diagonal ones.  Forward and reverse sweeps of the rows alone look
// at all 8 neighbours of every cell, so a round of sweeps that changes nothing has found the fixed point.
MW_HD bool sweep_line(uint16_t *f, int n, int nlines, int line, int sk, int sl, bool rev)
{
    bool changed = false;
    int prev = MW_NAV_BLOCKED, pu = MW_NAV_BLOCKED, pd = MW_NAV_BLOCKED;
    const bool hu = line > 0, hd = line < nlines - 1;
    for (int t = 0; t < n; ++t) {
        const int c = line * sl + (rev ? n - 1 - t : t) * sk;
        int v = f[c];
        const int u = hu ? (int)f[c - sl] : MW_NAV_BLOCKED, d = hd ? (int)f[c + sl] : MW_NAV_BLOCKED;
        if (v != MW_NAV_BLOCKED) {
            int b = lower(via(prev, 5), lower(via(u, 5), via(d, 5)));
            if (prev != MW_NAV_BLOCKED && u != MW_NAV_BLOCKED) b = lower(b, via(pu, 7));
            if (prev != MW_NAV_BLOCKED && d != MW_NAV_BLOCKED) b = lower(b, via(pd, 7));
            if (b < v && b < MW_NAV_UNREACHED) { f[c] = (uint16_t)b; v = b; changed = true; }
        }
        prev = v; pu = u; pd = d;
    }
    return changed;
}
// sweep direction `dir` (0 rows forward, 1 rows back, 2 columns forward, 3 columns back) over the lines lane, lane + stride, ...
MW_HD bool sweep(uint16_t *f, int gx, int gz, int dir, int lane, int stride)
{
    const bool rows = dir < 2;
    const int nlines = rows ? gz : gx, n = rows ? gx : gz, sk = rows ? 1 : gx, sl = rows ? gx : 1;
    bool changed = false;
    for (int line = lane; line < nlines; line += stride) changed = sweep_line(f, n, nlines, line, sk, sl, (dir & 1) != 0) || changed;
    return changed;
}
// at the fixed point: an unreached cell with a way in would cost 0xFFFE or more
MW_HD bool too_far(const uint16_t *f, int gx, int gz, int lane, int stride)
{
    bool far = false;
    for (int c = lane; c < gx * gz; c += stride)
        if (f[c] == MW_NAV_UNREACHED && best_via(f, gx, gz, c / gx, c % gx) != kNone) far = true;
    return far;
}
// the hard bound on passes of either kind: a pass that changes anything lowers a cell, and the longest chain of first arrivals is one
// cell per pass
MW_HD int max_passes(int gx, int gz) { return gx * gz + 1; }

// ---- the query -------------------------------------------------------------------------------------------------------------------

MW_HD int cell_of(double x, double org, double cell, int n)
{
    double c = floor((x - org) / cell);
    c = c > 0.0 ? c : 0.0;      // (a NaN: cell 0)
    c = c < (double)(n - 1) ? c : (double)(n - 1);
    return (int)c;
}
// (dj, di) of neighbour k, in the order ties are broken in
MW_HD int nb_dj(int k) { return k == 0 ? -1 : k == 1 ? 1 : k < 4 ? 0 : k < 6 ? -1 : 1; }
MW_HD int nb_di(int k) { return k < 2 ? 0 : k == 2 ? -1 : k == 3 ? 1 : (k & 1) ? 1 : -1; }

MW_HD Answer query(const Grid &g, const uint16_t *f, const Target &t, double x, double z)
{
    const int gx = g.gx, gz = g.gz;
    int j = cell_of(z, g.min_z, g.cell, gz), i = cell_of(x, g.min_x, g.cell, gx);
    int v = at(f, gx, gz, j, i);
    if (v == MW_NAV_BLOCKED) {
        // an agent may stand between agent_radius and agent_radius + margin from a wall: the best unblocked cell around stands in
        int bj = j, bi = i;
        for (int k = 0; k < 8; ++k) {
            const int w = at(f, gx, gz, j + nb_dj(k), i + nb_di(k));
            if (w < v) { v = w; bj = j + nb_dj(k); bi = i + nb_di(k); }
        }
        j = bj; i = bi;
    }
    if (v >= MW_NAV_UNREACHED) return {-1, -1, x, z};
    if (v == 0) return {0, j * gx + i, t.x, t.z};
    int best = v, nj = j, ni = i;
    for (int k = 0; k < 8; ++k) {
        const int dj = nb_dj(k), di = nb_di(k);
        const int w = at(f, gx, gz, j + dj, i + di);
        if (w >= best) continue;
        if (k >= 4 && (at(f, gx, gz, j + dj, i) == MW_NAV_BLOCKED || at(f, gx, gz, j, i + di) == MW_NAV_BLOCKED)) continue;
        best = w; nj = j + dj; ni = i + di;
    }
    return {v, nj * gx + ni, centre(g.min_x, ni, g.cell), centre(g.min_z, nj, g.cell)};
}

// ---- a whole build by one worker: the host's path (tests/hostcheck/nav_field.cpp); the kernel runs the same phases ----------------
// returns false, and a row of 0xFFFF, for an env the kernel would refuse; sweeps != 0: directional sweeps, else whole-grid passes
inline bool build_one(const MwNavArgs &a, const mw_nav_params &p, const double *d_target, size_t env, uint16_t *f, int sweeps, int *passes)
{
    const Grid g = grid_of(a, p, env);
    bool ok = covers(g);
    init_cells(g, f, !ok, 0, 1);
    if (passes) *passes = 0;
    if (!ok) return false;
    const double *segs = segs_of(a, env);
    for (int s = 0; s < nsegs_of(a, env); ++s) block_seg(g, f, segs + (size_t)s * 4, a.agent_radius + p.margin, 0, 1);
    for (int s = 0; s < a.E; ++s)
        if (slot_blocks(a, p, !d_target, env, s)) block_ent(g, f, ent_pos(a, env, s, 0), ent_pos(a, env, s, 2), a.agent_radius + ent_radius(a, env, s) + p.margin, 0, 1);
    mark_sources(g, f, target_of(a, p, d_target, env), 0, 1);
    int n = 0;
    bool settled = false;
    while (!settled && n < max_passes(g.gx, g.gz)) {
        bool changed = false;
        if (sweeps) for (int dir = 0; dir < 4; ++dir) changed = sweep(f, g.gx, g.gz, dir, 0, 1) || changed;
        else changed = jacobi_pass(f, g.gx, g.gz, 0, 1);
        ++n;
        settled = !changed;
    }
    if (passes) *passes = n;
    ok = settled && !too_far(f, g.gx, g.gz, 0, 1);
    if (!ok) init_cells(g, f, true, 0, 1);
    return ok;
}

}  // namespace mwnav
