// Explored-area maps (mw_seen_update, include/mwengine.h; kernel: mw_seen.hip): which cells of a nav grid over its floor plan each
// agent has seen so far, and how many of them are new.  Plain C++: the kernel calls these functions per lane or with (lane, stride) of
// a workgroup, tests/hostcheck/seen_map.cpp calls update_one on the host, which runs the same phases with (0, 1).
//
// Nothing of the arithmetic is this file's own: the grid is mw_nav.h's (grid_of, centre, beyond, covers, box_of), the line of sight a
// ray of mw_ray.h (wall_of, disc_of, ray_wall, ray_circle, take) from the agent to the cell's centre with max_t = 1 and radius 0, the
// heading the fan of mw_ray_cast at offset 0 (ray_of).  All float64, + - * / and sqrt only, uncontracted, in this order:
//   1  the cell's centre c is not beyond the extent
//   2  v = c - o; dist = sqrt(vx * vx + vz * vz); dist <= range
//   3  cos_half == -1.0, or dist == 0.0, or vx * hx + vz * hz >= cos_half * dist
//   4  the ray (o, v) meets nothing at t < 1: walls in index order, then — with MW_SEEN_ENTITIES — the listed slots
// Every test is written so that a NaN fails it: a NaN pose marks nothing.  A cell has one owner per call and the counts are integer
// sums, so the result does not depend on how cells are spread over lanes.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mwengine.h"
#include "mw_hd.h"
#include "mw_nav.h"
#include "mw_ray.h"

// The launch (mw_seen.hip; the arithmetic of it: mwpolicy::seen_launch): lanes per workgroup, the entries of the candidate list a round
// of the kernel fills, and the bytes of LDS behind the staged walls and discs: the list (a uint16 cell index per entry) and four words
// (the two list lengths that alternate between rounds, the count of new cells, one spare).
#ifndef MW_SEEN_THREADS         // (measurements: `make EXTRA=-DMW_SEEN_THREADS=...`, a multiple of 64)
#define MW_SEEN_THREADS 128
#endif
#define MW_SEEN_CANDS 1024
#define MW_SEEN_TAIL_BYTES (MW_SEEN_CANDS * 2 + 16)

namespace mwseen {

struct Sight { double range, cos_half; int32_t flags; };
struct View { double ox, oz, hx, hz; };     // the agent's position and heading (cos, -sin)

// the ray parameters under which walls and discs are staged and met: a plain ray to the cell's centre
MW_HD mw_ray_params ray_params(const Sight &s) { return {1.0, 0.0, 1, (s.flags & MW_SEEN_ENTITIES) ? MW_RAY_ENTITIES : 0}; }

// the agent as mw_ray_cast's fan sees it at offset 0
MW_HD View view_of(const MwRayArgs &a, const Sight &s, size_t env)
{
    const double off0 = 0.0;
    const mwray::Ray r = mwray::ray_of(a, ray_params(s), env, 0, nullptr, nullptr, &off0);
    return {r.ox, r.oz, r.dx, r.dz};
}
// the cells whose centre can lie within range of the agent (mwnav::axis_range: a NaN pose gives the whole grid, where every test fails)
MW_HD mwnav::Box box_of(const mwnav::Grid &g, const View &v, const Sight &s) { return mwnav::box_of(g, v.ox, v.ox, v.oz, v.oz, s.range); }

// the ray from the agent to the centre of cell (j, i)
MW_HD mwray::Ray ray_to(const mwnav::Grid &g, const View &v, int j, int i)
{
    return {v.ox, v.oz, mwnav::centre(g.min_x, i, g.cell) - v.ox, mwnav::centre(g.min_z, j, g.cell) - v.oz};
}
// tests 2 - 3 of the ray r from the agent to a point: within range and inside the cone about the heading (mw_ego.h asks it of its
// window points too)
MW_HD bool in_cone(const View &v, const Sight &s, const mwray::Ray &r)
{
    const double dist = sqrt(r.dx * r.dx + r.dz * r.dz);
    if (!(dist <= s.range)) return false;
    return s.cos_half == -1.0 || dist == 0.0 || r.dx * v.hx + r.dz * v.hz >= s.cos_half * dist;
}
// tests 1 - 3: no division, no obstacle
MW_HD bool in_sight(const mwnav::Grid &g, const View &v, const Sight &s, int j, int i)
{
    if (mwnav::beyond(g, j, i)) return false;
    return in_cone(v, s, ray_to(g, v, j, i));
}
// test 4 on staged obstacles.  mw_ray_cast's result is h = (1, -1) exactly when no candidate was taken, and a taken candidate is never
// given back: the walk may stop at the first one.
MW_HD bool free_line(const mwray::Ray &r, const mwray::Wall *walls, int ns, const mwray::Disc *discs, int ne)
{
    mwray::Hit h{1.0, -1};
    if (mwray::bad_ray(r)) return false;        // (never a cell in sight: test 2 fails for a NaN)
    for (int i = 0; i < ns; ++i) {      // (two walls in flight per lane, as in mw_ray_lanes_kernel, were measured: no gain here)
        mwray::take(h, mwray::ray_wall(r, walls[i], 0.0), i);
        if (h.code != -1) return false;
    }
    for (int k = 0; k < ne; ++k) {
        if (discs[k].listed == 0.0) continue;
        mwray::take(h, mwray::ray_circle(r, discs[k].x, discs[k].z, discs[k].R), MW_RAY_ENT + k);
        if (h.code != -1) return false;
    }
    return h.t == 1.0;
}
// a visible cell: 1 when it went 0 -> 1
MW_HD int set_cell(uint8_t *row, int c)
{
    if (row[c] != 0) return 0;
    row[c] = 1;
    return 1;
}

// ---- the phases of a call; `lane` of `stride` workers share each ------------------------------------------------------------------

MW_HD int ents_of(const MwRayArgs &a, const Sight &s) { return (s.flags & MW_SEEN_ENTITIES) ? a.w.E : 0; }
// walls[max_segs], discs[E]: the env's obstacles as the casts see them
MW_HD void stage(const MwRayArgs &a, const Sight &s, size_t env, mwray::Wall *walls, mwray::Disc *discs, int lane, int stride)
{
    const double *segs = mwnav::segs_of(a.w, env);
    const int ns = mwnav::nsegs_of(a.w, env), ne = ents_of(a, s);
    const mw_ray_params rp = ray_params(s);
    for (int i = lane; i < ns; i += stride) walls[i] = mwray::wall_of(segs + (size_t)i * 4, 0.0);
    for (int k = lane; k < ne; k += stride) discs[k] = mwray::disc_of(a, rp, env, k);
}
MW_HD void zero_row(uint8_t *row, int cells, int lane, int stride)
{
    for (int c = lane; c < cells; c += stride) row[c] = 0;
}
// the cells of the box, all four tests at once: the cells this worker turned 0 -> 1
MW_HD int mark(const mwnav::Grid &g, const View &v, const Sight &s, const mwnav::Box &b, const mwray::Wall *walls, int ns, const mwray::Disc *discs,
               int ne, uint8_t *row, int lane, int stride)
{
    const int w = mwnav::box_w(b), n = mwnav::box_cells(b);
    int newly = 0;
    for (int k = lane; k < n; k += stride) {
        const int j = b.j0 + k / w, i = b.i0 + k % w;
        if (in_sight(g, v, s, j, i) && free_line(ray_to(g, v, j, i), walls, ns, discs, ne)) newly += set_cell(row, j * g.gx + i);
    }
    return newly;
}

// ---- a whole call for one env by one worker: the host's path (tests/hostcheck/seen_map.cpp); the kernel runs the same phases ---------
// walls and discs are the caller's scratch, max_segs and E entries; returns false for an env whose extent the grid does not cover
inline bool update_one(const MwRayArgs &a, const mw_nav_params &p, const Sight &s, size_t env, bool clear, mwray::Wall *walls, mwray::Disc *discs,
                       uint8_t *row, int32_t *count, int32_t *newly)
{
    const mwnav::Grid g = mwnav::grid_of(a.w, p, env);
    if (!mwnav::covers(g)) {
        zero_row(row, g.gx * g.gz, 0, 1);
        *count = 0;
        if (newly) *newly = 0;
        return false;
    }
    stage(a, s, env, walls, discs, 0, 1);
    if (clear) zero_row(row, g.gx * g.gz, 0, 1);
    const View v = view_of(a, s, env);
    const int n = mark(g, v, s, box_of(g, v, s), walls, mwnav::nsegs_of(a.w, env), discs, ents_of(a, s), row, 0, 1);
    *count = (clear ? 0 : *count) + n;
    if (newly) *newly = n;
    return true;
}

}  // namespace mwseen
