// Egocentric map windows (mw_ego_map, include/mwengine.h; kernel: mw_ego.hip): a size x size window of points centred on each agent
// and turned with its heading — which of them lie in a wall, in an entity, in sight, and what a grid over the floor plan holds there.
// Plain C++: the kernel calls these functions with (lane, stride) of a workgroup, tests/hostcheck/ego_map.cpp calls window_one on the
// host, which runs the same phases with (0, 1).
//
// Nothing of the obstacle arithmetic is this file's own: the wall distance is mwnav::seg_dist, an entity's circle mwray::disc_of under
// radius = entity_pad, the heading the fan of mw_ray_cast at offset 0 (mwray::ray_of through mwseen::view_of), range and cone
// mwseen::in_cone, the line of sight mwseen::free_line over mwray::wall_of's walls — a ray from the origin to the point with max_t = 1 and
// radius 0.  All float64, + - * / floor and sqrt only, uncontracted, in this order (S = size, row r, column c):
//   lat = (((double)c + 0.5) - (double)S * 0.5) * cell
//   fwd = (((double)S * 0.5 - ((double)r + 0.5)) + back) * cell
//   f = (hx, hz), the heading (cos, -sin) of agent_dir, and rt = (-hz, hx); with MW_EGO_NORTH f = (0, -1) and rt = (1, 0)
//   px = ox + (fwd * fx + lat * rtx); pz = oz + (fwd * fz + lat * rtz); o the agent's position or the caller's row
//   WALL     0 iff px >= min_x && px <= max_x && pz >= min_z && pz <= max_z and seg_dist(seg, px, pz) < wall_radius for no segment
//   ENTITY   1 + the lowest listed slot with dx * dx + dz * dz < R * R, d = p - its (x, z), R = radius(slot) + entity_pad; else 0
//   VISIBLE  v = p - o; dist = sqrt(vx * vx + vz * vz) <= range; the cone about the agent's heading; a free line from o along v
//   sample   fi = floor((px - min_x) / src_cell), fj = floor((pz - min_z) / src_cell); inside iff fi >= 0.0 && fi < (double)gx &&
//            fj >= 0.0 && fj < (double)gz: src[(int)fj][(int)fi]; else fill
// Every test is written so that a NaN fails it: a NaN pose gives WALL 1, ENTITY 0, VISIBLE 0 and fill.  A cell has one owner per
// call, so the result does not depend on how cells are spread over lanes.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mwengine.h"
#include "mw_hd.h"
#include "mw_nav.h"
#include "mw_ray.h"
#include "mw_seen.h"

// The launch (mw_ego.hip; the arithmetic of it: mwpolicy::ego_launch): lanes per workgroup, and the bytes of LDS a raw segment takes
// beside the staged walls and discs of mw_ray.h.
#ifndef MW_EGO_THREADS          // (measurements: `make EXTRA=-DMW_EGO_THREADS=...`, a multiple of 64)
#define MW_EGO_THREADS 256
#endif
#define MW_EGO_SEG_BYTES 32

namespace mwego {

struct Window { double cell, back, wall_radius, entity_pad; int32_t size, planes, flags; };
// the sampled grid: src null = no sample; bytes 1 or 2 per element of src and out
struct Source { double cell; int32_t gx, gz, bytes; uint32_t fill; };
struct Frame { double ox, oz, fx, fz, rx, rz; mwseen::View view; };      // origin, the window's axes, the agent as sight sees it
// an env's obstacles as the asked planes need them (null / 0: not staged)
struct Staged { double *segs; mwray::Wall *walls; mwray::Disc *ents, *blockers; };

MW_HD int plane_count(int planes) { return (planes & 1) + ((planes >> 1) & 1) + ((planes >> 2) & 1); }
MW_HD int plane_index(int planes, int bit) { return plane_count(planes & (bit - 1)); }
// the slots the line of sight meets
MW_HD int blockers_of(const MwRayArgs &a, const Window &w) { return ((w.planes & MW_EGO_VISIBLE) && (w.flags & MW_EGO_ENTITIES)) ? a.w.E : 0; }
MW_HD mwseen::Sight sight_of(const Window &w, double range, double cos_half) { return {range, cos_half, (w.flags & MW_EGO_ENTITIES) ? MW_SEEN_ENTITIES : 0}; }

// bytes of the staged obstacles, from the engine's capacities: raw segments for WALL, discs under entity_pad for ENTITY, the casts' walls
// and discs for VISIBLE
MW_HD size_t staged_bytes(int max_segs, int max_ents, int planes)
{
    size_t n = 0;
    if (planes & MW_EGO_VISIBLE) n += (size_t)max_segs * MW_RAY_WALL_BYTES + (size_t)max_ents * MW_RAY_DISC_BYTES;
    if (planes & MW_EGO_WALL) n += (size_t)max_segs * MW_EGO_SEG_BYTES;
    if (planes & MW_EGO_ENTITY) n += (size_t)max_ents * MW_RAY_DISC_BYTES;
    return (n + 15) / 16 * 16;
}
// ... and where each part lies in a block of that size (every part a whole number of doubles)
MW_HD Staged carve(void *base, int max_segs, int max_ents, int planes)
{
    Staged st{nullptr, nullptr, nullptr, nullptr};
    char *p = static_cast<char *>(base);
    if (planes & MW_EGO_VISIBLE) {
        st.walls = reinterpret_cast<mwray::Wall *>(p);
        p += (size_t)max_segs * MW_RAY_WALL_BYTES;
        st.blockers = reinterpret_cast<mwray::Disc *>(p);
        p += (size_t)max_ents * MW_RAY_DISC_BYTES;
    }
    if (planes & MW_EGO_WALL) {
        st.segs = reinterpret_cast<double *>(p);
        p += (size_t)max_segs * MW_EGO_SEG_BYTES;
    }
    if (planes & MW_EGO_ENTITY) st.ents = reinterpret_cast<mwray::Disc *>(p);
    return st;
}

// the origin — the agent or row `env` of pos — and the axes; the heading is always the agent's
MW_HD Frame frame_of(const MwRayArgs &a, const Window &w, const mwseen::Sight &s, size_t env, const double *pos)
{
    Frame f;
    f.view = mwseen::view_of(a, s, env);
    f.ox = pos ? pos[env * 3] : f.view.ox;
    f.oz = pos ? pos[env * 3 + 2] : f.view.oz;
    f.view.ox = f.ox;
    f.view.oz = f.oz;
    const bool north = (w.flags & MW_EGO_NORTH) != 0;
    f.fx = north ? 0.0 : f.view.hx;
    f.fz = north ? -1.0 : f.view.hz;
    f.rx = north ? 1.0 : -f.view.hz;
    f.rz = north ? 0.0 : f.view.hx;
    return f;
}
// the point of row r, column c
MW_HD void point_of(const Frame &f, const Window &w, int r, int c, double &px, double &pz)
{
    const double S = (double)w.size;
    const double lat = (((double)c + 0.5) - S * 0.5) * w.cell;
    const double fwd = ((S * 0.5 - ((double)r + 0.5)) + w.back) * w.cell;
    px = f.ox + (fwd * f.fx + lat * f.rx);
    pz = f.oz + (fwd * f.fz + lat * f.rz);
}
// WALL: outside the extent, or closer than wall_radius to a segment (the walk stops at the first one)
MW_HD uint8_t wall_at(const mwnav::Grid &g, const double *segs, int ns, double wall_radius, double px, double pz)
{
    if (!(px >= g.min_x && px <= g.max_x && pz >= g.min_z && pz <= g.max_z)) return 1;
    for (int i = 0; i < ns; ++i)
        if (mwnav::seg_dist(segs + (size_t)i * 4, px, pz) < wall_radius) return 1;
    return 0;
}
// ENTITY: 1 + the lowest listed slot whose padded circle holds the point
MW_HD uint8_t entity_at(const mwray::Disc *ents, int ne, double px, double pz)
{
    for (int k = 0; k < ne; ++k) {
        if (ents[k].listed == 0.0) continue;
        const double dx = px - ents[k].x, dz = pz - ents[k].z;
        if (dx * dx + dz * dz < ents[k].R * ents[k].R) return (uint8_t)(1 + k);
    }
    return 0;
}
// VISIBLE: tests 2 - 4 of mw_seen_update with the point in the cell centre's place
MW_HD uint8_t visible_at(const Frame &f, const mwseen::Sight &s, const mwray::Wall *walls, int ns, const mwray::Disc *blockers, int nb, double px, double pz)
{
    const mwray::Ray r{f.ox, f.oz, px - f.ox, pz - f.oz};
    return mwseen::in_cone(f.view, s, r) && mwseen::free_line(r, walls, ns, blockers, nb) ? 1 : 0;
}
// the sample: the source's element under the point, or fill
MW_HD uint32_t sample_at(const mwnav::Grid &g, const Source &q, const void *src_row, double px, double pz)
{
    const double fi = floor((px - g.min_x) / q.cell), fj = floor((pz - g.min_z) / q.cell);
    if (!(fi >= 0.0 && fi < (double)q.gx && fj >= 0.0 && fj < (double)q.gz)) return q.fill;
    const size_t at = (size_t)(int)fj * (size_t)q.gx + (size_t)(int)fi;
    return q.bytes == 2 ? (uint32_t) static_cast<const uint16_t *>(src_row)[at] : (uint32_t) static_cast<const uint8_t *>(src_row)[at];
}

// ---- the phases of a call; `lane` of `stride` workers share each ------------------------------------------------------------------

// the env's obstacles, only those the asked planes need
MW_HD void stage(const MwRayArgs &a, const Window &w, const mwseen::Sight &s, size_t env, const Staged &st, int lane, int stride)
{
    const double *segs = mwnav::segs_of(a.w, env);
    const int ns = mwnav::nsegs_of(a.w, env);
    if (w.planes & MW_EGO_VISIBLE) mwseen::stage(a, s, env, st.walls, st.blockers, lane, stride);
    if (w.planes & MW_EGO_WALL)
        for (int i = lane; i < ns * 4; i += stride) st.segs[i] = segs[i];
    if (w.planes & MW_EGO_ENTITY) {
        const mw_ray_params padded{1.0, w.entity_pad, 1, MW_RAY_ENTITIES};
        for (int k = lane; k < a.w.E; k += stride) st.ents[k] = mwray::disc_of(a, padded, env, k);
    }
}
// the cells of the window, row by row: consecutive workers take consecutive columns.  planes: the env's [P][S][S] bytes; src_row /
// out_row: the env's rows of the source and the sample (null: no sample)
MW_HD void cells(const MwRayArgs &a, const Window &w, const mwseen::Sight &s, const Source &q, size_t env, const Frame &f, const Staged &st,
                 uint8_t *planes, const void *src_row, void *out_row, int lane, int stride)
{
    const mwnav::Grid g = mwnav::grid_of(a.w, mw_nav_params{q.cell, 0.0, 0.0, q.gx, q.gz, 0, 0}, env);
    const int S = w.size, n = S * S, ns = mwnav::nsegs_of(a.w, env), nb = blockers_of(a, w);
    uint8_t *wall = (w.planes & MW_EGO_WALL) ? planes + (size_t)plane_index(w.planes, MW_EGO_WALL) * n : nullptr;
    uint8_t *entity = (w.planes & MW_EGO_ENTITY) ? planes + (size_t)plane_index(w.planes, MW_EGO_ENTITY) * n : nullptr;
    uint8_t *visible = (w.planes & MW_EGO_VISIBLE) ? planes + (size_t)plane_index(w.planes, MW_EGO_VISIBLE) * n : nullptr;
    for (int k = lane; k < n; k += stride) {
        double px, pz;
        point_of(f, w, k / S, k % S, px, pz);
        if (wall) wall[k] = wall_at(g, st.segs, ns, w.wall_radius, px, pz);
        if (entity) entity[k] = entity_at(st.ents, a.w.E, px, pz);
        if (visible) visible[k] = visible_at(f, s, st.walls, ns, st.blockers, nb, px, pz);
        if (out_row) {
            const uint32_t v = sample_at(g, q, src_row, px, pz);
            if (q.bytes == 2) static_cast<uint16_t *>(out_row)[k] = (uint16_t)v;
            else static_cast<uint8_t *>(out_row)[k] = (uint8_t)v;
        }
    }
}

// ---- a whole call for one env by one worker: the host's path (tests/hostcheck/ego_map.cpp); the kernel runs the same phases ---------
// scratch: staged_bytes(max_segs, E, planes) bytes, aligned for doubles
inline void window_one(const MwRayArgs &a, const Window &w, const mwseen::Sight &s, const Source &q, size_t env, const double *pos, void *scratch,
                       uint8_t *planes, const void *src_row, void *out_row)
{
    const Staged st = carve(scratch, a.w.max_segs, a.w.E, w.planes);
    stage(a, w, s, env, st, 0, 1);
    cells(a, w, s, q, env, frame_of(a, w, s, env, pos), st, planes, src_row, out_row, 0, 1);
}

}  // namespace mwego
