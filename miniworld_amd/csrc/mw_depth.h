// Depth projection (mw_depth_project, include/mwengine.h; kernel: mw_depth.hip): the map a depth sensor gives.  Every pixel of an env's
// depth map (float32 [H][W], eye depth in metres, row 0 the top: what mw_step / mw_render write) is unprojected with the env's own camera
// and pose, classed by its height — floor, obstacle, neither — and counted into a cell of an egocentric window (mw_ego_map's) or of a
// grid over the floor plan (mw_nav_build's).  It stands in for what a user does with get_depth_map (opengl.py:400-435) under the camera of
// miniworld.py:1200-1222 and entity.py:477-503.  Plain C++: the kernel calls these functions with (lane, stride) of a workgroup,
// tests/hostcheck/depth_project.cpp calls window_one / map_one on the host, which run the same phases with (0, 1).
//
// The heading and the axes are mwego::frame_of's, the grid mwnav::grid_of's, sin and cos mw::sincos_det.  All float64, only + - * /,
// floor and sincos_det, uncontracted, in this order (W x H the frame, pixel row v from the top, column u):
//   per env   o = the agent's (x, z); f = (hx, hz) the heading, rt = (-hz, hx); cam = (height, fwd_disp, pitch_deg, fov_deg)
//             (sp, cp) = sincos_det(pitch_deg * M_PI / 180.0); (sh, ch) = sincos_det(fov_deg * 0.5 * M_PI / 180.0); th = sh / ch
//             aspect = (double)W / (double)H; tx = th * aspect
//   per pixel d = (double)depth[v][u]; dropped unless d >= min_range && d <= max_range (a NaN is dropped)
//             xn = (((double)u + sub_x) * 2.0) / (double)W - 1.0;  yn = 1.0 - (((double)v + sub_y) * 2.0) / (double)H
//             lat = (xn * tx) * d;  yc = (yn * th) * d
//             fwd = fwd_disp + (d * cp - yc * sp);  up = height + (d * sp + yc * cp)       (up: above the agent's own pos.y)
//             floor iff up >= -floor_tol && up <= floor_tol; obstacle iff up > floor_tol && up <= top; else dropped
//             px = ox + (fwd * fx + lat * rtx);  pz = oz + (fwd * fz + lat * rtz)
//   window    a = lat, b = fwd; with MW_EGO_NORTH a = px - ox, b = -(pz - oz)
//             c = floor(a / cell + (double)S * 0.5);  r = floor(((double)S * 0.5 + back) - b / cell)
//             kept iff c >= 0.0 && c < (double)S && r >= 0.0 && r < (double)S; the cell is [(int)r][(int)c]
//   map       fi = floor((px - min_x) / cell), fj = floor((pz - min_z) / cell); kept iff fi >= 0.0 && fi < (double)gx && fj >= 0.0 &&
//             fj < (double)gz (mwego::sample_at's test); the cell is [(int)fj][(int)fi]
// (sub_x, sub_y): where in the pixel the depth was sampled.  The engine resolves a frame's depth from sample 0 of its multisample pattern
// ("G8 resolve"), (sx, sy) / 16 in GL space, y up: sub_x = sx / 16, sub_y = 1 - sy / 16 (sample0_of; the pattern is
// mwrec::kPat's first entries, which tests/test_depth_cpu.py compares with this copy: mw_records.h is device code).
// Every test is written so that a NaN fails it.  A count is a sum of ones: the result does not depend on the order of the pixels.
//
// What the sensor cannot do: the depth map is a function of a 16-bit depth value, and one step of that value at eye depth z is
// z * z * (far - near) / (far * near * 65535) metres with near = 0.04 and far = 100: 3.8 mm at 3 m, 3.8 cm at 10 m.  The binding's default
// max_range is 8 m: a step of 2.4 cm there, a tenth of the default cell of 0.25 m, so a wall's points stay in the cells that hold it.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mwengine.h"
#include "mw_hd.h"
#include "mw_math.h"
#include "mw_nav.h"
#include "mw_ray.h"
#include "mw_seen.h"
#include "mw_ego.h"

// The launch (mw_depth.hip; the arithmetic of it: mwpolicy::depth_launch): lanes per workgroup, the bytes of LDS per cell (a uint32: the
// floor points in the low half, the obstacle points in the high half — a frame of at most MW_DEPTH_MAX_PIXELS pixels cannot carry from
// one into the other), and the cells that fit 64 KiB.
#ifndef MW_DEPTH_THREADS        // (measurements: `make EXTRA=-DMW_DEPTH_THREADS=...`, a multiple of 64)
#define MW_DEPTH_THREADS 256
#endif
#ifndef MW_DEPTH_WAVE_MERGE     // (measurements: 1 adds equal bins of a wavefront up before the LDS add)
#define MW_DEPTH_WAVE_MERGE 0
#endif
#define MW_DEPTH_CELL_BYTES 4
#define MW_DEPTH_MAX_CELLS 16384
#define MW_DEPTH_OBSTACLE 0x10000u       // what an obstacle point adds to its cell; a floor point adds 1

namespace mwdepth {

// what to keep of a pixel, and where in the pixel its depth was taken
struct Sensor { double min_range, max_range, floor_tol, top, sub_x, sub_y; int32_t W, H; };
struct Window { double cell, back; int32_t size, flags; };        // flags: MW_EGO_NORTH
struct Camera { double ox, oz, fx, fz, rx, rz, height, fwd_disp, sp, cp, th, tx; };
struct Point { double lat, fwd, px, pz; uint32_t add; };           // add: 1 floor, MW_DEPTH_OBSTACLE, 0 dropped

// sample 0 of the engine's pattern for `msaa` samples in 1/16 pixel, GL space (mwrec::kPat[pat_index(msaa)][0])
MW_HD void sample0_of(int msaa, int &sx, int &sy)
{
    sx = msaa == 1 ? 8 : msaa == 4 ? 6 : 9;
    sy = msaa == 1 ? 8 : msaa == 4 ? 2 : msaa == 8 ? 5 : 9;
}
MW_HD void subpixel_of(int msaa, double &sub_x, double &sub_y)
{
    int sx, sy;
    sample0_of(msaa, sx, sy);
    sub_x = (double)sx / 16.0;
    sub_y = 1.0 - (double)sy / 16.0;
}

// the env's pose and camera; cam: [4][N] height, fwd_disp, pitch, fov_y
MW_HD Camera camera_of(const MwRayArgs &a, const double *cam, const Sensor &s, size_t env)
{
    const mwego::Frame f = mwego::frame_of(a, mwego::Window{1.0, 0.0, 0.0, 0.0, 1, 0, 0}, mwseen::Sight{1.0, -1.0, 0}, env, nullptr);
    const size_t N = (size_t)a.w.N;
    Camera c;
    c.ox = f.ox; c.oz = f.oz; c.fx = f.fx; c.fz = f.fz; c.rx = f.rx; c.rz = f.rz;
    c.height = cam[env];
    c.fwd_disp = cam[N + env];
    const mw::SinCos p = mw::sincos_det(cam[2 * N + env] * M_PI / 180.0);
    const mw::SinCos h = mw::sincos_det(cam[3 * N + env] * 0.5 * M_PI / 180.0);
    c.sp = p.s; c.cp = p.c;
    c.th = h.s / h.c;
    const double aspect = (double)s.W / (double)s.H;
    c.tx = c.th * aspect;
    return c;
}
// pixel k = v * W + u of depth d
MW_HD Point point_of(const Camera &c, const Sensor &s, int k, float depth)
{
    Point p{0.0, 0.0, 0.0, 0.0, 0u};
    const double d = (double)depth;
    if (!(d >= s.min_range && d <= s.max_range)) return p;
    const int v = k / s.W, u = k % s.W;
    const double xn = (((double)u + s.sub_x) * 2.0) / (double)s.W - 1.0;
    const double yn = 1.0 - (((double)v + s.sub_y) * 2.0) / (double)s.H;
    p.lat = (xn * c.tx) * d;
    const double yc = (yn * c.th) * d;
    p.fwd = c.fwd_disp + (d * c.cp - yc * c.sp);
    const double up = c.height + (d * c.sp + yc * c.cp);
    if (up >= -s.floor_tol && up <= s.floor_tol) p.add = 1u;
    else if (up > s.floor_tol && up <= s.top) p.add = MW_DEPTH_OBSTACLE;
    p.px = c.ox + (p.fwd * c.fx + p.lat * c.rx);
    p.pz = c.oz + (p.fwd * c.fz + p.lat * c.rz);
    return p;
}
// the window's cell of a point, -1 outside
MW_HD int window_bin(const Camera &c, const Window &w, const Point &p)
{
    const bool north = (w.flags & MW_EGO_NORTH) != 0;
    const double a = north ? p.px - c.ox : p.lat, b = north ? -(p.pz - c.oz) : p.fwd;
    const double S = (double)w.size;
    const double col = floor(a / w.cell + S * 0.5);
    const double row = floor((S * 0.5 + w.back) - b / w.cell);
    if (!(col >= 0.0 && col < S && row >= 0.0 && row < S)) return -1;
    return (int)row * w.size + (int)col;
}
// the grid's cell of a point, -1 outside
MW_HD int map_bin(const mwnav::Grid &g, const Point &p)
{
    const double fi = floor((p.px - g.min_x) / g.cell), fj = floor((p.pz - g.min_z) / g.cell);
    if (!(fi >= 0.0 && fi < (double)g.gx && fj >= 0.0 && fj < (double)g.gz)) return -1;
    return (int)fj * g.gx + (int)fi;
}
// the bin of pixel k under either target (to_map: the grid g, else the window w) and what it adds there (0: nothing)
MW_HD int bin_of(const Camera &c, const Sensor &s, const Window &w, const mwnav::Grid &g, bool to_map, int k, float depth, uint32_t &add)
{
    const Point p = point_of(c, s, k, depth);
    add = p.add;
    if (!add) return -1;
    const int b = to_map ? map_bin(g, p) : window_bin(c, w, p);
    if (b < 0) add = 0u;
    return b;
}
MW_HD uint8_t clamp255(uint32_t n) { return (uint8_t)(n > 255u ? 255u : n); }
// a cell of the map under a call's count: 1 when it went 0 -> 1.  A cleared row is rewritten whole.
MW_HD int map_cell(uint8_t *row, int c, bool hit, bool cleared)
{
    if (cleared) {
        row[c] = hit ? 1 : 0;
        return hit ? 1 : 0;
    }
    if (!hit || row[c] != 0) return 0;
    row[c] = 1;
    return 1;
}

// ---- the phases of a call; `lane` of `stride` workers share each ------------------------------------------------------------------
// (the host's add is a plain one: it has one worker.  The kernel's phases are the same loops around atomicAdd, mw_depth.hip.)

MW_HD void zero_cells(uint32_t *cells, int n, int lane, int stride)
{
    for (int k = lane; k < n; k += stride) cells[k] = 0u;
}
inline void count_pixels(const Camera &c, const Sensor &s, const Window &w, const mwnav::Grid &g, bool to_map, const float *depth, uint32_t *cells, int lane,
                         int stride)
{
    for (int k = lane; k < s.W * s.H; k += stride) {
        uint32_t add;
        const int b = bin_of(c, s, w, g, to_map, k, depth[k], add);
        if (add) cells[b] += add;
    }
}
// the window's planes: [2][S][S], floor points then obstacle points, clamped to 255
MW_HD void write_planes(const uint32_t *cells, int n, uint8_t *planes, int lane, int stride)
{
    for (int k = lane; k < n; k += stride) {
        const uint32_t v = cells[k];
        planes[k] = clamp255(v & 0xFFFFu);
        planes[(size_t)n + k] = clamp255(v >> 16);
    }
}
// the map's rows: [2][gz][gx], free then obstacle; the cells this worker turned 0 -> 1 in each
MW_HD void or_map(const uint32_t *cells, int n, uint32_t min_points, bool cleared, uint8_t *rows, int &new_free, int &new_obstacle, int lane, int stride)
{
    for (int k = lane; k < n; k += stride) {
        const uint32_t v = cells[k];
        new_free += map_cell(rows, k, (v & 0xFFFFu) >= min_points, cleared);
        new_obstacle += map_cell(rows + n, k, (v >> 16) >= min_points, cleared);
    }
}
MW_HD void zero_rows(uint8_t *rows, int n, int lane, int stride)
{
    for (int k = lane; k < 2 * n; k += stride) rows[k] = 0;
}

// ---- a whole call for one env by one worker: the host's path (tests/hostcheck/depth_project.cpp) ------------------------------------
// cells: the caller's scratch, size * size entries
inline void window_one(const MwRayArgs &a, const double *cam, const Sensor &s, const Window &w, size_t env, const float *depth, uint32_t *cells,
                       uint8_t *planes)
{
    const int n = w.size * w.size;
    zero_cells(cells, n, 0, 1);
    count_pixels(camera_of(a, cam, s, env), s, w, mwnav::Grid{0.0, 0.0, 0.0, 0.0, 1.0, 1, 1}, false, depth, cells, 0, 1);
    write_planes(cells, n, planes, 0, 1);
}
// cells: gx * gz entries; rows: the env's [2][gz][gx]; count, newly: its [2].  false for an env whose extent the grid does not cover
inline bool map_one(const MwRayArgs &a, const double *cam, const Sensor &s, const mw_nav_params &p, int min_points, size_t env, bool clear,
                    const float *depth, uint32_t *cells, uint8_t *rows, int32_t *count, int32_t *newly)
{
    const mwnav::Grid g = mwnav::grid_of(a.w, p, env);
    const int n = g.gx * g.gz;
    if (!mwnav::covers(g)) {
        zero_rows(rows, n, 0, 1);
        count[0] = count[1] = 0;
        if (newly) newly[0] = newly[1] = 0;
        return false;
    }
    zero_cells(cells, n, 0, 1);
    count_pixels(camera_of(a, cam, s, env), s, Window{p.cell, 0.0, 1, 0}, g, true, depth, cells, 0, 1);
    int nf = 0, no = 0;
    or_map(cells, n, (uint32_t)min_points, clear, rows, nf, no, 0, 1);
    count[0] = (clear ? 0 : count[0]) + nf;
    count[1] = (clear ? 0 : count[1]) + no;
    if (newly) { newly[0] = nf; newly[1] = no; }
    return true;
}

}  // namespace mwdepth
