// Label frames (mw_label_frame, include/mwengine.h; kernel: mw_label.hip): what every pixel of an env's observation shows.  The label of
// pixel (u, v) is what the ray from the env's camera through the pixel's depth sample (mwdepth::subpixel_of: sample 0 of the multisample
// pattern, where the frame's depth was taken) meets first among the env's static polygons as drawn, its Box slots and its mesh slots.  It
// stands in for what a user writes against env.entities and the GL matrices of miniworld.py:1197-1221 (gluPerspective, gluLookAt),
// entity.py:150-161 (MeshEnt.render), 409-432 (Box.render), 205-207 (the frames' transform) and objmesh.py:280-292.  Plain C++: the kernel
// runs frame_env with (lane, stride) of a workgroup and the LDS operations, tests/hostcheck/label_frame.cpp with (0, 1) and plain ones.
//
// All float64, only + - * /, sqrt, floor / ceil (the pruning rectangle alone) and mw::sincos_det, uncontracted, in exactly this order
// (W x H the frame, pixel row v from the top, column u; c the env's mwdepth::camera_of; a float is widened before anything else):
//   eye       ex = ox + fwd_disp * fx;  ey = agent_y + height;  ez = oz + fwd_disp * fz
//   ray       xn = (((double)u + sub_x) * 2.0) / (double)W - 1.0;  yn = 1.0 - (((double)v + sub_y) * 2.0) / (double)H
//             lat = xn * tx;  yt = yn * th;  up = sp + yt * cp;  fwd = cp - yt * sp
//             dx = fwd * fx + lat * rx;  dy = up;  dz = fwd * fz + lat * rz          the point at eye depth t is eye + t * d
//             a NaN in the eye or in d: the pixel shows nothing
//   vertex    of a static polygon: (x, y, z) = v[i]; with MW_POLY_XF (s, c) = sincos_det((double)xf[3] * M_PI / 180.0) and
//             (x, y, z) = ((c * x + s * z) + xf[0], y + xf[1], (c * z - s * x) + xf[2])
//             of triangle j of a mesh slot: (s, c) = sincos_det(dir); rx = c * x + s * z; rz = c * z - s * x;
//             (pos.x + scale * rx, pos.y + scale * y, pos.z + scale * rz)                (|dir| >= 1e6 or NaN: the slot shows nothing)
//   plane     a = V1 - V0, b = V2 - V0;  n = (ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx)
//             k = ((nx * (V0x - ex) + ny * (V0y - ey)) + nz * (V0z - ez))
//             edge i, V_i -> V_(i + 1 mod nv): e = V_(i + 1) - V_i;  m = (ny * ez - nz * ey, nz * ex - nx * ez, nx * ey - ny * ex);
//             mc = ((mx * V_ix + my * V_iy) + mz * V_iz)
//   plane hit den = ((nx * dx + ny * dy) + nz * dz); none unless den < 0 or den > 0 — for a mesh triangle unless den < 0: the reference
//             draws with GL_CULL_FACE (miniworld.py:512), so a triangle seen from behind is not there —;  t = k / den
//   inside    p = (ex + t * dx, ey + t * dy, ez + t * dz); for every edge ((mx * px + my * py) + mz * pz) - mc >= 0.0: the edge itself
//             counts, so two polygons that share it leave no hole
//   Box       (s, c) = sincos_det(dir); q = eye - pos;  o = (c * qx - s * qz, qy, s * qx + c * qz);  l = (c * dx - s * dz, dy, s * dx + c * dz)
//             per axis with lo .. hi = -sx / 2 .. sx / 2, 0 .. sy, -sz / 2 .. sz / 2:  l == 0: none unless o >= lo && o <= hi; else
//             t1 = (lo - o) / l, t2 = (hi - o) / l, tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1, none unless tn <= tf;
//             enter = the largest tn, leave = the smallest tf (x, y, z in turn, replaced on > and <); a hit iff enter <= leave; t = enter
//   cylinder  (MW_LABEL_MESH_BOUNDS) w = (ex - pos.x, ez - pos.z); A = dx * dx + dz * dz; B = wx * dx + wz * dz;
//             C = (wx * wx + wz * wz) - R * R;  A == 0: none unless C <= 0; else disc = B * B - A * C, none unless disc >= 0,
//             q = sqrt(disc), tn = (-B - q) / A, tf = (-B + q) / A;  then the y axis as a Box's with o = ey - pos.y, lo .. hi = 0 .. height
//   taking    a candidate t counts when near <= t && t <= far && t < best, from best = +infinity; then best = t + 0.0.  Polygons in index
//             order, Box slots in slot order, mesh slots in slot order: equal t goes to the lowest code.  Every test fails on a NaN.
// The result per pixel is the minimum of (t, place in that order) over the candidates, so it does not depend on how the work is spread:
// the mesh phase takes a triangle per worker and lowers the pixel's t with an atomic minimum on its bits (t >= near >= 0: they order as
// unsigned integers); whoever lowers it writes the slot's code, the same for all of a slot's triangles, and the slots take turns.
//
// The pruning rectangle of a mesh triangle: its vertices' pixel coordinates u = ((lat / z) / tx + 1.0) * W / 2, v = (1.0 - (yv / z) / th)
// * H / 2 with z = fwd * cp + up * sp, yv = up * cp - fwd * sp in the camera's axes, floor / ceil of their extremes minus / plus
// sub_x, sub_y, widened by a pixel on every side, clamped to the frame; the whole frame when a vertex has z < 1e-6 or a NaN; no pixel
// at all when all three have z < near (1 - 1e-9) - 1e-9: a hit's t is the z of a point of the triangle, and most objects behind the
// agent end here.  It only bounds the work (the exact test decides), as mwnav::axis_range does: tests/label_reference.py has no such
// thing, and the two agree bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mwengine.h"
#include "mw_asset_types.h"
#include "mw_depth.h"
#include "mw_hd.h"
#include "mw_math.h"

// The launch (mw_label.hip; the arithmetic of it: mwpolicy::label_launch): lanes per workgroup, the polygons staged at a time, the
// bytes of LDS per staged polygon, per entity slot (its volume, its five statistics words) and per pixel of a band of rows (the bits
// of t, a 16-bit code), and what a 16-bit code can name.
#ifndef MW_LABEL_THREADS        // (measurements: `make EXTRA=-DMW_LABEL_THREADS=...`, a multiple of 64)
#define MW_LABEL_THREADS 256
#endif
#define MW_LABEL_CHUNK 64
#define MW_LABEL_PLANE_BYTES 160
#define MW_LABEL_SLAB_BYTES 72
#define MW_LABEL_STAT_BYTES 20
#define MW_LABEL_PIXEL_BYTES 10
#define MW_LABEL_MAX_POLYS 0xF000       // a polygon's index, then MW_LABEL_ENT16 + slot, 0xFFFF nothing
#define MW_LABEL_MAX_ENTS 0x0FFF
#define MW_LABEL_ENT16 0xF000u
#define MW_LABEL_NONE16 0xFFFFu

// what the kernel needs of the engine beside the queries' view
struct MwLabelArgs {
    MwRayArgs r;
    const double *ay;           // [N]
    const double *cam;          // [4][N]
    const double *edir;         // [E][N]
    const int32_t *emesh;       // [E][N]
    const mw_poly *polys;       // [sets][max_polys]
    const int32_t *npolys;      // [sets]
    const MwMeshDesc *mesh;     // [n_mesh] or null
    const float *mesh_pos;      // [tris][MW_MESH_POS_STRIDE]
    int32_t max_polys, n_mesh, W, H, msaa, pad;
};

namespace mwlabel {

constexpr double kNone = -1.0;                  // "no candidate": fails near <= t
constexpr uint64_t kNoBits = ~(uint64_t)0;      // a pixel's t before anything was taken

struct Cam { double ex, ey, ez, fx, fz, rx, rz, sp, cp, th, tx, sub_x, sub_y; int32_t W, H; };
struct Dir { double x, y, z; };
struct Plane { double nx, ny, nz, k; double m[4][4]; };
struct Slab { double ox, oy, oz, c, s, hx, hy, hz, kind; };     // a slot as the rays see it; kind: MW_ENT_* as a double
struct Rect { int u0, v0, u1, v1; };
struct Out { uint8_t *cls; int32_t *code; float *depth; int32_t *ent_pixels, *ent_box; };      // one env's rows; all but cls may be null
static_assert(sizeof(Plane) == MW_LABEL_PLANE_BYTES && sizeof(Slab) == MW_LABEL_SLAB_BYTES, "the LDS plan of the label kernel");
static_assert(sizeof(mw_label_params) == 24 && offsetof(mw_label_params, far) == 8 && offsetof(mw_label_params, flags) == 16, "engine.py: MwLabelParams");

MW_HD double from_bits(uint64_t b) { double t; memcpy(&t, &b, 8); return t; }
MW_HD uint64_t to_bits(double t) { uint64_t b; memcpy(&b, &t, 8); return b; }

MW_HD Cam cam_of(const MwLabelArgs &a, size_t env)
{
    const mwdepth::Sensor s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, a.W, a.H};
    const mwdepth::Camera c = mwdepth::camera_of(a.r, a.cam, s, env);
    Cam o;
    o.ex = c.ox + c.fwd_disp * c.fx;
    o.ey = a.ay[env] + c.height;
    o.ez = c.oz + c.fwd_disp * c.fz;
    o.fx = c.fx; o.fz = c.fz; o.rx = c.rx; o.rz = c.rz; o.sp = c.sp; o.cp = c.cp; o.th = c.th; o.tx = c.tx;
    mwdepth::subpixel_of(a.msaa, o.sub_x, o.sub_y);
    o.W = a.W; o.H = a.H;
    return o;
}
MW_HD Dir dir_of(const Cam &c, int u, int v)
{
    const double xn = (((double)u + c.sub_x) * 2.0) / (double)c.W - 1.0;
    const double yn = 1.0 - (((double)v + c.sub_y) * 2.0) / (double)c.H;
    const double lat = xn * c.tx, yt = yn * c.th;
    const double up = c.sp + yt * c.cp, fwd = c.cp - yt * c.sp;
    return {fwd * c.fx + lat * c.rx, up, fwd * c.fz + lat * c.rz};
}
MW_HD bool bad_ray(const Cam &c, const Dir &d) { return c.ex != c.ex || c.ey != c.ey || c.ez != c.ez || d.x != d.x || d.y != d.y || d.z != d.z; }
MW_HD bool in_domain(double ang) { return ang > -1e6 && ang < 1e6; }       // sincos_det's; false for a NaN

MW_HD const mw_poly *polys_of(const MwLabelArgs &a, size_t env) { return a.polys + (a.r.w.shared_geom ? 0 : env) * (size_t)a.max_polys; }
MW_HD int npolys_of(const MwLabelArgs &a, size_t env)
{
    const int n = a.npolys[a.r.w.shared_geom ? 0 : env];
    return n < 0 ? 0 : (n > a.max_polys ? a.max_polys : n);
}
MW_HD int nv_of(const mw_poly &p) { return (p.nv & 0xFF) == 3 ? 3 : 4; }
MW_HD void vertex_of(const mw_poly &p, int i, double *V)
{
    const double x = (double)p.v[i][0], y = (double)p.v[i][1], z = (double)p.v[i][2];
    if (p.nv & MW_POLY_XF) {
        const mw::SinCos r = mw::sincos_det((double)p.xf[3] * M_PI / 180.0);
        V[0] = (r.c * x + r.s * z) + (double)p.xf[0];
        V[1] = y + (double)p.xf[1];
        V[2] = (r.c * z - r.s * x) + (double)p.xf[2];
    } else {
        V[0] = x; V[1] = y; V[2] = z;
    }
}
// the class of a static polygon (MW_LABEL_*): its flags, and for a GL_POLYGON the way its own vertices' normal points (a turn about +y leaves it)
MW_HD int class_of(const mw_poly &p)
{
    if (p.nv & MW_POLY_ENTITY) return MW_LABEL_FRAME;
    if (p.nv & MW_POLY_QUAD) return MW_LABEL_WALL;
    const double ax = (double)p.v[1][0] - (double)p.v[0][0], az = (double)p.v[1][2] - (double)p.v[0][2];
    const double bx = (double)p.v[2][0] - (double)p.v[0][0], bz = (double)p.v[2][2] - (double)p.v[0][2];
    return az * bx - ax * bz > 0.0 ? MW_LABEL_FLOOR : MW_LABEL_CEILING;
}
// the plane and the edges of nv vertices V[nv][3] as the eye sees them (the edges beyond nv: zeros, which pass)
MW_HD Plane plane_of(const double (*V)[3], int nv, const Cam &c)
{
    Plane p;
    const double ax = V[1][0] - V[0][0], ay = V[1][1] - V[0][1], az = V[1][2] - V[0][2];
    const double bx = V[2][0] - V[0][0], by = V[2][1] - V[0][1], bz = V[2][2] - V[0][2];
    p.nx = ay * bz - az * by;
    p.ny = az * bx - ax * bz;
    p.nz = ax * by - ay * bx;
    p.k = (p.nx * (V[0][0] - c.ex) + p.ny * (V[0][1] - c.ey)) + p.nz * (V[0][2] - c.ez);
    for (int i = 0; i < 4; ++i) {
        if (i >= nv) { p.m[i][0] = p.m[i][1] = p.m[i][2] = p.m[i][3] = 0.0; continue; }
        const int j = i + 1 == nv ? 0 : i + 1;
        const double ex = V[j][0] - V[i][0], ey = V[j][1] - V[i][1], ez = V[j][2] - V[i][2];
        p.m[i][0] = p.ny * ez - p.nz * ey;
        p.m[i][1] = p.nz * ex - p.nx * ez;
        p.m[i][2] = p.nx * ey - p.ny * ex;
        p.m[i][3] = (p.m[i][0] * V[i][0] + p.m[i][1] * V[i][1]) + p.m[i][2] * V[i][2];
    }
    return p;
}
MW_HD Plane plane_of_poly(const mw_poly &q, const Cam &c)
{
    double V[4][3];
    const int nv = nv_of(q);
    for (int i = 0; i < nv; ++i) vertex_of(q, i, V[i]);
    return plane_of(V, nv, c);
}
MW_HD double plane_t(const Plane &p, const Dir &d, bool cull)
{
    const double den = (p.nx * d.x + p.ny * d.y) + p.nz * d.z;
    if (!(den < 0.0 || (!cull && den > 0.0))) return kNone;
    return p.k / den;
}
MW_HD bool inside(const Plane &p, int nv, const Cam &c, const Dir &d, double t)
{
    const double px = c.ex + t * d.x, py = c.ey + t * d.y, pz = c.ez + t * d.z;
    for (int i = 0; i < nv; ++i)
        if (!(((p.m[i][0] * px + p.m[i][1] * py) + p.m[i][2] * pz) - p.m[i][3] >= 0.0)) return false;
    return true;
}
MW_HD bool counts(double t, const mw_label_params &p, double best) { return p.near <= t && t <= p.far && t < best; }

MW_HD double ent_geom(const MwLabelArgs &a, size_t env, int slot, int k) { return a.r.w.egeom[((size_t)k * (size_t)a.r.w.E + (size_t)slot) * (size_t)a.r.w.N + env]; }
MW_HD double ent_dir(const MwLabelArgs &a, size_t env, int slot) { return a.edir[(size_t)slot * (size_t)a.r.w.N + env]; }
// a slot's volume in the eye's terms: a Box's inverse transform and half extents, a mesh slot's cylinder (MW_LABEL_MESH_BOUNDS)
MW_HD Slab slab_of(const MwLabelArgs &a, size_t env, int slot, const Cam &c)
{
    Slab b{0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, (double)mwnav::ent_kind(a.r.w, env, slot)};
    const double qx = c.ex - mwnav::ent_pos(a.r.w, env, slot, 0), qy = c.ey - mwnav::ent_pos(a.r.w, env, slot, 1), qz = c.ez - mwnav::ent_pos(a.r.w, env, slot, 2);
    if (b.kind == (double)MW_ENT_BOX) {
        const double dir = ent_dir(a, env, slot);
        mw::SinCos r{NAN, NAN};
        if (in_domain(dir)) r = mw::sincos_det(dir);
        b.c = r.c; b.s = r.s;
        b.ox = r.c * qx - r.s * qz; b.oy = qy; b.oz = r.s * qx + r.c * qz;
        b.hx = ent_geom(a, env, slot, 0) / 2.0; b.hy = ent_geom(a, env, slot, 1); b.hz = ent_geom(a, env, slot, 2) / 2.0;
    } else {
        b.ox = qx; b.oy = qy; b.oz = qz;
        b.hx = ent_geom(a, env, slot, 7); b.hy = ent_geom(a, env, slot, 8);
    }
    return b;
}
// one axis of a slab test: narrows enter .. leave, false when the ray misses the axis' interval
MW_HD bool axis(double o, double l, double lo, double hi, double &enter, double &leave)
{
    if (l == 0.0) return o >= lo && o <= hi;
    const double t1 = (lo - o) / l, t2 = (hi - o) / l;
    const double tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1;
    if (!(tn <= tf)) return false;
    if (tn > enter) enter = tn;
    if (tf < leave) leave = tf;
    return true;
}
MW_HD double box_t(const Slab &b, const Dir &d)
{
    const double lx = b.c * d.x - b.s * d.z, lz = b.s * d.x + b.c * d.z;
    double enter = -INFINITY, leave = INFINITY;
    if (!axis(b.ox, lx, -b.hx, b.hx, enter, leave) || !axis(b.oy, d.y, 0.0, b.hy, enter, leave) || !axis(b.oz, lz, -b.hz, b.hz, enter, leave)) return kNone;
    return enter <= leave ? enter : kNone;
}
MW_HD double cylinder_t(const Slab &b, const Dir &d)
{
    const double A = d.x * d.x + d.z * d.z, B = b.ox * d.x + b.oz * d.z, C = (b.ox * b.ox + b.oz * b.oz) - b.hx * b.hx;
    double enter = -INFINITY, leave = INFINITY;
    if (A == 0.0) {
        if (!(C <= 0.0)) return kNone;
    } else {
        const double disc = B * B - A * C;
        if (!(disc >= 0.0)) return kNone;
        const double q = sqrt(disc);
        enter = (-B - q) / A;
        leave = (-B + q) / A;
        if (!(enter <= leave)) return kNone;
    }
    if (!axis(b.oy, d.y, 0.0, b.hy, enter, leave)) return kNone;
    return enter <= leave ? enter : kNone;
}

// the mesh of a slot, null where it has none the pools hold
MW_HD const MwMeshDesc *mesh_of(const MwLabelArgs &a, size_t env, int slot)
{
    const int id = a.emesh[(size_t)slot * (size_t)a.r.w.N + env];
    if (!a.mesh || !a.mesh_pos || id < 0 || id >= a.n_mesh || a.mesh[id].ntris == 0) return nullptr;
    return a.mesh + id;
}
struct MeshXf { double px, py, pz, scale, s, c; };
MW_HD MeshXf mesh_xf(const MwLabelArgs &a, size_t env, int slot)
{
    const double dir = ent_dir(a, env, slot);
    mw::SinCos r{NAN, NAN};
    if (in_domain(dir)) r = mw::sincos_det(dir);
    return {mwnav::ent_pos(a.r.w, env, slot, 0), mwnav::ent_pos(a.r.w, env, slot, 1), mwnav::ent_pos(a.r.w, env, slot, 2), ent_geom(a, env, slot, 6), r.s, r.c};
}
MW_HD void mesh_vertex(const MeshXf &x, const float *v, double *V)
{
    const double vx = (double)v[0], vy = (double)v[1], vz = (double)v[2];
    const double rx = x.c * vx + x.s * vz, rz = x.c * vz - x.s * vx;
    V[0] = x.px + x.scale * rx;
    V[1] = x.py + x.scale * vy;
    V[2] = x.pz + x.scale * rz;
}
// the pixels a triangle's hits can lie in (see the header): the exact test decides
MW_HD Rect rect_of(const Cam &c, const double (*V)[3], double near)
{
    const Rect all{0, 0, c.W - 1, c.H - 1};
    double ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
    bool whole = false;
    int behind = 0;
    for (int i = 0; i < 3; ++i) {
        const double qx = V[i][0] - c.ex, qy = V[i][1] - c.ey, qz = V[i][2] - c.ez;
        const double fwd = qx * c.fx + qz * c.fz, lat = qx * c.rx + qz * c.rz;
        const double z = fwd * c.cp + qy * c.sp, yv = qy * c.cp - fwd * c.sp;
        if (z < near * (1.0 - 1e-9) - 1e-9) ++behind;
        if (!(z >= 1e-6)) { whole = true; continue; }
        const double u = ((lat / z) / c.tx + 1.0) * (double)c.W / 2.0, v = (1.0 - (yv / z) / c.th) * (double)c.H / 2.0;
        if (!(u == u && v == v)) { whole = true; continue; }
        ulo = u < ulo ? u : ulo; uhi = u > uhi ? u : uhi;
        vlo = v < vlo ? v : vlo; vhi = v > vhi ? v : vhi;
    }
    if (behind == 3) return {0, 0, -1, -1};
    if (whole) return all;
    // clamped as doubles before the conversion: a huge value becomes an edge of the frame, never an int out of range
    double u0 = floor(ulo - c.sub_x) - 1.0, u1 = ceil(uhi - c.sub_x) + 1.0, v0 = floor(vlo - c.sub_y) - 1.0, v1 = ceil(vhi - c.sub_y) + 1.0;
    u0 = u0 > 0.0 ? u0 : 0.0; v0 = v0 > 0.0 ? v0 : 0.0;
    u0 = u0 < (double)c.W ? u0 : (double)c.W; v0 = v0 < (double)c.H ? v0 : (double)c.H;
    u1 = u1 < (double)(c.W - 1) ? u1 : (double)(c.W - 1); v1 = v1 < (double)(c.H - 1) ? v1 : (double)(c.H - 1);
    u1 = u1 > -1.0 ? u1 : -1.0; v1 = v1 > -1.0 ? v1 : -1.0;
    return {(int)u0, (int)v0, (int)u1, (int)v1};
}

// ---- the LDS plan: where a band's arrays lie in the workgroup's bytes (mwpolicy::label_launch sizes them) ---------------------------
struct Plan {
    uint64_t *tbits;        // [band pixels] the bits of the best t, kNoBits for none
    Plane *planes;          // [chunk]
    Slab *slabs;            // [E]
    int32_t *stats;         // [E][5] pixels, u0, v0, u1, v1
    uint16_t *code;         // [band pixels]
};
MW_HD size_t plan_bytes(int band_pixels, int chunk, int E)
{
    return ((size_t)band_pixels * MW_LABEL_PIXEL_BYTES + (size_t)chunk * MW_LABEL_PLANE_BYTES + (size_t)E * (MW_LABEL_SLAB_BYTES + MW_LABEL_STAT_BYTES) + 15) / 16 * 16;
}
MW_HD Plan plan_of(void *lds, int band_pixels, int chunk, int E)
{
    Plan p;
    char *at = static_cast<char *>(lds);
    p.tbits = reinterpret_cast<uint64_t *>(at); at += (size_t)band_pixels * 8;
    p.planes = reinterpret_cast<Plane *>(at); at += (size_t)chunk * MW_LABEL_PLANE_BYTES;
    p.slabs = reinterpret_cast<Slab *>(at); at += (size_t)E * MW_LABEL_SLAB_BYTES;
    p.stats = reinterpret_cast<int32_t *>(at); at += (size_t)E * MW_LABEL_STAT_BYTES;
    p.code = reinterpret_cast<uint16_t *>(at);
    return p;
}

// what the phases need of their workers: the host's are plain (one worker), the kernel's the LDS atomics and the barrier (mw_label.hip)
struct HostOps {
    static inline void sync() {}
    static inline uint64_t min64(uint64_t *p, uint64_t v) { const uint64_t old = *p; if (v < old) *p = v; return old; }
    static inline void add(int32_t *p, int32_t v) { *p += v; }
    static inline void lower(int32_t *p, int32_t v) { if (v < *p) *p = v; }
    static inline void raise(int32_t *p, int32_t v) { if (v > *p) *p = v; }
};

// ---- a whole call for one env; `lane` of `stride` workers share each phase, Ops::sync() between them ---------------------------------
// lds: plan_bytes(band_rows * W, chunk, E) bytes; band_rows >= 1 rows of pixels are labelled at a time; prune == false: every triangle
// against every pixel of the band (measurements and tests: the same bits)
template <typename Ops>
MW_HD void frame_env(const MwLabelArgs &a, const mw_label_params &p, size_t env, void *lds, int band_rows, int chunk, bool prune, const Out &out, int lane,
                     int stride)
{
    const int W = a.W, H = a.H, E = a.r.w.E;
    const Plan L = plan_of(lds, band_rows * W, chunk, E);
    const Cam c = cam_of(a, env);
    const mw_poly *polys = polys_of(a, env);
    const int np = npolys_of(a, env);
    const bool exact = !(p.flags & MW_LABEL_MESH_BOUNDS);
    for (int s = lane; s < E; s += stride) {
        L.slabs[s] = slab_of(a, env, s, c);
        int32_t *st = L.stats + s * 5;
        st[0] = 0; st[1] = W; st[2] = H; st[3] = -1; st[4] = -1;
    }
    for (int row0 = 0; row0 < H; row0 += band_rows) {
        const int rows = H - row0 < band_rows ? H - row0 : band_rows, pixels = rows * W;
        for (int k = lane; k < pixels; k += stride) { L.tbits[k] = kNoBits; L.code[k] = (uint16_t)MW_LABEL_NONE16; }
        // the static polygons, a chunk at a time
        for (int first = 0; first < np; first += chunk) {
            const int n = np - first < chunk ? np - first : chunk;
            Ops::sync();        // the chunk before has been read (and, the first time, the slabs and the band's cells are written)
            for (int i = lane; i < n; i += stride) L.planes[i] = plane_of_poly(polys[first + i], c);
            Ops::sync();
            for (int k = lane; k < pixels; k += stride) {
                const Dir d = dir_of(c, k % W, row0 + k / W);
                if (bad_ray(c, d)) continue;
                double best = L.tbits[k] == kNoBits ? INFINITY : from_bits(L.tbits[k]);
                int code = -1;
                for (int i = 0; i < n; ++i) {
                    const double t = plane_t(L.planes[i], d, false);
                    if (counts(t, p, best) && inside(L.planes[i], 4, c, d, t)) { best = t + 0.0; code = first + i; }
                }
                if (code >= 0) { L.tbits[k] = to_bits(best); L.code[k] = (uint16_t)code; }
            }
        }
        Ops::sync();
        // the Box slots, then with MW_LABEL_MESH_BOUNDS the mesh slots' cylinders
        for (int k = lane; k < pixels; k += stride) {
            const Dir d = dir_of(c, k % W, row0 + k / W);
            if (bad_ray(c, d)) continue;
            double best = L.tbits[k] == kNoBits ? INFINITY : from_bits(L.tbits[k]);
            int code = -1;
            for (int s = 0; s < E; ++s)
                if (L.slabs[s].kind == (double)MW_ENT_BOX) {
                    const double t = box_t(L.slabs[s], d);
                    if (counts(t, p, best)) { best = t + 0.0; code = s; }
                }
            if (!exact)
                for (int s = 0; s < E; ++s)
                    if (L.slabs[s].kind == (double)MW_ENT_MESH) {
                        const double t = cylinder_t(L.slabs[s], d);
                        if (counts(t, p, best)) { best = t + 0.0; code = s; }
                    }
            if (code >= 0) { L.tbits[k] = to_bits(best); L.code[k] = (uint16_t)(MW_LABEL_ENT16 + (unsigned)code); }
        }
        // the mesh slots' own triangles, a slot at a time, a triangle per worker
        if (exact)
            for (int s = 0; s < E; ++s) {
                if (L.slabs[s].kind != (double)MW_ENT_MESH) continue;
                const MwMeshDesc *m = mesh_of(a, env, s);
                if (!m) continue;
                Ops::sync();        // the pixel phase, or the slot before, has finished with the band's cells
                const MeshXf x = mesh_xf(a, env, s);
                const float *tri = a.mesh_pos + (size_t)m->first * MW_MESH_POS_STRIDE;
                for (int j = lane; j < (int)m->ntris; j += stride) {
                    double V[3][3];
                    for (int i = 0; i < 3; ++i) mesh_vertex(x, tri + (size_t)j * MW_MESH_POS_STRIDE + i * 3, V[i]);
                    const Plane q = plane_of(V, 3, c);
                    Rect r = prune ? rect_of(c, V, p.near) : Rect{0, 0, W - 1, H - 1};
                    r.v0 = r.v0 > row0 ? r.v0 : row0;
                    r.v1 = r.v1 < row0 + rows - 1 ? r.v1 : row0 + rows - 1;
                    for (int v = r.v0; v <= r.v1; ++v)
                        for (int u = r.u0; u <= r.u1; ++u) {
                            const Dir d = dir_of(c, u, v);
                            if (bad_ray(c, d)) continue;
                            const double t = plane_t(q, d, true);
                            if (!(p.near <= t && t <= p.far) || !inside(q, 3, c, d, t)) continue;
                            const int k = (v - row0) * W + u;
                            const uint64_t bits = to_bits(t + 0.0);
                            if (bits < Ops::min64(L.tbits + k, bits)) L.code[k] = (uint16_t)(MW_LABEL_ENT16 + (unsigned)s);
                        }
                }
            }
        Ops::sync();
        // the band's rows of the outputs, and the slots' statistics
        for (int k = lane; k < pixels; k += stride) {
            const int u = k % W, v = row0 + k / W;
            const unsigned c16 = L.code[k];
            int cls = MW_LABEL_NOTHING, code = -1;
            if (c16 >= MW_LABEL_ENT16 && c16 != MW_LABEL_NONE16) {
                const int s = (int)(c16 - MW_LABEL_ENT16);
                cls = L.slabs[s].kind == (double)MW_ENT_BOX ? MW_LABEL_BOX : MW_LABEL_MESH;
                code = MW_RAY_ENT + s;
                int32_t *st = L.stats + s * 5;
                Ops::add(st, 1);
                Ops::lower(st + 1, u); Ops::lower(st + 2, v); Ops::raise(st + 3, u); Ops::raise(st + 4, v);
            } else if (c16 != MW_LABEL_NONE16) {
                cls = class_of(polys[c16]);
                code = (int)c16;
            }
            const size_t at = (size_t)v * W + u;
            out.cls[at] = (uint8_t)cls;
            if (out.code) out.code[at] = code;
            if (out.depth) out.depth[at] = c16 == MW_LABEL_NONE16 ? (float)p.far : (float)from_bits(L.tbits[k]);
        }
        Ops::sync();        // the next band clears the cells
    }
    for (int s = lane; s < E; s += stride) {
        if (out.ent_pixels) out.ent_pixels[s] = L.stats[s * 5];
        if (out.ent_box)
            for (int i = 0; i < 4; ++i) out.ent_box[s * 4 + i] = L.stats[s * 5 + 1 + i];
    }
}

}  // namespace mwlabel
