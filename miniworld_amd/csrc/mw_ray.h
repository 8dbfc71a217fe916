// Ray casts (mw_ray_cast, include/mwengine.h; kernels: mw_ray.hip): what a ray — or a disc swept along it — from a point of an env's
// floor plan meets first among the env's collision segments and, on request, its entities.  Plain C++: the kernels call these
// functions per lane, tests/hostcheck/ray_cast.cpp calls cast_one on the host.  The step kernels' code is not shared (their code
// objects stay as they are); the closest-point distance is mwnav::seg_dist, the restatement mw_nav.h already keeps.
//
// Arithmetic, all float64, only + - * / and sqrt, no contraction (the build's -ffp-contract=off), in exactly this order:
//   fan            ang = agent_dir + offset; (s, c) = mw::sincos_det(ang); d = (c, -s).  |ang| >= 1e6 (sincos_det's domain) or NaN: d = NaN
//   a NaN in o, d  no obstacle is looked at: t = max_t, hit = -1
//   ray_seg        e = b - a; den = dx * ez - dz * ex; den == 0: none.  w = a - o; t = (wx * ez - wz * ex) / den;
//                  s = (wx * dz - wz * dx) / den; a candidate when t >= 0 and 0 <= s <= 1
//   ray_circle     w = o - c; A = dx * dx + dz * dz; B = wx * dx + wz * dz; C = (wx * wx + wz * wz) - R * R; C < 0: t = 0 (inside);
//                  disc = B * B - A * C; disc < 0: none; t = (-B - sqrt(disc)) / A; a candidate when t >= 0
//   wall, r = 0    ray_seg(a, b)
//   wall, r > 0    seg_dist(o) < r: t = 0 (the ray starts inside the capsule).  Else len = sqrt(ex * ex + ez * ez);
//                  n = ((ez / len) * r, (-ex / len) * r); the smallest candidate of ray_circle(a, r), ray_circle(b, r),
//                  ray_seg(a + n, b + n), ray_seg(a - n, b - n)
//   entity slot    ray_circle(pos.x, pos.z, radius(slot) + r)
//   taking         a candidate t counts when t >= 0 and t < best, from best = max_t; then best = t + 0.0 (a -0 becomes +0: equal
//                  results are equal bits).  Walls in index order, then entities in slot order: equal t goes to the lowest code.
// Every test is written so that a NaN fails it.  The result is the minimum over the obstacles of (t, code) in that order, so it does
// not depend on how obstacles are spread over lanes.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mwengine.h"
#include "mw_hd.h"
#include "mw_math.h"
#include "mw_nav.h"

// what the kernels need of the engine: MwNavArgs (unchanged: the nav kernels take it by value) and the agents' headings
struct MwRayArgs {
    MwNavArgs w;
    const double *adir;         // [N]
};

// The launch forms (mw_ray.hip; the choice: mwpolicy::ray_launch).  Lanes per workgroup of the ray-per-lane form at most, wavefronts
// (= rays) per workgroup of the obstacle-per-lane form, and the bytes of LDS the first stages per wall and per entity slot.
#define MW_RAY_THREADS 256
#define MW_RAY_WAVES 4
#define MW_RAY_WALL_BYTES 48
#define MW_RAY_DISC_BYTES 32

namespace mwray {

constexpr double kNone = -1.0;      // "no candidate": fails t >= 0

struct Ray { double ox, oz, dx, dz; };
struct Hit { double t; int32_t code; };
struct Wall { double ax, az, bx, bz, nx, nz; };     // a segment and its offset vector (0, 0 for a plain ray)
struct Disc { double x, z, R, listed; };            // an entity slot as an obstacle; listed: 1.0 or 0.0
static_assert(sizeof(Wall) == MW_RAY_WALL_BYTES && sizeof(Disc) == MW_RAY_DISC_BYTES, "the LDS plan of the ray-per-lane kernel");

MW_HD bool bad_ray(const Ray &r) { return r.ox != r.ox || r.oz != r.oz || r.dx != r.dx || r.dz != r.dz; }

// ray k of env `env`: the origin row or the agent, the direction row or the fan
MW_HD Ray ray_of(const MwRayArgs &a, const mw_ray_params &p, size_t env, int k, const double *origin, const double *dir, const double *offsets)
{
    const size_t row = env * (size_t)p.rays + (size_t)k;
    Ray r;
    r.ox = origin ? origin[row * 3] : a.w.ax[env];
    r.oz = origin ? origin[row * 3 + 2] : a.w.az[env];
    if (dir) {
        r.dx = dir[row * 2];
        r.dz = dir[row * 2 + 1];
    } else {
        const double ang = a.adir[env] + offsets[k];
        if (ang > -1e6 && ang < 1e6) {
            const mw::SinCos sc = mw::sincos_det(ang);
            r.dx = sc.c;
            r.dz = -sc.s;
        } else {
            r.dx = r.dz = NAN;
        }
    }
    return r;
}

MW_HD double ray_seg(const Ray &r, double ax, double az, double bx, double bz)
{
    const double ex = bx - ax, ez = bz - az;
    const double den = r.dx * ez - r.dz * ex;
    if (den == 0.0) return kNone;
    const double wx = ax - r.ox, wz = az - r.oz;
    const double t = (wx * ez - wz * ex) / den;
    const double s = (wx * r.dz - wz * r.dx) / den;
    return (t >= 0.0 && s >= 0.0 && s <= 1.0) ? t : kNone;
}

MW_HD double ray_circle(const Ray &r, double cx, double cz, double R)
{
    const double wx = r.ox - cx, wz = r.oz - cz;
    const double A = r.dx * r.dx + r.dz * r.dz;
    const double B = wx * r.dx + wz * r.dz;
    const double C = (wx * wx + wz * wz) - R * R;
    if (C < 0.0) return 0.0;
    const double disc = B * B - A * C;
    if (disc < 0.0) return kNone;
    const double t = (-B - sqrt(disc)) / A;
    return t >= 0.0 ? t : kNone;
}

// a wall as the casts see it: for a swept disc with its offset vector — one sqrt and two divisions per wall, not per ray
MW_HD Wall wall_of(const double *s, double radius)
{
    Wall w{s[0], s[1], s[2], s[3], 0.0, 0.0};
    if (radius > 0.0) {
        const double ex = s[2] - s[0], ez = s[3] - s[1];
        const double len = sqrt(ex * ex + ez * ez);
        w.nx = (ez / len) * radius;
        w.nz = (-ex / len) * radius;
    }
    return w;
}

MW_HD double lower(double best, double t) { return (t >= 0.0 && (!(best >= 0.0) || t < best)) ? t : best; }

// the first t at which the ray (radius 0) or the disc swept along it meets the wall, or kNone
MW_HD double ray_wall(const Ray &r, const Wall &w, double radius)
{
    if (!(radius > 0.0)) return ray_seg(r, w.ax, w.az, w.bx, w.bz);
    const double s[4] = {w.ax, w.az, w.bx, w.bz};
    if (mwnav::seg_dist(s, r.ox, r.oz) < radius) return 0.0;
    double t = ray_circle(r, w.ax, w.az, radius);
    t = lower(t, ray_circle(r, w.bx, w.bz, radius));
    t = lower(t, ray_seg(r, w.ax + w.nx, w.az + w.nz, w.bx + w.nx, w.bz + w.nz));
    t = lower(t, ray_seg(r, w.ax - w.nx, w.az - w.nz, w.bx - w.nx, w.bz - w.nz));
    return t;
}

MW_HD void take(Hit &h, double t, int32_t code)
{
    if (t >= 0.0 && t < h.t) {
        h.t = t + 0.0;
        h.code = code;
    }
}
// of two results the one that comes first in (t, code): what lanes that each hold a part of the obstacles combine theirs with
MW_HD bool before(const Hit &a, const Hit &b) { return a.t < b.t || (a.t == b.t && (uint32_t)a.code < (uint32_t)b.code); }

// is the slot an obstacle: mwnav::slot_blocks without the target exception
MW_HD bool listed(const MwRayArgs &a, size_t env, int slot) { return mwnav::ent_kind(a.w, env, slot) != MW_ENT_NONE && slot != a.w.carry[env]; }
MW_HD Disc disc_of(const MwRayArgs &a, const mw_ray_params &p, size_t env, int slot)
{
    return {mwnav::ent_pos(a.w, env, slot, 0), mwnav::ent_pos(a.w, env, slot, 2), mwnav::ent_radius(a.w, env, slot) + p.radius, listed(a, env, slot) ? 1.0 : 0.0};
}
MW_HD int ents_of(const MwRayArgs &a, const mw_ray_params &p) { return (p.flags & MW_RAY_ENTITIES) ? a.w.E : 0; }

// One ray against every obstacle in index order: the host's path and the definition of the result.
MW_HD Hit cast_one(const MwRayArgs &a, const mw_ray_params &p, size_t env, const Ray &r)
{
    Hit h{p.max_t, -1};
    if (bad_ray(r)) return h;
    const double *segs = mwnav::segs_of(a.w, env);
    const int ns = mwnav::nsegs_of(a.w, env);
    for (int i = 0; i < ns; ++i) take(h, ray_wall(r, wall_of(segs + (size_t)i * 4, p.radius), p.radius), i);
    for (int s = 0; s < ents_of(a, p); ++s) {
        const Disc d = disc_of(a, p, env, s);
        if (d.listed != 0.0) take(h, ray_circle(r, d.x, d.z, d.R), MW_RAY_ENT + s);
    }
    return h;
}

}  // namespace mwray
