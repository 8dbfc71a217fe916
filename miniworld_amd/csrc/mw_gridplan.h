// Grid rollouts (mw_grid_plan, include/mwengine.h; kernel: mw_gridplan.hip): P plans of T actions per env run through the agent's own
// kinematics against the caller's uint8 obstacle plane, each scored against a nav field and a cost plane.  Plain C++ like mw_gridray.h:
// the kernel calls run() per lane, tests/hostcheck/grid_plan.cpp calls it per plan on the host, over bits staged with (lane, stride) = (0, 1).
//
// The rule (the header states it in full), float64, uncontracted: a turn is turn_agent's dir + turn * (pi / 180), a move move_agent's
//   sc = sincos_det(dir); nx = x + sc.c * f + sc.s * drift; nz = z + (-sc.s) * f + sc.c * drift
// refused iff blocked(nx, nz): with u = (nx - min_x) / cell, w likewise, rc = radius / cell, some opaque cell of the box
// floor(u - rc) .. floor(u + rc) x floor(w - rc) .. floor(w + rc) lies closer than rc to (u, w) — d2 < rc * rc, d2 from the clamped
// per-axis distances to the cell's square — or is the point's own cell.  An OR over a set: nothing depends on the order it is taken in.
//
// THE PLANE.  The obstacle bytes become a bit per cell inside a ring of one cell, which is set iff cells outside the grid are opaque:
// cell (row j, column c), -1 <= j <= gz, -1 <= c <= gx, is bit (j + 1) * (gx + 2) + (c + 1) of a flat array of 32-bit words — 12.3 KiB
// for the 1 x 32768 grid, the worst the cell limit allows, and 4.2 KiB for 128 x 256.  (Rows padded to whole words would take 128 KiB
// there.)  A row of the box is at most 18 consecutive bits: two words, one 64-bit shift, one mask (row_bits), and a row of zeros — free
// space — costs no float arithmetic; only the set bits get the distance test.  The array ends in a spare word, so that the second word
// of the last row's read is the array's own.
// The ring is exact.  A point outside the grid under MW_GPLAN_OUTSIDE_BLOCKS is blocked by its own cell.  Otherwise the box is clamped to
// the ring's rows and columns: an outside cell (j, c) of the box has the ring cell it clamps to in the same box — a box is a range per
// axis and holds a cell of the grid's range or the ring cell itself — at no greater dx and dz ((double)c - u and u - (double)(c + 1)
// are monotone in c, rounding keeps that, and so do max, the squares and their sum), and that ring cell is an outside cell of the box
// itself: the OR over the clamped box is the OR over the whole one.  With cells outside open the ring's bits are 0 and the clamped box
// holds the cells of the grid alone.
#pragma once
#include <math.h>
#include <string.h>

#include "mw_nav_grid.h"
#include "mw_ray.h"

#define MW_GPLAN_THREADS 256            // lanes of mw_gridplan_kernel's workgroup at most: a plan per lane
#define MW_GPLAN_AHEAD 8                // actions a lane holds in registers ahead of the step it executes

namespace mwgplan {

constexpr double kBound = 1073741824.0;         // 2^30 cells: mw_scan_project's bound
constexpr double kPi = 3.14159265358979323846;  // turn_agent's (mw_setup_common.h)
constexpr int kNoField = 0xFFFF;

// what a call fixes for all its envs, by value (the step sizes: the config's defaults; an env's row of d_step replaces them)
struct Call {
    double radius, fwd, drift, turn;
    int32_t flags, T, P, stop_at;
};
// ... and for one env
struct Env {
    mwnav::Grid g;
    double rc, r2, fwd, drift, dturn;
    bool outside, covered;
};

MW_HD int stride_of(int gx) { return gx + 2; }
MW_HD int plane_words(int gx, int gz) { return (int)(((long long)(gx + 2) * (gz + 2) + 31) / 32) + 1; }
MW_HD size_t plane_bytes(int gx, int gz) { return ((size_t)plane_words(gx, gz) * 4 + 15) / 16 * 16; }
MW_HD int bit_of(int gx, int j, int c) { return (j + 1) * stride_of(gx) + (c + 1); }

MW_HD Env env_of(const MwNavArgs &a, const mw_nav_params &p, const Call &c, const double *step, size_t env)
{
    Env e;
    e.g = mwnav::grid_of(a, p, env);
    e.rc = c.radius / e.g.cell;
    e.r2 = e.rc * e.rc;
    e.fwd = step ? step[env * 3] : c.fwd;
    e.drift = step ? step[env * 3 + 1] : c.drift;
    e.dturn = (step ? step[env * 3 + 2] : c.turn) * (kPi / 180.0);
    e.outside = (c.flags & MW_GPLAN_OUTSIDE_BLOCKS) != 0;
    e.covered = mwnav::covers(e.g);
    return e;
}

// ---- staging, by workers (lane, stride); `set` ors a bit into a word other workers set bits of too.  A barrier lies between the two.
MW_HD void zero_plane(uint32_t *bits, int gx, int gz, int lane, int stride)
{
    for (int w = lane; w < plane_words(gx, gz); w += stride) bits[w] = 0u;
}
template <typename Set>
MW_HD void stage_plane(const uint8_t *row, uint32_t *bits, int gx, int gz, bool ring, int lane, int stride, Set set)
{
    const auto put = [bits, gx, set](int j, int c) { const int b = bit_of(gx, j, c); set(bits + (b >> 5), 1u << (b & 31)); };
    mwnav::each_byte(row, gx * gz, lane, stride, [gx, put](int c, uint8_t b) { if (b) put(c / gx, c % gx); });
    if (!ring) return;
    const int s = stride_of(gx);
    for (int k = lane; k < 2 * s + 2 * gz; k += stride) {
        if (k < 2 * s) put(k < s ? -1 : gz, k % s - 1);
        else put((k - 2 * s) >> 1, ((k - 2 * s) & 1) ? gx : -1);
    }
}

// n <= 33 bits of the plane from bit b on
MW_HD uint64_t row_bits(const uint32_t *bits, int b, int n)
{
    const uint64_t two = (uint64_t)bits[b >> 5] | ((uint64_t)bits[(b >> 5) + 1] << 32);
    return (two >> (b & 31)) & (((uint64_t)1 << n) - 1);
}

// a point of the plane: whether a disc there is refused, and its own cell's flat index, -1 outside the grid
struct Spot { bool blocked; int cell; };
MW_HD int clamp_lo(double v, int lo) { return v < (double)lo ? lo : (int)v; }       // (|v| < 2^30 + 9: the conversion is exact)
MW_HD int clamp_hi(double v, int hi) { return v > (double)hi ? hi : (int)v; }
MW_HD double gap(double lo, double v) { const double a = lo - v, b = v - (lo + 1.0), m = a > b ? a : b; return m > 0.0 ? m : 0.0; }

MW_HD Spot spot_of(const Env &e, const uint32_t *bits, double px, double pz)
{
    const int gx = e.g.gx, gz = e.g.gz;
    const double u = (px - e.g.min_x) / e.g.cell, w = (pz - e.g.min_z) / e.g.cell;
    if (!(fabs(u) < kBound) || !(fabs(w) < kBound)) return {true, -1};          // (a NaN fails)
    const double fu = floor(u), fw = floor(w);
    const bool in = fu >= 0.0 && fu < (double)gx && fw >= 0.0 && fw < (double)gz;
    const int cell = in ? (int)fw * gx + (int)fu : -1;
    if (!in && e.outside) return {true, cell};
    if (in && row_bits(bits, bit_of(gx, (int)fw, (int)fu), 1)) return {true, cell};
    const int c0 = clamp_lo(floor(u - e.rc), -1), c1 = clamp_hi(floor(u + e.rc), gx);
    const int j0 = clamp_lo(floor(w - e.rc), -1), j1 = clamp_hi(floor(w + e.rc), gz);
    if (c0 > c1) return {false, cell};
    for (int j = j0; j <= j1; ++j) {
        uint64_t m = row_bits(bits, bit_of(gx, j, c0), c1 - c0 + 1);
        if (!m) continue;
        const double dz = gap((double)j, w), dz2 = dz * dz;
        do {
            const int c = c0 + __builtin_ctzll(m);
            const double dx = gap((double)c, u);
            if (dx * dx + dz2 < e.r2) return {true, cell};
            m &= m - 1;
        } while (m);
    }
    return {false, cell};
}

MW_HD int action_at(const void *plans, bool bytes, size_t at)
{
    return bytes ? (int)static_cast<const uint8_t *>(plans)[at] : (int)static_cast<const int32_t *>(plans)[at];
}
MW_HD void put3(double *row, double x, double z, double dir) { row[0] = x; row[1] = z; row[2] = dir; }

// plan p of env `env` (N envs, P plans: the arrays' strides), from (x, z, dir).  field and extra are the env's own planes or null.
MW_HD void run(const Env &e, const Call &q, size_t N, const uint32_t *bits, const void *plans, size_t env, size_t p, double x, double z, double dir,
               const uint16_t *field, const uint8_t *extra, double *pose_out, int32_t *stats, double *trace)
{
    const size_t P = (size_t)q.P, row = env * P + p;
    const bool bytes = (q.flags & MW_GPLAN_BYTE_PLANS) != 0;
    int reach = kNoField, reach_step = 0, steps = 0, bumps = 0, cost = 0;
    if (!e.covered) {
        if (trace)
            for (int k = 0; k < q.T; ++k) put3(trace + (((size_t)k * N + env) * P + p) * 3, x, z, dir);
    } else {
        // what the pose's cell holds: looked up again when a move is taken, and only then
        int v = kNoField, xv = 0;
        const auto look = [&](int cell) {
            v = field && cell >= 0 ? (int)field[cell] : kNoField;
            xv = extra && cell >= 0 ? (int)extra[cell] : 0;
        };
        // a start pose does not have to be free: only its cell is asked for
        {
            const double u = (x - e.g.min_x) / e.g.cell, w = (z - e.g.min_z) / e.g.cell;
            const double fu = floor(u), fw = floor(w);
            look(fu >= 0.0 && fu < (double)e.g.gx && fw >= 0.0 && fw < (double)e.g.gz ? (int)fw * e.g.gx + (int)fu : -1);
        }
        reach = v;
        bool active = !(q.stop_at >= 0 && reach <= q.stop_at), fresh = false;
        mw::SinCos sc{NAN, NAN};
        for (int k0 = 0; k0 < q.T && (active || trace); k0 += MW_GPLAN_AHEAD) {
            int acts[MW_GPLAN_AHEAD];
            for (int j = 0; j < MW_GPLAN_AHEAD; ++j)
                acts[j] = active && k0 + j < q.T ? action_at(plans, bytes, ((size_t)(k0 + j) * N + env) * P + p) : -1;
            for (int j = 0; j < MW_GPLAN_AHEAD && k0 + j < q.T; ++j) {
                const int k = k0 + j, a = acts[j];
                if (active) {
                    if (a == 0 || a == 1) {
                        dir = dir + (a == 0 ? e.dturn : -e.dturn);
                        fresh = false;
                    } else if (a == 2 || a == 3) {
                        if (!fresh) {       // (sincos_det's domain, as mwray::ray_of keeps it: beyond it a NaN, which no move survives)
                            sc = dir > -1e6 && dir < 1e6 ? mw::sincos_det(dir) : mw::SinCos{NAN, NAN};
                            fresh = true;
                        }
                        const double f = a == 2 ? e.fwd : -e.fwd;
                        const double nx = x + sc.c * f + sc.s * e.drift;
                        const double nz = z + (-sc.s) * f + sc.c * e.drift;
                        const Spot s = spot_of(e, bits, nx, nz);
                        if (s.blocked) {
                            ++bumps;
                        } else {
                            x = nx; z = nz;
                            look(s.cell);
                        }
                    }
                    cost += xv;
                    if (v < reach) { reach = v; reach_step = k + 1; }
                    steps = k + 1;
                    active = !(q.stop_at >= 0 && reach <= q.stop_at);
                }
                if (trace) put3(trace + (((size_t)k * N + env) * P + p) * 3, x, z, dir);
            }
        }
    }
    put3(pose_out + row * 3, x, z, dir);
    int32_t *s = stats + row * 5;
    s[0] = reach; s[1] = reach_step; s[2] = steps; s[3] = bumps; s[4] = cost;
}

}  // namespace mwgplan
