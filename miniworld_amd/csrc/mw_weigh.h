// Scan weighing and resampling (mw_scan_weigh, mw_resample, include/mwengine.h; kernels: mw_weigh.hip): the measurement update and the
// resampling step of Monte Carlo localisation on the caller's own map.  Plain C++ like mw_match.h: the kernels call these functions with
// (lane, stride) of a workgroup or a wavefront, tests/hostcheck/scan_weigh.cpp calls weigh_one and resample_one on the host, which run
// the same phases with the workers taken in turn.
//
// The weighing rule (the header states it in full), float64, only + - * / and floor, no contraction, in this order:
//   per beam:      t; gu = dx / cell; gw = dz / cell                                                 (mw_scan_match's, mw_match.h)
//   per particle (x, z, c, s):  u0 = (x - min_x) / cell; w0 = (z - min_z) / cell
//   per pair:      ru = c * gu + s * gw; rw = c * gw - s * gu; u1 = u0 + t * ru; w1 = w0 + t * rw
//   a beam counts iff t >= 0 && t < max_range and u0, w0, u1, w1 are all strictly inside -2^30 .. 2^30; its end cell (floor(w1), floor(u1))
//   score = the sum of the score bytes under the counting beams' end cells inside the grid; inside = how many of them are
//   best: the highest score, the lowest p on ties
// The arrays (LDS in the kernel, the caller's on the host):
//   plane   the env's score bytes as they are, a byte per cell (mwmatch::stage's byte form)
//   beams   the env's beams that pass the t test — it does not depend on the particle —, compacted once: (t, gu, gw), 24 bytes each.
//           t * ru is not premultiplied: ru depends on the particle, and the rule's order is (c * gu + s * gw) first.
//   tail    a fill word (the beams listed) and the 64-bit key of the best particle so far
// A particle's key: score << 32 | ~p in the low word.  score <= 4096 * 255 < 2^20, p < 4096: the greatest key is the rule's best, and no
// particle's key is 0.  The sums are over integers, so neither the order of the list nor who adds which beam matters: both forms — a
// particle per lane that walks the whole list, a wavefront per particle with the list dealt over its lanes — give the same bits.
//
// The resampling rule, unsigned 64-bit integers: S = the sum of the P weights; S == 0: ancestor[j] = j; else o = offset % S, C_p the
// inclusive prefix sums, T_j = (j * S + o) / P and ancestor[j] = the least p with C_p > T_j.  T_j <= ((P - 1) S + S - 1) / P < S = C_{P-1}:
// the search always ends inside; j * S + o < P * S <= 2^12 * 2^12 * 2^32 = 2^56.
//   prefix  C_p, a 64-bit word per particle; behind it a word per wavefront (its lanes' total) in the kernel
#pragma once
#include "mw_match.h"

#ifndef MW_WEIGH_THREADS
#define MW_WEIGH_THREADS 256            // lanes of mw_weigh_kernel's and mw_resample_kernel's workgroup, a multiple of 64
#endif

namespace mwweigh {

constexpr int kWave = 64;
constexpr int kTailBytes = 16;          // behind the beams: the fill word, then the key, 8-aligned

MW_HD size_t plane_bytes(long long cells) { return mwmatch::plane_bytes(cells, false); }
MW_HD size_t beams_bytes(int rays) { return (size_t)rays * 24; }
MW_HD size_t prefix_bytes(int particles) { return (size_t)particles * 8 + (size_t)(MW_WEIGH_THREADS / kWave) * 8; }

// what a call reads of one env, by value
struct Weigh {
    mwnav::Grid g;
    double max_range;
    const double *t, *dir;      // the env's rows [R], [R][2]
    int R;
};

// ---- weighing: the phases; `lane` of `stride` workers share each -----------------------------------------------------------------------

// an entry of the beam list: the shared counter gives the place; the host's one worker counts plainly
MW_HD int place(uint32_t *fill)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)atomicAdd(fill, 1u);
#else
    return (int)(*fill)++;
#endif
}
// phase 1, a beam per worker: the beams with t >= 0 && t < max_range (a NaN fails) as (t, gu, gw).  *fill is 0 before and at most R after.
MW_HD void list_beams(const Weigh &w, double *beams, uint32_t *fill, int lane, int stride)
{
    for (int b = lane; b < w.R; b += stride) {
        const double t = w.t[b];
        if (!(t >= 0.0 && t < w.max_range)) continue;
        double *to = beams + 3 * (size_t)place(fill);
        to[0] = t;
        to[1] = w.dir[2 * b] / w.g.cell;
        to[2] = w.dir[2 * b + 1] / w.g.cell;
    }
}
// a particle's start in cells: false where no beam of it can count
MW_HD bool start_of(const mwnav::Grid &g, const double *pose, double &u0, double &w0)
{
    u0 = (pose[0] - g.min_x) / g.cell;
    w0 = (pose[1] - g.min_z) / g.cell;
    return mwscan::bounded(u0) && mwscan::bounded(w0);
}
// phase 2: beams first, first + step, ... of the list under the particle (u0, w0, c, s), added to score and inside.  The flat index is
// formed only after 0 <= row < gz and 0 <= col < gx: it is below the cell count.
MW_HD void walk(const uint8_t *plane, int gx, int gz, const double *beams, int n, double u0, double w0, double c, double s, int first, int step, int32_t &score,
                int32_t &inside)
{
    for (int k = first; k < n; k += step) {
        const double t = beams[3 * k], gu = beams[3 * k + 1], gw = beams[3 * k + 2];
        const double ru = c * gu + s * gw, rw = c * gw - s * gu;
        const double u1 = u0 + t * ru, w1 = w0 + t * rw;
        if (!(mwscan::bounded(u1) && mwscan::bounded(w1))) continue;
        const int row = (int)floor(w1), col = (int)floor(u1);
        if ((unsigned)row < (unsigned)gz && (unsigned)col < (unsigned)gx) {
            score += plane[row * gx + col];
            ++inside;
        }
    }
}
MW_HD uint64_t key_of(int32_t score, int p) { return (uint64_t)(uint32_t)score << 32 | (uint64_t)(~(uint32_t)p); }
MW_HD void decode(uint64_t key, int32_t *best)
{
    best[0] = (int32_t)~(uint32_t)key;
    best[1] = (int32_t)(key >> 32);
}
// an env whose extent the grid does not cover: zeros
MW_HD void write_none(int P, int32_t *out, int32_t *inside, int32_t *best, int lane, int stride)
{
    for (int p = lane; p < P; p += stride) {
        out[p] = 0;
        if (inside) inside[p] = 0;
    }
    if (best && lane == 0) best[0] = best[1] = 0;
}

// ---- a whole call for one env by one worker: the host's path; the kernel runs the same phases ----------------------------------------
// t, dir, score, pose: the env's rows; plane: plane_bytes(cells) bytes; beams: 3 R doubles; out, inside (or null), best (or null): the env's
// rows.  waves: the host's form 2 — each particle's list dealt over 64 workers taken in turn.  false for an env the grid does not cover
inline bool weigh_one(const MwNavArgs &a, const mw_nav_params &p, double max_range, int R, int P, bool waves, size_t env, const double *t, const double *dir,
                      const uint8_t *score, const double *pose, uint8_t *plane, double *beams, int32_t *out, int32_t *inside, int32_t *best)
{
    const mwnav::Grid g = mwnav::grid_of(a, p, env);
    if (!mwnav::covers(g)) {
        write_none(P, out, inside, best, 0, 1);
        return false;
    }
    const Weigh w{g, max_range, t, dir, R};
    mwmatch::stage(score, plane, g.gx * g.gz, false, 0, 1);
    uint32_t fill = 0;
    list_beams(w, beams, &fill, 0, 1);
    uint64_t key = 0;
    for (int q = 0; q < P; ++q) {
        const double *row = pose + 4 * (size_t)q;
        double u0, w0;
        int32_t sum = 0, in = 0;
        if (start_of(g, row, u0, w0))
            for (int l = 0; l < (waves ? kWave : 1); ++l) walk(plane, g.gx, g.gz, beams, (int)fill, u0, w0, row[2], row[3], l, waves ? kWave : 1, sum, in);
        out[q] = sum;
        if (inside) inside[q] = in;
        const uint64_t mine = key_of(sum, q);
        key = mine > key ? mine : key;
    }
    if (best) decode(key, best);
    return true;
}

// ---- resampling: the phases ------------------------------------------------------------------------------------------------------------

// worker `lane` of `stride` scans the run lo .. hi - 1 of consecutive particles
MW_HD void run_of(int P, int lane, int stride, int &lo, int &hi)
{
    const int per = (P + stride - 1) / stride;
    lo = lane * per < P ? lane * per : P;
    hi = lo + per < P ? lo + per : P;
}
MW_HD uint64_t run_sum(const uint32_t *weight, int lo, int hi)
{
    uint64_t sum = 0;
    for (int k = lo; k < hi; ++k) sum += weight[k];
    return sum;
}
// the run's inclusive prefix sums behind `carry`, the sum of every particle before lo
MW_HD void run_prefix(const uint32_t *weight, int lo, int hi, uint64_t carry, uint64_t *prefix)
{
    for (int k = lo; k < hi; ++k) {
        carry += weight[k];
        prefix[k] = carry;
    }
}
// ancestor[j]: the least p with C_p > T_j, by bisection (C is non-decreasing, C_{P-1} = S > T_j)
MW_HD int draw(const uint64_t *prefix, int P, uint64_t S, uint64_t o, int j)
{
    const uint64_t T = ((uint64_t)j * S + o) / (uint64_t)P;
    int lo = 0, hi = P - 1;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (prefix[mid] > T) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
MW_HD void draw_all(const uint64_t *prefix, int P, uint64_t offset, int32_t *ancestor, const double *pose, double *pose_out, int lane, int stride)
{
    const uint64_t S = prefix[P - 1], o = S ? offset % S : 0;
    for (int j = lane; j < P; j += stride) {
        const int p = S ? draw(prefix, P, S, o, j) : j;
        ancestor[j] = p;
        if (pose)
            for (int k = 0; k < 4; ++k) pose_out[4 * (size_t)j + k] = pose[4 * (size_t)p + k];
    }
}
// a whole call for one env on the host: `stride` workers' runs taken in turn, their totals carried as the kernel's wavefront scan does
inline void resample_one(int P, int stride, const uint32_t *weight, uint64_t offset, uint64_t *prefix, int32_t *ancestor, const double *pose, double *pose_out)
{
    uint64_t carry = 0;
    for (int l = 0; l < stride; ++l) {
        int lo, hi;
        run_of(P, l, stride, lo, hi);
        run_prefix(weight, lo, hi, carry, prefix);
        carry += run_sum(weight, lo, hi);
    }
    for (int l = 0; l < stride; ++l) draw_all(prefix, P, offset, ancestor, pose, pose_out, l, stride);
}

}  // namespace mwweigh
