// Grid ray casts (mw_grid_ray_cast, include/mwengine.h; kernels: mw_gridray.hip): what a ray from a point meets first on the caller's
// own uint8 grid, and at which parameter — the inverse of mw_scan_project on the same arithmetic.  Plain C++ like mw_scan.h and
// mw_sight.h: the kernels call these functions per lane, tests/hostcheck/grid_ray.cpp calls cast_one on the host, which runs either
// form's walk with one worker.
//
// The rule (the header states it in full), float64, only + - * / and floor, no contraction, in this order: with E = max_t
//   u0 = (ox - min_x) / cell; w0 = (oz - min_z) / cell; gu = dx / cell; gw = dz / cell; u1 = u0 + E * gu; w1 = w0 + E * gw
//   dropped (t = max_t, hit = -1) unless u0, w0, u1, w1 are all strictly inside -2^30 .. 2^30: mwscan::beam_of with t = max_range = E
//   candidates (s, cell): the start cell (floor(w0), floor(u0)) at s = 0; per x line L of mwscan::lines_of — s = ((double)L - u0) / gu
//   + 0.0, column gu > 0 ? L : L - 1, row floor(w0 + s * gw) —; the mirrored ones per z line.  One counts when row and column lie in the
//   grid (mwscan::inside) and its opaque byte is != 0.  The hit is the counting candidate of least (s, row * gx + col).
// The + 0.0 makes the -0 of a ray that starts on a line and leaves it backwards the +0 of its start cell: equal values, equal bits.
//
// A HALF-RAY is one axis' lines in the order the ray crosses them: line j = 0 .. n - 1 is L = first + j for g > 0 and first + n - 1 - j
// for g < 0.  (double)L - a0 is monotone in that order, rounding and the division by one g keep it so: s never falls along a half-ray,
// and for s >= 0 the bits of s, read as an unsigned integer, order as the values do.  So a worker that goes along a half-ray may leave
// once its next s is ABOVE the least s anybody has found for the ray so far (the `key`, a 64-bit word lowered by an atomic min) — only
// above: consecutive lines can share an s (a quotient that underflows), and then the lower index among them decides.  The bits of s
// fill the key's 64, so the index stays with the worker (Best) and the workers' Bests are combined by first(): the result is the least
// (s, index) over all candidates, whoever looked at which.
#pragma once
#include <string.h>

#include "mw_ray.h"
#include "mw_scan.h"
#include "mw_sight.h"

#define MW_GRIDRAY_THREADS 256          // lanes of either kernel's workgroup: 128 half-ray pairs, or 4 wavefronts = 2 rays
#define MW_GRIDRAY_PAIRS (MW_GRIDRAY_THREADS / 2)

namespace mwgray {

constexpr uint64_t kNoKey = ~(uint64_t)0;       // above the bits of every s >= 0 (and of an infinity)

MW_HD uint64_t to_bits(double s) { uint64_t b; memcpy(&b, &s, 8); return b; }
MW_HD double from_bits(uint64_t b) { double s; memcpy(&s, &b, 8); return s; }

// the bytes of dynamic LDS of the staged form: a key per pair, then the opaque row as a bit per cell (mwsight::bits_bytes)
MW_HD size_t key_bytes() { return (size_t)MW_GRIDRAY_PAIRS * 8; }
struct Half { double a0, g, b0, h; int first, n; bool x; };      // own axis: a0, g; the other: b0, h; x: the lines are x lines
MW_HD size_t staged_bytes(long long cells) { return key_bytes() + mwsight::bits_bytes(cells); }
struct Best { uint64_t s; int32_t cell; };                       // a worker's least (s, index); s == kNoKey: none

MW_HD Half half_of(const mwscan::Beam &b, bool x)
{
    if (!b.keep) return {0.0, 0.0, 0.0, 0.0, 0, 0, x};
    return x ? Half{b.u0, b.gu, b.w0, b.gw, b.xl, b.nx, true} : Half{b.w0, b.gw, b.u0, b.gu, b.zl, b.nz, false};
}
MW_HD double line_of(const Half &h, int j) { return (double)(h.g > 0.0 ? h.first + j : h.first + h.n - 1 - j); }
MW_HD double s_of(const Half &h, double L) { return (L - h.a0) / h.g + 0.0; }
// the cell entered at line L, -1 outside the grid
MW_HD int cell_at(const Half &h, double L, double s, int gx, int gz)
{
    const double own = h.g > 0.0 ? L : L - 1.0, other = floor(h.b0 + s * h.h);
    return h.x ? mwscan::inside(other, own, gx, gz) : mwscan::inside(own, other, gx, gz);
}
MW_HD void take(Best &b, uint64_t s, int32_t cell)
{
    if (s < b.s || (s == b.s && cell < b.cell)) b = {s, cell};
}
MW_HD Best first(const Best &a, const Best &b) { Best r = a; take(r, b.s, b.cell); return r; }

// the ray of (env, k) and its beam: mw_ray_cast's own ray_of — `a.adir` is the caller's heading row where one was given —, then
// mwscan::beam_of with t = max_range = max_t, which is the rule's u1, w1, its bound test and its line ranges
MW_HD mwscan::Beam beam_of(const mwnav::Grid &g, const mwray::Ray &r, double max_t) { return mwscan::beam_of(g, r.ox, r.oz, max_t, r.dx, r.dz, max_t); }
MW_HD mw_ray_params fan_of(int R, double max_t) { mw_ray_params p{}; p.max_t = max_t; p.rays = R; return p; }

// the start cell, once per ray: `key` is lowered to 0 where it is opaque
template <typename Probe, typename Key>
MW_HD void look_start(const mwscan::Beam &b, int gx, int gz, Probe probe, Key key, Best &best)
{
    const int c = mwscan::inside(floor(b.w0), floor(b.u0), gx, gz);
    if (c >= 0 && probe(c)) { take(best, 0, c); key.lower(0); }
}

// ---- the staged form's walk, a half-ray per worker: next line, one division, the entered cell, one probe; no merge branch.  It leaves
// once its s is above the key, which its own first hit makes true at the next distinct s.
template <typename Probe, typename Key>
MW_HD void walk_lines(const Half &h, int gx, int gz, Probe probe, Key key, Best &best)
{
    for (int j = 0; j < h.n; ++j) {
        const double L = line_of(h, j), s = s_of(h, L);
        const uint64_t sb = to_bits(s);
        if (sb > key.load()) break;
        const int c = cell_at(h, L, s, gx, gz);
        if (c >= 0 && probe(c)) { take(best, sb, c); key.lower(sb); }
    }
}

// ---- the unstaged form, a wavefront per half-ray: worker `lane` of 64 looks at line base + lane; the wavefront leaves once the s of
// line `base` is above the key (wave_goes_on), and the first worker with a hit lowers the key.
MW_HD bool wave_goes_on(const Half &h, int base, uint64_t key) { return to_bits(s_of(h, line_of(h, base))) <= key; }
template <typename Probe>
MW_HD Best look_line(const Half &h, int j, int gx, int gz, Probe probe)
{
    if (j >= h.n) return {kNoKey, 0};
    const double L = line_of(h, j), s = s_of(h, L);
    const int c = cell_at(h, L, s, gx, gz);
    return (c >= 0 && probe(c)) ? Best{to_bits(s), c} : Best{kNoKey, 0};
}

// the answer of a ray from the Bests of its two halves
MW_HD mwray::Hit hit_of(const Best &b, double max_t)
{
    if (b.s == kNoKey) return {max_t, -1};
    const double s = from_bits(b.s);
    return {s < max_t ? s : max_t, b.cell};
}

// ---- a whole ray by one worker: the host's path (tests/hostcheck/grid_ray.cpp).  form 0: the staged form's walk over `bits` (staged
// from `opaque` by the caller); 1: the unstaged form's batches of 64 lines over the bytes, the 64 workers one after another.
struct HostKey {
    uint64_t *p;
    uint64_t load() const { return *p; }
    void lower(uint64_t s) const { if (s < *p) *p = s; }
};
inline mwray::Hit cast_one(const mwnav::Grid &g, const mwray::Ray &r, double max_t, const uint8_t *opaque, const uint32_t *bits, int form)
{
    const mwscan::Beam b = beam_of(g, r, max_t);
    if (!b.keep) return {max_t, -1};
    uint64_t word = kNoKey;
    const HostKey key{&word};
    Best best{kNoKey, 0};
    if (form == 0) {
        const auto probe = [bits](int c) { return mwsight::opaque_at(bits, c); };
        look_start(b, g.gx, g.gz, probe, key, best);
        for (int x = 1; x >= 0; --x) walk_lines(half_of(b, x != 0), g.gx, g.gz, probe, key, best);
    } else {
        const auto probe = [opaque](int c) { return opaque[c] != 0; };
        look_start(b, g.gx, g.gz, probe, key, best);
        for (int x = 1; x >= 0; --x) {
            const Half h = half_of(b, x != 0);
            for (int base = 0; base < h.n && wave_goes_on(h, base, key.load()); base += 64) {
                bool lowered = false;
                for (int lane = 0; lane < 64; ++lane) {
                    const Best m = look_line(h, base + lane, g.gx, g.gz, probe);
                    if (m.s == kNoKey) continue;
                    take(best, m.s, m.cell);
                    if (!lowered) key.lower(m.s);
                    lowered = true;
                }
            }
        }
    }
    return hit_of(best, max_t);
}

}  // namespace mwgray
