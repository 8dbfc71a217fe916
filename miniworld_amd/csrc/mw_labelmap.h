// Object maps (mw_label_project, include/mwengine.h; kernel: mw_labelmap.hip): labelled pixels projected onto the maps a depth sensor
// gives.  Every pixel of an env's depth map that mw_depth_project would count — floor or obstacle, its bin inside the target — carries
// its label's id into the cell it falls in: the cell keeps the lowest id of its pixels.  The camera, the sample position, the range test,
// the height classes, px / pz and both bins are mw_depth.h's own functions (mwdepth::camera_of, point_of, window_bin, map_bin), called,
// not restated.  Plain C++: the kernel calls these phases with (lane, stride) of a workgroup and LDS atomics (Ops: mw_labelmap.hip),
// tests/hostcheck/label_project.cpp calls window_one / map_one on the host, which run the same phases with (0, 1) and HostOps.
//
// Per pixel k that counts:  id = code[k] - base, valid iff code[k] >= base && code[k] - base <= 254 (compared before the subtraction: no
// overflow); key = id where valid, else MW_LABELMAP_NONE ("seen, no object").  A cell's key is the minimum of its pixels' keys from
// MW_LABELMAP_UNSEEN ("not seen by this frame"): the lowest id wins, whatever the order of arrival.  A byte is 1 + key for key <= 254,
// else 0.  The window's plane is written in full; a map's byte is rewritten where the env is cleared or the cell's key is not
// MW_LABELMAP_UNSEEN — the last observation wins: a cell seen empty forgets its object, a cell out of view keeps what it knew.
// Per id q < K, over the WHOLE map of the env after the update: n = the cells whose byte is 1 + q, si / sj the integer sums of their column
// / row indices (exact, order-free, below 2^28: at most 16384 cells of an index below 16384);
//   pos = (min_x + ((double)si / (double)n + 0.5) * cell, 0.0, min_z + ((double)sj / (double)n + 0.5) * cell), three quiet NaNs for n == 0.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mw_depth.h"

// The launch (mw_labelmap.hip; the arithmetic of it: mwpolicy::labelmap_launch): lanes per workgroup, the bytes of an LDS word — one per
// cell of the target, then three per id (n, si, sj) —, the most cells and ids.
#define MW_LABELMAP_THREADS 256
#ifndef MW_LABELMAP_HOLD        // (measurements: `make EXTRA=-DMW_LABELMAP_HOLD=0` issues every pixel's atomicMin at once)
#define MW_LABELMAP_HOLD 1
#endif
#define MW_LABELMAP_WORD_BYTES 4
#define MW_LABELMAP_MAX_CELLS 16384
#define MW_LABELMAP_MAX_IDS 255
#define MW_LABELMAP_UNSEEN 0xFFFFu
#define MW_LABELMAP_NONE 0xFFFEu

namespace mwlabelmap {

using mwdepth::Camera;
using mwdepth::Sensor;
using mwdepth::Window;

// one env's call: its camera, the target (to_map: the grid g, else the window w) and what turns a code into an id
struct Call { Camera c; Sensor s; Window w; mwnav::Grid g; bool to_map; int32_t base; };
// the bin a lane holds and the lowest key that met it (bin < 0: nothing held)
struct Held { int bin; uint32_t key; };
// 16 bytes of a row, loaded at once where the host says `wide`
struct alignas(16) Depth4 { float v[4]; };
struct alignas(16) Code4 { int32_t v[4]; };

// the host's one worker: plain read-modify-writes
struct HostOps {
    static MW_HD void lowest(uint32_t *p, uint32_t v) { if (v < *p) *p = v; }
    static MW_HD void add(uint32_t *p, uint32_t v) { *p += v; }
};

MW_HD uint32_t key_of(int32_t code, int32_t base) { return code >= base && code - base <= 254 ? (uint32_t)(code - base) : MW_LABELMAP_NONE; }
MW_HD uint8_t byte_of(uint32_t key) { return key <= 254u ? (uint8_t)(1u + key) : (uint8_t)0; }
// the bin of pixel k where mw_depth_project counts it, -1 where it does not (the inside test precedes the conversion: mwdepth's bins)
MW_HD int bin_of(const Call &q, int k, float depth)
{
    const mwdepth::Point p = mwdepth::point_of(q.c, q.s, k, depth);
    if (!p.add) return -1;
    return q.to_map ? mwdepth::map_bin(q.g, p) : mwdepth::window_bin(q.c, q.w, p);
}

// ---- the phases of a call; `lane` of `stride` workers share each ------------------------------------------------------------------

// keys: n cells, then the 3 * K words of the sums
MW_HD void fill_keys(uint32_t *keys, int n, int K, int lane, int stride)
{
    for (int k = lane; k < n; k += stride) keys[k] = MW_LABELMAP_UNSEEN;
    for (int k = lane; k < 3 * K; k += stride) keys[n + k] = 0u;
}
template <class Ops>
MW_HD void flush(uint32_t *keys, const Held &h)
{
    if (h.bin >= 0) Ops::lowest(keys + h.bin, h.key);
}
// pixel k joins the held bin, or the held key goes to its cell and the new bin is held
template <class Ops>
MW_HD void take(const Call &q, int k, float depth, int32_t code, uint32_t *keys, Held &h)
{
    const int b = bin_of(q, k, depth);
    if (b < 0) return;
    const uint32_t key = key_of(code, q.base);
#if MW_LABELMAP_HOLD
    if (b != h.bin) {
        flush<Ops>(keys, h);
        h = {b, key};
    } else if (key < h.key) {
        h.key = key;
    }
#else
    (void)h;
    Ops::lowest(keys + b, key);
#endif
}
// consecutive workers take consecutive pixels; four at a time as two 16-byte loads where `wide` (W * H a multiple of 4, both rows aligned)
template <class Ops>
MW_HD void lowest_keys(const Call &q, const float *depth, const int32_t *code, bool wide, uint32_t *keys, int lane, int stride)
{
    const int pixels = q.s.W * q.s.H;
    if (wide) {
        const Depth4 *d4 = reinterpret_cast<const Depth4 *>(depth);
        const Code4 *c4 = reinterpret_cast<const Code4 *>(code);
        for (int g = lane; g < pixels / 4; g += stride) {
            const Depth4 d = d4[g];
            const Code4 c = c4[g];
            Held h{-1, MW_LABELMAP_UNSEEN};
            for (int j = 0; j < 4; ++j) take<Ops>(q, g * 4 + j, d.v[j], c.v[j], keys, h);
            flush<Ops>(keys, h);
        }
    } else {
        for (int k = lane; k < pixels; k += stride) {
            Held h{-1, MW_LABELMAP_UNSEEN};
            take<Ops>(q, k, depth[k], code[k], keys, h);
            flush<Ops>(keys, h);
        }
    }
}
// the window's plane: [S][S], written in full
MW_HD void write_plane(const uint32_t *keys, int n, uint8_t *plane, int lane, int stride)
{
    for (int k = lane; k < n; k += stride) plane[k] = byte_of(keys[k]);
}
// the map's row [gz][gx] under the call's keys, and every cell's (1, i, j) into the sums of its id: sums = [3][K] n, si, sj
// (byte - 1 < K is tested before it indexes them; K = 0: no sums)
template <class Ops>
MW_HD void merge_map(const uint32_t *keys, int n, int gx, bool cleared, uint8_t *row, int K, uint32_t *sums, int lane, int stride)
{
    for (int k = lane; k < n; k += stride) {
        const uint32_t key = keys[k];
        uint8_t b = row[k];
        if (cleared || key != MW_LABELMAP_UNSEEN) {
            b = byte_of(key);
            row[k] = b;
        }
        if (b != 0 && (int)b - 1 < K) {
            const int id = (int)b - 1;
            Ops::add(sums + id, 1u);
            Ops::add(sums + K + id, (uint32_t)(k % gx));
            Ops::add(sums + 2 * K + id, (uint32_t)(k / gx));
        }
    }
}
MW_HD void zero_row(uint8_t *row, int n, int lane, int stride)
{
    for (int k = lane; k < n; k += stride) row[k] = 0;
}
// row q of the two outputs (either may be null); sums null: an env the call refused, every n is 0
MW_HD void write_objects(const mwnav::Grid &g, const uint32_t *sums, int K, int32_t *cells, double *pos, int lane, int stride)
{
    for (int id = lane; id < K; id += stride) {
        const uint32_t n = sums ? sums[id] : 0u;
        if (cells) cells[id] = (int32_t)n;
        if (!pos) continue;
        double x = __builtin_nan(""), y = __builtin_nan(""), z = __builtin_nan("");
        if (n) {
            x = g.min_x + ((double)sums[K + id] / (double)n + 0.5) * g.cell;
            y = 0.0;
            z = g.min_z + ((double)sums[2 * K + id] / (double)n + 0.5) * g.cell;
        }
        pos[(size_t)id * 3] = x;
        pos[(size_t)id * 3 + 1] = y;
        pos[(size_t)id * 3 + 2] = z;
    }
}

// ---- a whole call for one env by one worker: the host's path (tests/hostcheck/label_project.cpp) -------------------------------------
// keys: the caller's scratch, size * size words
inline void window_one(const MwRayArgs &a, const double *cam, const Sensor &s, const Window &w, size_t env, const float *depth, const int32_t *code, int32_t base,
                       bool wide, uint32_t *keys, uint8_t *plane)
{
    const int n = w.size * w.size;
    const Call q{mwdepth::camera_of(a, cam, s, env), s, w, mwnav::Grid{0.0, 0.0, 0.0, 0.0, 1.0, 1, 1}, false, base};
    fill_keys(keys, n, 0, 0, 1);
    lowest_keys<HostOps>(q, depth, code, wide, keys, 0, 1);
    write_plane(keys, n, plane, 0, 1);
}
// keys: gx * gz + 3 * K words; row: the env's [gz][gx]; cells, pos: its [K] and [K][3], or null.  false for an env whose extent the grid
// does not cover
inline bool map_one(const MwRayArgs &a, const double *cam, const Sensor &s, const mw_nav_params &p, size_t env, bool clear, const float *depth,
                    const int32_t *code, int32_t base, bool wide, uint32_t *keys, uint8_t *row, int K, int32_t *cells, double *pos)
{
    const mwnav::Grid g = mwnav::grid_of(a.w, p, env);
    const int n = g.gx * g.gz;
    if (!mwnav::covers(g)) {
        zero_row(row, n, 0, 1);
        write_objects(g, nullptr, K, cells, pos, 0, 1);
        return false;
    }
    const Call q{mwdepth::camera_of(a, cam, s, env), s, Window{p.cell, 0.0, 1, 0}, g, true, base};
    fill_keys(keys, n, K, 0, 1);
    lowest_keys<HostOps>(q, depth, code, wide, keys, 0, 1);
    merge_map<HostOps>(keys, n, g.gx, clear, row, K, keys + n, 0, 1);
    write_objects(g, keys + n, K, cells, pos, 0, 1);
    return true;
}

}  // namespace mwlabelmap
