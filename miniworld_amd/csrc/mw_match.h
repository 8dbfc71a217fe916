// Scan matching (mw_scan_match, include/mwengine.h; kernel: mw_match.hip): Olson's brute-force correlative scan matcher on the map's own
// lattice — every rotation of a list and every whole-cell translation of a window is scored by the sum of the likelihood bytes under
// the scan's end cells, and the best candidate wins.  Plain C++ like mw_scan.h and mw_clear.h: the kernel calls these functions with
// (lane, stride) of a workgroup, tests/hostcheck/grid_match.cpp calls match_one on the host, which runs the same phases with (0, 1).
//
// The rule (the header states it in full), float64, only + - * / and floor, no contraction, in this order:
//   u0 = (ox - min_x) / cell; w0 = (oz - min_z) / cell; gu = dx / cell; gw = dz / cell             (mw_scan_project's, mw_scan.h)
//   per rotation (c, s):  ru = c * gu + s * gw; rw = c * gw - s * gu; u1 = u0 + t * ru; w1 = w0 + t * rw
//   a beam counts iff t >= 0 && t < max_range and u0, w0, u1, w1 are all strictly inside -2^30 .. 2^30; its end cell (floor(w1), floor(u1))
//   score(r, b, a) = the sum over rotation r's counting beams of score[row + b][col + a], 0 outside the grid; a, b in -W .. W
//   best: the highest score; then the least a^2 + b^2, the lowest r, the lowest b, the lowest a
// A counting beam's four coordinates are below 2^30 in magnitude, so the floors are ints; row + b and col + a are ints below 2^30 + 32.
//
// The arrays (LDS in the kernel, the caller's on the host):
//   plane   the env's score bytes as they are, a byte per cell, unpadded.  The byte form reads it in place: a lookup is two unsigned
//           compares and one byte.  The quad form keeps kQuadPad zeroed bytes before and behind it, so that the two aligned words
//           around any four bytes of a row the window can reach exist; which of the four count is still decided by compares.
//   ends    two buffers of `batch` lists of R words, used in turn by the batches of rotations: the end cells of the counting beams that
//           SOME translation of the window brings into the grid (-W <= row < gz + W, -W <= col < gx + W), packed (row + W) << 16 |
//           (col + W) — both below 32768 + 64
//   fill    a word per rotation: how many entries its list holds
//   key     one 64-bit word: the best candidate so far
// A candidate's key: score << 36 | ~((a^2 + b^2) << 19 | flat) in the low 36 bits, flat = (r * side + b + W) * side + a + W with side =
// 2 W + 1.  flat < 64 * 65 * 65 < 2^19, a^2 + b^2 <= 2048 < 2^12, score <= 4096 * 255 < 2^20: the fields do not meet, the key is below
// 2^56, and the greatest key is the rule's best: flat orders (r, b, a) as the rule's ties do.  No candidate's key is 0.
// The sums are over integers, so neither the order of a list nor who scores which candidate matters: both forms give the same bits.
// A batch: the rotations r0 .. r0 + nb - 1 whose lists are live together; their candidates are ONE flat task list over the workers, so
// that a window with fewer candidates than the workgroup has lanes still fills it (mwpolicy::match_launch picks the batch).
#pragma once
#include "mw_scan.h"

#ifndef MW_MATCH_THREADS
#define MW_MATCH_THREADS 256            // lanes of mw_match_kernel's workgroup, a multiple of 64
#endif

// the rotations of a call, by value in the kernel's arguments: n pairs (c, s)
struct MwMatchRot { int32_t n; int32_t pad; double cs[MW_MATCH_MAX_ROT][2]; };

namespace mwmatch {

constexpr int kTailBytes = 16;          // behind the fill words: the key, 8-aligned
constexpr int kQuadPad = 72;            // the quad form's bytes before and behind the plane: 2 * MW_MATCH_MAX_WINDOW and a word, a multiple of 8

// the bytes of the staged plane, of the two buffers of lists and of the fill words with the tail, each rounded up to 16
MW_HD size_t plane_bytes(long long cells, bool quad) { return ((size_t)cells + (quad ? 2 * kQuadPad : 0) + 15) / 16 * 16; }
MW_HD size_t ends_bytes(int rays, int batch) { return (2 * (size_t)batch * (size_t)rays * 4 + 15) / 16 * 16; }
MW_HD size_t fill_bytes() { return (size_t)MW_MATCH_MAX_ROT * 4 + kTailBytes; }

// what a call reads of one env, by value
struct Match {
    mwnav::Grid g;
    double ox, oz, max_range;
    const double *t, *dir;      // the env's rows [R], [R][2]
    int R, W;
};

// ---- the rule ------------------------------------------------------------------------------------------------------------------------
// the end cell of beam b under (c, s): false for a beam that does not count
MW_HD bool end_of(const Match &m, int b, double c, double s, int &row, int &col)
{
    const double t = m.t[b];
    const double u0 = (m.ox - m.g.min_x) / m.g.cell, w0 = (m.oz - m.g.min_z) / m.g.cell;
    const double gu = m.dir[2 * b] / m.g.cell, gw = m.dir[2 * b + 1] / m.g.cell;
    const double ru = c * gu + s * gw, rw = c * gw - s * gu;
    const double u1 = u0 + t * ru, w1 = w0 + t * rw;
    if (!(t >= 0.0 && t < m.max_range && mwscan::bounded(u0) && mwscan::bounded(w0) && mwscan::bounded(u1) && mwscan::bounded(w1))) return false;
    row = (int)floor(w1);
    col = (int)floor(u1);
    return true;
}
MW_HD uint64_t key_of(int32_t score, int r, int b, int a, int W)
{
    const int side = 2 * W + 1;
    const uint64_t rank = (uint64_t)(a * a + b * b) << 19 | (uint64_t)((r * side + b + W) * side + a + W);
    return (uint64_t)score << 36 | (~rank & 0xFFFFFFFFFull);
}
// best[3] = (r, a, b) and the score of a key
MW_HD void decode(uint64_t key, int W, int32_t *best, int32_t *best_score)
{
    const int side = 2 * W + 1, flat = (int)(~key & 0x7FFFFull);
    best[0] = flat / (side * side);
    best[1] = flat % side - W;
    best[2] = flat / side % side - W;
    *best_score = (int32_t)(key >> 36);
}

// ---- the phases of a call; `lane` of `stride` workers share each ----------------------------------------------------------------------

// phase 0: the env's score bytes into the plane, by aligned words of the caller's row (mwnav::each_byte's split); the quad form's
// plane starts kQuadPad bytes in, between zeroed pads
MW_HD void stage(const uint8_t *row, uint8_t *plane, int cells, bool quad, int lane, int stride)
{
    uint8_t *to = plane + (quad ? kQuadPad : 0);
    mwnav::each_byte(row, cells, lane, stride, [to](int c, uint8_t v) { to[c] = v; });
    if (quad)
        for (int k = lane; k < 2 * kQuadPad; k += stride) plane[k < kQuadPad ? k : cells + k] = 0;
}
// an entry of a list: the shared counter gives the place; the host's one worker counts plainly
MW_HD void push(uint32_t *ends, uint32_t *fill, uint32_t e)
{
#if defined(__HIP_DEVICE_COMPILE__)
    ends[atomicAdd(fill, 1u)] = e;
#else
    ends[(*fill)++] = e;
#endif
}
// phase 1, a beam per worker: rotation (c, s)'s end cells that the window can bring into the grid.  *fill is 0 before and at most R after.
MW_HD void list_ends(const Match &m, double c, double s, uint32_t *ends, uint32_t *fill, int lane, int stride)
{
    for (int b = lane; b < m.R; b += stride) {
        int row, col;
        if (!end_of(m, b, c, s, row, col)) continue;
        if (row < -m.W || row >= m.g.gz + m.W || col < -m.W || col >= m.g.gx + m.W) continue;
        push(ends, fill, (uint32_t)(row + m.W) << 16 | (uint32_t)(col + m.W));
    }
}
// phase 2, the byte form, a translation per worker, consecutive workers consecutive a: the score of candidate (r, b, a) of the batch's
// nb rotations from r0 into the volume, and the worker's best key so far.  ends: the batch's lists, R words apart; fill[r]: rotation r's
// count.  (row + W) + (b - W) = row + b; one unsigned compare tests 0 <= v < n.
MW_HD uint64_t correlate(const uint8_t *plane, int gx, int gz, int W, int r0, int nb, const uint32_t *ends, int R, const uint32_t *fill, int32_t *volume,
                         uint64_t key, int lane, int stride)
{
    const int side = 2 * W + 1, per = side * side;
    for (int k = lane; k < nb * per; k += stride) {
        const int g = k / per, q = k % per, r = r0 + g, b = q / side - W, a = q % side - W, n = (int)fill[r];
        const uint32_t *list = ends + (size_t)g * R;
        int32_t sum = 0;
        for (int e = 0; e < n; ++e) {
            const uint32_t v = list[e];
            const int row = (int)(v >> 16) + (b - W), col = (int)(v & 0xFFFFu) + (a - W);
            if ((unsigned)row < (unsigned)gz && (unsigned)col < (unsigned)gx) sum += plane[row * gx + col];
        }
        if (volume) volume[(size_t)r * per + q] = sum;
        const uint64_t mine = key_of(sum, r, b, a, W);
        key = mine > key ? mine : key;
    }
    return key;
}
// 0xFF for each of the four columns col .. col + 3 that lies in 0 .. gx - 1
MW_HD uint32_t column_mask(int col, int gx)
{
    uint32_t m = 0u;
    for (int j = 0; j < 4; ++j)
        if ((unsigned)(col + j) < (unsigned)gx) m |= 0xFFu << (8 * j);
    return m;
}
// phase 2, the quad form, four adjacent a per worker: a0 = -W, -W + 4, ... (the last group of a row may reach past W: those sums are
// dropped).  Per end cell in a row of the grid the two aligned words around bytes row * gx + col .. + 3 of the padded plane, shifted
// into one word of four score bytes (little-endian, like every target here); the bytes of columns outside 0 .. gx - 1 are masked off —
// they are a neighbouring row's, or the pad's.  The bytes add up in two words of two 16-bit fields, emptied every 256 end cells (256 *
// 255 < 2^16).  The padded index is at least kQuadPad - 2 W >= 8 and the second word ends at most at cells + 2 W + kQuadPad + 7 <
// cells + 2 kQuadPad.
MW_HD uint64_t correlate4(const uint8_t *plane, int gx, int gz, int W, int r0, int nb, const uint32_t *ends, int R, const uint32_t *fill, int32_t *volume,
                          uint64_t key, int lane, int stride)
{
    const int side = 2 * W + 1, groups = (side + 3) / 4, per = side * groups;
    for (int k = lane; k < nb * per; k += stride) {
        const int g = k / per, q = k % per, r = r0 + g, b = q / groups - W, a0 = q % groups * 4 - W, n = (int)fill[r];
        const uint32_t *list = ends + (size_t)g * R;
        int32_t sum[4] = {0, 0, 0, 0};
        for (int e0 = 0; e0 < n; e0 += 256) {
            const int e1 = e0 + 256 < n ? e0 + 256 : n;
            uint32_t even = 0u, odd = 0u;
            for (int e = e0; e < e1; ++e) {
                const uint32_t v = list[e];
                const int row = (int)(v >> 16) + (b - W), col = (int)(v & 0xFFFFu) + (a0 - W);
                if ((unsigned)row >= (unsigned)gz) continue;
                const int at = row * gx + col + kQuadPad;
                uint32_t w[2];
                __builtin_memcpy(w, __builtin_assume_aligned(plane + (at & ~3), 4), 8);
                uint32_t four = (uint32_t)(((uint64_t)w[1] << 32 | w[0]) >> (8 * (at & 3)));
                if (col < 0 || col + 4 > gx) four &= column_mask(col, gx);
                even += four & 0x00FF00FFu;
                odd += (four >> 8) & 0x00FF00FFu;
            }
            sum[0] += (int32_t)(even & 0xFFFFu); sum[1] += (int32_t)(odd & 0xFFFFu);
            sum[2] += (int32_t)(even >> 16); sum[3] += (int32_t)(odd >> 16);
        }
        for (int j = 0; j < 4 && a0 + j <= W; ++j) {
            if (volume) volume[(size_t)r * side * side + (size_t)(b + W) * side + (a0 + j + W)] = sum[j];
            const uint64_t mine = key_of(sum[j], r, b, a0 + j, W);
            key = mine > key ? mine : key;
        }
    }
    return key;
}
// an env whose extent the grid does not cover: zeros.  (The kernel returns behind this, as it does for a masked-off env: either
// condition is the env's, the same for every lane of its workgroup, so no lane is left waiting at a barrier.)
MW_HD void write_none(int32_t *best, int32_t *best_score, int32_t *volume, size_t entries, int lane, int stride)
{
    if (volume)
        for (size_t k = (size_t)lane; k < entries; k += (size_t)stride) volume[k] = 0;
    if (lane == 0) {
        best[0] = best[1] = best[2] = 0;
        *best_score = 0;
    }
}

// ---- a whole call for one env by one worker: the host's path (tests/hostcheck/grid_match.cpp); the kernel runs the same phases ---------
// origin: the env's [3] or null = the agent; t, dir, score: the env's rows; plane: plane_bytes(cells, quad) bytes, 4-aligned; ends: R words
// (a batch of one); best: the env's [3]; volume: its [K][side][side] or null.  false for an env whose extent the grid does not cover
inline bool match_one(const MwNavArgs &a, const mw_nav_params &p, double max_range, int R, const MwMatchRot &rot, int W, bool quad, size_t env, const double *origin,
                      const double *t, const double *dir, const uint8_t *score, uint8_t *plane, uint32_t *ends, int32_t *best, int32_t *best_score,
                      int32_t *volume)
{
    const mwnav::Grid g = mwnav::grid_of(a, p, env);
    const int side = 2 * W + 1;
    if (!mwnav::covers(g)) {
        write_none(best, best_score, volume, (size_t)rot.n * side * side, 0, 1);
        return false;
    }
    const Match m{g, origin ? origin[0] : a.ax[env], origin ? origin[2] : a.az[env], max_range, t, dir, R, W};
    stage(score, plane, g.gx * g.gz, quad, 0, 1);
    uint64_t key = 0;
    uint32_t fill[MW_MATCH_MAX_ROT] = {};
    for (int r = 0; r < rot.n; ++r) {
        list_ends(m, rot.cs[r][0], rot.cs[r][1], ends, fill + r, 0, 1);
        key = (quad ? correlate4 : correlate)(plane, g.gx, g.gz, W, r, 1, ends, R, fill, volume, key, 0, 1);
    }
    decode(key, W, best, best_score);
    return true;
}

}  // namespace mwmatch
