// Scan evidence (mw_scan_evidence, include/mwengine.h; kernel: mw_evidence.hip): the beams of a range scan counted into a signed evidence
// plane — the cell a beam ends in gains evidence, the cells it passes through lose some, the sum is clamped, and the thresholded planes
// and a likelihood plane come out of the same pass.  The beams, their cells and `hit` are mw_scan.h's, called as they stand; what is new
// is the counting.  Plain C++ like mw_scan.h: the kernel calls these functions with (lane, stride) of a workgroup,
// tests/hostcheck/scan_evidence.cpp calls evidence_one on the host, which runs the same phases with (0, 1).
//
// The rule (the header states it in full), per cell c of an updated env, int32:
//   hits(c)    the kept beams with hit whose end cell is c
//   passes(c)  the kept beams that have c among their cells, a beam once per cell
//   delta(c) = hits(c) > 0 ? hit * min(hits(c), cap) : -miss * min(passes(c), cap)
//   ev'(c)   = min(max((cleared ? 0 : ev(c)) + delta(c), lo), hi)
//   free = ev' <= free_at, obstacle = ev' >= occ_at, score = max(ev', 0); count: the cells of each plane, changed: those whose membership
//   differs between ev (0 under clear) and ev'
//
// The arrays (LDS in the kernel, the caller's on the host):
//   cnt     a 32-bit word per cell: passes in the low 16 bits, hits in the high 16 — a beam counts once per cell, so both stay below
//           MW_RAY_MAX + 1 < 2^16 and no carry crosses.  The resolve phase overwrites a cell's word with its ev' (as int32), which the
//           emit phases read: each output plane is then written along its own 4-byte boundaries.
//   pre     R + 1 int32: a beam's task count (0: dropped), then the exclusive prefix sums, pre[R] the total (mw_scan.h's deal)
// Three things keep the counting cheap:
//   the start cell is every kept beam's, so it is no task: the kept beams are counted once (count_beams returns each worker's share) and
//   added by one operation (`first` = 1: a beam's tasks are mw_scan.h's 1 .. nx + nz; first = 0 deals the start cell like any other:
//   MW_EVIDENCE_FORM 1, for measurements);
//   a beam names a cell twice only through an x task and a z task at an exact corner (two x tasks differ in column, two z tasks in row),
//   so a z task looks up the one x task of its column and drops itself if that names the same cell: O(1), no sort, no second plane;
//   every sum is of integers, so nothing depends on who adds what or when.
#pragma once
#include "mw_scan.h"

#ifndef MW_EVIDENCE_THREADS
#define MW_EVIDENCE_THREADS 512         // lanes of mw_evidence_kernel's workgroup, a multiple of 64
#endif
#ifndef MW_EVIDENCE_FORM
#define MW_EVIDENCE_FORM 0              // 0: the start cell folded, an LDS atomic per task; 1: the start cell dealt as a task; 2: 0 with equal
#endif                                  // cells of a wavefront added by one lane (mw_evidence.hip) — 1 and 2 for measurements (profiles/r48)

namespace mwevid {

constexpr uint32_t kHit = 1u << 16;                                     // one hit in a cnt word; one pass is 1
constexpr int kSums = 4;                                                // count free, count obstacle, changed free, changed obstacle
constexpr int kTailWords = kSums + 1 + MW_EVIDENCE_THREADS / 64;        // behind pre: the sums, the kept beams, a word per wavefront for the prefix

// the bytes of the counting plane and of the prefix with its tail, either rounded up to 16
MW_HD size_t count_bytes(long long cells) { return ((size_t)cells * 4 + 15) / 16 * 16; }
MW_HD size_t prefix_bytes(int rays) { return (((size_t)rays + 1 + kTailWords) * 4 + 15) / 16 * 16; }

// the seven integers of a call, by value
struct Rule { int hit, miss, cap, lo, hi, free_at, occ_at; };
// the first parameter outside its range, null for a rule the call takes (include/mwengine.h: the table)
MW_HD const char *out_of_range(const Rule &r)
{
    if (r.hit < 0 || r.hit > 127) return "hit";
    if (r.miss < 0 || r.miss > 127) return "miss";
    if (r.cap < 1 || r.cap > MW_RAY_MAX) return "cap";
    if (r.lo < -127 || r.lo > -1) return "lo";
    if (r.hi < 1 || r.hi > 127) return "hi";
    if (r.free_at < r.lo || r.free_at > -1) return "free_at";
    if (r.occ_at < 1 || r.occ_at > r.hi) return "occ_at";
    return nullptr;
}

// v more in a cell's word: the workgroup's lanes share the words, the host's one worker does not
MW_HD void add_count(uint32_t *cnt, int c, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(cnt + c, v);
#else
    cnt[c] += v;
#endif
}

// ---- the phases of a call; `lane` of `stride` workers share each ------------------------------------------------------------------

// phase 1, a beam per worker: its task count, and a hit in its end cell's word; returns the worker's kept beams
MW_HD int count_beams(const mwscan::Scan &s, uint32_t *cnt, int32_t *pre, int first, int lane, int stride)
{
    int kept = 0;
    for (int b = lane; b < s.R; b += stride) {
        const mwscan::Beam m = mwscan::beam(s, b);
        pre[b] = m.keep ? mwscan::tasks_of(m) - first : 0;
        if (!m.keep) continue;
        ++kept;
        if (m.hit) {
            const int c = mwscan::end_cell(m, s.g.gx, s.g.gz);
            if (c >= 0) add_count(cnt, c, kHit);
        }
    }
    return kept;
}
// behind phase 1, one worker: every kept beam's pass through the start cell, (floor(w0), floor(u0)) of mwscan::beam_of — the same for all
// of an env's beams —, by one addition
MW_HD void fold_start(const mwscan::Scan &s, uint32_t *cnt, int first, int kept)
{
    const int c = mwscan::inside(floor((s.oz - s.g.min_z) / s.g.cell), floor((s.ox - s.g.min_x) / s.g.cell), s.g.gx, s.g.gz);
    if (first && kept > 0 && c >= 0) add_count(cnt, c, (uint32_t)kept);
}
// the cell of task c (mw_scan.h's numbering) that counts a pass: -1 outside the grid, and for a z task whose cell the x task of the same
// column names too
MW_HD int pass_cell(const mwscan::Beam &m, int gx, int gz, int c)
{
    const int cell = mwscan::task_cell(m, gx, gz, c);
    if (cell < 0 || c <= m.nx) return cell;
    const int col = cell % gx, j = (m.gu > 0.0 ? col : col + 1) - m.xl;         // the x line that enters `col`, as a task of the beam
    if (j >= 0 && j < m.nx && mwscan::task_cell(m, gx, gz, 1 + j) == cell) return -1;
    return cell;
}
// phase 2, a task per worker: add(cell) once per round for every worker, -1 where it has no task or the task no cell — the rounds are
// the same for all, so that `add` may be a wavefront's joint operation
template <typename Add>
MW_HD void deal_tasks(const mwscan::Scan &s, const int32_t *pre, int first, int lane, int stride, Add add)
{
    const int total = pre[s.R];
    for (int base = 0; base < total; base += stride) {
        const int k = base + lane;
        int c = -1;
        if (k < total) {
            const int b = mwscan::beam_of_task(pre, s.R, k);
            c = pass_cell(mwscan::beam(s, b), s.g.gx, s.g.gz, k - pre[b] + first);
        }
        add(c);
    }
}

struct Sums { int free, obstacle, changed_free, changed_obstacle; };

MW_HD int resolved(uint32_t word, int ev, const Rule &r)
{
    const int h = (int)(word >> 16), p = (int)(word & 0xFFFFu);
    const int v = ev + (h > 0 ? r.hit * (h < r.cap ? h : r.cap) : -r.miss * (p < r.cap ? p : r.cap));
    return v < r.lo ? r.lo : v > r.hi ? r.hi : v;
}
MW_HD void resolve_byte(uint32_t *cnt, int8_t *row, int c, bool cleared, const Rule &r, Sums &s)
{
    const int before = cleared ? 0 : row[c], after = resolved(cnt[c], before, r);
    row[c] = (int8_t)after;
    cnt[c] = (uint32_t)after;
    const bool f0 = before <= r.free_at, f1 = after <= r.free_at, o0 = before >= r.occ_at, o1 = after >= r.occ_at;
    s.free += f1; s.obstacle += o1; s.changed_free += f0 != f1; s.changed_obstacle += o0 != o1;
}
// phase 3: the counts into the env's row of evidence, and each cell's ev' into its word.  The row starts at any byte: up to 3 head bytes
// singly, then aligned 32-bit words of four cells — unpacked, resolved and packed again, the memberships a bit per byte and summed by
// popcount; a word that stays as it is is not stored —, then the tail (mwscan::merge_plane's split)
MW_HD void resolve_plane(uint32_t *cnt, int n, bool cleared, const Rule &r, int8_t *row, Sums &s, int lane, int stride)
{
    int head = (int)((4 - ((uintptr_t)row & 3)) & 3);
    head = head < n ? head : n;
    const int words = (n - head) / 4, tail = head + words * 4;
    for (int c = lane; c < head; c += stride) resolve_byte(cnt, row, c, cleared, r, s);
    for (int w = lane; w < words; w += stride) {
        const int c0 = head + 4 * w;
        void *p = __builtin_assume_aligned(row + c0, 4);
        uint32_t v = 0u, out = 0u, f0 = 0u, f1 = 0u, o0 = 0u, o1 = 0u;
        if (!cleared) __builtin_memcpy(&v, p, 4);
        for (int k = 0; k < 4; ++k) {                   // (little-endian, like every target here)
            const int before = (int)(int8_t)(v >> (8 * k)), after = resolved(cnt[c0 + k], before, r);
            cnt[c0 + k] = (uint32_t)after;
            out |= (uint32_t)(uint8_t)after << (8 * k);
            f0 |= (uint32_t)(before <= r.free_at) << k; f1 |= (uint32_t)(after <= r.free_at) << k;
            o0 |= (uint32_t)(before >= r.occ_at) << k; o1 |= (uint32_t)(after >= r.occ_at) << k;
        }
        if (cleared || out != v) __builtin_memcpy(p, &out, 4);
        s.free += __builtin_popcount(f1); s.obstacle += __builtin_popcount(o1);
        s.changed_free += __builtin_popcount(f0 ^ f1); s.changed_obstacle += __builtin_popcount(o0 ^ o1);
    }
    for (int c = tail + lane; c < n; c += stride) resolve_byte(cnt, row, c, cleared, r, s);
}
// phase 4, once per output plane: byte(ev') of every cell into the plane's row, rewritten whole, by the row's own split
template <typename Byte>
MW_HD void emit_plane(const uint32_t *cnt, int n, uint8_t *row, int lane, int stride, Byte byte)
{
    int head = (int)((4 - ((uintptr_t)row & 3)) & 3);
    head = head < n ? head : n;
    const int words = (n - head) / 4, tail = head + words * 4;
    for (int c = lane; c < head; c += stride) row[c] = byte((int)cnt[c]);
    for (int w = lane; w < words; w += stride) {
        const int c0 = head + 4 * w;
        uint32_t out = 0u;
        for (int k = 0; k < 4; ++k) out |= (uint32_t)byte((int)cnt[c0 + k]) << (8 * k);
        __builtin_memcpy(__builtin_assume_aligned(row + c0, 4), &out, 4);
    }
    for (int c = tail + lane; c < n; c += stride) row[c] = byte((int)cnt[c]);
}
// map: the env's [2][n] or null; score: its [n] or null
MW_HD void emit_planes(const uint32_t *cnt, int n, const Rule &r, uint8_t *map, uint8_t *score, int lane, int stride)
{
    if (map) {
        emit_plane(cnt, n, map, lane, stride, [r](int e) { return (uint8_t)(e <= r.free_at); });
        emit_plane(cnt, n, map + n, lane, stride, [r](int e) { return (uint8_t)(e >= r.occ_at); });
    }
    if (score) emit_plane(cnt, n, score, lane, stride, [](int e) { return (uint8_t)(e > 0 ? e : 0); });
}
// an env whose extent the grid does not cover: every row zeroed
MW_HD void zero_rows(int8_t *ev, uint8_t *map, uint8_t *score, int n, int lane, int stride)
{
    for (int k = lane; k < n; k += stride) {
        ev[k] = 0;
        if (map) map[k] = map[n + k] = 0;
        if (score) score[k] = 0;
    }
}

// ---- a whole call for one env by one worker: the host's path (tests/hostcheck/scan_evidence.cpp); the kernel runs the same phases -----
// origin: the env's [3] or null = the agent; t, dir: the env's rows; cnt: a word per cell; pre: R + 1 entries; ev: the env's [gz][gx];
// map: its [2][gz][gx] or null; score: its [gz][gx] or null; count: its [2]; changed: its [2] or null.  first: 1, or 0 for the form
// that deals the start cell.  false for an env whose extent the grid does not cover
inline bool evidence_one(const MwNavArgs &a, const mw_nav_params &p, double max_range, int R, size_t env, const double *origin, const double *t, const double *dir,
                         bool clear, const Rule &r, int first, uint32_t *cnt, int32_t *pre, int8_t *ev, uint8_t *map, uint8_t *score, int32_t *count, int32_t *changed)
{
    const mwnav::Grid g = mwnav::grid_of(a, p, env);
    const int n = g.gx * g.gz;
    if (!mwnav::covers(g)) {
        zero_rows(ev, map, score, n, 0, 1);
        count[0] = count[1] = 0;
        if (changed) changed[0] = changed[1] = 0;
        return false;
    }
    const mwscan::Scan s{g, origin ? origin[0] : a.ax[env], origin ? origin[2] : a.az[env], max_range, t, dir, R};
    mwscan::zero_words(cnt, n, 0, 1);
    const int kept = count_beams(s, cnt, pre, first, 0, 1);
    int32_t sum = 0;
    for (int b = 0; b < R; ++b) { const int32_t v = pre[b]; pre[b] = sum; sum += v; }
    pre[R] = sum;
    fold_start(s, cnt, first, kept);
    deal_tasks(s, pre, first, 0, 1, [cnt](int c) { if (c >= 0) add_count(cnt, c, 1u); });
    Sums sums{0, 0, 0, 0};
    resolve_plane(cnt, n, clear, r, ev, sums, 0, 1);
    emit_planes(cnt, n, r, map, score, 0, 1);
    count[0] = sums.free; count[1] = sums.obstacle;
    if (changed) { changed[0] = sums.changed_free; changed[1] = sums.changed_obstacle; }
    return true;
}

}  // namespace mwevid
