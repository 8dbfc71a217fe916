// Grid regions (mw_grid_regions, include/mwengine.h; kernel: mw_regions.hip): the connected regions of a byte mask on a nav grid — a
// frontier mask's clusters, the cells a field can reach, an obstacle plane's specks —, each with its size, the sums of its rows and
// columns and one cell of its own to go to.  Plain C++ like mw_sight.h and mw_nav_grid.h: the kernel calls these functions with
// (lane, stride) of a workgroup, tests/hostcheck/grid_regions.cpp calls regions_one on the host, which runs the same phases with (0, 1).
//
// The rule (the header states it in full): member cells are joined over the 4 edge neighbours, with connectivity 8 over the 4 corner
// neighbours too; a region's root is its lowest flat index j * gx + i; the regions of at least min_cells cells are listed in the order of
// their roots; the representative minimises (size * j - sum_j)^2 + (size * i - sum_i)^2, ties to the lowest flat index.
//
// What the arrays hold:
//   label   uint16 per cell: the flat index of a cell of the same region, never above the cell's own, kNone (0xFFFF) off the mask.  It
//           starts as the cell's own index and is lowered — a round is a hook pass, then jump passes until nothing moves — until a round
//           changes nothing: then every cell holds its region's root.  kNone is above every index (cells <= MW_NAV_MAX_CELLS = 32768), so a minimum over neighbours ignores the
//           cells off the mask by itself.  A label names a cell of the same region, so label[c] = label[label[c]] is a valid lowering too
//           (jump_pass), and so is handing a neighbour's label to the cell a label names (hook_pass).  Every store puts a label of the
//           region in place of a higher one, and a store is one 16-bit write: a reader sees the value of before or of after.  A pass that
//           changes nothing has read a stable array, and hook_pass looks at every neighbour of every cell: so the fixed point is the
//           unique one and no result depends on the schedule; only the number of rounds may.
//   sizes   uint16 per cell, used at the roots: first the region's size — at most 32768, so the kernel adds into the 32-bit word a
//           pair of them shares and no carry crosses —, then, once the qualified roots are ranked, the region's code: k + 1 for the k-th
//           listed region, kNone for one that is not listed.
//   table   an Entry per listed region.
// Sizes, sums and the least distance are gathered run by run: a worker walks kRun consecutive cells and hands on one (key, first, last)
// per stretch of equal keys, so that a large region costs an atomic per stretch and not per cell.
#pragma once
#include "mw_nav_grid.h"

#define MW_REGIONS_THREADS 256          // lanes of mw_regions_kernel's workgroup, a multiple of 64

namespace mwregions {

constexpr int kNone = 0xFFFF;
// cells a worker walks in one go.  18 cells are 9 words of labels: an odd count, so the 32 lanes of a half wavefront read 32 banks.
constexpr int kRun = 18;

// a listed region: the least distance of a cell to size * centroid and the lowest cell at it; the sums of rows and columns; the size
struct Entry { unsigned long long best; int32_t sj, si, size, cell; };
constexpr unsigned long long kFar = ~0ull;
constexpr int32_t kNoCell = 0x7FFFFFFF;

// the bytes of dynamic LDS: labels, sizes, the table, a word per lane for the ranks' prefix; each rounded up to 16
MW_HD size_t label_bytes(long long cells) { return ((size_t)cells * sizeof(uint16_t) + 15) / 16 * 16; }
MW_HD size_t table_bytes(int K) { return ((size_t)K * sizeof(Entry) + 15) / 16 * 16; }
MW_HD size_t scan_bytes() { return (size_t)MW_REGIONS_THREADS * sizeof(int32_t); }

// ---- staging: a member cell's label is its own index; sizes and table start empty
MW_HD void stage(const uint8_t *row, uint16_t *label, uint16_t *sizes, int cells, int lane, int stride)
{
    mwnav::each_byte(row, cells, lane, stride, [label, sizes](int c, uint8_t b) { label[c] = (uint16_t)(b ? c : kNone); sizes[c] = 0; });
}
MW_HD void clear_table(Entry *tab, int K, int lane, int stride)
{
    for (int k = lane; k < K; k += stride) tab[k] = Entry{kFar, 0, 0, 0, kNoCell};
}

// ---- labelling
MW_HD int lower(int a, int b) { return a < b ? a : b; }
// hooking: a cell whose neighbours hold a lower label than its own hands the lowest of them to the cell its label names — after the
// jumps the end of its chain, which every cell of that chain points to — and takes it itself.  Several workers may hand labels to one
// cell in one pass, and the last store wins: whichever it is, it is a label of the region below the one the pass began with, so a pass
// that stores anything lowers the labels' sum and the rounds end; which of them won decides how many rounds it takes, never the fixed
// point.  Every cell looks at all its neighbours, so a pass that changes nothing has found it.
MW_HD bool hook_pass(uint16_t *label, int gx, int gz, bool diag, int lane, int stride)
{
    bool changed = false;
    for (int c = lane; c < gx * gz; c += stride) {
        const int v = label[c];
        if (v == kNone) continue;
        const int j = c / gx, i = c % gx;
        const bool l = i > 0, r = i < gx - 1, u = j > 0, d = j < gz - 1;
        int m = v;
        if (l) m = lower(m, label[c - 1]);
        if (r) m = lower(m, label[c + 1]);
        if (u) m = lower(m, label[c - gx]);
        if (d) m = lower(m, label[c + gx]);
        if (diag) {
            if (u && l) m = lower(m, label[c - gx - 1]);
            if (u && r) m = lower(m, label[c - gx + 1]);
            if (d && l) m = lower(m, label[c + gx - 1]);
            if (d && r) m = lower(m, label[c + gx + 1]);
        }
        if (m < v) {
            if (m < (int)label[v]) label[v] = (uint16_t)m;
            label[c] = (uint16_t)m;
            changed = true;
        }
    }
    return changed;
}
// pointer jumping: a cell takes the label of the cell its label names.  Repeated until nothing moves, every cell holds the label of the
// cell its chain of labels ends in: at most log2(cells) + 1 passes, each halving the chains.
MW_HD bool jump_pass(uint16_t *label, int cells, int lane, int stride)
{
    bool changed = false;
    for (int c = lane; c < cells; c += stride) {
        const int v = label[c];
        if (v == kNone) continue;
        const int w = label[v];
        if (w < v) { label[c] = (uint16_t)w; changed = true; }
    }
    return changed;
}
// the hard bound on rounds: a round that changes anything brings at least one more cell to its root (mwnav::max_passes' argument);
// on the host, where a pass goes cell after cell, the serpentine, the spiral and the staircase of 32768 cells take 3 (tests/test_regions_cpu.py)
MW_HD int max_rounds(int cells) { return cells + 1; }

// ---- runs: worker `lane` walks the cells q * kRun .. q * kRun + kRun - 1 for q = lane, lane + stride, ...; key(c) >= 0 names what the
// cell counts for (< 0: nothing), flush(key, first, last) gets every stretch first .. last - 1 of one key
template <typename Key, typename Flush>
MW_HD void each_run(int cells, int lane, int stride, Key key, Flush flush)
{
    for (int first = lane * kRun; first < cells; first += stride * kRun) {
        const int last = first + kRun < cells ? first + kRun : cells;
        int k = -1, a = first;
        for (int c = first; c < last; ++c) {
            const int kc = key(c);
            if (kc == k) continue;
            if (k >= 0) flush(k, a, c);
            k = kc;
            a = c;
        }
        if (k >= 0) flush(k, a, last);
    }
}

// sizes, at the roots.  add(sizes, root, n): sizes[root] += n, other workers adding to it and to the other half of its word too.
template <typename Add>
MW_HD void count_sizes(const uint16_t *label, uint16_t *sizes, int cells, int lane, int stride, Add add)
{
    each_run(cells, lane, stride, [label](int c) { const int v = label[c]; return v == kNone ? -1 : v; },
             [sizes, add](int root, int a, int b) { add(sizes, root, b - a); });
}

// ---- the list: the qualified roots in scan order.  Worker `lane` of `stride` owns the cells lane * per .. lane * per + per - 1, per =
// ceil(cells / stride): it counts its qualified roots, the caller turns the counts into each worker's first rank, and the worker
// then files its roots: a listed one (rank < K) gets its table entry's size and the code rank + 1, every other root the code kNone.
MW_HD bool qualified(const uint16_t *label, const uint16_t *sizes, int c, int min_cells) { return label[c] == c && (int)sizes[c] >= min_cells; }
MW_HD int own_first(int cells, int lane, int stride) { const int per = (cells + stride - 1) / stride, a = lane * per; return a < cells ? a : cells; }
MW_HD int own_last(int cells, int lane, int stride) { const int per = (cells + stride - 1) / stride, b = (lane + 1) * per; return b < cells ? b : cells; }
MW_HD int count_qualified(const uint16_t *label, const uint16_t *sizes, int cells, int min_cells, int lane, int stride)
{
    int n = 0;
    for (int c = own_first(cells, lane, stride); c < own_last(cells, lane, stride); ++c) n += qualified(label, sizes, c, min_cells) ? 1 : 0;
    return n;
}
MW_HD void file_roots(const uint16_t *label, uint16_t *sizes, Entry *tab, int cells, int min_cells, int K, int rank, int lane, int stride)
{
    for (int c = own_first(cells, lane, stride); c < own_last(cells, lane, stride); ++c) {
        if (label[c] != c) continue;
        int code = kNone;
        if ((int)sizes[c] >= min_cells) {
            if (rank < K) { tab[rank].size = (int32_t)sizes[c]; code = rank + 1; }
            ++rank;
        }
        sizes[c] = (uint16_t)code;
    }
}
// the code of a cell: 0 off the mask, k + 1 in the k-th listed region, kNone in a region that is not listed
MW_HD int code_of(const uint16_t *label, const uint16_t *sizes, int c) { const int v = label[c]; return v == kNone ? 0 : (int)sizes[v]; }
// ... as each_run's key: the listed region's index, -1 for any other cell
MW_HD int listed_of(const uint16_t *label, const uint16_t *sizes, int c) { const int code = code_of(label, sizes, c); return code == 0 || code == kNone ? -1 : code - 1; }

// ---- sums of rows and columns.  add(word, n): *word += n, shared.  A sum is at most 32768 cells * 32767 < 2^30.
template <typename Add>
MW_HD void sum_cells(const uint16_t *label, const uint16_t *sizes, Entry *tab, int cells, int gx, int lane, int stride, Add add)
{
    each_run(cells, lane, stride, [label, sizes](int c) { return listed_of(label, sizes, c); },
             [tab, gx, add](int k, int a, int b) {
                 int32_t sj = 0, si = 0;
                 for (int c = a; c < b; ++c) { sj += c / gx; si += c % gx; }
                 add(&tab[k].sj, sj);
                 add(&tab[k].si, si);
             });
}

// ---- the representative.  |size * j - sum_j| <= 32768 * 32767 < 2^30, so a term is below 2^60 and the sum below 2^61.
MW_HD unsigned long long distance(const Entry &e, int j, int i)
{
    const long long dj = (long long)e.size * j - e.sj, di = (long long)e.size * i - e.si;
    return (unsigned long long)(dj * dj) + (unsigned long long)(di * di);
}
// least(word, d): *word = min(*word, d), shared.  The entry's value only falls, so a cell farther than what a plain read shows is none.
template <typename Least>
MW_HD void least_distance(const uint16_t *label, const uint16_t *sizes, Entry *tab, int cells, int gx, int lane, int stride, Least least)
{
    each_run(cells, lane, stride, [label, sizes](int c) { return listed_of(label, sizes, c); },
             [tab, gx, least](int k, int a, int b) {
                 unsigned long long d = kFar;
                 for (int c = a; c < b; ++c) { const unsigned long long dc = distance(tab[k], c / gx, c % gx); d = dc < d ? dc : d; }
                 if (d < *(volatile unsigned long long *)&tab[k].best) least(&tab[k].best, d);
             });
}
// lowest(word, c): *word = min(*word, c), shared: the lowest cell at the least distance
template <typename Lowest>
MW_HD void lowest_cell(const uint16_t *label, const uint16_t *sizes, Entry *tab, int cells, int gx, int lane, int stride, Lowest lowest)
{
    for (int c = lane; c < cells; c += stride) {
        const int k = listed_of(label, sizes, c);
        if (k >= 0 && distance(tab[k], c / gx, c % gx) == tab[k].best) lowest(&tab[k].cell, (int32_t)c);
    }
}

// ---- the outputs: every element of the env's rows; `total` qualified regions, of which min(total, K) are listed
MW_HD void write_list(const Entry *tab, int K, int32_t *size, int32_t *cell, int32_t *sum, int lane, int stride)
{
    for (int k = lane; k < K; k += stride) {
        const bool have = tab[k].size > 0;
        size[k] = tab[k].size;
        cell[k] = have ? tab[k].cell : -1;
        if (sum) { sum[2 * k] = tab[k].sj; sum[2 * k + 1] = tab[k].si; }
    }
}
MW_HD void write_labels(const uint16_t *label, const uint16_t *sizes, int16_t *out, int cells, int lane, int stride)
{
    for (int c = lane; c < cells; c += stride) {
        const int code = code_of(label, sizes, c);
        out[c] = (int16_t)(code == kNone ? -1 : code);
    }
}

// ---- a whole call for one env by one worker: the host's path (tests/hostcheck/grid_regions.cpp); the kernel runs the same phases -----
// label, sizes: cells elements of the caller's, tab: K entries; member, size, cell, sum, out: the env's own rows (sum, out may be null).
// Returns the number of qualified regions, -1 if the labelling did not settle within its bound; *rounds: the rounds it took.
inline int regions_one(int gx, int gz, int connectivity, int min_cells, int K, const uint8_t *member, uint16_t *label, uint16_t *sizes, Entry *tab,
                       int32_t *size, int32_t *cell, int32_t *sum, int16_t *out, int *rounds)
{
    const int cells = gx * gz;
    const bool diag = connectivity == 8;
    stage(member, label, sizes, cells, 0, 1);
    clear_table(tab, K, 0, 1);
    int n = 0;
    bool settled = false;
    while (!settled && n < max_rounds(cells)) {
        bool changed = hook_pass(label, gx, gz, diag, 0, 1);
        for (bool moved = true; moved;) {
            moved = jump_pass(label, cells, 0, 1);
            changed = changed || moved;
        }
        ++n;
        settled = !changed;
    }
    if (rounds) *rounds = n;
    if (!settled) return -1;
    count_sizes(label, sizes, cells, 0, 1, [](uint16_t *s, int root, int k) { s[root] = (uint16_t)(s[root] + k); });
    const int total = count_qualified(label, sizes, cells, min_cells, 0, 1);
    file_roots(label, sizes, tab, cells, min_cells, K, 0, 0, 1);
    sum_cells(label, sizes, tab, cells, gx, 0, 1, [](int32_t *w, int32_t v) { *w += v; });
    least_distance(label, sizes, tab, cells, gx, 0, 1, [](unsigned long long *w, unsigned long long d) { *w = d < *w ? d : *w; });
    lowest_cell(label, sizes, tab, cells, gx, 0, 1, [](int32_t *w, int32_t c) { *w = c < *w ? c : *w; });
    write_list(tab, K, size, cell, sum, 0, 1);
    if (out) write_labels(label, sizes, out, cells, 0, 1);
    return total;
}

}  // namespace mwregions
