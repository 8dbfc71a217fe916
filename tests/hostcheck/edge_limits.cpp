// The raster records' integer arithmetic (miniworld_amd/csrc/mw_edge_rec.h: the text the record writer of mw_records.h and the tile and
// quad kernels call — A, B, the low word of C, the sample thresholds with their extremes, the tile bounds, the per-pixel edge value by
// 24-bit multiplies, the classification of tiles and quads) as a stand-alone host program against the exact definition: for a frame, a
// sample count and a family of triangles in window coordinates it runs mwgl::setup_triangle_pos and counts where the modelled verdicts
// differ from c_k + dcdy_k fy - dcdx_k fx > 0 in 64 bits (the form of tests/hostcheck/mwhost.cpp's mwhost_render), at every sample of
// every pixel of the raster grid — the frame rounded up to whole 16 x 4 tiles, padding pixels included — and, for the touch / full
// classification of every tile and 2 x 2 quad, from the definition of mwhost_rect_counts (touched: every edge positive at SOME sample of
// the rectangle; covered: every edge positive at EVERY sample).  tests/test_edge_limits_cpu.py drives it.
//
//   edge_limits [--formula records|halved] [--threads N] [--random N] [--seed N]       queries on standard input, one per line:  W H S
//
// The triangles: every triple of the points {0, 1/256, 1/2, W/2, W - 1/256, W} x {0, 1/256, 1/2, H/2, H - 1/256, H} in both windings
// (setup keeps the front-facing one; a triangle's three rotations hold the same three edges, and the arithmetic treats the edges alike,
// so one rotation is taken) — the frame's two diagonals in both directions and the full-width and full-height edges with both signs of
// their coefficient are among them —, then `--random` seeded random triangles with vertices on the 1/256 lattice inside the frame.
// --formula: `records` is what mw_records.h writes and the kernels multiply (A = -256 dcdx, B = 256 dcdy; mul24(A, px) + mul24(B, gy) +
// C); `halved` is the exact form DESIGN.md section 9 keeps as a lever (mul24(A / 2, 2 px) + mul24(B / 2, 2 gy) + C).
// One answer per query, `name value` pairs:
//   tris            front-facing triangles of the family            covered     samples inside a triangle, by the definition
//   samples         samples whose modelled verdict (every E_k > thr_k[s]) differs from the definition
//   samples_a23 / samples_b23   ... of them on triangles that hold A = +2^23 / B = +2^23
//   outside_box     samples inside by the definition whose tile the record's tile bounds leave out
//   thr             thresholds, tmin or tmax that differ from their 64-bit values
//   qtile_touch qtile_full qquad_touch qquad_full     tiles / quads the quad kernel's classification (edge value at the first pixel against
//                   T, F) files differently from the definition;  ttile_touch ttile_full: the tile kernels' (classify_prim)
//   op24            triangles with a coefficient outside the signed 24 bits    a23 / b23   triangles with A = +2^23 / B = +2^23
//   sum32           triangles whose exact edge value leaves the signed 32 bits at some pixel of the grid    maxabs   its largest magnitude
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../miniworld_amd/csrc/mw_edge_rec.h"
#include "../../miniworld_amd/csrc/mw_glmath.h"

namespace {

// the sample patterns, 1/16 pixel (restated from the definition's side: mwhost.cpp)
const int PAT4[4][2] = {{6, 2}, {14, 6}, {2, 10}, {10, 14}};
const int PAT8[8][2] = {{9, 5}, {7, 11}, {13, 9}, {5, 3}, {3, 13}, {1, 7}, {11, 15}, {15, 1}};

struct Counts {
    long long tris = 0, covered = 0, samples = 0, samples_a23 = 0, samples_b23 = 0, outside_box = 0, thr = 0;
    long long qtile_touch = 0, qtile_full = 0, qquad_touch = 0, qquad_full = 0, ttile_touch = 0, ttile_full = 0;
    long long op24 = 0, a23 = 0, b23 = 0, sum32 = 0, maxabs = 0;
    void add(const Counts &o)
    {
        tris += o.tris; covered += o.covered; samples += o.samples; samples_a23 += o.samples_a23; samples_b23 += o.samples_b23;
        outside_box += o.outside_box; thr += o.thr; qtile_touch += o.qtile_touch; qtile_full += o.qtile_full; qquad_touch += o.qquad_touch;
        qquad_full += o.qquad_full; ttile_touch += o.ttile_touch; ttile_full += o.ttile_full; op24 += o.op24; a23 += o.a23; b23 += o.b23;
        sum32 += o.sum32; maxabs = o.maxabs > maxabs ? o.maxabs : maxabs;
    }
};

struct Tri { float w[3][4]; };

bool fits24(int v) { return v >= -(1 << 23) && v < (1 << 23); }

template <int S>
void check_triangle(const Tri &t, int W, int H, bool halved, Counts &n)
{
    mwgl::TriEdges te;
    if (!mwgl::setup_triangle_pos(t.w[0], t.w[1], t.w[2], true, te)) return;
    ++n.tris;
    const int (*pat)[2] = S == 8 ? PAT8 : PAT4;
    const int Wg = (W + MW_TILE_W - 1) / MW_TILE_W * MW_TILE_W, Hg = (H + MW_TILE_H - 1) / MW_TILE_H * MW_TILE_H;
    const int tiles_x = Wg / MW_TILE_W, tiles_y = Hg / MW_TILE_H;

    // the record, as write_tri_s makes it
    int A[3], B[3], C[3], thr[3][16], tmin[3], tmax[3];
    int64_t xthr[3][8], xmin[3], xmax[3];
    bool op24 = false, a23 = false, b23 = false;
    for (int k = 0; k < 3; ++k) {
        mwrec::edge_coeffs(te.dcdx[k], te.dcdy[k], A[k], B[k]);
        mwrec::edge_thresholds<S>(te.dcdx[k], te.dcdy[k], thr[k], tmin[k], tmax[k]);
        C[k] = (int)(uint32_t)te.c[k];
        op24 |= !fits24(A[k]) || !fits24(B[k]);
        a23 |= A[k] == (1 << 23); b23 |= B[k] == (1 << 23);
        xmin[k] = INT64_MAX; xmax[k] = INT64_MIN;
        for (int s = 0; s < S; ++s) {
            xthr[k][s] = (int64_t)te.dcdx[k] * (pat[s][0] * 16) - (int64_t)te.dcdy[k] * (pat[s][1] * 16);
            xmin[k] = xthr[k][s] < xmin[k] ? xthr[k][s] : xmin[k]; xmax[k] = xthr[k][s] > xmax[k] ? xthr[k][s] : xmax[k];
            n.thr += (int64_t)thr[k][s] != xthr[k][s];
        }
        n.thr += ((int64_t)tmin[k] != xmin[k]) + ((int64_t)tmax[k] != xmax[k]);
    }
    n.op24 += op24; n.a23 += a23; n.b23 += b23;
    const MwTileBox box = mw_qb_box(mwrec::tile_bounds(false, te.minx, te.maxx, te.miny, te.maxy, W, H), tiles_x, tiles_y);

    // the modelled and the exact edge values as column and row terms: the value at (px, gy) is their sum (the model's wraps).  gy runs
    // from H - Hg (the lowest padding row of a ragged frame, negative) to H - 1; row index r = gy - (H - Hg)
    std::vector<uint32_t> mcol((size_t)3 * Wg), mrow((size_t)3 * Hg);
    std::vector<int64_t> xcol((size_t)3 * Wg), xrow((size_t)3 * Hg);
    const int gy0 = H - Hg;
    for (int k = 0; k < 3; ++k) {
        for (int px = 0; px < Wg; ++px) {
            // edge_at's own terms (its sum with C and the row term is taken below, in the same wrapping 32 bits)
            mcol[(size_t)k * Wg + px] = halved ? (uint32_t)mw_qb_mul24(A[k] / 2, 2 * px) : (uint32_t)mwrec::edge_at(A[k], 0, 0, px, 0);
            xcol[(size_t)k * Wg + px] = -(int64_t)te.dcdx[k] * ((int64_t)px * 256);
        }
        for (int r = 0; r < Hg; ++r) {
            const int gy = gy0 + r;
            mrow[(size_t)k * Hg + r] = halved ? (uint32_t)mw_qb_mul24(B[k] / 2, 2 * gy) + (uint32_t)C[k] : (uint32_t)mwrec::edge_at(0, B[k], C[k], 0, gy);
            xrow[(size_t)k * Hg + r] = te.c[k] + (int64_t)te.dcdy[k] * ((int64_t)gy * 256);
        }
    }
    auto model_at = [&](int k, int px, int gy) { return (int)(mcol[(size_t)k * Wg + px] + mrow[(size_t)k * Hg + (gy - gy0)]); };

    int Tt[3], Ft[3], Tq[3], Fq[3];
    for (int k = 0; k < 3; ++k) {
        mwrec::rect_thresholds(A[k], B[k], tmin[k], tmax[k], MW_TILE_W, MW_TILE_H, Tt[k], Ft[k]);
        mwrec::rect_thresholds(A[k], B[k], tmin[k], tmax[k], 2, 2, Tq[k], Fq[k]);
    }

    long long bad = 0, covered = 0, outside_box = 0;
    int64_t lo = INT64_MAX, hi = INT64_MIN;         // the exact edge values' range over the grid
    for (int ty = 0; ty < tiles_y; ++ty)
        for (int tx = 0; tx < tiles_x; ++tx) {
            const bool in_box = mw_qb_box_row(box, ty) && box.x0 <= tx && tx <= box.x1;
            bool tsome[3] = {false, false, false}, tevery[3] = {true, true, true};
            for (int qy = 0; qy < MW_TILE_H / 2; ++qy)
                for (int qx = 0; qx < MW_TILE_W / 2; ++qx) {
                    bool qsome[3] = {false, false, false}, qevery[3] = {true, true, true};
                    const int pxq = tx * MW_TILE_W + qx * 2, pyq = ty * MW_TILE_H + qy * 2;     // the quad's first column, its upper image row
                    for (int i = 0; i < 4; ++i) {
                        const int px = pxq + (i & 1), gy = H - 1 - (pyq + (i >> 1));
                        int m[3];
                        int64_t x[3];
                        bool m_all = true, x_all = true, m_none = false, x_none = false;
                        for (int k = 0; k < 3; ++k) {
                            m[k] = model_at(k, px, gy);
                            x[k] = xcol[(size_t)k * Wg + px] + xrow[(size_t)k * Hg + (gy - gy0)];
                            m_all &= m[k] > tmax[k]; m_none |= m[k] <= tmin[k];
                            const bool some = x[k] > xmin[k], every = x[k] > xmax[k];
                            x_all &= every; x_none |= !some;
                            qsome[k] |= some; qevery[k] &= every;
                            lo = x[k] < lo ? x[k] : lo; hi = x[k] > hi ? x[k] : hi;
                        }
                        if (x_all) { covered += S; if (!in_box) outside_box += S; }
                        if ((m_all && x_all) || (m_none && x_none)) continue;
                        for (int s = 0; s < S; ++s) {
                            const bool min_ = m[0] > thr[0][s] && m[1] > thr[1][s] && m[2] > thr[2][s];
                            const bool xin = x[0] > xthr[0][s] && x[1] > xthr[1][s] && x[2] > xthr[2][s];
                            bad += min_ != xin;
                            if (xin && !x_all) { ++covered; if (!in_box) ++outside_box; }
                        }
                    }
                    // the quad kernel's verdict of the quad: the edge value at its first pixel (pxlo, gylo: the lower GL row) against Tq, Fq
                    bool touch = true, full = true;
                    for (int k = 0; k < 3; ++k) {
                        const int E = model_at(k, pxq, H - 1 - (pyq + 1));
                        touch &= E > Tq[k]; full &= E > Fq[k];
                        tsome[k] |= qsome[k]; tevery[k] &= qevery[k];
                    }
                    n.qquad_touch += touch != (qsome[0] && qsome[1] && qsome[2]);
                    n.qquad_full += full != (qevery[0] && qevery[1] && qevery[2]);
                }
            const int pxlo = tx * MW_TILE_W, pxhi = pxlo + MW_TILE_W - 1, gyhi = H - 1 - ty * MW_TILE_H, gylo = gyhi - (MW_TILE_H - 1);
            const bool want_touch = tsome[0] && tsome[1] && tsome[2], want_full = tevery[0] && tevery[1] && tevery[2];
            bool touch = true, full = true, ttouch = true, tfull = true;
            for (int k = 0; k < 3; ++k) {
                const int E = model_at(k, pxlo, gylo);
                touch &= E > Tt[k]; full &= E > Ft[k];
                int emax, emin;
                mwrec::edge_extremes(A[k], B[k], C[k], pxlo, pxhi, gylo, gyhi, emax, emin);
                ttouch &= emax > tmin[k]; tfull &= emin > tmax[k];
            }
            n.qtile_touch += touch != want_touch; n.qtile_full += full != want_full;
            n.ttile_touch += ttouch != want_touch; n.ttile_full += tfull != want_full;
        }
    n.samples += bad;
    if (a23) n.samples_a23 += bad;
    if (b23) n.samples_b23 += bad;
    n.covered += covered; n.outside_box += outside_box;
    n.sum32 += hi > INT32_MAX || lo < INT32_MIN;
    const long long maxabs = -lo > hi ? -lo : hi;
    n.maxabs = maxabs > n.maxabs ? maxabs : n.maxabs;
}

std::vector<Tri> family(int W, int H, int n_random, uint64_t seed)
{
    // the points in 1/256 pixel (exact as floats)
    const int xs[6] = {0, 1, 128, W * 128, W * 256 - 1, W * 256}, ys[6] = {0, 1, 128, H * 128, H * 256 - 1, H * 256};
    std::vector<Tri> out;
    auto put = [&](const int (&p)[3][2]) {
        Tri t;
        for (int v = 0; v < 3; ++v) { t.w[v][0] = (float)p[v][0] * (1.0f / 256.0f); t.w[v][1] = (float)p[v][1] * (1.0f / 256.0f); t.w[v][2] = 0.5f; t.w[v][3] = 1.0f; }
        out.push_back(t);
    };
    for (int a = 0; a < 36; ++a)
        for (int b = a + 1; b < 36; ++b)
            for (int c = a + 1; c < 36; ++c) {
                if (c == b) continue;
                const int p[3][2] = {{xs[a % 6], ys[a / 6]}, {xs[b % 6], ys[b / 6]}, {xs[c % 6], ys[c / 6]}};
                put(p);
            }
    uint64_t state = seed * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
    auto next = [&](int below) {        // splitmix64
        state += 0x9E3779B97F4A7C15ull;
        uint64_t z = state;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
        return (int)(z % (uint64_t)below);
    };
    for (int i = 0; i < n_random; ++i) {
        const int p[3][2] = {{next(W * 256 + 1), next(H * 256 + 1)}, {next(W * 256 + 1), next(H * 256 + 1)}, {next(W * 256 + 1), next(H * 256 + 1)}};
        put(p);
    }
    return out;
}

}  // namespace

int main(int argc, char **argv)
{
    bool halved = false;
    int threads = 1, n_random = 2000;
    uint64_t seed = 37;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (i + 1 >= argc) { std::fputs("bad arguments\n", stderr); return 2; }
        const std::string v = argv[++i];
        if (a == "--formula" && (v == "records" || v == "halved")) halved = v == "halved";
        else if (a == "--threads") threads = std::atoi(v.c_str());
        else if (a == "--random") n_random = std::atoi(v.c_str());
        else if (a == "--seed") seed = (uint64_t)std::atoll(v.c_str());
        else { std::fputs("bad arguments\n", stderr); return 2; }
    }
    if (threads < 1 || threads > 64 || n_random < 0) { std::fputs("bad arguments\n", stderr); return 2; }
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        long long W, H, S;
        if (!(in >> W)) continue;
        in >> H >> S;
        // (the sizes the engine accepts hold 24.8 coordinates and the column / row tables far below any limit of this program)
        if (!in || W < 1 || H < 1 || W > 4080 || H > 1020 || (S != 8 && S != 4)) { std::puts("bad query"); return 2; }
        const std::vector<Tri> tris = family((int)W, (int)H, n_random, seed);
        std::vector<Counts> part((size_t)threads);
        std::atomic<size_t> next{0};
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)
            pool.emplace_back([&, t] {
                for (size_t lo; (lo = next.fetch_add(32)) < tris.size();)
                    for (size_t i = lo; i < lo + 32 && i < tris.size(); ++i) {
                        if (S == 8) check_triangle<8>(tris[i], (int)W, (int)H, halved, part[(size_t)t]);
                        else check_triangle<4>(tris[i], (int)W, (int)H, halved, part[(size_t)t]);
                    }
            });
        for (std::thread &th : pool) th.join();
        Counts n;
        for (const Counts &p : part) n.add(p);
        std::printf("tris %lld covered %lld samples %lld samples_a23 %lld samples_b23 %lld outside_box %lld thr %lld qtile_touch %lld qtile_full %lld "
                    "qquad_touch %lld qquad_full %lld ttile_touch %lld ttile_full %lld op24 %lld a23 %lld b23 %lld sum32 %lld maxabs %lld\n",
                    n.tris, n.covered, n.samples, n.samples_a23, n.samples_b23, n.outside_box, n.thr, n.qtile_touch, n.qtile_full, n.qquad_touch,
                    n.qquad_full, n.ttile_touch, n.ttile_full, n.op24, n.a23, n.b23, n.sum32, n.maxabs);
        std::fflush(stdout);
    }
    return 0;
}
