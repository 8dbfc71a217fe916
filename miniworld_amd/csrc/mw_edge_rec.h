// The integer part of a triangle's raster records and the edge values the tile and quad kernels read from them, host + device: the
// record writer (mw_records.h) and the kernels (mw_raster_common.h, mw_rasterq.hip) call these functions, and
// tests/hostcheck/edge_limits.cpp runs the same text on the host against the exact definition (64-bit edge functions at every sample).
//
// The multiplies of the per-pixel edge values are the device's 24-bit ones (mw_qb_mul24: v_mul_i32_i24 reads the sign-extended low 24
// bits of each operand); the sums wrap in 32 bits and the compares are signed.  A coefficient A_k = -(dcdx_k * 256), B_k = dcdy_k * 256
// is read as written for -2^23 <= coefficient < 2^23: vertices are snapped to 1/256 pixel inside [0, W] x [0, H], so
// |dcdy| <= 256 W and |dcdx| <= 256 H, and a frame with W >= 128 or H >= 128 can hold B = +2^23 (an edge over the whole width, dcdy =
// +256 W) or A = +2^23 (an edge over the whole height, dcdx = -256 H), which the multiply reads as -2^23: the edge value is then off by
// 2^24 px (2^24 gy) modulo 2^32 at every pixel column (row) but the first.  mw_policy.h::edge_coeffs_fit keeps such frames away from
// these kernels.
#pragma once
#include <stdint.h>

#include "mw_hd.h"
#include "mw_quad_bin.h"
#include "mw_shape.h"

namespace mwrec {

// the sample patterns as compile-time constants, in 1/16 pixel inside the pixel, GL frame-buffer space (y up): kPat's rows
// (mw_records.h), so that the record writer's thresholds fold to multiply-adds
template <int S> struct Pat;
template <> struct Pat<1> { static constexpr int x[1] = {8}, y[1] = {8}; };
template <> struct Pat<4> { static constexpr int x[4] = {6, 14, 2, 10}, y[4] = {2, 6, 10, 14}; };
template <> struct Pat<8> { static constexpr int x[8] = {9, 7, 13, 5, 3, 1, 11, 15}, y[8] = {5, 11, 9, 3, 13, 7, 15, 1}; };
template <> struct Pat<16> {
    static constexpr int x[16] = {9, 7, 5, 12, 3, 10, 13, 11, 6, 8, 4, 2, 0, 15, 14, 1}, y[16] = {9, 5, 10, 7, 6, 13, 11, 3, 14, 1, 2, 12, 8, 4, 15, 0};
};

// edge k of a record: the coefficients of the pixel's coordinates ...
MW_HD void edge_coeffs(int dcdx, int dcdy, int &A, int &B)
{
    A = -(dcdx * 256);
    B = dcdy * 256;
}

// ... and the thresholds of an S-sample buffer's samples, thr[s] = dcdx sx_s - dcdy sy_s (sx, sy: the sample's 24.8 offset inside the
// pixel; a single-sampled buffer's snapped coordinates are relative to pixel centres: offset 0), 0x7fffffff for s >= S, with their
// smallest and largest
template <int S>
MW_HD void edge_thresholds(int dcdx, int dcdy, int (&thr)[16], int &tmin, int &tmax)
{
    int mn = 0x7fffffff, mx = (int)0x80000000;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int s = 0; s < 16; ++s) {
        const int sx = S == 1 ? 0 : Pat<S>::x[s < S ? s : 0] * 16, sy = S == 1 ? 0 : Pat<S>::y[s < S ? s : 0] * 16;
        const int v = dcdx * sx - dcdy * sy;
        thr[s] = s < S ? v : 0x7fffffff;
        if (s < S) { mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    }
    tmin = mn; tmax = mx;
}

// tile bounds from the snapped vertices' bounds (24.8): the tiles of a W x H frame with a pixel whose samples the triangle can cover,
// x0 | x1 << 8 | y0 << 16 | y1 << 24 (tile columns, image tile rows, both ends included; 0x00ff00ff: none)
MW_HD uint32_t tile_bounds(bool single_sampled, int minx, int maxx, int miny, int maxy, int W, int H)
{
    const int off = single_sampled ? 128 : 0;       // single-sampled: coordinates are relative to pixel centres
    int px0 = (minx + off) >> 8, px1 = (maxx + off) >> 8, gy0 = (miny + off) >> 8, gy1 = (maxy + off) >> 8;
    px0 = px0 < 0 ? 0 : px0; gy0 = gy0 < 0 ? 0 : gy0;
    px1 = px1 > W - 1 ? W - 1 : px1; gy1 = gy1 > H - 1 ? H - 1 : gy1;
    // image rows: py = H - 1 - gy
    const int py0 = H - 1 - gy1, py1 = H - 1 - gy0;
    uint32_t bbox = 0x000000ffu | (0xffu << 16);            // empty
    if (px0 <= px1 && gy0 <= gy1)
        bbox = (uint32_t)(px0 / MW_TILE_W) | ((uint32_t)(px1 / MW_TILE_W) << 8) | ((uint32_t)(py0 / MW_TILE_H) << 16) | ((uint32_t)(py1 / MW_TILE_H) << 24);
    return bbox;
}

// the edge value at GL pixel (px, gy) — sample s is inside edge k iff edge_at(A_k, B_k, C_k, px, gy) > thr_k[s] —: two 24-bit
// multiplies and two adds that wrap
MW_HD int edge_at(int A, int B, int C, int px, int gy)
{
    return (int)((uint32_t)mw_qb_mul24(A, px) + (uint32_t)mw_qb_mul24(B, gy) + (uint32_t)C);
}

// the tile kernels' classification of a tile (mw_raster_common.h, classify_prim): the edge value's largest and smallest over the pixels
// [pxlo, pxhi] x [gylo, gyhi] — it is monotone along x and y, so they sit at corners —, by full 32-bit multiplies that wrap
MW_HD void edge_extremes(int A, int B, int C, int pxlo, int pxhi, int gylo, int gyhi, int &emax, int &emin)
{
    emax = (int)((uint32_t)A * (uint32_t)(A > 0 ? pxhi : pxlo) + (uint32_t)B * (uint32_t)(B > 0 ? gyhi : gylo) + (uint32_t)C);
    emin = (int)((uint32_t)A * (uint32_t)(A > 0 ? pxlo : pxhi) + (uint32_t)B * (uint32_t)(B > 0 ? gylo : gyhi) + (uint32_t)C);
}

// the quad kernel's classification thresholds of a w x h rectangle against the edge value at its first pixel (pxlo, gylo):
// touched iff E > T, covered iff E > F:  T = tmin - max(A, 0) (w - 1) - max(B, 0) (h - 1),  F = tmax - min(A, 0) (w - 1) - min(B, 0) (h - 1)
MW_HD void rect_thresholds(int A, int B, int tmin, int tmax, int w, int h, int &T, int &F)
{
    const int ap = A > 0 ? A : 0, an = A < 0 ? A : 0, bp = B > 0 ? B : 0, bn = B < 0 ? B : 0;
    T = (int)((uint32_t)tmin - (uint32_t)ap * (uint32_t)(w - 1) - (uint32_t)bp * (uint32_t)(h - 1));
    F = (int)((uint32_t)tmax - (uint32_t)an * (uint32_t)(w - 1) - (uint32_t)bn * (uint32_t)(h - 1));
}

}  // namespace mwrec
