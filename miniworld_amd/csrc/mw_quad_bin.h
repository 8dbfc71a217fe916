// The quad kernel's binning arithmetic (mw_rasterq.hip, phases A and B), shared with the host (tests/hostcheck/quad_binning.cpp).
//
// A rectangle of the frame (a 16x4 tile, a 2x2 quad) is classified against a triangle by the three edge values at its first pixel
// (pxlo, gylo), E_k = mul24(A_k, pxlo) + mul24(B_k, gylo) + C_k: touched iff E_k > T_k for every k, covered iff E_k > F_k (the
// thresholds of the rectangle's size: QRec's CT quads).  Neighbouring rectangles share the triangle and their edge values differ by
// a constant, so a lane evaluates the triple once and STEPS it: mul24 is the low 32 bits of the product of the sign-extended low 24
// bits, hence mul24(A, px + d) = mul24(A, px) + mul24(A, d) modulo 2^32 wherever px, d and px + d fit 24 bits (every frame the tile
// and quad kernels draw).  The sums are unsigned (they wrap) and the compares signed: a stepped value is the flat formula's value bit
// for bit, and so is every verdict.
#pragma once
#include <stdint.h>

#include "mw_hd.h"

struct MwEdge3 { uint32_t e[3]; };

// the low 32 bits of the product of the operands' sign-extended low 24 bits (the device's v_mul_i32_i24)
MW_HD int32_t mw_qb_mul24(int32_t a, int32_t b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __mul24(a, b);
#else
    const int64_t a24 = (int64_t)(int32_t)((uint32_t)a << 8) >> 8, b24 = (int64_t)(int32_t)((uint32_t)b << 8) >> 8;
    return (int32_t)(uint32_t)(uint64_t)(a24 * b24);
#endif
}

// the edge triple at the rectangle whose first pixel is (px, gy): the flat formula
MW_HD MwEdge3 mw_qb_start(const int32_t (&A)[3], const int32_t (&B)[3], const int32_t (&C)[3], int32_t px, int32_t gy)
{
    MwEdge3 v;
    for (int k = 0; k < 3; ++k) v.e[k] = (uint32_t)mw_qb_mul24(A[k], px) + (uint32_t)mw_qb_mul24(B[k], gy) + (uint32_t)C[k];
    return v;
}

// what the triple gains over dx pixels to the right and dy rows up (gy grows upwards; image rows grow downwards: dy = -rows)
MW_HD MwEdge3 mw_qb_delta(const int32_t (&A)[3], const int32_t (&B)[3], int32_t dx, int32_t dy)
{
    MwEdge3 d;
    for (int k = 0; k < 3; ++k) d.e[k] = (uint32_t)mw_qb_mul24(A[k], dx) + (uint32_t)mw_qb_mul24(B[k], dy);
    return d;
}

MW_HD void mw_qb_step(MwEdge3 &v, const MwEdge3 &d)
{
    for (int k = 0; k < 3; ++k) v.e[k] += d.e[k];
}

MW_HD void mw_qb_verdict(const MwEdge3 &v, const int32_t (&T)[3], const int32_t (&F)[3], bool &touch, bool &full)
{
    touch = true; full = true;
    for (int k = 0; k < 3; ++k) {
        touch &= (int32_t)v.e[k] > T[k];
        full &= (int32_t)v.e[k] > F[k];
    }
}

// The tile bounding box of a triangle (mw_records.h: x0 | x1 << 8 | y0 << 16 | y1 << 24, tile columns and image tile rows, both ends
// included; 0x00ff00ff is the empty box), held inside a frame of tiles_x x tiles_y tiles.  A walk over it takes the rows y0 .. y1 and
// in each the columns x0 .. x1: none at all when the box is empty.
struct MwTileBox { int32_t x0, x1, y0, y1; };
MW_HD MwTileBox mw_qb_box(uint32_t bbox, int32_t tiles_x, int32_t tiles_y)
{
    MwTileBox b;
    b.x0 = (int32_t)(bbox & 255u); b.x1 = (int32_t)((bbox >> 8) & 255u);
    b.y0 = (int32_t)((bbox >> 16) & 255u); b.y1 = (int32_t)(bbox >> 24);
    b.x1 = b.x1 < tiles_x - 1 ? b.x1 : tiles_x - 1;
    b.y1 = b.y1 < tiles_y - 1 ? b.y1 : tiles_y - 1;
    return b;
}
MW_HD bool mw_qb_box_row(const MwTileBox &b, int32_t ty) { return b.x0 <= b.x1 && b.y0 <= ty && ty <= b.y1; }
