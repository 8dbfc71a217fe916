// Asset preparation: the host arithmetic between the caller's arrays and what the engine uploads — the seed of numpy's PCG64
// stream, a texture's mip pyramid, a mesh's tables.  No HIP and no engine state: mw_engine.hip includes it and so does the host
// test library (tests/hostcheck/mwhost.cpp, tests/test_engine_math_cpu.py); no kernel unit does.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>
#include "mw_asset_types.h"
#include "mw_rng.h"

namespace mwasset {
// the seed of numpy's PCG64 stream for a non-negative integer seed: state hi, lo, increment hi, lo — the arithmetic is mw_rng.h's
// (mw::pcg64_seed), shared with the kernels that seed on the device
inline void pcg64_seed(uint64_t seed, uint64_t out[4]) { mw::pcg64_seed(seed, out); }

// Mip pyramid as glGenerateMipmap builds it on the reference's driver (llvmpipe: a GL_LINEAR blit of the previous level):
// destination texel i of dn reads source texels i0, i1 with an 8-bit weight — 24.8 fixed-point coordinate
// iround((i + 0.5) n / dn * 256) - 128, CLAMP_TO_EDGE; 2i, 2i + 1 with weight 128 on an even axis — and
// lerp a + ((w (b - a) + 128) >> 8), x first, then y.  tests/golden/gl_meta.npz holds the driver's own levels (checksums).
struct Taps { int i0, i1, w; };
inline Taps axis_taps(int n, int dn, int i)
{
    Taps t{0, 0, 0};
    if (n == 1) return t;
    const double sc = ((double)i + 0.5) * (double)n / (double)dn * 256.0;
    const long fixed = lrint(sc) - 128;         // round half to even
    const long ip = fixed >> 8;
    t.w = (int)(fixed & 255);
    t.i0 = ip < 0 ? 0 : (ip > n - 1 ? n - 1 : (int)ip);
    t.i1 = ip + 1 < 0 ? 0 : (ip + 1 > n - 1 ? n - 1 : (int)(ip + 1));
    return t;
}
inline int lerp8(int a, int b, int w) { return a + ((w * (b - a) + 128) >> 8); }

inline void build_pyramid(const uint8_t *rgb, int w, int h, std::vector<uint32_t> &out, MwTexDesc &desc)
{
    std::vector<uint8_t> cur(rgb, rgb + (size_t)w * h * 3), nxt;
    desc.w = (uint32_t)w; desc.h = (uint32_t)h; desc.nlevels = 0; desc.pad = 0;
    out.clear();
    for (;;) {
        // a level is stored as one 32-byte record per texel (i, j): its GL_LINEAR footprint (i, j), (i+1, j), (i, j+1),
        // (i+1, j+1), GL_REPEAT applied, laid out for the filter's first step.  The lerp along x of a channel's two texels
        // a, b under the 8-bit weight w, a + ((w (b - a) + 128) >> 8), is ((a * 256 + 128) + w * (b - a)) >> 8 in 16-bit
        // arithmetic (the sum stays in [128, 65408]); a record holds A = a * 256 + 128 and D = (b - a) mod 2^16, two
        // channels to a dword: row j as (A_r | A_b << 16, D_r | D_b << 16, A_g, D_g), then row j + 1 the same.  A bilinear
        // tap is two 16-byte loads, needs neither the neighbours' indices nor their wrap nor any unpacking, and its
        // x step is one packed multiply-add and one packed shift per pair of channels (8x the memory of the texels: the
        // coarse levels an 80x60 frame samples stay cache resident all the same).  Level::off counts records from the
        // start of the pool.
        desc.lvl[desc.nlevels++] = MwTexDesc::Level{(uint32_t)(out.size() / 8), (uint32_t)w, (uint32_t)w - 1u, (uint32_t)h - 1u, (float)w, (float)h, (uint32_t)h, 0u};
        auto chan = [&](int i, int j, int c) { return (uint32_t)cur[((size_t)(j % h) * w + (size_t)(i % w)) * 3 + c]; };
        auto A = [&](int i, int j, int c) { return chan(i, j, c) * 256u + 128u; };
        auto D = [&](int i, int j, int c) { return (chan(i + 1, j, c) - chan(i, j, c)) & 0xFFFFu; };
        for (int j = 0; j < h; ++j)
            for (int i = 0; i < w; ++i)
                for (int r = 0; r < 2; ++r) {
                    out.push_back(A(i, j + r, 0) | (A(i, j + r, 2) << 16)); out.push_back(D(i, j + r, 0) | (D(i, j + r, 2) << 16));
                    out.push_back(A(i, j + r, 1)); out.push_back(D(i, j + r, 1));
                }
        if ((w == 1 && h == 1) || desc.nlevels == MW_MAX_LEVELS) break;
        const int nw = std::max(1, w / 2), nh = std::max(1, h / 2);
        nxt.assign((size_t)nw * nh * 3, 0);
        for (int j = 0; j < nh; ++j) {
            const Taps ty = axis_taps(h, nh, j);
            for (int i = 0; i < nw; ++i) {
                const Taps tx = axis_taps(w, nw, i);
                for (int c = 0; c < 3; ++c) {
                    const int t0 = lerp8(cur[((size_t)ty.i0 * w + tx.i0) * 3 + c], cur[((size_t)ty.i0 * w + tx.i1) * 3 + c], tx.w);
                    const int t1 = lerp8(cur[((size_t)ty.i1 * w + tx.i0) * 3 + c], cur[((size_t)ty.i1 * w + tx.i1) * 3 + c], tx.w);
                    nxt[((size_t)j * nw + i) * 3 + c] = (uint8_t)lerp8(t0, t1, ty.w);
                }
            }
        }
        cur.swap(nxt);
        w = nw; h = nh;
    }
}

// A mesh as the engine keeps it on the host: everything of it that the pools and the descriptor table are repacked from.
// `desc` holds the fields that depend on the mesh alone; first and vfirst are the pools' (mw_upload_mesh assigns them).
struct HostMesh {
    std::vector<float> pos;         // [ntris][MW_MESH_POS_STRIDE], drawing order: 9 coordinates, the i-th triangle of the rasterisation order
    std::vector<float> nrm, rgb, uv;        // [ntris][9], [9], [6] (zeros without texcoords)
    std::vector<float> vtab;        // [nverts][4]: the distinct positions
    std::vector<uint32_t> itab;     // [ntris][2], rasterisation order: three 16-bit indices into vtab, the triangle's index
    std::vector<float> stream;      // [ntris][12], rasterisation order: the entity kernel's triangles (9 coordinates, the triangle's index)
    std::vector<float> attr;        // [ntris][24] ... and their vertex attributes (normals, colours, texture coordinates)
    MwMeshDesc desc{};
};

// pos, nrm, rgb: [ntris][3][3]; uv: [ntris][3][2] or null
inline HostMesh prepare_mesh(const float *pos, const float *nrm, const float *uv, const float *rgb, int ntris, int tex_id)
{
    HostMesh m;
    // storage order: triangles sorted by the direction of their face normal (octahedral map, 6 + 6 bit Morton code,
    // stable), mw_asset_types.h: MW_MESH_POS_STRIDE
    std::vector<uint32_t> order((size_t)ntris), key((size_t)ntris);
    for (int t = 0; t < ntris; ++t) {
        const float *p = pos + (size_t)t * 9;
        const double ax = p[3] - p[0], ay = p[4] - p[1], az = p[5] - p[2], bx = p[6] - p[0], by = p[7] - p[1], bz = p[8] - p[2];
        double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        double l1 = std::fabs(nx) + std::fabs(ny) + std::fabs(nz);
        if (!(l1 > 0.0)) { nx = nrm[(size_t)t * 9]; ny = nrm[(size_t)t * 9 + 1]; nz = nrm[(size_t)t * 9 + 2]; l1 = std::fabs(nx) + std::fabs(ny) + std::fabs(nz); }
        if (!(l1 > 0.0)) { nx = 0; ny = 1; nz = 0; l1 = 1; }
        double u = nx / l1, v = nz / l1;
        if (ny < 0.0) {     // lower hemisphere folded outwards
            const double uu = (1.0 - std::fabs(v)) * (u >= 0 ? 1.0 : -1.0), vv = (1.0 - std::fabs(u)) * (v >= 0 ? 1.0 : -1.0);
            u = uu; v = vv;
        }
        const uint32_t qu = (uint32_t)std::min(63.0, std::max(0.0, (u * 0.5 + 0.5) * 64.0)), qv = (uint32_t)std::min(63.0, std::max(0.0, (v * 0.5 + 0.5) * 64.0));
        uint32_t mc = 0;
        for (int b = 0; b < 6; ++b) mc |= ((qu >> b) & 1u) << (2 * b) | ((qv >> b) & 1u) << (2 * b + 1);
        key[t] = mc; order[t] = (uint32_t)t;
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    m.pos.assign((size_t)ntris * MW_MESH_POS_STRIDE, 0.0f);
    m.nrm.assign(nrm, nrm + (size_t)ntris * 9); m.rgb.assign(rgb, rgb + (size_t)ntris * 9);
    if (uv) m.uv.assign(uv, uv + (size_t)ntris * 6); else m.uv.assign((size_t)ntris * 6, 0.0f);
    for (int i = 0; i < ntris; ++i) {
        memcpy(&m.pos[(size_t)i * MW_MESH_POS_STRIDE], pos + (size_t)i * 9, 36);
        memcpy(&m.pos[(size_t)i * MW_MESH_POS_STRIDE + 9], &order[i], 4);      // the i-th triangle of the rasterisation order
    }
    // the table of distinct positions (bit patterns: -0 and 0 stay apart) and the triangles' indices into it, in
    // rasterisation order; a mesh with more than MW_MESH_VCAP positions keeps none (the entity kernel then takes its
    // triangles through the vertex stage one by one)
    std::map<std::array<uint32_t, 3>, uint32_t> seen;
    m.itab.assign((size_t)ntris * 2, 0u);
    bool fits = true;
    for (int k = 0; k < ntris && fits; ++k) {
        const uint32_t tri = order[k];
        uint32_t ix[3];
        for (int c = 0; c < 3; ++c) {
            const float *pp = pos + ((size_t)tri * 3 + c) * 3;
            std::array<uint32_t, 3> bits; memcpy(bits.data(), pp, 12);
            auto it = seen.find(bits);
            if (it == seen.end()) {
                if (seen.size() >= MW_MESH_VCAP) { fits = false; break; }
                it = seen.emplace(bits, (uint32_t)seen.size()).first;
                m.vtab.insert(m.vtab.end(), {pp[0], pp[1], pp[2], 0.0f});
            }
            ix[c] = it->second;
        }
        m.itab[(size_t)k * 2] = ix[0] | (ix[1] << 16);
        m.itab[(size_t)k * 2 + 1] = ix[2] | (tri << 16);
    }
    if (!fits) m.vtab.clear();
    // the entity kernel's stream: the triangles in rasterisation order, 48 bytes each (9 coordinates, the triangle's index),
    // and their vertex attributes in the same order, 96 bytes each (normals, colours, texture coordinates)
    m.stream.assign((size_t)ntris * 12, 0.0f); m.attr.assign((size_t)ntris * 24, 0.0f);
    for (size_t k = 0; k < (size_t)ntris; ++k) {
        const uint32_t tri = order[k];
        memcpy(&m.stream[k * 12], pos + (size_t)tri * 9, 36);
        memcpy(&m.stream[k * 12 + 9], &tri, 4);
        memcpy(&m.attr[k * 24], &m.nrm[(size_t)tri * 9], 36);
        memcpy(&m.attr[k * 24 + 9], &m.rgb[(size_t)tri * 9], 36);
        memcpy(&m.attr[k * 24 + 18], &m.uv[(size_t)tri * 6], 24);
    }
    MwMeshDesc &md = m.desc;
    md.ntris = (uint32_t)ntris; md.tex = tex_id; md.nverts = (uint32_t)(m.vtab.size() / 4);
    memcpy(md.last_n, nrm + ((size_t)(ntris - 1) * 3 + 2) * 3, 12);
    // the sphere about the origin; the bounding box, its centre, the sphere about the centre (doubles: the radius rounds up)
    float r2 = 0.0f;
    for (int c = 0; c < 3; ++c) { md.bmin[c] = pos[c]; md.bmax[c] = pos[c]; }
    for (size_t i = 0; i < (size_t)ntris * 3; ++i) {
        r2 = std::max(r2, pos[i * 3] * pos[i * 3] + pos[i * 3 + 1] * pos[i * 3 + 1] + pos[i * 3 + 2] * pos[i * 3 + 2]);
        for (int c = 0; c < 3; ++c) { md.bmin[c] = std::min(md.bmin[c], pos[i * 3 + c]); md.bmax[c] = std::max(md.bmax[c], pos[i * 3 + c]); }
    }
    const float r = std::sqrt(r2) * 1.0001f;
    memcpy(&md.bound_bits, &r, 4);
    for (int c = 0; c < 3; ++c) md.center[c] = 0.5f * (md.bmin[c] + md.bmax[c]);
    double rc2 = 0.0;
    for (size_t i = 0; i < (size_t)ntris * 3; ++i) {
        double d2 = 0.0;
        for (int c = 0; c < 3; ++c) { const double d = (double)pos[i * 3 + c] - (double)md.center[c]; d2 += d * d; }
        rc2 = std::max(rc2, d2);
    }
    md.radius = (float)(std::sqrt(rc2) * 1.0001 + 1e-6);
    return m;
}

}  // namespace mwasset
