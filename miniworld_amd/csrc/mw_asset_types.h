// The texture and mesh descriptors, as the kernels read them and as asset preparation (mw_assets.h) fills them: plain types and
// constants, no HIP — the host tests compile them with a plain C++ compiler (tests/hostcheck/mwhost.cpp).
#pragma once
#include <stdint.h>
#define MW_MAX_LEVELS 16
#define MW_MESH_VCAP 3568       // distinct positions of a mesh whose vertex stage runs per vertex (mw_mesh_entity_kernel: 16 bytes of LDS each, 57 088 B + the kernel's 8 204 B of queues = 65 292 B, within a workgroup's 64 KB; static_assert in mw_raster_mesh.hip)

struct MwTexDesc {
    uint32_t w, h, nlevels, pad;
    // per mip level, everything a bilinear fetch needs, so that a lane gets it with two 16-byte loads instead of
    // shifting / clamping / converting the level-0 size itself (8 VALU instructions per level and fetch)
    struct Level {
        uint32_t off;              // first texel (dword index into the texel pool)
        uint32_t w;                // row length in texels
        uint32_t wmask, hmask;     // w - 1, h - 1 (wrap masks of power-of-two levels)
        float fw, fh;              // (float)w, (float)h
        uint32_t h, pad;
    } lvl[MW_MAX_LEVELS];
};

struct MwMeshDesc {
    uint32_t ntris;
    int32_t tex;
    uint32_t first;                // first triangle in the mesh pools
    uint32_t bound_bits;           // float bits: max |vertex| (radius of the bounding sphere about the mesh origin)
    float last_n[3];               // vertex normal of the LAST triangle's last vertex in drawing order (GL's current
    uint32_t pad;                  //   normal after the mesh, for the top view's agent marker)
    uint32_t vfirst, nverts;       // the mesh's table of distinct positions in the vertex pool (nverts = 0: more than MW_MESH_VCAP, no table)
    float bmin[3], bmax[3];        // bounding box of the vertices (object space), its centre and the radius of the sphere about the centre
    float center[3];               //   that holds them: the geometry kernel's view test and tile rectangle (a ball's origin lies at its
    float radius;                  //   foot: the sphere about the ORIGIN has twice the ball's radius, four times its tiles)
};

// Mesh pools: per-face-vertex arrays in drawing order (= draw ids, GL's first-drawn-wins on equal depth, the oracle's
// triangle indices).  The mesh kernels RASTERISE the triangles in another order — sorted by the direction of their face
// normal (mw_assets.h: prepare_mesh), so that the 64 triangles of a wavefront face the same way and back-face culling retires
// whole waves instead of half the lanes of each: a position record is 9 floats + one word, the index of the i-th triangle of
// that order.  (Shading looks a triangle up by its draw id directly: no indirection on the tile phase's critical path.)
#define MW_MESH_POS_STRIDE 10
