// Label frames on the device (mw_label_frame, mw_engine_label.hip; the arithmetic and every phase: mw_label.h).
//
// mw_label_kernel: one workgroup of MW_LABEL_THREADS lanes per env; a masked-off env's leaves before any barrier.  The phases are
// mwlabel::frame_env's, run with (lane, MW_LABEL_THREADS) and the LDS operations below; the frame is labelled in bands of band_rows whole
// rows, each band's state in dynamic LDS (mwlabel::plan_of; sized by mwpolicy::label_launch, at most 64 KiB):
//   per pixel of the band   the bits of the best t so far (64 bits, all ones for none) and a 16-bit code
//   the staged scene        `chunk` polygons as planes and edges (160 bytes each), every slot's volume (72) and statistics words (20)
//   1  a polygon per lane is staged, then a pixel per lane walks the staged polygons itself, in index order: ties fall out of the order;
//      chunk by chunk between barriers where max_polys > MW_LABEL_CHUNK
//   2  a pixel per lane walks the Box slots (and, with MW_LABEL_MESH_BOUNDS, the mesh slots' cylinders) in slot order
//   3  the mesh slots one at a time in slot order, between barriers: a triangle per lane, its plane and edges in registers, the exact test
//      on the pixels of its pruning rectangle only, the minimum per pixel as a 64-bit LDS atomic min on the bits of t (non-negative, so
//      they order as unsigned integers).  A lane whose t went below what the pixel held stores the slot's code — every lane of the phase
//      would store the same —, so equal t stays with the earlier candidate and the result does not depend on the spread over lanes
//   4  a pixel per lane writes the band's rows of the outputs (consecutive lanes, consecutive elements) and counts its slot's pixels and
//      box into the slot's LDS words with 32-bit atomics; the words are written out behind the last band
// Indices: a band pixel is below band_rows * W, the product the LDS was sized with; a rectangle is clamped to the frame as doubles
// before its conversion and to the band's rows after it; a staged polygon is below chunk, a polygon below npolys <= max_polys, a slot
// below E; a mesh id is checked against n_mesh before its descriptor is read (mwlabel::mesh_of) and its triangles are first .. first +
// ntris of the pool the descriptor was made for.  Every barrier sits in a loop whose bounds are the env's alone.
#include "mw_kernels.h"

namespace {

// (the host pass of this unit parses the kernel too: there the operations are empty, and nothing calls them)
struct LdsOps {
#ifdef __HIP_DEVICE_COMPILE__
    static __device__ inline void sync() { __syncthreads(); }
    static __device__ inline uint64_t min64(uint64_t *p, uint64_t v)
    {
        return (uint64_t)atomicMin(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
    }
    static __device__ inline void add(int32_t *p, int32_t v) { atomicAdd(p, v); }
    static __device__ inline void lower(int32_t *p, int32_t v) { atomicMin(p, v); }
    static __device__ inline void raise(int32_t *p, int32_t v) { atomicMax(p, v); }
#else
    static inline void sync() {}
    static inline uint64_t min64(uint64_t *, uint64_t) { return 0; }
    static inline void add(int32_t *, int32_t) {}
    static inline void lower(int32_t *, int32_t) {}
    static inline void raise(int32_t *, int32_t) {}
#endif
};

}  // namespace

extern "C" __global__ __launch_bounds__(MW_LABEL_THREADS) void mw_label_kernel(MwLabelArgs a, mw_label_params p, int band_rows, int chunk, int prune,
                                                                                const uint8_t *__restrict__ mask, uint8_t *__restrict__ cls,
                                                                                int32_t *__restrict__ code, float *__restrict__ depth,
                                                                                int32_t *__restrict__ ent_pixels, int32_t *__restrict__ ent_box)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char label_lds[];
    const size_t env = blockIdx.x;
    if (mask && !mask[env]) return;
    const size_t pixels = (size_t)a.W * (size_t)a.H, E = (size_t)a.r.w.E;
    const mwlabel::Out out{cls + env * pixels, code ? code + env * pixels : nullptr, depth ? depth + env * pixels : nullptr,
                           ent_pixels ? ent_pixels + env * E : nullptr, ent_box ? ent_box + env * E * 4 : nullptr};
    mwlabel::frame_env<LdsOps>(a, p, env, label_lds, band_rows, chunk, prune != 0, out, (int)threadIdx.x, MW_LABEL_THREADS);
}
