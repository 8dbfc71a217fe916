// Object maps on the device (mw_label_project, mw_engine_labelmap.hip; the arithmetic and every phase: mw_labelmap.h).
//
// mw_labelmap_kernel: one workgroup of MW_LABELMAP_THREADS lanes per env; a masked-off env's leaves before any barrier.  Dynamic LDS holds
// a uint32 key per cell of the target — the window's size * size or the grid's gx * gz, at most MW_LABELMAP_MAX_CELLS — and behind the
// keys 3 * K words, the n, si and sj of every id: 68 596 bytes at the largest map with K = 255, above 64 KiB; the engine asks for it as
// for mw_nav_grid_kernel (a CU has 160 KiB).  The phases:
//   1  the keys to MW_LABELMAP_UNSEEN, the sums to 0; barrier
//   2  consecutive lanes take consecutive pixels of the env's depth and code rows — four at a time as one 16-byte load of each where
//      `wide` (W * H a multiple of 4 and both bases aligned; the host decides) —, bin each with mwdepth::point_of / window_bin / map_bin
//      and lower the cell's key with an LDS atomicMin: the minimum does not depend on the order of arrival.  A lane's four pixels are
//      neighbours in a row and mostly share a cell: the lane holds the running minimum of a bin and flushes it when the bin changes,
//      as the depth kernel holds its sum.  Barrier
//   3  a cell per lane, MW_LABELMAP_THREADS a round: the window's plane (consecutive lanes store consecutive bytes), or the map's bytes
//      merged — rewritten where the env is cleared or the frame saw the cell —; with K > 0 every cell of the map, touched by this frame
//      or not, adds (1, i, j) to the three words of its byte's id with LDS integer atomics.  Barrier; lanes q < K write row q of
//      obj_cells and obj_pos
// An env whose extent the grid does not cover gets its map zeroed, its cells 0, its positions NaN and MW_ST_LABELMAP_BAD.
// Indices: a pixel index is below W * H <= MW_DEPTH_MAX_PIXELS (the wide form reads pixels / 4 whole groups of a row whose length is a
// multiple of 4); a bin's inside test precedes its conversion to an index (mwdepth::window_bin, map_bin), so a cell index is below
// n <= MW_LABELMAP_MAX_CELLS, and -1 is never an index: a pixel without a bin returns before its key is made, a lane that holds nothing
// flushes nothing (flush tests bin >= 0); byte - 1 < K is tested before it indexes the sums, whose words n .. n + 3 * K - 1 are the ones
// mwpolicy::labelmap_launch allots; an output row's index is below K.
#include "mw_kernels.h"

namespace {

// the workgroup's LDS words
struct LdsOps {
    static __device__ inline void lowest(uint32_t *p, uint32_t v) { atomicMin(p, v); }
    static __device__ inline void add(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
};

}  // namespace

extern "C" __global__ __launch_bounds__(MW_LABELMAP_THREADS) void mw_labelmap_kernel(MwRayArgs a, const double *__restrict__ cam, mwdepth::Sensor s, mwdepth::Window w,
                                                                                      mw_nav_params p, int wide, const float *__restrict__ depth,
                                                                                      const int32_t *__restrict__ code, int32_t base, const uint8_t *__restrict__ mask,
                                                                                      const uint8_t *__restrict__ clear, uint8_t *__restrict__ plane,
                                                                                      uint8_t *__restrict__ map, int K, int32_t *__restrict__ obj_cells,
                                                                                      double *__restrict__ obj_pos)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t labelmap_keys[];
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (mask && !mask[env]) return;
    const bool to_map = map != nullptr;
    const mwnav::Grid g = mwnav::grid_of(a.w, p, env);
    const int n = to_map ? g.gx * g.gz : w.size * w.size;
    uint8_t *row = (to_map ? map : plane) + env * (size_t)n;
    int32_t *cells = obj_cells ? obj_cells + env * (size_t)K : nullptr;
    double *pos = obj_pos ? obj_pos + env * (size_t)K * 3 : nullptr;
    if (to_map && !mwnav::covers(g)) {
        mwlabelmap::zero_row(row, n, lane, MW_LABELMAP_THREADS);
        mwlabelmap::write_objects(g, nullptr, K, cells, pos, lane, MW_LABELMAP_THREADS);
        if (lane == 0) atomicOr(a.w.status, MW_ST_LABELMAP_BAD);
        return;
    }
    mwlabelmap::fill_keys(labelmap_keys, n, K, lane, MW_LABELMAP_THREADS);
    __syncthreads();
    const mwlabelmap::Call q{mwdepth::camera_of(a, cam, s, env), s, w, g, to_map, base};
    const size_t first = env * (size_t)(s.W * s.H);
    mwlabelmap::lowest_keys<LdsOps>(q, depth + first, code + first, wide != 0, labelmap_keys, lane, MW_LABELMAP_THREADS);
    __syncthreads();
    if (!to_map) {
        mwlabelmap::write_plane(labelmap_keys, n, row, lane, MW_LABELMAP_THREADS);
        return;
    }
    uint32_t *sums = labelmap_keys + n;
    mwlabelmap::merge_map<LdsOps>(labelmap_keys, n, g.gx, clear && clear[env], row, K, sums, lane, MW_LABELMAP_THREADS);
    if (K == 0) return;         // (K is the launch's: every lane leaves or none)
    __syncthreads();
    mwlabelmap::write_objects(g, sums, K, cells, pos, lane, MW_LABELMAP_THREADS);
}
