// Depth projection on the device (mw_depth_project, mw_engine_depth.hip; the arithmetic and every phase: mw_depth.h).
//
// mw_depth_kernel: one workgroup of MW_DEPTH_THREADS lanes per env; a masked-off env's leaves before any barrier.  The counts live in
// dynamic LDS, a uint32 per cell of the target — the window's size * size or the grid's gx * gz, at most MW_DEPTH_MAX_CELLS: floor points
// in the low half, obstacle points in the high half.  A frame has at most MW_DEPTH_MAX_PIXELS = 65535 pixels, so the low half cannot carry
// into the high one and neither can wrap (the host refuses a larger frame for this reason).  The phases:
//   1  zero the cells; barrier
//   2  consecutive lanes take consecutive pixels of the env's depth row — four at a time as one 16-byte load where `wide` (W * H a
//      multiple of 4 and the base aligned; the host decides) —, unproject, class and bin each (mwdepth::bin_of) and add 1 or 1 << 16 to
//      the cell with an LDS atomic; the sum does not depend on the order of arrival.  A lane's four pixels are neighbours in a row and
//      mostly share a cell: equal bins are added up in the lane first, one atomic for them.  Barrier
//   3  a cell per lane, MW_DEPTH_THREADS a round: the window's two planes (consecutive lanes store consecutive bytes), or the map's two
//      rows — a byte goes 0 -> 1 once the call's count reaches min_points; a cleared env's rows are rewritten whole in the same pass —,
//      whose new cells are summed over each wavefront by a butterfly and over the workgroup through LDS words that reuse the first cells
//      behind one more barrier; lane 0 writes `newly` and carries `count`
// An env whose extent the grid does not cover gets its rows zeroed, its counts 0 and MW_ST_DEPTH_BAD.
// Indices: a pixel index is below W * H <= 65535, a cell index below n <= MW_DEPTH_MAX_CELLS (the bins' inside tests precede the
// conversion; -1 is never used as an index: add is 0 then), a plane's offset below 2 * n, a reduction word below 2 * waves <= the LDS words
// mwpolicy::depth_launch allots (at least 2 * MW_DEPTH_THREADS / 64).
#include "mw_kernels.h"

namespace {

__device__ inline void add_point(uint32_t *cells, int b, uint32_t add)
{
#if MW_DEPTH_WAVE_MERGE
    // equal bins of the wavefront, added up by the first lane that holds one (measured against the plain add: DESIGN.md section 8)
    unsigned long long todo = __ballot(add != 0u);
    const int wl = (int)threadIdx.x & 63;
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int lb = __shfl(b, lead);
        const bool same = add != 0u && b == lb;
        uint32_t sum = same ? add : 0u;
        for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
        if (wl == lead) atomicAdd(cells + lb, sum);
        todo &= ~__ballot(same);
    }
#else
    if (add) atomicAdd(cells + b, add);
#endif
}

}  // namespace

extern "C" __global__ __launch_bounds__(MW_DEPTH_THREADS) void mw_depth_kernel(MwRayArgs a, const double *__restrict__ cam, mwdepth::Sensor s, mwdepth::Window w,
                                                                                mw_nav_params p, int min_points, int wide, const float *__restrict__ depth,
                                                                                const uint8_t *__restrict__ mask, const uint8_t *__restrict__ clear,
                                                                                uint8_t *__restrict__ planes, uint8_t *__restrict__ map,
                                                                                int32_t *__restrict__ count, int32_t *__restrict__ newly)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t depth_cells[];
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (mask && !mask[env]) return;
    const bool to_map = map != nullptr;
    const mwnav::Grid g = mwnav::grid_of(a.w, p, env);
    const int n = to_map ? g.gx * g.gz : w.size * w.size;
    uint8_t *rows = to_map ? map + env * 2 * (size_t)n : planes + env * 2 * (size_t)n;
    if (to_map && !mwnav::covers(g)) {
        mwdepth::zero_rows(rows, n, lane, MW_DEPTH_THREADS);
        if (lane == 0) {
            count[env * 2] = count[env * 2 + 1] = 0;
            if (newly) newly[env * 2] = newly[env * 2 + 1] = 0;
            atomicOr(a.w.status, MW_ST_DEPTH_BAD);
        }
        return;
    }
    mwdepth::zero_cells(depth_cells, n, lane, MW_DEPTH_THREADS);
    __syncthreads();
    const mwdepth::Camera c = mwdepth::camera_of(a, cam, s, env);
    const int pixels = s.W * s.H;
    const float *row = depth + env * (size_t)pixels;
    if (wide && !MW_DEPTH_WAVE_MERGE) {
        const float4 *row4 = reinterpret_cast<const float4 *>(row);
        for (int q = lane; q < pixels / 4; q += MW_DEPTH_THREADS) {
            const float4 d4 = row4[q];
            int held = -1;
            uint32_t sum = 0u;
            // a pixel of the four: its bin's add joins the held one's, or the held sum goes to LDS and the new bin is held
            auto one = [&](int k, float d) {
                uint32_t add;
                const int b = mwdepth::bin_of(c, s, w, g, to_map, k, d, add);
                if (!add) return;
                if (b != held) {
                    add_point(depth_cells, held, sum);
                    held = b;
                    sum = 0u;
                }
                sum += add;
            };
            one(q * 4, d4.x);
            one(q * 4 + 1, d4.y);
            one(q * 4 + 2, d4.z);
            one(q * 4 + 3, d4.w);
            add_point(depth_cells, held, sum);
        }
    } else {
        for (int k0 = 0; k0 < pixels; k0 += MW_DEPTH_THREADS) {        // (whole wavefronts run every turn: the merge is the wavefront's)
            const int k = k0 + lane;
            uint32_t add = 0u;
            const int b = k < pixels ? mwdepth::bin_of(c, s, w, g, to_map, k, row[k], add) : -1;
            add_point(depth_cells, b, add);
        }
    }
    __syncthreads();
    if (!to_map) {
        mwdepth::write_planes(depth_cells, n, rows, lane, MW_DEPTH_THREADS);
        return;
    }
    const bool cleared = clear && clear[env];
    int nf = 0, no = 0;
    mwdepth::or_map(depth_cells, n, (uint32_t)min_points, cleared, rows, nf, no, lane, MW_DEPTH_THREADS);
    for (int m = 32; m >= 1; m >>= 1) {
        nf += __shfl_xor(nf, m);
        no += __shfl_xor(no, m);
    }
    __syncthreads();        // every lane has read its cells: the first words now carry the wavefronts' sums
    const int wave = lane >> 6;
    if ((lane & 63) == 0) {
        depth_cells[wave * 2] = (uint32_t)nf;
        depth_cells[wave * 2 + 1] = (uint32_t)no;
    }
    __syncthreads();
    if (lane == 0) {
        int tf = 0, to = 0;
        for (int k = 0; k < MW_DEPTH_THREADS / 64; ++k) {
            tf += (int)depth_cells[k * 2];
            to += (int)depth_cells[k * 2 + 1];
        }
        count[env * 2] = (cleared ? 0 : count[env * 2]) + tf;
        count[env * 2 + 1] = (cleared ? 0 : count[env * 2 + 1]) + to;
        if (newly) {
            newly[env * 2] = tf;
            newly[env * 2 + 1] = to;
        }
    }
}
