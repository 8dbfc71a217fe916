// Grid sight on the device (mw_grid_sight, mw_engine_sight.hip; the rule, the walk and every phase: mw_sight.h).
//
// mw_sight_kernel: one workgroup of MW_SIGHT_THREADS lanes per env; a masked-off env's leaves before any barrier.  Dynamic LDS
// (mwpolicy::sight_launch): the env's opaque row as a bit per cell — 4 KiB at MW_NAV_MAX_CELLS, so one word answers up to 32 probes of
// a walk and a whole row of a 103-wide grid is four words —, behind it the weight row as bytes when there is one, then a gain word per
// viewpoint.  Phases, a barrier between each:
//   1. zero the bit words and the gain words
//   2. stage the rows with mwnav::each_byte (aligned words, peeled ends: an env's row starts at byte env * gx * gz); an opaque byte
//      ors its bit into the word with an LDS atomic — 3 to 15 % of the cells on a sensed map —, a weight byte is stored as it is
//   3. the viewpoints.  A task is (viewpoint, 64 consecutive cells of its range box); every box has at most `chunks` tasks — the
//      unclamped box's, a number the host works out — and wavefront w takes the tasks w, w + waves, ...: with one viewpoint the
//      wavefronts share its box, with many each takes its own, and a box of fewer cells than lanes costs one wavefront, not the
//      workgroup.  A lane tests range and cone for its cell and walks the line (at most 3 probes per step, the first opaque cell ends
//      it), adds the cell's weight and stores the seen byte: a plain same-value store, idempotent.  The wavefront's sum goes through a
//      butterfly and lane 0 adds it to the viewpoint's gain word in LDS.
//   4. the gain words go to the caller's row
// Indices: a cell index is below gx * gz <= MW_NAV_MAX_CELLS (checked before the launch, with the bytes of LDS): the staging runs over
// 0 .. cells - 1 of rows the caller sized [N][gz][gx], an eye is a checked cell (eye_of_cell) or a clamped one (mwnav::cell_of), its box
// is clamped to the grid (mwsight::box_of) and a walk stays in the bounding box of two cells of the grid; a viewpoint index is below
// views <= MW_SIGHT_MAX_VIEWS, the size of d_cells', d_dirs' and d_gain's rows.
#include "mw_kernels.h"

extern "C" __global__ __launch_bounds__(MW_SIGHT_THREADS) void mw_sight_kernel(MwRayArgs a, mw_nav_params p, mwseen::Sight s, int views, int R, int chunks,
                                                                              const uint8_t *__restrict__ mask, const uint8_t *__restrict__ opaque,
                                                                              const uint8_t *__restrict__ weight, const int32_t *__restrict__ cells,
                                                                              const double *__restrict__ dirs, int32_t *__restrict__ gain, uint8_t *seen)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sight_lds[];
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (mask && !mask[env]) return;
    const int gx = p.gx, gz = p.gz, n = gx * gz;
    int32_t *out = gain + env * (size_t)views;
    mwnav::Grid g{0.0, 0.0, 0.0, 0.0, p.cell, gx, gz};
    if (!cells) {
        g = mwnav::grid_of(a.w, p, env);
        if (!mwnav::covers(g)) {
            if (lane == 0) {
                out[0] = 0;
                atomicOr(a.w.status, MW_ST_SEEN_BAD);
            }
            return;
        }
    }
    uint32_t *bits = sight_lds;
    uint8_t *w = weight ? reinterpret_cast<uint8_t *>(sight_lds) + mwsight::bits_bytes(n) : nullptr;
    int32_t *sums = reinterpret_cast<int32_t *>(reinterpret_cast<uint8_t *>(sight_lds) + mwsight::bits_bytes(n) + mwsight::weight_bytes(n, weight != nullptr));
    mwsight::zero_bits(bits, n, lane, MW_SIGHT_THREADS);
    for (int v = lane; v < views; v += MW_SIGHT_THREADS) sums[v] = 0;
    __syncthreads();
    mwsight::stage_bits(opaque + env * (size_t)n, bits, n, lane, MW_SIGHT_THREADS, [](uint32_t *word, uint32_t bit) { atomicOr(word, bit); });
    if (weight) mwnav::stage_extra(weight + env * (size_t)n, w, n, lane, MW_SIGHT_THREADS);
    __syncthreads();
    uint8_t *row = seen ? seen + env * (size_t)n : nullptr;
    const int wave = lane >> 6, wl = lane & 63;
    for (int task = wave; task < views * chunks; task += MW_SIGHT_THREADS / 64) {      // (task, v and the eye are the wavefront's)
        const int v = task / chunks, first = (task % chunks) * 64;
        const mwsight::Eye e = cells ? mwsight::eye_of_cell(s, gx, gz, cells, dirs, env * (size_t)views + (size_t)v) : mwsight::eye_of_agent(a, g, s, env);
        if (!e.ok) continue;
        const mwnav::Box b = mwsight::box_of(e, R, gx, gz);
        const int cnt = mwnav::box_cells(b);
        if (first >= cnt) continue;
        int32_t mine = mwsight::look(bits, w, gx, p.cell, s, e, b, first, first + 64 < cnt ? first + 64 : cnt, row, wl, 64);
        for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m);
        if (wl == 0 && mine) atomicAdd(sums + v, mine);
    }
    __syncthreads();
    for (int v = lane; v < views; v += MW_SIGHT_THREADS) out[v] = sums[v];
}
