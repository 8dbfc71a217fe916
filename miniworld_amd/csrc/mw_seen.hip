// Explored-area maps on the device (mw_seen_update, mw_engine_seen.hip; the tests and every phase: mw_seen.h).
//
// mw_seen_kernel: one workgroup of MW_SEEN_THREADS lanes per env; a masked-off env's leaves before any barrier.  The env's walls and,
// with MW_SEEN_ENTITIES, its entity slots as circles are staged once in dynamic LDS as mw_ray_lanes_kernel stages them (MW_RAY_WALL_BYTES
// per segment of max_segs, MW_RAY_DISC_BYTES per slot), behind them the candidate list and four words (MW_SEEN_TAIL_BYTES; the sum is
// checked against 64 KiB before the launch).  A cleared env's row is zeroed by the workgroup itself.  Then the cells of the box around the
// agent, MW_SEEN_CANDS of them per round:
//   A  a cell per lane, tests 1 - 3 (no division, no obstacle); a ballot compacts the survivors' cell indices into the LDS list — a
//      wavefront's leader reserves the wavefront's entries with one LDS add, order within the list is irrelevant
//   B  a candidate per lane walks the obstacles in index order — every lane reads the same LDS address (a broadcast) — and stops at
//      its first hit; a free line loads the cell's byte and stores a 1 where it was 0
// A round holds at most as many candidates as the list has entries, so the list never overflows; its two length words alternate
// between rounds (lane 0 zeroes the next round's during B), which leaves two barriers per round.  The lanes' counts of new cells are
// summed over each wavefront by a butterfly and over the workgroup by an LDS add; lane 0 writes d_new and carries the count.
// Indices: a cell index is below gx * gz <= MW_NAV_MAX_CELLS < 2^16 (boxes are clamped to the grid, mwnav::axis_range), a list index
// below MW_SEEN_CANDS, a wall index below nsegs_of() <= max_segs, a slot below E.
#include "mw_kernels.h"

extern "C" __global__ __launch_bounds__(MW_SEEN_THREADS) void mw_seen_kernel(MwRayArgs a, mw_nav_params p, mwseen::Sight s, const uint8_t *__restrict__ mask,
                                                                             const uint8_t *__restrict__ clear, uint8_t *seen, int32_t *__restrict__ count,
                                                                             int32_t *__restrict__ newly)
{
    extern __shared__ __attribute__((aligned(16))) double seen_lds[];
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (mask && !mask[env]) return;
    const mwnav::Grid g = mwnav::grid_of(a.w, p, env);
    const int cells = g.gx * g.gz;
    uint8_t *row = seen + env * (size_t)cells;
    if (!mwnav::covers(g)) {
        mwseen::zero_row(row, cells, lane, MW_SEEN_THREADS);
        if (lane == 0) {
            count[env] = 0;
            if (newly) newly[env] = 0;
            atomicOr(a.w.status, MW_ST_SEEN_BAD);
        }
        return;
    }
    const bool cleared = clear && clear[env];
    const int ns = mwnav::nsegs_of(a.w, env), ne = mwseen::ents_of(a, s);
    mwray::Wall *walls = reinterpret_cast<mwray::Wall *>(seen_lds);
    mwray::Disc *discs = reinterpret_cast<mwray::Disc *>(walls + a.w.max_segs);
    // (the tail starts at the staged obstacles' bytes rounded up to 16, as mwpolicy::seen_launch sizes it)
    const size_t staged = ((size_t)a.w.max_segs * MW_RAY_WALL_BYTES + (size_t)a.w.E * MW_RAY_DISC_BYTES + 15) / 16 * 16;
    uint16_t *cands = reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(seen_lds) + staged);
    int *words = reinterpret_cast<int *>(cands + MW_SEEN_CANDS);       // [0], [1]: the list's length, by round parity; [2]: new cells
    mwseen::stage(a, s, env, walls, discs, lane, MW_SEEN_THREADS);
    if (cleared) mwseen::zero_row(row, cells, lane, MW_SEEN_THREADS);
    if (lane < 4) words[lane] = 0;
    __syncthreads();
    const mwseen::View v = mwseen::view_of(a, s, env);
    const mwnav::Box b = mwseen::box_of(g, v, s);
    const int w = mwnav::box_w(b), n = mwnav::box_cells(b);
    const int wl = lane & 63;
    int mine = 0;
    for (int base = 0, round = 0; base < n; base += MW_SEEN_CANDS, ++round) {       // (base, n and round are the workgroup's)
        int *len = words + (round & 1);
        const int end = base + MW_SEEN_CANDS < n ? base + MW_SEEN_CANDS : n;
        for (int k0 = base; k0 < end; k0 += MW_SEEN_THREADS) {      // (whole wavefronts run every turn: the ballot is the wavefront's)
            const int k = k0 + lane;
            int c = 0;
            bool ok = false;
            if (k < end) {
                const int j = b.j0 + k / w, i = b.i0 + k % w;
                ok = mwseen::in_sight(g, v, s, j, i);
                c = j * g.gx + i;
            }
            const unsigned long long found = __ballot(ok);
            if (found) {
                int at = 0;
                if (wl == 0) at = atomicAdd(len, __popcll(found));
                at = __shfl(at, 0);
                if (ok) cands[at + __popcll(found & ((1ull << wl) - 1ull))] = (uint16_t)c;
            }
        }
        __syncthreads();
        const int nc = *len;
        if (lane == 0) words[(round + 1) & 1] = 0;
        for (int q = lane; q < nc; q += MW_SEEN_THREADS) {
            const int c = cands[q];
            if (mwseen::free_line(mwseen::ray_to(g, v, c / g.gx, c % g.gx), walls, ns, discs, ne)) mine += mwseen::set_cell(row, c);
        }
        __syncthreads();
    }
    for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m);
    if (wl == 0 && mine) atomicAdd(words + 2, mine);
    __syncthreads();
    if (lane == 0) {
        const int total = words[2];
        count[env] = (cleared ? 0 : count[env]) + total;
        if (newly) newly[env] = total;
    }
}
