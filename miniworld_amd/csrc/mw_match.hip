// Scan matching on the device (mw_scan_match, mw_engine_match.hip; the rule, the arrays and every phase: mw_match.h).
//
// mw_match_kernel: one workgroup of MW_MATCH_THREADS lanes per env; a masked-off env's leaves before any barrier, and so does one of an
// env the grid does not cover: both conditions are the env's, uniform over its workgroup.  Dynamic LDS (mwpolicy::match_launch), sized
// by the env's cell count, the beams and the batch: the score plane, a byte per cell (32 KiB at MW_NAV_MAX_CELLS; the Maze's 103 x 103:
// 10.4 KiB; the quad form adds 144 bytes of pads), then two buffers of `batch` end-cell lists of R words (2 x 16 KiB at MW_RAY_MAX with a
// batch of one; 4 KiB at 256 beams and a batch of two), a fill word per rotation and the 64-bit key.  Two forms of the correlation,
// the same bits, chosen by the launch: a translation per lane reading a byte per end cell, or four adjacent columns per lane reading two
// words per end cell (mw_match.h).  Either serves every grid and window.  Phases:
//   0. stage the plane by aligned words of the caller's row, zero the fill words and the key, list the first batch's end cells; barrier
//   r0. per batch of rotations r0 .. r0 + nb - 1, ONE barrier at its end: every lane first lists the next batch's end cells into the
//      other buffer — a beam per lane per rotation, the counting beams compacted through an LDS counter (fill[r], zero since phase 0),
//      those the window cannot bring into the grid dropped — and then scores its candidates of this batch, dealt flat over the batch's
//      rotations: lane l takes tasks l, l + lanes, ..., consecutive lanes consecutive columns: the list entry is one LDS word the
//      lanes of a rotation read together (a broadcast), the score bytes of a wavefront lie in a few consecutive words per row it spans.
//      The sums go to the volume and into the lane's 64-bit key (score, then the tie rank) in registers.
//      The barrier orders the next batch's lists complete before they are read, and this batch's read before the batch after the next overwrites them.
//   K. a butterfly max of the key over each wavefront, one 64-bit LDS atomicMax per wavefront, a barrier, lane 0 decodes best and score.
// An env whose extent the grid does not cover gets zeros and MW_ST_DEPTH_BAD (mw_scan_project's own bit there).
// Indices: a beam index is below R, so t is read below N * R and dir below N * R * 2; origin at env * 3 and + 2; the score row is read at
// env * cells + 0 .. cells - 1 and the plane written at the same 0 .. cells - 1 (behind kQuadPad in the quad form, whose pads are
// 2 kQuadPad more bytes inside plane_bytes); list g of buffer h starts at (h * batch + g) * R < 2 * batch * R words and holds at most R
// entries (each beam pushes at most once per rotation) at fill[r]'s old value 0 .. R - 1, r < K <= MW_MATCH_MAX_ROT fill words; a byte
// lookup's row * gx + col is formed only after 0 <= row < gz and 0 <= col < gx, so it is below cells; a quad lookup's words: mw_match.h,
// at correlate4; a volume entry is env * K * T + r * T + k with k < T = (2 W + 1)^2 of a tensor the caller sized [N][K][2 W + 1][2 W + 1];
// best at env * 3 + 0 .. 2, best_score at env.
#include "mw_kernels.h"

extern "C" __global__ __launch_bounds__(MW_MATCH_THREADS) void mw_match_kernel(MwNavArgs a, mw_nav_params p, double max_range, int R, MwMatchRot rot, int W, int batch, int quad,
                                                                               const uint8_t *__restrict__ score, const double *__restrict__ t,
                                                                               const double *__restrict__ dir, const double *__restrict__ origin,
                                                                               const uint8_t *__restrict__ mask, int32_t *__restrict__ best,
                                                                               int32_t *__restrict__ best_score, int32_t *__restrict__ volume)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t match_lds[];
    constexpr int T = MW_MATCH_THREADS;
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (mask && !mask[env]) return;
    const mwnav::Grid g = mwnav::grid_of(a, p, env);
    const int n = g.gx * g.gz, side = 2 * W + 1, K = rot.n;
    int32_t *vol = volume ? volume + env * (size_t)K * side * side : nullptr;
    if (!mwnav::covers(g)) {
        mwmatch::write_none(best + env * 3, best_score + env, vol, (size_t)K * side * side, lane, T);
        if (lane == 0) atomicOr(a.status, MW_ST_DEPTH_BAD);
        return;
    }
    uint8_t *plane = match_lds;
    uint32_t *ends = reinterpret_cast<uint32_t *>(match_lds + mwmatch::plane_bytes(n, quad != 0));
    uint32_t *fill = reinterpret_cast<uint32_t *>(match_lds + mwmatch::plane_bytes(n, quad != 0) + mwmatch::ends_bytes(R, batch));
    unsigned long long *top = reinterpret_cast<unsigned long long *>(fill + MW_MATCH_MAX_ROT);
    const mwmatch::Match m{g, origin ? origin[env * 3] : a.ax[env], origin ? origin[env * 3 + 2] : a.az[env], max_range,
                           t + env * (size_t)R, dir + env * (size_t)R * 2, R, W};

    mwmatch::stage(score + env * (size_t)n, plane, n, quad != 0, lane, T);
    for (int k = lane; k < MW_MATCH_MAX_ROT + mwmatch::kTailBytes / 4; k += T) fill[k] = 0u;
    __syncthreads();
    for (int i = 0; i < batch && i < K; ++i) mwmatch::list_ends(m, rot.cs[i][0], rot.cs[i][1], ends + (size_t)i * R, fill + i, lane, T);
    __syncthreads();
    uint64_t key = 0;
    for (int r0 = 0, buf = 0; r0 < K; r0 += batch, buf ^= 1) {
        for (int i = 0, r = r0 + batch; i < batch && r < K; ++i, ++r)
            mwmatch::list_ends(m, rot.cs[r][0], rot.cs[r][1], ends + ((size_t)(buf ^ 1) * batch + i) * R, fill + r, lane, T);
        const int nb = K - r0 < batch ? K - r0 : batch;
        const uint32_t *lists = ends + (size_t)buf * batch * R;
        key = quad ? mwmatch::correlate4(plane, g.gx, g.gz, W, r0, nb, lists, R, fill, vol, key, lane, T)
                   : mwmatch::correlate(plane, g.gx, g.gz, W, r0, nb, lists, R, fill, vol, key, lane, T);
        __syncthreads();
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), d);
        const uint64_t other = (uint64_t)hi << 32 | lo;
        key = other > key ? other : key;
    }
    if ((lane & 63) == 0) atomicMax(top, (unsigned long long)key);
    __syncthreads();
    if (lane == 0) mwmatch::decode((uint64_t)*top, W, best + env * 3, best_score + env);
}
