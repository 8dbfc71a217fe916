// Scan weighing and resampling on the device (mw_scan_weigh, mw_resample, mw_engine_weigh.hip; the rules, the arrays and every phase:
// mw_weigh.h).
//
// mw_weigh_kernel: one workgroup of MW_WEIGH_THREADS lanes per env; a masked-off env's leaves before any barrier, and so does one of an
// env the grid does not cover: both conditions are the env's, uniform over its workgroup.  Dynamic LDS (mwpolicy::weigh_launch), sized by
// the env's cell count and the beams: the score plane, a byte per cell (32 KiB at MW_NAV_MAX_CELLS), then the beam list, 24 bytes per
// beam (96 KiB at MW_RAY_MAX), a fill word and the 64-bit key: under 129 KiB of a CU's 160.  Phases:
//   0. stage the plane by aligned words of the caller's row, zero the fill word and the key; barrier
//   1. a beam per lane: the beams that pass the t test, as (t, gu, gw), compacted through the LDS counter; barrier.  From here on the
//      plane and the list are only read.
//   2. form 1, a particle per lane, dealt in rounds of the workgroup: every lane walks the whole list — the entry is three LDS words the
//      lanes read together (a broadcast), the score bytes are a gather — and keeps its sums in registers.
//      form 2, a wavefront per particle, dealt in rounds of the workgroup's wavefronts: lane l takes entries l, l + 64, ...; the pose is
//      one address for the wavefront; the two sums meet in a butterfly of adds, lane 0 stores them.
//      Either way each lane keeps the 64-bit key (score, then ~p) of its best particle.
//   3. a butterfly max of the key over each wavefront, one 64-bit LDS atomicMax per wavefront, a barrier, lane 0 decodes best.
// An env whose extent the grid does not cover gets zeros and MW_ST_DEPTH_BAD (mw_scan_project's own bit there).
// Indices: a beam index is below R, so t is read below N * R and dir below N * R * 2; the list holds at most R entries (each beam is pushed
// at most once) at the fill word's old value 0 .. R - 1, three doubles each inside beams_bytes(R); the score row is read at env * cells +
// 0 .. cells - 1 and the plane written at the same 0 .. cells - 1; a lookup's row * gx + col is formed only after 0 <= row < gz and 0 <=
// col < gx, so it is below cells; a particle index is below P: pose at (env * P + p) * 4 + 0 .. 3, out and inside at env * P + p, best at
// env * 2 + 0 .. 1.
//
// mw_resample_kernel: one workgroup of MW_WEIGH_THREADS lanes per env, no view read.  Dynamic LDS: a 64-bit prefix sum per particle and a
// word per wavefront (32 KiB and 32 bytes at MW_WEIGH_MAX_PARTICLES).  Phases:
//   0. lane l sums its run of ceil(P / lanes) consecutive weights; an inclusive scan of the sums over each wavefront by shifts of 1, 2, ...
//      32 lanes; the last lane files the wavefront's total; barrier
//   1. a lane's carry — its wavefront's sums before it and the totals of the wavefronts before its own — and its run's prefix sums into
//      LDS; barrier
//   2. a particle per lane: T_j, then a bisection over the LDS array; the ancestor and, if asked, its pose row
// Indices: a run lies in 0 .. P - 1 (mwweigh::run_of clamps both ends): weight is read at env * P + k, the prefix written at k; the
// bisection keeps 0 <= lo <= mid < hi <= P - 1; ancestor at env * P + j, pose rows at (env * P + p) * 4 + 0 .. 3 with p, j < P; offset at env.
#include "mw_kernels.h"

namespace {

__device__ inline uint64_t shfl_xor64(uint64_t v, int d)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
    return (uint64_t)hi << 32 | lo;
}
__device__ inline uint64_t shfl_up64(uint64_t v, int d)
{
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
    return (uint64_t)hi << 32 | lo;
}

}  // namespace

extern "C" __global__ __launch_bounds__(MW_WEIGH_THREADS) void mw_weigh_kernel(MwNavArgs a, mw_nav_params p, double max_range, int R, int P, int waves,
                                                                               const uint8_t *__restrict__ score, const double *__restrict__ t,
                                                                               const double *__restrict__ dir, const double *__restrict__ pose,
                                                                               const uint8_t *__restrict__ mask, int32_t *__restrict__ out,
                                                                               int32_t *__restrict__ inside, int32_t *__restrict__ best)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t weigh_lds[];
    constexpr int T = MW_WEIGH_THREADS, kWave = mwweigh::kWave;
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (mask && !mask[env]) return;
    const mwnav::Grid g = mwnav::grid_of(a, p, env);
    const int n = g.gx * g.gz;
    int32_t *row_out = out + env * (size_t)P, *row_in = inside ? inside + env * (size_t)P : nullptr;
    if (!mwnav::covers(g)) {
        mwweigh::write_none(P, row_out, row_in, best ? best + env * 2 : nullptr, lane, T);
        if (lane == 0) atomicOr(a.status, MW_ST_DEPTH_BAD);
        return;
    }
    uint8_t *plane = weigh_lds;
    double *beams = reinterpret_cast<double *>(weigh_lds + mwweigh::plane_bytes(n));
    uint32_t *fill = reinterpret_cast<uint32_t *>(weigh_lds + mwweigh::plane_bytes(n) + mwweigh::beams_bytes(R));
    unsigned long long *top = reinterpret_cast<unsigned long long *>(fill + 2);
    const mwweigh::Weigh w{g, max_range, t + env * (size_t)R, dir + env * (size_t)R * 2, R};
    const double *poses = pose + env * (size_t)P * 4;

    mwmatch::stage(score + env * (size_t)n, plane, n, false, lane, T);
    if (lane < mwweigh::kTailBytes / 4) fill[lane] = 0u;
    __syncthreads();
    mwweigh::list_beams(w, beams, fill, lane, T);
    __syncthreads();
    const int listed = (int)*fill;
    uint64_t key = 0;
    if (!waves) {
        for (int q = lane; q < P; q += T) {
            const double *row = poses + 4 * (size_t)q;
            double u0, w0;
            int32_t sum = 0, in = 0;
            if (mwweigh::start_of(g, row, u0, w0)) mwweigh::walk(plane, g.gx, g.gz, beams, listed, u0, w0, row[2], row[3], 0, 1, sum, in);
            row_out[q] = sum;
            if (row_in) row_in[q] = in;
            const uint64_t mine = mwweigh::key_of(sum, q);
            key = mine > key ? mine : key;
        }
    } else {
        for (int q = lane / kWave; q < P; q += T / kWave) {
            const double *row = poses + 4 * (size_t)q;
            double u0, w0;
            int32_t sum = 0, in = 0;
            if (mwweigh::start_of(g, row, u0, w0)) mwweigh::walk(plane, g.gx, g.gz, beams, listed, u0, w0, row[2], row[3], lane % kWave, kWave, sum, in);
            for (int d = kWave / 2; d >= 1; d >>= 1) {
                sum += __shfl_xor(sum, d);
                in += __shfl_xor(in, d);
            }
            if (lane % kWave == 0) {
                row_out[q] = sum;
                if (row_in) row_in[q] = in;
            }
            const uint64_t mine = mwweigh::key_of(sum, q);
            key = mine > key ? mine : key;
        }
    }
    if (!best) return;      // (the call's, uniform)
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const uint64_t other = shfl_xor64(key, d);
        key = other > key ? other : key;
    }
    if (lane % kWave == 0) atomicMax(top, (unsigned long long)key);
    __syncthreads();
    if (lane == 0) mwweigh::decode((uint64_t)*top, best + env * 2);
}

extern "C" __global__ __launch_bounds__(MW_WEIGH_THREADS) void mw_resample_kernel(MwNavArgs a, int P, const uint32_t *__restrict__ weight,
                                                                                  const uint64_t *__restrict__ offset, const uint8_t *__restrict__ mask,
                                                                                  int32_t *__restrict__ ancestor, const double *__restrict__ pose,
                                                                                  double *__restrict__ pose_out)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t resample_lds[];
    constexpr int T = MW_WEIGH_THREADS, kWave = mwweigh::kWave;
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x, wl = lane % kWave, wave = lane / kWave;
    if (mask && !mask[env]) return;
    uint64_t *prefix = reinterpret_cast<uint64_t *>(resample_lds), *totals = prefix + P;
    const uint32_t *row = weight + env * (size_t)P;
    int lo, hi;
    mwweigh::run_of(P, lane, T, lo, hi);
    const uint64_t mine = mwweigh::run_sum(row, lo, hi);
    uint64_t upto = mine;
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t other = shfl_up64(upto, d);
        if (wl >= d) upto += other;
    }
    if (wl == kWave - 1) totals[wave] = upto;
    __syncthreads();
    uint64_t carry = upto - mine;
    for (int k = 0; k < wave; ++k) carry += totals[k];
    mwweigh::run_prefix(row, lo, hi, carry, prefix);
    __syncthreads();
    mwweigh::draw_all(prefix, P, offset[env], ancestor + env * (size_t)P, pose ? pose + env * (size_t)P * 4 : nullptr,
                      pose ? pose_out + env * (size_t)P * 4 : nullptr, lane, T);
}
