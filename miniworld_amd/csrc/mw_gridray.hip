// Grid ray casts on the device (mw_grid_ray_cast, mw_engine_gridray.hip; the rule, the half-rays, the key and every walk: mw_gridray.h).
// Two launch forms that produce the same bits — the result is the least (s, index) over a ray's candidates, whoever looks at which —,
// chosen from the ray count alone (mwpolicy::gridray_launch).
//
// mw_gridray_bits_kernel, a half-ray per lane (many rays per env: a predicted scan): one workgroup of MW_GRIDRAY_THREADS lanes per env,
//   a masked-off env's leaves before any barrier.  Dynamic LDS: a 64-bit key per pair of lanes, then the env's opaque row as a bit per
//   cell, staged by mwsight::stage_bits (4 KiB at MW_NAV_MAX_CELLS: one word answers 32 probes).  Then rounds of 128 rays: lane 2k takes
//   the x lines of ray k of the round, lane 2k + 1 its z lines; both make the ray and its beam (the loads coalesce), both store the empty
//   key — the same value into the pair's own word, which no other pair touches —, lane 2k probes the start cell, and each walks its
//   lines: next L, one division, the cell, one bit probe.  A hit lowers the pair's key with an LDS atomic min; every step polls the key
//   and the lane leaves once its s is above it, so the half that would run on behind the other's hit stops there.  A pair is two
//   neighbouring lanes of one wavefront: when both are through, one shuffle brings the partner's (s, index) and lane 2k stores the
//   first of the two.  No barrier inside the rounds: a pair shares its key with nobody, and a wavefront's LDS operations keep their order.
// mw_gridray_waves_kernel, a wavefront per half-ray (few rays per env: string pulling's 6, a free-path test's 1): a workgroup of 4
//   wavefronts per two rays of one env — wavefront 2q the x lines of its ray, 2q + 1 the z lines —, nothing staged: the lanes take 64
//   consecutive lines at a time and probe the bytes in global memory, one ballot per 64 lines finds whether any is opaque and the first
//   such lane lowers the ray's key (static LDS).  The wavefront leaves once the s of its next first line is above the key.  A butterfly
//   leaves the wavefront's first (s, index) in lane 0, which puts it into LDS; behind one barrier the x wavefront's lane 0 stores the
//   first of the two.  A masked-off env's workgroups leave before the barrier; a spare pair of wavefronts (an odd R) goes through it idle.
// Indices: a ray index k is below R, so origin is read below N * R * 3, dir below N * R * 2, offsets below R, heading at env; t, hit and
// dir_out are written at env * R + k.  A cell index comes out of mwscan::inside, 0 .. cells - 1: its bit lies below bits_bytes(cells), its
// byte inside the env's own row of a tensor the caller sized [N][gz][gx].  A key index is lane >> 1 < MW_GRIDRAY_PAIRS, or the ray of the
// workgroup, 0 or 1.  A line index j is below the half's n <= max(gx, gz) + 1.
#include "mw_kernels.h"

namespace {

struct LdsKey {
    uint64_t *p;
    __device__ uint64_t load() const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    // ... as one value for the whole wavefront (its first lane's): what a wavefront decides on together
    __device__ uint64_t load_uniform() const
    {
        const uint64_t v = load();
        return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    }
    __device__ void reset() const { __hip_atomic_store(p, mwgray::kNoKey, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ void lower(uint64_t s) const { atomicMin(reinterpret_cast<unsigned long long *>(p), (unsigned long long)s); }
};

__device__ inline mwgray::Best shuffled(const mwgray::Best &b, int mask)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)b.s, mask), hi = (uint32_t)__shfl_xor((int)(uint32_t)(b.s >> 32), mask);
    return {((uint64_t)hi << 32) | lo, __shfl_xor(b.cell, mask)};
}

// a ray's row of the results: the answer, and the direction used where the caller asked for it
__device__ inline void store(const mwray::Hit &h, const mwray::Ray &r, size_t row, double *t_out, int32_t *hit_out, double *dir_out)
{
    t_out[row] = h.t;
    if (hit_out) hit_out[row] = h.code;
    if (dir_out) { dir_out[row * 2] = r.dx; dir_out[row * 2 + 1] = r.dz; }
}

}  // namespace

extern "C" __global__ __launch_bounds__(MW_GRIDRAY_THREADS) void mw_gridray_bits_kernel(MwRayArgs a, mw_nav_params p, double max_t, int R,
                                                                                        const uint8_t *__restrict__ mask, const uint8_t *__restrict__ opaque,
                                                                                        const double *__restrict__ origin, const double *__restrict__ dir,
                                                                                        const double *__restrict__ offsets, const double *__restrict__ heading,
                                                                                        double *__restrict__ t_out, int32_t *__restrict__ hit_out,
                                                                                        double *__restrict__ dir_out)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t gridray_lds[];
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x, pair = lane >> 1;
    const bool xhalf = (lane & 1) == 0;
    if (mask && !mask[env]) return;
    if (heading) a.adir = heading;
    const mwnav::Grid g = mwnav::grid_of(a.w, p, env);
    const mw_ray_params fan = mwgray::fan_of(R, max_t);
    const bool covered = mwnav::covers(g);
    if (!covered && lane == 0) atomicOr(a.w.status, MW_ST_DEPTH_BAD);
    const int n = g.gx * g.gz;
    uint64_t *keys = gridray_lds;
    uint32_t *bits = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(gridray_lds) + mwgray::key_bytes());
    if (covered) {          // (the env's, so the workgroup's: every lane meets the barriers or none)
        mwsight::zero_bits(bits, n, lane, MW_GRIDRAY_THREADS);
        __syncthreads();
        mwsight::stage_bits(opaque + env * (size_t)n, bits, n, lane, MW_GRIDRAY_THREADS, [](uint32_t *word, uint32_t bit) { atomicOr(word, bit); });
        __syncthreads();
    }
    const LdsKey key{keys + pair};
    const auto probe = [bits](int c) { return mwsight::opaque_at(bits, c); };
    for (int k0 = 0; k0 < R; k0 += MW_GRIDRAY_PAIRS) {
        const int k = k0 + pair < R ? k0 + pair : R - 1;        // (a spare pair of the last round repeats the last ray and stores nothing)
        const bool mine = k0 + pair < R;
        const mwray::Ray r = mwray::ray_of(a, fan, env, k, origin, dir, offsets);
        mwscan::Beam b = mwgray::beam_of(g, r, max_t);
        b.keep = b.keep && covered && mine;
        mwgray::Best best{mwgray::kNoKey, 0};
        key.reset();
        __builtin_amdgcn_wave_barrier();
        if (b.keep) {
            if (xhalf) mwgray::look_start(b, g.gx, g.gz, probe, key, best);
            mwgray::walk_lines(mwgray::half_of(b, xhalf), g.gx, g.gz, probe, key, best);
        }
        best = mwgray::first(best, shuffled(best, 1));
        if (mine && xhalf) store(mwgray::hit_of(best, max_t), r, env * (size_t)R + (size_t)k, t_out, hit_out, dir_out);
    }
}

extern "C" __global__ __launch_bounds__(MW_GRIDRAY_THREADS) void mw_gridray_waves_kernel(MwRayArgs a, mw_nav_params p, double max_t, int R,
                                                                                         const uint8_t *__restrict__ mask, const uint8_t *__restrict__ opaque,
                                                                                         const double *__restrict__ origin, const double *__restrict__ dir,
                                                                                         const double *__restrict__ offsets, const double *__restrict__ heading,
                                                                                         double *__restrict__ t_out, int32_t *__restrict__ hit_out,
                                                                                         double *__restrict__ dir_out)
{
    __shared__ uint64_t keys[2];
    __shared__ mwgray::Best found[4];
    const int per_env = (R + 1) / 2;                                    // workgroups per env
    const size_t env = blockIdx.x / (unsigned)per_env;
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63), q = wave >> 1;
    const bool xhalf = (wave & 1) == 0;
    if (mask && !mask[env]) return;
    if (heading) a.adir = heading;
    const int k_ = (int)(blockIdx.x % (unsigned)per_env) * 2 + q;
    const bool mine = k_ < R;
    const int k = mine ? k_ : R - 1;
    const mwnav::Grid g = mwnav::grid_of(a.w, p, env);
    const bool covered = mwnav::covers(g);
    if (!covered && threadIdx.x == 0) atomicOr(a.w.status, MW_ST_DEPTH_BAD);
    const mwray::Ray r = mwray::ray_of(a, mwgray::fan_of(R, max_t), env, k, origin, dir, offsets);
    mwscan::Beam b = mwgray::beam_of(g, r, max_t);
    b.keep = b.keep && covered && mine;
    const uint8_t *row = opaque + env * (size_t)(g.gx * g.gz);
    const auto probe = [row](int c) { return row[c] != 0; };
    const LdsKey key{keys + q};
    mwgray::Best best{mwgray::kNoKey, 0};
    if (lane == 0 && xhalf) key.reset();
    __syncthreads();
    if (b.keep) {       // (the wavefront's: b is made of the wavefront's ray)
        if (xhalf && lane == 0) mwgray::look_start(b, g.gx, g.gz, probe, key, best);
        const mwgray::Half h = mwgray::half_of(b, xhalf);
        for (int base = 0; base < h.n && mwgray::wave_goes_on(h, base, key.load_uniform()); base += 64) {
            const mwgray::Best m = mwgray::look_line(h, base + lane, g.gx, g.gz, probe);
            const unsigned long long any = __ballot(m.s != mwgray::kNoKey);
            if (!any) continue;
            mwgray::take(best, m.s, m.cell);
            if (lane == __ffsll(any) - 1) key.lower(m.s);
        }
    }
    for (int m = 32; m >= 1; m >>= 1) best = mwgray::first(best, shuffled(best, m));
    if (lane == 0) found[wave] = best;
    __syncthreads();
    if (mine && xhalf && lane == 0)
        store(mwgray::hit_of(mwgray::first(found[wave], found[wave + 1]), max_t), r, env * (size_t)R + (size_t)k, t_out, hit_out, dir_out);
}
