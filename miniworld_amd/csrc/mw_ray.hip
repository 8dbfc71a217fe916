// Ray casts on the device (mw_ray_cast, mw_engine_ray.hip; the arithmetic and the definition of the result: mw_ray.h).  Two launch
// forms that produce the same bits — the result is the minimum of (t, code) over the obstacles, whichever lane looks at which —, chosen
// from the ray count alone (mwpolicy::ray_launch).
//
// mw_ray_lanes_kernel, a ray per lane (many rays per env: the range sensor): one workgroup per env, a masked-off env's leaves at
//   once.  The env's walls — for a swept disc with their offset vectors, one sqrt and two divisions per wall instead of per ray — and,
//   with MW_RAY_ENTITIES, its entity slots as circles are staged once in dynamic LDS (MW_RAY_WALL_BYTES per segment of max_segs,
//   MW_RAY_DISC_BYTES per slot; checked against 64 KiB before the launch).  Lane j then takes rays j, j + lanes, ... and walks the
//   obstacles in index order; every lane reads the same LDS address (a broadcast, no bank conflict).  The f64 division and
//   square-root chains dominate: two walls are kept in flight per lane.
// mw_ray_waves_kernel, an obstacle per lane (few rays per env: line of sight, string pulling): one wavefront per (env, ray),
//   MW_RAY_WAVES of them per workgroup.  Its lanes stride over the segments and the slots straight from global memory, each keeping
//   its first (t, code); a butterfly over the wavefront leaves the first of all in every lane.
// Indices: a wall index is below nsegs_of() <= max_segs, a slot below E, a row below N * R (the grid is sized from N and R; the
// last workgroup's spare wavefronts leave).
#include "mw_kernels.h"

extern "C" __global__ __launch_bounds__(MW_RAY_THREADS) void mw_ray_lanes_kernel(MwRayArgs a, mw_ray_params p, const uint8_t *__restrict__ mask,
                                                                                 const double *__restrict__ origin, const double *__restrict__ dir,
                                                                                 const double *__restrict__ offsets, double *__restrict__ t_out,
                                                                                 int32_t *__restrict__ hit_out, double *__restrict__ dir_out)
{
    extern __shared__ __attribute__((aligned(16))) double ray_lds[];
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x, lanes = (int)blockDim.x;
    if (mask && !mask[env]) return;
    mwray::Wall *walls = reinterpret_cast<mwray::Wall *>(ray_lds);
    mwray::Disc *discs = reinterpret_cast<mwray::Disc *>(walls + a.w.max_segs);
    const double *segs = mwnav::segs_of(a.w, env);
    const int ns = mwnav::nsegs_of(a.w, env), ne = mwray::ents_of(a, p);
    for (int i = lane; i < ns; i += lanes) walls[i] = mwray::wall_of(segs + (size_t)i * 4, p.radius);
    for (int s = lane; s < ne; s += lanes) discs[s] = mwray::disc_of(a, p, env, s);
    __syncthreads();
    for (int k = lane; k < p.rays; k += lanes) {
        const mwray::Ray r = mwray::ray_of(a, p, env, k, origin, dir, offsets);
        mwray::Hit h{p.max_t, -1};
        if (!mwray::bad_ray(r)) {
#pragma unroll 2
            for (int i = 0; i < ns; ++i) mwray::take(h, mwray::ray_wall(r, walls[i], p.radius), i);
            for (int s = 0; s < ne; ++s)
                if (discs[s].listed != 0.0) mwray::take(h, mwray::ray_circle(r, discs[s].x, discs[s].z, discs[s].R), MW_RAY_ENT + s);
        }
        const size_t row = env * (size_t)p.rays + (size_t)k;
        t_out[row] = h.t;
        if (hit_out) hit_out[row] = h.code;
        if (dir_out) { dir_out[row * 2] = r.dx; dir_out[row * 2 + 1] = r.dz; }
    }
}

extern "C" __global__ __launch_bounds__(MW_RAY_WAVES * 64) void mw_ray_waves_kernel(MwRayArgs a, mw_ray_params p, const uint8_t *__restrict__ mask,
                                                                                    const double *__restrict__ origin, const double *__restrict__ dir,
                                                                                    const double *__restrict__ offsets, double *__restrict__ t_out,
                                                                                    int32_t *__restrict__ hit_out, double *__restrict__ dir_out)
{
    const size_t row = (size_t)blockIdx.x * MW_RAY_WAVES + (threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63);
    if (row >= (size_t)a.w.N * (size_t)p.rays) return;
    const size_t env = row / (size_t)p.rays;
    const int k = (int)(row % (size_t)p.rays);
    if (mask && !mask[env]) return;
    const mwray::Ray r = mwray::ray_of(a, p, env, k, origin, dir, offsets);
    mwray::Hit h{p.max_t, -1};
    if (!mwray::bad_ray(r)) {
        const double *segs = mwnav::segs_of(a.w, env);
        const int ns = mwnav::nsegs_of(a.w, env), ne = mwray::ents_of(a, p);
        for (int i = lane; i < ns; i += 64) mwray::take(h, mwray::ray_wall(r, mwray::wall_of(segs + (size_t)i * 4, p.radius), p.radius), i);
        for (int s = lane; s < ne; s += 64) {
            const mwray::Disc d = mwray::disc_of(a, p, env, s);
            if (d.listed != 0.0) mwray::take(h, mwray::ray_circle(r, d.x, d.z, d.R), MW_RAY_ENT + s);
        }
    }
    // (every lane of the wavefront is here: row, the mask byte and the ray are the wavefront's)
    for (int m = 32; m >= 1; m >>= 1) {
        const mwray::Hit o{__shfl_xor(h.t, m), __shfl_xor(h.code, m)};
        if (mwray::before(o, h)) h = o;
    }
    if (lane == 0) {
        t_out[row] = h.t;
        if (hit_out) hit_out[row] = h.code;
        if (dir_out) { dir_out[row * 2] = r.dx; dir_out[row * 2 + 1] = r.dz; }
    }
}
