// mwengine host runtime: ray casts (mw_ray_cast; kernels: mw_ray.hip, arithmetic: mw_ray.h, launch form: mw_policy.h).
//
// Like the nav calls (mw_engine_nav.hip), and for the reason given there word for word, the call does not wait for the Maze's
// side-stream refills: the refill kernel generates into the spare arrays — the spare's own segs / nsegs, extent and entity slabs among
// them — and touches the env's random stream and refill_mask beside them; the live segs, nsegs, ekind, epos, egeom, carry and agent pose
// that these kernels read are written on the caller's stream alone (K1's take-over of a spare, the resets, the state writes), behind
// which the call is ordered by being on that stream.
#include <math.h>

#include "mw_engine.h"
#include "mw_policy.h"

using namespace mwhost;

extern "C" {

int mw_ray_cast(mw_engine *e, const mw_ray_params *params, const uint8_t *d_mask, const double *d_origin, const double *d_dir, const double *d_offsets,
                double *d_t, int32_t *d_hit, double *d_dir_out, void *stream)
{
    const char *what = "mw_ray_cast";
    if (!e) return MW_E_INVALID;
    if (!params || !d_t) return fail(e, MW_E_INVALID, "%s: %s is null", what, params ? "d_t" : "params");
    if (params->rays < 1 || params->rays > MW_RAY_MAX) return fail(e, MW_E_INVALID, "%s: %d rays outside 1 .. %d", what, (int)params->rays, MW_RAY_MAX);
    if (!(params->max_t > 0.0) || !isfinite(params->max_t)) return fail(e, MW_E_INVALID, "%s: max_t %g is not a positive finite number", what, params->max_t);
    if (!(params->radius >= 0.0) || !isfinite(params->radius)) return fail(e, MW_E_INVALID, "%s: radius %g is not a finite number >= 0", what, params->radius);
    if (params->flags & ~MW_RAY_ENTITIES) return fail(e, MW_E_INVALID, "%s: unknown flags 0x%x", what, (unsigned)params->flags);
    if ((d_dir != nullptr) == (d_offsets != nullptr)) return fail(e, MW_E_INVALID, "%s: exactly one of d_dir and d_offsets is given, not %s", what, d_dir ? "both" : "neither");
    const MwArgs &a = e->args;
    const mwpolicy::RayLaunch l = mwpolicy::ray_launch(a.N, params->rays, a.max_segs, a.E, e->ray_form);
    if (!l.fits) return fail(e, MW_E_INVALID, "%s: %d segments and %d slots need %zu bytes of LDS > 64 KiB", what, a.max_segs, a.E, l.lds);
    if (mwpolicy::grid_too_large(l.grid)) return fail(e, MW_E_INVALID, "%s: %llu workgroups", what, l.grid);
    ON_DEVICE(e);
    const MwRayArgs ra{{a.segs, a.nsegs, a.extent, a.ekind, a.epos, a.egeom, a.carry, a.ax, a.az, a.status, a.N, a.E, a.max_segs, a.shared_geom, a.agent_radius,
                        a.max_forward_step},
                       a.adir};
    if (l.per_lane) {
        if ((int)l.lds > e->ray_lds_set) {
            HIP_TRY(e, hipFuncSetAttribute((const void *)mw_ray_lanes_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds));
            e->ray_lds_set = (int)l.lds;
        }
        hipLaunchKernelGGL(mw_ray_lanes_kernel, dim3((unsigned)l.grid), dim3((unsigned)l.threads), l.lds, (hipStream_t)stream, ra, *params, d_mask, d_origin, d_dir,
                           d_offsets, d_t, d_hit, d_dir_out);
    } else {
        hipLaunchKernelGGL(mw_ray_waves_kernel, dim3((unsigned)l.grid), dim3((unsigned)l.threads), 0, (hipStream_t)stream, ra, *params, d_mask, d_origin, d_dir,
                           d_offsets, d_t, d_hit, d_dir_out);
    }
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_debug_set_ray_form(mw_engine *e, int form)
{
    if (!e) return MW_E_INVALID;
    if (form < 0 || form > 2) return fail(e, MW_E_INVALID, "mw_debug_set_ray_form: form %d outside 0 .. 2", form);
    e->ray_form = form;
    return MW_OK;
}

}  // extern "C"
