// mwengine host runtime: ray casts (mw_ray_cast; kernels: mw_ray.hip, arithmetic: mw_ray.h, launch form: mw_policy.h).
//
// The call does not wait for the Maze's side-stream refills: mw_engine.h, at world_view().
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
    if (const int rc = positive_check(e, what, "max_t", params->max_t)) return rc;
    if (const int rc = nonnegative_check(e, what, "radius", params->radius)) return rc;
    if (params->flags & ~MW_RAY_ENTITIES) return fail(e, MW_E_INVALID, "%s: unknown flags 0x%x", what, (unsigned)params->flags);
    if ((d_dir != nullptr) == (d_offsets != nullptr)) return fail(e, MW_E_INVALID, "%s: exactly one of d_dir and d_offsets is given, not %s", what, d_dir ? "both" : "neither");
    const MwArgs &a = e->args;
    const mwpolicy::RayLaunch l = mwpolicy::ray_launch(a.N, params->rays, a.max_segs, a.E, e->ray_form);
    if (!l.fits) return fail(e, MW_E_INVALID, "%s: %d segments and %d slots need %zu bytes of LDS > 64 KiB", what, a.max_segs, a.E, l.lds);
    if (l.per_lane)
        return launch_query(e, what, mw_ray_lanes_kernel, ray_view, l.grid, l.threads, l.lds, &e->ray_lds_set, stream, *params, d_mask, d_origin, d_dir, d_offsets, d_t,
                            d_hit, d_dir_out);
    return launch_query(e, what, mw_ray_waves_kernel, ray_view, l.grid, l.threads, 0, nullptr, stream, *params, d_mask, d_origin, d_dir, d_offsets, d_t, d_hit, d_dir_out);
}

int mw_debug_set_ray_form(mw_engine *e, int form)
{
    if (!e) return MW_E_INVALID;
    if (form < 0 || form > 2) return fail(e, MW_E_INVALID, "mw_debug_set_ray_form: form %d outside 0 .. 2", form);
    e->ray_form = form;
    return MW_OK;
}

}  // extern "C"
