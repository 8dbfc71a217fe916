// mwengine host runtime: grid ray casts (mw_grid_ray_cast; kernels: mw_gridray.hip, rule, half-rays and walks: mw_gridray.h, launch
// form: mw_policy.h).
//
// The call does not wait for the Maze's side-stream refills: mw_engine.h, at world_view().  (Of the world it reads each env's extent
// and, in fan mode or without d_origin, the agent's pose.)
#include "mw_engine.h"
#include "mw_policy.h"

using namespace mwhost;

extern "C" {

int mw_grid_ray_cast(mw_engine *e, const mw_nav_params *grid, const double *host_range, int32_t R, const uint8_t *d_mask, const uint8_t *d_opaque,
                     const double *d_origin, const double *d_dir, const double *d_offsets, const double *d_heading, double *d_t, int32_t *d_hit, double *d_dir_out,
                     void *stream)
{
    const char *what = "mw_grid_ray_cast";
    if (!e) return MW_E_INVALID;
    if (!grid || !host_range || !d_opaque || !d_t)
        return fail(e, MW_E_INVALID, "%s: %s is null", what, !grid ? "grid" : !host_range ? "host_range" : !d_opaque ? "d_opaque" : "d_t");
    const double max_t = host_range[0];
    if (const int rc = grid_check(e, what, grid)) return rc;
    if (!std::isfinite(grid->cell)) return fail(e, MW_E_INVALID, "%s: cell %g is not finite", what, grid->cell);
    if (R < 1 || R > MW_RAY_MAX) return fail(e, MW_E_INVALID, "%s: %d rays per env outside 1 .. %d", what, (int)R, MW_RAY_MAX);
    if (const int rc = positive_check(e, what, "max_t", max_t)) return rc;
    if ((d_dir != nullptr) == (d_offsets != nullptr)) return fail(e, MW_E_INVALID, "%s: exactly one of d_dir and d_offsets is given, not %s", what, d_dir ? "both" : "neither");
    if (d_heading && d_dir) return fail(e, MW_E_INVALID, "%s: d_heading with d_dir: a heading turns the fan of d_offsets", what);
    const mwpolicy::GridRayLaunch l = mwpolicy::gridray_launch(e->cfg.num_envs, (long long)grid->gx * grid->gz, R, e->ray_form);
    if (!l.fits) return fail(e, MW_E_INVALID, "%s: %d x %d cells and %d rays do not fit", what, (int)grid->gx, (int)grid->gz, (int)R);
    if (l.staged)
        return launch_query(e, what, mw_gridray_bits_kernel, ray_view, l.grid, l.threads, l.lds, nullptr, stream, *grid, max_t, (int)R, d_mask, d_opaque, d_origin, d_dir,
                            d_offsets, d_heading, d_t, d_hit, d_dir_out);
    return launch_query(e, what, mw_gridray_waves_kernel, ray_view, l.grid, l.threads, 0, nullptr, stream, *grid, max_t, (int)R, d_mask, d_opaque, d_origin, d_dir, d_offsets,
                        d_heading, d_t, d_hit, d_dir_out);
}

}  // extern "C"
