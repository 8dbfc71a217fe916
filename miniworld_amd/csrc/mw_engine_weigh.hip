// mwengine host runtime: scan weighing and resampling (mw_scan_weigh, mw_resample; kernels: mw_weigh.hip, rules, arrays and phases:
// mw_weigh.h, launches: mw_policy.h).
//
// mw_scan_weigh does not wait for the Maze's side-stream refills, and neither does mw_resample: mw_engine.h, at world_view().  (Of the
// world mw_scan_weigh reads each env's extent; mw_resample reads nothing of it.)
#include "mw_engine.h"
#include "mw_policy.h"

using namespace mwhost;

extern "C" {

int mw_scan_weigh(mw_engine *e, const mw_nav_params *grid, const double *host_range, int32_t R, int32_t P, const uint8_t *d_score, const double *d_t,
                  const double *d_dir, const double *d_pose, const uint8_t *d_mask, int32_t *d_out, int32_t *d_inside, int32_t *d_best, void *stream)
{
    const char *what = "mw_scan_weigh";
    if (!e) return MW_E_INVALID;
    if (!grid || !host_range || !d_score || !d_t || !d_dir || !d_pose || !d_out)
        return fail(e, MW_E_INVALID, "%s: %s is null", what, !grid ? "grid" : !host_range ? "host_range" : !d_score ? "d_score" : !d_t ? "d_t" : !d_dir ? "d_dir"
                                                              : !d_pose ? "d_pose" : "d_out");
    const double max_range = host_range[0];
    if (const int rc = grid_check(e, what, grid)) return rc;
    if (!std::isfinite(grid->cell)) return fail(e, MW_E_INVALID, "%s: cell %g is not finite", what, grid->cell);
    if (R < 1 || R > MW_RAY_MAX) return fail(e, MW_E_INVALID, "%s: %d beams per env outside 1 .. %d", what, (int)R, MW_RAY_MAX);
    if (P < 1 || P > MW_WEIGH_MAX_PARTICLES) return fail(e, MW_E_INVALID, "%s: %d particles per env outside 1 .. %d", what, (int)P, MW_WEIGH_MAX_PARTICLES);
    if (const int rc = positive_check(e, what, "max_range", max_range)) return rc;
    const mwpolicy::WeighLaunch l = mwpolicy::weigh_launch(e->cfg.num_envs, (long long)grid->gx * grid->gz, R, P, e->weigh_form);
    if (!l.fits) return fail(e, MW_E_INVALID, "%s: %d x %d cells, %d beams and %d particles do not fit", what, (int)grid->gx, (int)grid->gz, (int)R, (int)P);
    return launch_query(e, what, mw_weigh_kernel, world_view, l.grid, l.threads, l.lds, &e->weigh_lds_set, stream, *grid, max_range, (int)R, (int)P, l.waves ? 1 : 0, d_score,
                        d_t, d_dir, d_pose, d_mask, d_out, d_inside, d_best);
}

int mw_debug_set_weigh_form(mw_engine *e, int form)
{
    if (!e) return MW_E_INVALID;
    if (form < 0 || form > 2) return fail(e, MW_E_INVALID, "mw_debug_set_weigh_form: form %d outside 0 .. 2", form);
    e->weigh_form = form;
    return MW_OK;
}

int mw_resample(mw_engine *e, int32_t P, const uint32_t *d_weight, const uint64_t *d_offset, const uint8_t *d_mask, int32_t *d_ancestor, const double *d_pose,
                double *d_pose_out, void *stream)
{
    const char *what = "mw_resample";
    if (!e) return MW_E_INVALID;
    if (!d_weight || !d_offset || !d_ancestor)
        return fail(e, MW_E_INVALID, "%s: %s is null", what, !d_weight ? "d_weight" : !d_offset ? "d_offset" : "d_ancestor");
    if (P < 1 || P > MW_WEIGH_MAX_PARTICLES) return fail(e, MW_E_INVALID, "%s: %d particles per env outside 1 .. %d", what, (int)P, MW_WEIGH_MAX_PARTICLES);
    if ((d_pose != nullptr) != (d_pose_out != nullptr)) return fail(e, MW_E_INVALID, "%s: d_pose and d_pose_out go together, not %s alone", what, d_pose ? "d_pose" : "d_pose_out");
    const mwpolicy::Launch l = mwpolicy::resample_launch(e->cfg.num_envs, P);
    return launch_query(e, what, mw_resample_kernel, world_view, l.grid, l.threads, l.lds, nullptr, stream, (int)P, d_weight, d_offset, d_mask, d_ancestor, d_pose, d_pose_out);
}

}  // extern "C"
