// mwengine host runtime: grid rollouts (mw_grid_plan; kernel: mw_gridplan.hip, rule, bit plane and the plan's loop: mw_gridplan.h, launch:
// mw_policy.h).
//
// The call does not wait for the Maze's side-stream refills: mw_engine.h, at world_view().  (Of the world it reads each env's extent
// and, without d_pose, the agent's pose; the step sizes are the config's, host values that no kernel writes.)
#include "mw_engine.h"
#include "mw_policy.h"

using namespace mwhost;

extern "C" {

int mw_grid_plan(mw_engine *e, const mw_nav_params *grid, const double *host_radius, int32_t flags, int32_t T, int32_t P, int32_t stop_at, const uint8_t *d_mask,
                 const uint8_t *d_opaque, const void *d_plans, const double *d_pose, const double *d_step, const uint16_t *d_field, const uint8_t *d_extra,
                 double *d_pose_out, int32_t *d_stats, double *d_trace, void *stream)
{
    const char *what = "mw_grid_plan";
    if (!e) return MW_E_INVALID;
    if (!grid || !host_radius || !d_opaque || !d_plans || !d_pose_out || !d_stats)
        return fail(e, MW_E_INVALID, "%s: %s is null", what,
                    !grid ? "grid" : !host_radius ? "host_radius" : !d_opaque ? "d_opaque" : !d_plans ? "d_plans" : !d_pose_out ? "d_pose_out" : "d_stats");
    const double radius = host_radius[0];
    if (const int rc = grid_check(e, what, grid)) return rc;
    if (!std::isfinite(grid->cell)) return fail(e, MW_E_INVALID, "%s: cell %g is not finite", what, grid->cell);
    if (T < 1 || T > MW_MAX_PLAN) return fail(e, MW_E_INVALID, "%s: horizon %d outside 1 .. %d", what, (int)T, MW_MAX_PLAN);
    if (P < 1 || P > MW_GPLAN_MAX_PLANS) return fail(e, MW_E_INVALID, "%s: %d plans per env outside 1 .. %d", what, (int)P, MW_GPLAN_MAX_PLANS);
    if (const int rc = nonnegative_check(e, what, "radius", radius)) return rc;
    if (radius > MW_GPLAN_MAX_RADIUS * grid->cell)
        return fail(e, MW_E_INVALID, "%s: radius %g is more than %d cells of %g", what, radius, MW_GPLAN_MAX_RADIUS, grid->cell);
    if (flags & ~(MW_GPLAN_OUTSIDE_BLOCKS | MW_GPLAN_BYTE_PLANS)) return fail(e, MW_E_INVALID, "%s: unknown flags 0x%x", what, (unsigned)flags);
    if (stop_at < -1 || stop_at > 0xFFFF) return fail(e, MW_E_INVALID, "%s: stop_at %d outside -1 .. 65535", what, (int)stop_at);
    if (stop_at >= 0 && !d_field) return fail(e, MW_E_INVALID, "%s: stop_at %d without d_field: there is nothing to reach", what, (int)stop_at);
    const mwpolicy::Launch l = mwpolicy::gridplan_launch(e->cfg.num_envs, grid->gx, grid->gz, P);
    if (!l.fits) return fail(e, MW_E_INVALID, "%s: %d x %d cells and %d plans do not fit", what, (int)grid->gx, (int)grid->gz, (int)P);
    const mwgplan::Call q{radius, e->args.fwd.def, e->args.drift.def, e->args.turn.def, flags, T, P, stop_at};
    return launch_query(e, what, mw_gridplan_kernel, ray_view, l.grid, l.threads, l.lds, nullptr, stream, *grid, q, d_mask, d_opaque, d_plans, d_pose, d_step, d_field,
                        d_extra, d_pose_out, d_stats, d_trace);
}

}  // extern "C"
