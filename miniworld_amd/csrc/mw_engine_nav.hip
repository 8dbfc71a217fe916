// mwengine host runtime: navigation fields (mw_nav_build, mw_nav_build_grid, mw_nav_query; kernels: mw_nav.hip, mw_nav_grid.hip,
// arithmetic: mw_nav.h, mw_nav_grid.h).
//
// None of the calls waits for the Maze's side-stream refills: mw_engine.h, at world_view().
#include "mw_engine.h"

using namespace mwhost;

namespace {

int nav_args(mw_engine *e, const char *what, const mw_nav_params *p, const double *d_target, const void *d_field)
{
    if (!p || !d_field) return fail(e, MW_E_INVALID, "%s: %s is null", what, p ? "d_field" : "params");
    if (const int rc = grid_check(e, what, p, " (the grid lives in LDS)")) return rc;
    if (!(p->margin >= 0.0)) return fail(e, MW_E_INVALID, "%s: margin %g < 0", what, p->margin);
    if (p->target_slot < 0 || p->target_slot >= e->cfg.max_ents) return fail(e, MW_E_INVALID, "%s: target slot %d outside 0 .. %d", what, (int)p->target_slot, e->cfg.max_ents - 1);
    if (d_target && !(p->reach > 0.0)) return fail(e, MW_E_INVALID, "%s: reach %g <= 0 with point targets", what, p->reach);
    return MW_OK;
}

}  // namespace

extern "C" {

int mw_nav_build(mw_engine *e, const mw_nav_params *params, const uint8_t *d_mask, const double *d_target, uint16_t *d_field, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (const int rc = nav_args(e, "mw_nav_build", params, d_target, d_field)) return rc;
    const int lds = (int)((size_t)params->gx * params->gz * sizeof(uint16_t) + 15) / 16 * 16;
    return launch_query(e, "mw_nav_build", mw_nav_build_kernel, world_view, e->cfg.num_envs, MW_NAV_THREADS, lds, &e->nav_lds_set, stream, *params, d_mask, d_target,
                        d_field, e->nav_passes);
}

int mw_nav_build_grid(mw_engine *e, const mw_nav_params *params, const uint8_t *d_mask, const uint8_t *d_blocked, const uint8_t *d_sources,
                      const double *d_target, const uint8_t *d_extra, uint16_t *d_field, void *stream)
{
    const char *what = "mw_nav_build_grid";
    if (!e) return MW_E_INVALID;
    if (!params || !d_blocked || !d_field) return fail(e, MW_E_INVALID, "%s: %s is null", what, !params ? "params" : !d_blocked ? "d_blocked" : "d_field");
    if (const int rc = grid_check(e, what, params, " (the grid lives in LDS)")) return rc;
    if (const int rc = nonnegative_check(e, what, "margin (the inflation radius)", params->margin)) return rc;
    if (params->flags & MW_NAV_ENTITIES) return fail(e, MW_E_INVALID, "%s: MW_NAV_ENTITIES: this call reads no entities, the caller rasterises what it knows", what);
    if (!d_sources && !d_target) return fail(e, MW_E_INVALID, "%s: neither d_sources nor d_target", what);
    if (d_target && !(params->reach > 0.0)) return fail(e, MW_E_INVALID, "%s: reach %g <= 0 with point targets", what, params->reach);
    const int R = mwnav::inflate_radius(params->cell, params->margin);
    if (R < 0)
        return fail(e, MW_E_INVALID, "%s: an inflation of %g m is more than %d cells of %g m", what, params->margin, MW_NAV_MAX_INFLATE, params->cell);
    const mwpolicy::Launch l = mwpolicy::nav_grid_launch(e->cfg.num_envs, (long long)params->gx * params->gz, d_extra != nullptr);
    return launch_query(e, what, mw_nav_grid_kernel, world_view, l.grid, l.threads, l.lds, &e->nav_grid_lds_set, stream, *params, R, d_mask, d_blocked, d_sources,
                        d_target, d_extra, d_field, e->nav_passes);
}

int mw_nav_query(mw_engine *e, const mw_nav_params *params, const double *d_target, const uint16_t *d_field, const double *d_pos, int32_t *d_cost,
                 int32_t *d_next, double *d_waypoint, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (const int rc = nav_args(e, "mw_nav_query", params, d_target, d_field)) return rc;
    const int N = e->cfg.num_envs;
    return launch_query(e, "mw_nav_query", mw_nav_query_kernel, world_view, (N + MW_NAV_QUERY_THREADS - 1) / MW_NAV_QUERY_THREADS, MW_NAV_QUERY_THREADS, 0, nullptr, stream,
                        *params, d_target, d_field, d_pos, d_cost, d_next, d_waypoint);
}

int mw_debug_set_nav_passes(mw_engine *e, int32_t *d_passes)
{
    if (!e) return MW_E_INVALID;
    e->nav_passes = d_passes;
    return MW_OK;
}

}  // extern "C"
