// mwengine host runtime: navigation fields (mw_nav_build, mw_nav_query; kernels: mw_nav.hip, arithmetic: mw_nav.h).
//
// Neither call waits for the Maze's side-stream refills: mw_engine.h, at world_view().
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
