// mwengine host runtime: grid sight (mw_grid_sight; kernel: mw_sight.hip, rule, walk and phases: mw_sight.h, launch: mw_policy.h).
//
// The call does not wait for the Maze's side-stream refills: mw_engine.h, at world_view().  (With d_cells it reads nothing of the world.)
#include "mw_engine.h"
#include "mw_policy.h"

using namespace mwhost;

extern "C" {

int mw_grid_sight(mw_engine *e, const mw_nav_params *grid, const double *host_sight, int32_t views, const uint8_t *d_mask, const uint8_t *d_opaque,
                  const uint8_t *d_weight, const int32_t *d_cells, const double *d_dirs, int32_t *d_gain, uint8_t *d_seen, void *stream)
{
    const char *what = "mw_grid_sight";
    if (!e) return MW_E_INVALID;
    if (!grid || !host_sight || !d_opaque || !d_gain)
        return fail(e, MW_E_INVALID, "%s: %s is null", what, !grid ? "grid" : !host_sight ? "host_sight" : !d_opaque ? "d_opaque" : "d_gain");
    if (const int rc = grid_check(e, what, grid)) return rc;
    const mwseen::Sight s{host_sight[0], host_sight[1], 0};
    if (const int rc = positive_check(e, what, "range", s.range)) return rc;
    if (!(s.cos_half >= -1.0 && s.cos_half <= 1.0)) return fail(e, MW_E_INVALID, "%s: cos_half %g outside -1 .. 1", what, s.cos_half);
    if (views < 1 || views > MW_SIGHT_MAX_VIEWS) return fail(e, MW_E_INVALID, "%s: %d viewpoints outside 1 .. %d", what, (int)views, MW_SIGHT_MAX_VIEWS);
    if (!d_cells && views != 1) return fail(e, MW_E_INVALID, "%s: %d viewpoints without d_cells: the agent is one", what, (int)views);
    if (!d_cells && d_dirs) return fail(e, MW_E_INVALID, "%s: d_dirs without d_cells: the agent's heading is its own", what);
    if (d_cells && !d_dirs && s.cos_half != -1.0) return fail(e, MW_E_INVALID, "%s: cos_half %g without d_dirs: a cone needs headings", what, s.cos_half);
    const mwpolicy::Launch l = mwpolicy::sight_launch(e->cfg.num_envs, (long long)grid->gx * grid->gz, d_weight != nullptr, views);
    if (!l.fits) return fail(e, MW_E_INVALID, "%s: %d x %d cells and %d viewpoints do not fit", what, (int)grid->gx, (int)grid->gz, (int)views);
    const int R = mwsight::reach_cells(grid->cell, s.range, grid->gx > grid->gz ? grid->gx : grid->gz);
    return launch_query(e, what, mw_sight_kernel, ray_view, l.grid, l.threads, l.lds, &e->sight_lds_set, stream, *grid, s, (int)views, R,
                        mwsight::chunks_of(R, grid->gx, grid->gz), d_mask, d_opaque, d_weight, d_cells, d_dirs, d_gain, d_seen);
}

}  // extern "C"
