// mwengine host runtime: grid clearance (mw_grid_clearance; kernel: mw_clear.hip, rule, array and phases: mw_clear.h, launch: mw_policy.h).
//
// The call does not wait for the Maze's side-stream refills: mw_engine.h, at world_view().  (It reads nothing of the world at all: the
// view is the launcher's first argument and the kernel leaves it alone.)
#include "mw_engine.h"
#include "mw_policy.h"

using namespace mwhost;

extern "C" {

int mw_grid_clearance(mw_engine *e, const mw_nav_params *grid, int32_t limit, const int32_t *host_bands, int32_t bands, const uint8_t *d_mask,
                      const uint8_t *d_marked, int32_t *d_dist2, int32_t *d_nearest, uint8_t *d_cost, void *stream)
{
    const char *what = "mw_grid_clearance";
    if (!e) return MW_E_INVALID;
    if (!grid || !d_marked || !d_dist2) return fail(e, MW_E_INVALID, "%s: %s is null", what, !grid ? "grid" : !d_marked ? "d_marked" : "d_dist2");
    if (const int rc = grid_check(e, what, grid)) return rc;
    if (limit < 0) return fail(e, MW_E_INVALID, "%s: limit %d < 0", what, (int)limit);
    if (bands < 0 || bands > MW_CLEAR_MAX_BANDS) return fail(e, MW_E_INVALID, "%s: %d bands outside 0 .. %d", what, (int)bands, MW_CLEAR_MAX_BANDS);
    if (bands > 0 && !host_bands) return fail(e, MW_E_INVALID, "%s: host_bands is null", what);
    if (const char *wrong = mwclear::bands_error(host_bands, bands)) return fail(e, MW_E_INVALID, "%s: the bands hold %s", what, wrong);
    if ((bands > 0) != (d_cost != nullptr)) return fail(e, MW_E_INVALID, "%s: %s", what, d_cost ? "d_cost without bands" : "bands without d_cost");
    const mwpolicy::Launch l = mwpolicy::clear_launch(e->cfg.num_envs, (long long)grid->gx * grid->gz);
    if (!l.fits) return fail(e, MW_E_INVALID, "%s: %d x %d cells do not fit", what, (int)grid->gx, (int)grid->gz);
    return launch_query(e, what, mw_clear_kernel, world_view, l.grid, l.threads, l.lds, &e->clear_lds_set, stream, (int)grid->gx, (int)grid->gz,
                        mwclear::bounded_limit(limit), mwclear::make_bands(host_bands, bands), d_mask, d_marked, d_dist2, d_nearest, d_cost);
}

}  // extern "C"
