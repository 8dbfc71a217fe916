// mwengine host runtime: grid regions (mw_grid_regions; kernel: mw_regions.hip, rule, arrays and phases: mw_regions.h, launch: mw_policy.h).
//
// The call does not wait for the Maze's side-stream refills: mw_engine.h, at world_view().  (It reads nothing of the world at all: the
// view is the launcher's first argument and the kernel leaves it alone.)
#include "mw_engine.h"
#include "mw_policy.h"

using namespace mwhost;

extern "C" {

int mw_grid_regions(mw_engine *e, const mw_nav_params *grid, int32_t connectivity, int32_t min_cells, int32_t max_regions, const uint8_t *d_mask,
                    const uint8_t *d_member, int32_t *d_count, int32_t *d_size, int32_t *d_cell, int32_t *d_sum, int16_t *d_label, void *stream)
{
    const char *what = "mw_grid_regions";
    if (!e) return MW_E_INVALID;
    if (!grid || !d_member || !d_count || !d_size || !d_cell)
        return fail(e, MW_E_INVALID, "%s: %s is null", what, !grid ? "grid" : !d_member ? "d_member" : !d_count ? "d_count" : !d_size ? "d_size" : "d_cell");
    if (const int rc = grid_check(e, what, grid)) return rc;
    if (connectivity != 4 && connectivity != 8) return fail(e, MW_E_INVALID, "%s: connectivity %d is neither 4 nor 8", what, (int)connectivity);
    if (min_cells < 1) return fail(e, MW_E_INVALID, "%s: min_cells %d < 1", what, (int)min_cells);
    if (max_regions < 1 || max_regions > MW_REGION_MAX) return fail(e, MW_E_INVALID, "%s: %d regions outside 1 .. %d", what, (int)max_regions, MW_REGION_MAX);
    const mwpolicy::Launch l = mwpolicy::regions_launch(e->cfg.num_envs, (long long)grid->gx * grid->gz, max_regions);
    if (!l.fits) return fail(e, MW_E_INVALID, "%s: %d x %d cells and %d regions do not fit", what, (int)grid->gx, (int)grid->gz, (int)max_regions);
    return launch_query(e, what, mw_regions_kernel, world_view, l.grid, l.threads, l.lds, &e->regions_lds_set, stream, (int)grid->gx, (int)grid->gz,
                        connectivity == 8 ? 1 : 0, (int)min_cells, (int)max_regions, d_mask, d_member, d_count, d_size, d_cell, d_sum, d_label);
}

}  // extern "C"
