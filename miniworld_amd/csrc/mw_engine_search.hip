// mwengine host runtime: scan search (mw_scan_search; kernel: mw_search.hip, arrays, key and phases: mw_search.h, launch: mw_policy.h).
//
// The call does not wait for the Maze's side-stream refills: mw_engine.h, at world_view().  (Of the world it reads each env's extent
// and, without d_origin, the agent's position.)
#include "mw_engine.h"
#include "mw_policy.h"

using namespace mwhost;

extern "C" {

int mw_scan_search(mw_engine *e, const mw_nav_params *grid, const double *host_range, const double *host_rot, int32_t K, int32_t window, int32_t R,
                   const uint8_t *d_score, const double *d_t, const double *d_dir, const double *d_origin, const uint8_t *d_mask, int32_t *d_best,
                   int32_t *d_best_score, int32_t *d_stats, void *stream)
{
    const char *what = "mw_scan_search";
    if (!e) return MW_E_INVALID;
    if (!grid || !host_range || !host_rot || !d_score || !d_t || !d_dir || !d_best || !d_best_score)
        return fail(e, MW_E_INVALID, "%s: %s is null", what, !grid ? "grid" : !host_range ? "host_range" : !host_rot ? "host_rot" : !d_score ? "d_score" : !d_t ? "d_t"
                                                              : !d_dir ? "d_dir" : !d_best ? "d_best" : "d_best_score");
    const double max_range = host_range[0];
    if (const int rc = grid_check(e, what, grid)) return rc;
    if (!std::isfinite(grid->cell)) return fail(e, MW_E_INVALID, "%s: cell %g is not finite", what, grid->cell);
    if (R < 1 || R > MW_RAY_MAX) return fail(e, MW_E_INVALID, "%s: %d beams per env outside 1 .. %d", what, (int)R, MW_RAY_MAX);
    if (K < 1 || K > MW_MATCH_MAX_ROT) return fail(e, MW_E_INVALID, "%s: %d rotations outside 1 .. %d", what, (int)K, MW_MATCH_MAX_ROT);
    if (window < 0 || window > MW_SEARCH_MAX_WINDOW) return fail(e, MW_E_INVALID, "%s: a window of %d cells outside 0 .. %d", what, (int)window, MW_SEARCH_MAX_WINDOW);
    MwMatchRot rot{};
    rot.n = K;
    for (int r = 0; r < K; ++r) {
        rot.cs[r][0] = host_rot[2 * r];
        rot.cs[r][1] = host_rot[2 * r + 1];
        if (!std::isfinite(rot.cs[r][0]) || !std::isfinite(rot.cs[r][1]))
            return fail(e, MW_E_INVALID, "%s: rotation %d (%g, %g) is not finite", what, r, rot.cs[r][0], rot.cs[r][1]);
    }
    if (const int rc = positive_check(e, what, "max_range", max_range)) return rc;
    const mwpolicy::SearchLaunch l = mwpolicy::search_launch(e->cfg.num_envs, grid->gz, grid->gx, R, window);
    if (!l.fits) return fail(e, MW_E_INVALID, "%s: %d x %d cells, %d beams and a window of %d do not fit", what, (int)grid->gx, (int)grid->gz, (int)R, (int)window);
    return launch_query(e, what, mw_search_kernel, world_view, l.grid, l.threads, l.lds, &e->search_lds_set, stream, *grid, max_range, (int)R, rot, (int)window, l.batch,
                        e->search_prune, d_score, d_t, d_dir, d_origin, d_mask, d_best, d_best_score, d_stats);
}

int mw_debug_set_search_prune(mw_engine *e, int on)
{
    if (!e) return MW_E_INVALID;
    if (on < 0 || on > 1) return fail(e, MW_E_INVALID, "mw_debug_set_search_prune: %d outside 0 .. 1", on);
    e->search_prune = on;
    return MW_OK;
}

}  // extern "C"
