// mwengine host runtime: scan evidence (mw_scan_evidence; kernel: mw_evidence.hip, rule, arrays and phases: mw_evidence.h, launch:
// mw_policy.h).
//
// The call does not wait for the Maze's side-stream refills: mw_engine.h, at world_view().  (Of the world it reads each env's extent
// and, without d_origin, the agent's position.)
#include "mw_engine.h"
#include "mw_policy.h"

using namespace mwhost;

extern "C" {

int mw_scan_evidence(mw_engine *e, const mw_nav_params *grid, const double *host_range, int32_t R, const double *d_t, const double *d_dir, const double *d_origin,
                     const uint8_t *d_mask, const uint8_t *d_clear, int32_t hit, int32_t miss, int32_t cap, int32_t lo, int32_t hi, int32_t free_at, int32_t occ_at,
                     int8_t *d_ev, uint8_t *d_map, uint8_t *d_score, int32_t *d_count, int32_t *d_changed, void *stream)
{
    const char *what = "mw_scan_evidence";
    if (!e) return MW_E_INVALID;
    if (!grid || !host_range || !d_t || !d_dir || !d_ev || !d_count)
        return fail(e, MW_E_INVALID, "%s: %s is null", what, !grid ? "grid" : !host_range ? "host_range" : !d_t ? "d_t" : !d_dir ? "d_dir" : !d_ev ? "d_ev" : "d_count");
    const double max_range = host_range[0];
    if (const int rc = grid_check(e, what, grid)) return rc;
    if (!std::isfinite(grid->cell)) return fail(e, MW_E_INVALID, "%s: cell %g is not finite", what, grid->cell);
    if (R < 1 || R > MW_RAY_MAX) return fail(e, MW_E_INVALID, "%s: %d beams per env outside 1 .. %d", what, (int)R, MW_RAY_MAX);
    if (const int rc = positive_check(e, what, "max_range", max_range)) return rc;
    const mwevid::Rule rule{hit, miss, cap, lo, hi, free_at, occ_at};
    if (const char *name = mwevid::out_of_range(rule))
        return fail(e, MW_E_INVALID, "%s: %s outside its range (hit %d, miss %d in 0 .. 127; cap %d in 1 .. %d; lo %d in -127 .. -1; hi %d in 1 .. 127; free_at %d in lo .. -1; "
                    "occ_at %d in 1 .. hi)", what, name, (int)hit, (int)miss, (int)cap, MW_RAY_MAX, (int)lo, (int)hi, (int)free_at, (int)occ_at);
    const mwpolicy::Launch l = mwpolicy::evidence_launch(e->cfg.num_envs, (long long)grid->gx * grid->gz, R);
    if (!l.fits) return fail(e, MW_E_INVALID, "%s: %d x %d cells and %d beams do not fit", what, (int)grid->gx, (int)grid->gz, (int)R);
    return launch_query(e, what, mw_evidence_kernel, world_view, l.grid, l.threads, l.lds, &e->evidence_lds_set, stream, *grid, max_range, (int)R, rule, d_t, d_dir,
                        d_origin, d_mask, d_clear, d_ev, d_map, d_score, d_count, d_changed);
}

}  // extern "C"
