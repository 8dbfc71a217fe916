// mwengine host runtime: explored-area maps (mw_seen_update; kernel: mw_seen.hip, tests and phases: mw_seen.h, launch: mw_policy.h).
//
// The call does not wait for the Maze's side-stream refills: mw_engine.h, at world_view().
#include "mw_engine.h"
#include "mw_policy.h"

using namespace mwhost;

extern "C" {

int mw_seen_update(mw_engine *e, const mw_nav_params *grid, const double *host_sight, int32_t flags, const uint8_t *d_mask, const uint8_t *d_clear,
                   uint8_t *d_seen, int32_t *d_count, int32_t *d_new, void *stream)
{
    const char *what = "mw_seen_update";
    if (!e) return MW_E_INVALID;
    if (!grid || !host_sight || !d_seen || !d_count)
        return fail(e, MW_E_INVALID, "%s: %s is null", what, !grid ? "grid" : !host_sight ? "host_sight" : !d_seen ? "d_seen" : "d_count");
    if (const int rc = grid_check(e, what, grid)) return rc;      // (every seen grid is a valid nav grid)
    const mwseen::Sight s{host_sight[0], host_sight[1], flags};
    if (const int rc = positive_check(e, what, "range", s.range)) return rc;
    if (!(s.cos_half >= -1.0 && s.cos_half <= 1.0)) return fail(e, MW_E_INVALID, "%s: cos_half %g outside -1 .. 1", what, s.cos_half);
    if (flags & ~MW_SEEN_ENTITIES) return fail(e, MW_E_INVALID, "%s: unknown flags 0x%x", what, (unsigned)flags);
    const MwArgs &a = e->args;
    const mwpolicy::Launch l = mwpolicy::seen_launch(a.N, a.max_segs, a.E);
    if (!l.fits) return fail(e, MW_E_INVALID, "%s: %d segments and %d slots need %zu bytes of LDS > 64 KiB", what, a.max_segs, a.E, l.lds);
    return launch_query(e, what, mw_seen_kernel, ray_view, l.grid, l.threads, l.lds, &e->seen_lds_set, stream, *grid, s, d_mask, d_clear, d_seen, d_count, d_new);
}

}  // extern "C"
