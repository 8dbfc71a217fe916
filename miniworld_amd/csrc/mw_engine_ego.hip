// mwengine host runtime: egocentric map windows (mw_ego_map; kernel: mw_ego.hip, point, tests and phases: mw_ego.h, launch: mw_policy.h).
//
// The call does not wait for the Maze's side-stream refills: mw_engine.h, at world_view().
#include <math.h>

#include "mw_engine.h"
#include "mw_policy.h"

using namespace mwhost;

extern "C" {

int mw_ego_map(mw_engine *e, const double *host_window, int32_t size, int32_t planes, int32_t flags, const uint8_t *d_mask, const double *d_pos,
               uint8_t *d_planes, const mw_nav_params *src_grid, const void *d_src, int32_t src_bytes, uint32_t fill, void *d_sample, void *stream)
{
    const char *what = "mw_ego_map";
    if (!e) return MW_E_INVALID;
    if (!host_window) return fail(e, MW_E_INVALID, "%s: host_window is null", what);
    const mwego::Window w{host_window[0], host_window[1], host_window[2], host_window[3], size, planes, flags};
    const mwseen::Sight s = mwego::sight_of(w, host_window[4], host_window[5]);
    if (size < 1 || size > MW_EGO_MAX_SIZE) return fail(e, MW_E_INVALID, "%s: size %d outside 1 .. %d", what, (int)size, MW_EGO_MAX_SIZE);
    if (const int rc = positive_check(e, what, "cell", w.cell)) return rc;
    if (!isfinite(w.back)) return fail(e, MW_E_INVALID, "%s: back %g is not finite", what, w.back);
    if (const int rc = nonnegative_check(e, what, "wall_radius", w.wall_radius)) return rc;
    if (const int rc = nonnegative_check(e, what, "entity_pad", w.entity_pad)) return rc;
    if (planes & ~(MW_EGO_WALL | MW_EGO_ENTITY | MW_EGO_VISIBLE)) return fail(e, MW_E_INVALID, "%s: unknown planes 0x%x", what, (unsigned)planes);
    if (flags & ~(MW_EGO_ENTITIES | MW_EGO_NORTH)) return fail(e, MW_E_INVALID, "%s: unknown flags 0x%x", what, (unsigned)flags);
    if (planes & MW_EGO_VISIBLE) {
        if (const int rc = positive_check(e, what, "range", s.range)) return rc;
        if (!(s.cos_half >= -1.0 && s.cos_half <= 1.0)) return fail(e, MW_E_INVALID, "%s: cos_half %g outside -1 .. 1", what, s.cos_half);
    }
    if (!planes && !d_src) return fail(e, MW_E_INVALID, "%s: neither a plane nor a source is asked for", what);
    if (planes && !d_planes) return fail(e, MW_E_INVALID, "%s: d_planes is null", what);
    mwego::Source q{0.0, 0, 0, 0, 0u};
    if (d_src) {
        if (!src_grid || !d_sample) return fail(e, MW_E_INVALID, "%s: a source without %s", what, !src_grid ? "src_grid" : "d_sample");
        if (src_bytes != 1 && src_bytes != 2) return fail(e, MW_E_INVALID, "%s: src_bytes %d is neither 1 nor 2", what, (int)src_bytes);
        if (const int rc = grid_check(e, what, src_grid)) return rc;
        q = {src_grid->cell, src_grid->gx, src_grid->gz, src_bytes, src_bytes == 2 ? (fill & 0xFFFFu) : (fill & 0xFFu)};
    }
    const MwArgs &a = e->args;
    if ((planes & MW_EGO_ENTITY) && a.E > 255) return fail(e, MW_E_INVALID, "%s: %d slots do not fit the entity plane's byte", what, a.E);
    const mwpolicy::Launch l = mwpolicy::ego_launch(a.N, a.max_segs, a.E, planes);
    if (!l.fits) return fail(e, MW_E_INVALID, "%s: %d segments and %d slots need %zu bytes of LDS > 64 KiB", what, a.max_segs, a.E, l.lds);
    return launch_query(e, what, mw_ego_kernel, ray_view, l.grid, l.threads, l.lds, &e->ego_lds_set, stream, w, s, q, d_mask, d_pos, planes ? d_planes : nullptr, d_src,
                        d_src ? d_sample : nullptr);
}

}  // extern "C"
