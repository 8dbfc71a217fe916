// mwengine host runtime: depth projection (mw_depth_project; kernel: mw_depth.hip, arithmetic and phases: mw_depth.h, launch: mw_policy.h).
//
// The call does not wait for the Maze's side-stream refills: mw_engine.h, at world_view().
#include <math.h>

#include "mw_engine.h"
#include "mw_policy.h"

using namespace mwhost;

namespace mwhost {

// What mw_depth_project and mw_label_project check alike, before anything of their own: the engine's frame, the sensor of host_params
// [0 .. 3] and the target — the window of `size`, `flags` and host_params[4 .. 5], or the map's `grid`.  Fills s, w or p, and cells.
int projection_check(mw_engine *e, const char *what, const double *host_params, const void *d_depth, int32_t size, int32_t flags, const mw_nav_params *grid,
                     mwdepth::Sensor &s, mwdepth::Window &w, mw_nav_params &p, long long &cells)
{
    if (!host_params) return fail(e, MW_E_INVALID, "%s: host_params is null", what);
    if (!d_depth) return fail(e, MW_E_INVALID, "%s: d_depth is null", what);
    const MwArgs &a = e->args;
    // the depth kernel counts a cell's floor and obstacle points in the two halves of one 32-bit word: more pixels could carry from one into the other
    if ((long long)a.W * (long long)a.H > MW_DEPTH_MAX_PIXELS)
        return fail(e, MW_E_INVALID, "%s: a frame of %d x %d pixels > %d (a cell's two counts share a 32-bit word)", what, a.W, a.H, MW_DEPTH_MAX_PIXELS);
    s = {host_params[0], host_params[1], host_params[2], host_params[3], 0.0, 0.0, a.W, a.H};
    mwdepth::subpixel_of(e->cfg.msaa, s.sub_x, s.sub_y);
    if (const int rc = positive_check(e, what, "min_range", s.min_range)) return rc;
    if (const int rc = positive_check(e, what, "max_range", s.max_range)) return rc;
    if (s.min_range > s.max_range) return fail(e, MW_E_INVALID, "%s: min_range %g > max_range %g", what, s.min_range, s.max_range);
    if (const int rc = nonnegative_check(e, what, "floor_tol", s.floor_tol)) return rc;
    if (!(s.top >= s.floor_tol) || !isfinite(s.top)) return fail(e, MW_E_INVALID, "%s: top %g is not a finite number >= floor_tol %g", what, s.top, s.floor_tol);
    w = {1.0, 0.0, 1, 0};
    p = {1.0, 0.0, 0.0, 1, 1, 0, 0};
    if (!grid) {        // the window target
        w = {host_params[4], host_params[5], size, flags};
        if (size < 1 || size > MW_EGO_MAX_SIZE) return fail(e, MW_E_INVALID, "%s: size %d outside 1 .. %d", what, (int)size, MW_EGO_MAX_SIZE);
        if (const int rc = positive_check(e, what, "cell", w.cell)) return rc;
        if (!isfinite(w.back)) return fail(e, MW_E_INVALID, "%s: back %g is not finite", what, w.back);
        if (flags & ~MW_EGO_NORTH) return fail(e, MW_E_INVALID, "%s: unknown flags 0x%x", what, (unsigned)flags);
        cells = (long long)size * size;
    } else {            // the map target
        if (flags) return fail(e, MW_E_INVALID, "%s: unknown flags 0x%x (a map has none)", what, (unsigned)flags);
        if (const int rc = grid_check(e, what, grid)) return rc;
        if (!isfinite(grid->cell)) return fail(e, MW_E_INVALID, "%s: cell %g is not finite", what, grid->cell);
        p = *grid;
        cells = (long long)p.gx * p.gz;
    }
    return MW_OK;
}

}  // namespace mwhost

extern "C" {

int mw_depth_project(mw_engine *e, const double *host_params, const float *d_depth, const uint8_t *d_mask, int32_t size, int32_t flags, uint8_t *d_planes,
                     const mw_nav_params *grid, int32_t min_points, const uint8_t *d_clear, uint8_t *d_map, int32_t *d_count, int32_t *d_new, void *stream)
{
    const char *what = "mw_depth_project";
    if (!e) return MW_E_INVALID;
    mwdepth::Sensor s;
    mwdepth::Window w;
    mw_nav_params p;
    long long cells;
    if (const int rc = projection_check(e, what, host_params, d_depth, size, flags, grid, s, w, p, cells)) return rc;
    const MwArgs &a = e->args;
    if (!grid) {
        if (!d_planes) return fail(e, MW_E_INVALID, "%s: d_planes is null", what);
    } else {
        if (!d_map || !d_count) return fail(e, MW_E_INVALID, "%s: %s is null", what, !d_map ? "d_map" : "d_count");
        if (min_points < 1 || min_points > 255) return fail(e, MW_E_INVALID, "%s: min_points %d outside 1 .. 255", what, (int)min_points);
    }
    const mwpolicy::Launch l = mwpolicy::depth_launch(a.N, cells);
    if (!l.fits)
        return fail(e, MW_E_INVALID, "%s: %lld cells need %zu bytes of LDS > 64 KiB (at most %d cells): use a larger cell", what, cells, l.lds, MW_DEPTH_MAX_CELLS);
    const int wide = (a.W * a.H) % 4 == 0 && mwpolicy::wide_units((uintptr_t)d_depth) ? 1 : 0;
    return launch_query(e, what, mw_depth_kernel, ray_view, l.grid, l.threads, l.lds, &e->depth_lds_set, stream, a.cam, s, w, p, grid ? min_points : 1, wide, d_depth,
                        d_mask, grid ? d_clear : nullptr, grid ? nullptr : d_planes, grid ? d_map : nullptr, grid ? d_count : nullptr, grid ? d_new : nullptr);
}

}  // extern "C"
