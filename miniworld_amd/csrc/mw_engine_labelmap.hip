// mwengine host runtime: object maps (mw_label_project; kernel: mw_labelmap.hip, arithmetic and phases: mw_labelmap.h, launch: mw_policy.h).
//
// The call does not wait for the Maze's side-stream refills: mw_engine.h, at world_view().
#include "mw_engine.h"
#include "mw_policy.h"

using namespace mwhost;

extern "C" {

int mw_label_project(mw_engine *e, const double *host_params, const float *d_depth, const int32_t *d_code, int32_t base, const uint8_t *d_mask, int32_t size,
                     int32_t flags, uint8_t *d_plane, const mw_nav_params *grid, const uint8_t *d_clear, uint8_t *d_map, int32_t ids, int32_t *d_obj_cells,
                     double *d_obj_pos, void *stream)
{
    const char *what = "mw_label_project";
    if (!e) return MW_E_INVALID;
    mwdepth::Sensor s;
    mwdepth::Window w;
    mw_nav_params p;
    long long cells;
    if (const int rc = projection_check(e, what, host_params, d_depth, size, flags, grid, s, w, p, cells)) return rc;
    if (!d_code) return fail(e, MW_E_INVALID, "%s: d_code is null", what);
    if (base < 0) return fail(e, MW_E_INVALID, "%s: base %d < 0", what, (int)base);
    if (ids < 0 || ids > MW_LABELMAP_MAX_IDS) return fail(e, MW_E_INVALID, "%s: ids %d outside 0 .. %d", what, (int)ids, MW_LABELMAP_MAX_IDS);
    if (!grid) {
        if (!d_plane) return fail(e, MW_E_INVALID, "%s: d_plane is null", what);
        if (ids > 0) return fail(e, MW_E_INVALID, "%s: ids %d with the window target (the per-object outputs are a map's)", what, (int)ids);
    } else {
        if (!d_map) return fail(e, MW_E_INVALID, "%s: d_map is null", what);
        if (ids > 0 && !d_obj_cells && !d_obj_pos) return fail(e, MW_E_INVALID, "%s: ids %d and neither d_obj_cells nor d_obj_pos", what, (int)ids);
    }
    const MwArgs &a = e->args;
    const mwpolicy::Launch l = mwpolicy::labelmap_launch(a.N, cells, ids);
    if (!l.fits)
        return fail(e, MW_E_INVALID, "%s: %lld cells > %d (a key of LDS per cell): use a larger cell", what, cells, MW_LABELMAP_MAX_CELLS);
    const int wide = (a.W * a.H) % 4 == 0 && mwpolicy::wide_units((uintptr_t)d_depth | (uintptr_t)d_code) ? 1 : 0;
    return launch_query(e, what, mw_labelmap_kernel, ray_view, l.grid, l.threads, l.lds, &e->labelmap_lds_set, stream, a.cam, s, w, p, wide, d_depth, d_code, base,
                        d_mask, grid ? d_clear : nullptr, grid ? nullptr : d_plane, grid ? d_map : nullptr, grid ? ids : 0, grid ? d_obj_cells : nullptr,
                        grid ? d_obj_pos : nullptr);
}

}  // extern "C"
