// mwengine host runtime: label frames (mw_label_frame; kernel: mw_label.hip, arithmetic and phases: mw_label.h, launch: mw_policy.h).
//
// The call does not wait for the Maze's side-stream refills: mw_engine.h, at world_view().  Beside the queries' view it reads the live
// polygons of the geometry sets, the slots' headings and mesh ids, and the mesh pools, all of which are written on the caller's stream or
// by synchronous calls alone.
#include <math.h>

#include "mw_engine.h"
#include "mw_policy.h"

using namespace mwhost;

namespace {

// the queries' view and what the frame needs beside it
MwLabelArgs label_view(const mw_engine *e)
{
    const MwArgs &a = e->args;
    MwLabelArgs la{};
    la.r = ray_view(e);
    la.ay = a.ay; la.cam = a.cam; la.edir = a.edir; la.emesh = a.emesh; la.polys = a.polys; la.npolys = a.npolys;
    la.mesh = e->have_meshes ? a.mesh : nullptr;
    la.mesh_pos = e->have_meshes ? a.mesh_pos : nullptr;
    la.max_polys = a.max_polys; la.n_mesh = MW_MAX_MESH; la.W = a.W; la.H = a.H; la.msaa = e->cfg.msaa;
    return la;
}

}  // namespace

extern "C" {

int mw_label_frame(mw_engine *e, const mw_label_params *params, const uint8_t *d_mask, uint8_t *d_class, int32_t *d_code, float *d_depth, int32_t *d_ent_pixels,
                   int32_t *d_ent_box, void *stream)
{
    const char *what = "mw_label_frame";
    if (!e) return MW_E_INVALID;
    if (!params) return fail(e, MW_E_INVALID, "%s: params is null", what);
    if (!d_class) return fail(e, MW_E_INVALID, "%s: d_class is null", what);
    const mw_label_params p = *params;
    if (p.flags & ~(MW_LABEL_MESH_BOUNDS | MW_LABEL_UNPRUNED)) return fail(e, MW_E_INVALID, "%s: unknown flags 0x%x", what, (unsigned)p.flags);
    if (!isfinite(p.near) || !isfinite(p.far)) return fail(e, MW_E_INVALID, "%s: near %g or far %g is not finite", what, p.near, p.far);
    if (p.near < 0.0) return fail(e, MW_E_INVALID, "%s: near %g < 0", what, p.near);
    if (!(p.near < p.far)) return fail(e, MW_E_INVALID, "%s: near %g >= far %g", what, p.near, p.far);
    const MwArgs &a = e->args;
    const mwpolicy::LabelLaunch l = mwpolicy::label_launch(a.N, a.W, a.H, a.max_polys, a.E);
    if (!l.fits)
        return fail(e, MW_E_INVALID, "%s: a frame %d pixels wide over a scene of %d polygons and %d slots does not fit the kernel's LDS plan (64 KiB; at most %d polygons, %d slots)",
                    what, a.W, a.max_polys, a.E, MW_LABEL_MAX_POLYS, MW_LABEL_MAX_ENTS);
    return launch_query(e, what, mw_label_kernel, label_view, l.grid, l.threads, l.lds, &e->label_lds_set, stream, p, l.band_rows, l.chunk,
                        (p.flags & MW_LABEL_UNPRUNED) ? 0 : 1, d_mask, d_class, d_code, d_depth, d_ent_pixels, d_ent_box);
}

}  // extern "C"
