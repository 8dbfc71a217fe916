// mwengine host runtime: explored-area maps (mw_seen_update; kernel: mw_seen.hip, tests and phases: mw_seen.h, launch: mw_policy.h).
//
// Like the nav and ray calls (mw_engine_nav.hip), and for the reason given there, the call does not wait for the Maze's side-stream
// refills: the refill kernel generates into the spare arrays — the spare's own segs / nsegs, extent and entity slabs among them — and
// touches the env's random stream and refill_mask beside them; the live segs, nsegs, extent, ekind, epos, egeom, carry and agent pose
// that this kernel reads are written on the caller's stream alone (K1's take-over of a spare, the resets, the state writes), behind
// which the call is ordered by being on that stream.
#include <math.h>

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
    // (the grid checks of mw_nav_build: every seen grid is a valid nav grid)
    if (!(grid->cell > 0.0)) return fail(e, MW_E_INVALID, "%s: cell %g <= 0", what, grid->cell);
    if (grid->gx < 1 || grid->gz < 1) return fail(e, MW_E_INVALID, "%s: a grid of %d x %d cells", what, (int)grid->gx, (int)grid->gz);
    if ((long long)grid->gx * (long long)grid->gz > MW_NAV_MAX_CELLS)
        return fail(e, MW_E_INVALID, "%s: %d x %d cells > %d: use a larger cell", what, (int)grid->gx, (int)grid->gz, MW_NAV_MAX_CELLS);
    const mwseen::Sight s{host_sight[0], host_sight[1], flags};
    if (!(s.range > 0.0) || !isfinite(s.range)) return fail(e, MW_E_INVALID, "%s: range %g is not a positive finite number", what, s.range);
    if (!(s.cos_half >= -1.0 && s.cos_half <= 1.0)) return fail(e, MW_E_INVALID, "%s: cos_half %g outside -1 .. 1", what, s.cos_half);
    if (flags & ~MW_SEEN_ENTITIES) return fail(e, MW_E_INVALID, "%s: unknown flags 0x%x", what, (unsigned)flags);
    const MwArgs &a = e->args;
    const mwpolicy::SeenLaunch l = mwpolicy::seen_launch(a.N, a.max_segs, a.E);
    if (!l.fits) return fail(e, MW_E_INVALID, "%s: %d segments and %d slots need %zu bytes of LDS > 64 KiB", what, a.max_segs, a.E, l.lds);
    if (mwpolicy::grid_too_large(l.grid)) return fail(e, MW_E_INVALID, "%s: %llu workgroups", what, l.grid);
    ON_DEVICE(e);
    const MwRayArgs ra{{a.segs, a.nsegs, a.extent, a.ekind, a.epos, a.egeom, a.carry, a.ax, a.az, a.status, a.N, a.E, a.max_segs, a.shared_geom, a.agent_radius,
                        a.max_forward_step},
                       a.adir};
    if ((int)l.lds > e->seen_lds_set) {
        HIP_TRY(e, hipFuncSetAttribute((const void *)mw_seen_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds));
        e->seen_lds_set = (int)l.lds;
    }
    hipLaunchKernelGGL(mw_seen_kernel, dim3((unsigned)l.grid), dim3((unsigned)l.threads), l.lds, (hipStream_t)stream, ra, *grid, s, d_mask, d_clear, d_seen, d_count,
                       d_new);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

}  // extern "C"
