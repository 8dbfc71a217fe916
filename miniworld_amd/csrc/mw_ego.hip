// Egocentric map windows on the device (mw_ego_map, mw_engine_ego.hip; the point, the tests and every phase: mw_ego.h).
//
// mw_ego_kernel: one workgroup of MW_EGO_THREADS lanes per env; a masked-off env's leaves before the barrier.  The env's obstacles are
// staged once in dynamic LDS, only those the asked planes need (mwego::carve; the bytes: mwego::staged_bytes, checked against 64 KiB
// before the launch): for VISIBLE the walls and — with MW_EGO_ENTITIES — the slots' circles as mw_seen_kernel stages them, for WALL the raw
// segments, for ENTITY the circles under entity_pad.  Then a window cell per lane, MW_EGO_THREADS cells a round in row-major order:
// consecutive lanes take consecutive columns, so a wavefront's byte stores into a plane are 64 consecutive bytes; every lane walks the
// obstacles in index order — all lanes read the same LDS address (a broadcast) — and stops at its first hit; a plane that was not asked
// for costs no loop, a call without planes stages nothing and has no barrier to wait at.
// Indices: a cell index is below size * size <= MW_EGO_MAX_SIZE^2 = 2^14, a plane's offset below 3 * 2^14, a segment index below
// nsegs_of() <= max_segs, a slot below E, a source index below gx * gz <= MW_NAV_MAX_CELLS (the inside test precedes the conversion).
#include "mw_kernels.h"

extern "C" __global__ __launch_bounds__(MW_EGO_THREADS) void mw_ego_kernel(MwRayArgs a, mwego::Window w, mwseen::Sight s, mwego::Source q,
                                                                            const uint8_t *__restrict__ mask, const double *__restrict__ pos,
                                                                            uint8_t *__restrict__ planes, const void *__restrict__ src,
                                                                            void *__restrict__ sample)
{
    extern __shared__ __attribute__((aligned(16))) double ego_lds[];
    const size_t env = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (mask && !mask[env]) return;
    const mwego::Staged st = mwego::carve(ego_lds, a.w.max_segs, a.w.E, w.planes);
    if (w.planes) {
        mwego::stage(a, w, s, env, st, lane, MW_EGO_THREADS);
        __syncthreads();
    }
    const size_t n = (size_t)w.size * (size_t)w.size;
    const size_t src_row = (size_t)q.gx * (size_t)q.gz * (size_t)q.bytes;
    mwego::cells(a, w, s, q, env, mwego::frame_of(a, w, s, env, pos), st, planes ? planes + env * (size_t)mwego::plane_count(w.planes) * n : nullptr,
                 src ? static_cast<const char *>(src) + env * src_row : nullptr, sample ? static_cast<char *>(sample) + env * n * (size_t)q.bytes : nullptr, lane,
                 MW_EGO_THREADS);
}
