// mwengine host runtime: snapshot records — states (mw_snapshot_save / mw_snapshot_load) and frames (mw_snapshot_save_frames /
// mw_snapshot_load_frames), their forms with chosen records (_at) and with a device mask over all envs (_where), their byte counts and
// their helpers.
#include "mw_engine.h"

using namespace mwhost;

namespace {

// mw_snapshot_save / mw_snapshot_load touch worlds that the Maze's refill kernel may still be writing on the side stream (spares and
// their refill_mask words, read behind the live stream).  The caller's stream waits for an event recorded behind those refills:
// the host does not block — a fork loop stays asynchronous, which ON_DEVICE_SYNC would not be — and everything the engine enqueues
// later on the side stream is ordered behind the caller's stream by launch_side_refill's own event.  The other refills are blocks
// of the step kernel itself, in stream order.  So between launches refill_mask is 0 or 1 (mw_snapshot.hip).
int snapshot_order(mw_engine *e, hipStream_t st)
{
    if (!e->side_refill_pending || !e->side_stream) return MW_OK;
    if (!e->ev_refill_done) HIP_TRY(e, make_event(e->ev_refill_done));
    HIP_TRY(e, hipEventRecord(e->ev_refill_done.get(), e->side_stream.get()));
    HIP_TRY(e, hipStreamWaitEvent(st, e->ev_refill_done.get(), 0));
    return MW_OK;
}

// the items of a call: a list of `count` of them, or (the _where forms) every env under a device mask — count is num_envs then, and the
// list form's limits on it do not apply: records repeat
enum Items { ITEMS_LIST, ITEMS_MASKED };

// the arguments both calls share, checked before anything is launched
int snapshot_args(mw_engine *e, const char *what, const void *d_snap, int32_t count, int32_t capacity, bool whole_batch_limit, Items items = ITEMS_LIST)
{
    if (!d_snap) return fail(e, MW_E_INVALID, "%s: the record buffer is null", what);
    if ((uintptr_t)d_snap & 15u) return fail(e, MW_E_INVALID, "%s: the record buffer is not 16-byte aligned", what);
    if (capacity < 0) return fail(e, MW_E_INVALID, "%s: capacity %d < 0", what, (int)capacity);
    if (items == ITEMS_MASKED) return MW_OK;
    if (count < 0 || count > capacity) return fail(e, MW_E_INVALID, "%s: count %d outside 0 .. capacity %d", what, (int)count, (int)capacity);
    if (whole_batch_limit && count > e->cfg.num_envs) return fail(e, MW_E_INVALID, "%s: count %d > num_envs %d", what, (int)count, e->cfg.num_envs);
    return MW_OK;
}

// What mw_snapshot_save and mw_snapshot_load share: the arguments checked, the engine's device, the grid of the call over `count` items (MW_E_INVALID past the 1-D grid limit) and the order behind the refills.
int snapshot_begin(mw_engine *e, const char *what, const void *d_snap, int32_t count, int32_t capacity, bool whole_batch_limit, hipStream_t st,
                   SnapshotGrid *g, Items items = ITEMS_LIST)
{
    if (const int rc = snapshot_args(e, what, d_snap, count, capacity, whole_batch_limit, items)) return rc;
    ON_DEVICE(e);
    *g = items == ITEMS_MASKED ? snapshot_where_grid(count, e->snap_layout.total_rows, e->snap_chunks_per_item)
                               : snapshot_grid(count, e->snap_layout.total_rows, e->snap_chunks_per_item);
    if (grid_too_large((unsigned long long)g->blocks))
        return fail(e, MW_E_INVALID, "%s: %d items need %lld workgroups, more than one launch holds: split the call", what, count, g->blocks);
    g->blocks = std::max<long long>(g->blocks, 1);
    return snapshot_order(e, st);
}

// Frame records (mw_snapshot_save_frames / mw_snapshot_load_frames; mw_snapframes.h): what of the engine's frame configuration shapes
// one under `flags`
MwSnapfConfig snapf_config(const mw_engine *e, int32_t flags)
{
    MwSnapfConfig c{};
    c.W = e->cfg.obs_width; c.H = e->cfg.obs_height; c.layout = e->obs_layout; c.flags = flags;
    c.stack_depth = (flags & MW_SNAPF_STACK) ? e->stack.depth : 0;
    c.frame_bytes = frame_bytes_of(e);
    return c;
}

// the arguments both calls share, checked before anything is launched; then the kernel's view of the call
int snapf_args(mw_engine *e, const char *what, const void *d_frames, const void *d_obs, const void *d_depth, int32_t count, int32_t n_recs,
               int32_t capacity, int32_t flags, bool whole_batch_limit, MwSnapfArgs *out, unsigned *grid, Items items = ITEMS_LIST)
{
    if (const int rc = snapshot_args(e, what, d_frames, count, capacity, whole_batch_limit, items)) return rc;
    if (n_recs < 0 || n_recs > capacity) return fail(e, MW_E_INVALID, "%s: n_recs %d outside 0 .. capacity %d", what, (int)n_recs, (int)capacity);
    if (!d_obs) return fail(e, MW_E_INVALID, "%s: d_obs is null", what);
    if (flags & ~(MW_SNAPF_DEPTH | MW_SNAPF_STACK)) return fail(e, MW_E_INVALID, "%s: unknown flag bits in %d", what, (int)flags);
    if ((flags & MW_SNAPF_DEPTH) && !d_depth) return fail(e, MW_E_INVALID, "%s: MW_SNAPF_DEPTH with a null d_depth", what);
    if ((flags & MW_SNAPF_STACK) && !e->stack.depth) return fail(e, MW_E_INVALID, "%s: MW_SNAPF_STACK without a frame stack (mw_set_frame_stack)", what);
    if (flags & MW_SNAPF_STACK)
        if (const int rc = stack_check(e, what)) return rc;
    const MwSnapfConfig c = snapf_config(e, flags);
    const MwSnapfLayout L = mw_snapf_layout(c, capacity);
    MwSnapfArgs a{};
    a.key = mw_snapf_key(c, capacity);
    for (int s = 0; s < MW_SF_COUNT; ++s) a.off[s] = L.off[s];
    a.frame_bytes = c.frame_bytes;
    a.depth_bytes = L.rec_bytes[MW_SF_DEPTH];
    a.N = e->cfg.num_envs; a.count = count; a.n_recs = n_recs;
    a.stack_depth = c.stack_depth;
    a.first_slot = c.stack_depth ? stack_phase_of(e) : 0;
    // 16-byte units: every base and every size a multiple of 16 (the sections always are: mw_snapframes.h)
    const uintptr_t bases = (uintptr_t)d_frames | (uintptr_t)d_obs | (uintptr_t)(a.depth_bytes ? d_depth : nullptr) | (uintptr_t)(c.stack_depth ? e->stack.ring : nullptr);
    const SnapfGrid g = items == ITEMS_MASKED ? snapf_where_grid(bases, a.frame_bytes, a.depth_bytes, c.stack_depth, count)
                                              : snapf_grid(bases, a.frame_bytes, a.depth_bytes, c.stack_depth, count);
    if (grid_too_large(g.blocks))
        return fail(e, MW_E_INVALID, "%s: %d items need %llu workgroups, more than one launch holds: split the call", what, (int)count, (unsigned long long)g.blocks);
    a.wide = g.wide;
    a.frame_chunks = (int32_t)g.frame_chunks; a.depth_chunks = (int32_t)g.depth_chunks; a.chunks_per_item = (int32_t)g.per_item;
    *out = a;
    *grid = (unsigned)std::max<uint64_t>(g.blocks, 1);
    return MW_OK;
}

}  // namespace

extern "C" {

int64_t mw_snapshot_bytes(const mw_engine *e, int32_t capacity)
{
    if (!e || capacity < 0) return MW_E_INVALID;
    return mw_snap_bytes(e->snap_layout, capacity);
}

int mw_snapshot_save(mw_engine *e, const int32_t *d_envs, int32_t count, uint8_t *d_snap, int32_t capacity, void *stream)
{
    if (!e) return MW_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    SnapshotGrid g;
    if (const int rc = snapshot_begin(e, "mw_snapshot_save", d_snap, count, capacity, d_envs == nullptr, st, &g)) return rc;
    hipLaunchKernelGGL(mw_snapshot_save_kernel, dim3((unsigned)g.blocks), dim3(MW_SNAP_THREADS), 0, st, (const MwSnapTable *)e->d_snap_tab, mw_snap_key(e->snap_cfg, capacity),
                       e->cfg.num_envs, (int)capacity, (int)count, g.item_chunks, d_envs, e->args.status, d_snap);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_snapshot_load(mw_engine *e, const int32_t *d_envs, const int32_t *d_recs, int32_t count, const uint8_t *d_snap, int32_t n_recs,
                     int32_t capacity, void *stream)
{
    if (!e) return MW_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    SnapshotGrid g;
    if (const int rc = snapshot_begin(e, "mw_snapshot_load", d_snap, count, capacity, true, st, &g)) return rc;
    if (n_recs < 0 || n_recs > capacity) return fail(e, MW_E_INVALID, "mw_snapshot_load: n_recs %d outside 0 .. capacity %d", (int)n_recs, (int)capacity);
    // (the frames in the caller's buffers are those of the states that are about to go, and so are the cached ones: a loaded env's
    // epoch is not part of its record)
    invalidate(e, snapshot_load_invalidation(false));
    hipLaunchKernelGGL(mw_snapshot_load_kernel, dim3((unsigned)g.blocks), dim3(MW_SNAP_THREADS), 0, st, (const MwSnapTable *)e->d_snap_tab, mw_snap_key(e->snap_cfg, capacity),
                       e->cfg.num_envs, (int)capacity, (int)count, g.item_chunks, d_envs, e->args.status, d_snap, d_recs, (int)n_recs, e->args.frame_clean,
                       e->cfg.shared_geometry ? nullptr : e->args.occ_valid, e->stack.depth ? stack_flags(e, e->stack.cur) : nullptr);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_snapshot_save_at(mw_engine *e, const int32_t *d_envs, const int32_t *d_recs, int32_t count, uint8_t *d_snap, int32_t capacity, void *stream)
{
    if (!e) return MW_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    SnapshotGrid g;
    if (const int rc = snapshot_begin(e, "mw_snapshot_save_at", d_snap, count, capacity, d_envs == nullptr, st, &g)) return rc;
    hipLaunchKernelGGL(mw_snapshot_save_at_kernel, dim3((unsigned)g.blocks), dim3(MW_SNAP_THREADS), 0, st, (const MwSnapTable *)e->d_snap_tab,
                       mw_snap_key(e->snap_cfg, capacity), e->cfg.num_envs, (int)capacity, (int)count, g.item_chunks, d_envs, e->args.status, d_snap, d_recs);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_snapshot_load_where(mw_engine *e, const uint8_t *d_mask, const int32_t *d_recs, const uint8_t *d_snap, int32_t n_recs, int32_t capacity,
                           void *stream)
{
    if (!e) return MW_E_INVALID;
    if (!d_mask) return fail(e, MW_E_INVALID, "mw_snapshot_load_where: d_mask is null");
    if (!d_recs) return fail(e, MW_E_INVALID, "mw_snapshot_load_where: d_recs is null (record i for env i: mw_snapshot_load)");
    hipStream_t st = (hipStream_t)stream;
    SnapshotGrid g;
    if (n_recs < 0 || n_recs > capacity) return fail(e, MW_E_INVALID, "mw_snapshot_load_where: n_recs %d outside 0 .. capacity %d", (int)n_recs, (int)capacity);
    if (const int rc = snapshot_begin(e, "mw_snapshot_load_where", d_snap, e->cfg.num_envs, capacity, false, st, &g, ITEMS_MASKED)) return rc;
    // (the held frame goes; the cached frames of the envs that are not written stay, and the kernel sees to the others: mw_policy.h)
    invalidate(e, snapshot_load_invalidation(true));
    hipLaunchKernelGGL(mw_snapshot_load_where_kernel, dim3((unsigned)g.blocks), dim3(MW_SNAP_THREADS), 0, st, (const MwSnapTable *)e->d_snap_tab,
                       mw_snap_key(e->snap_cfg, capacity), e->cfg.num_envs, (int)capacity, e->cfg.num_envs, g.item_chunks, (const int32_t *)nullptr, e->args.status,
                       d_snap, d_recs, (int)n_recs, e->args.frame_clean, e->cfg.shared_geometry ? nullptr : e->args.occ_valid,
                       e->stack.depth ? stack_flags(e, e->stack.cur) : nullptr, d_mask, e->args.fc_epoch);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int64_t mw_snapshot_frames_bytes(const mw_engine *e, int32_t capacity, int32_t flags)
{
    if (!e || capacity < 0 || (flags & ~(MW_SNAPF_DEPTH | MW_SNAPF_STACK))) return MW_E_INVALID;
    // (stacked frames are those of the layout the stack was set under, as for the two calls: stack_check's own test, no message)
    if ((flags & MW_SNAPF_STACK) && (!e->stack.depth || e->stack.layout != e->obs_layout || e->stack.frame_bytes != frame_bytes_of(e))) return MW_E_INVALID;
    return (int64_t)mw_snapf_layout(snapf_config(e, flags), capacity).total;
}

int mw_snapshot_save_frames(mw_engine *e, const int32_t *d_envs, int32_t count, const uint8_t *d_obs, const float *d_depth, uint8_t *d_frames,
                            int32_t capacity, int32_t flags, void *stream)
{
    if (!e) return MW_E_INVALID;
    MwSnapfArgs a;
    unsigned grid = 1;
    if (const int rc = snapf_args(e, "mw_snapshot_save_frames", d_frames, d_obs, d_depth, count, capacity, capacity, flags, d_envs == nullptr, &a, &grid)) return rc;
    ON_DEVICE(e);
    hipLaunchKernelGGL(mw_snapshot_save_frames_kernel, dim3(grid), dim3(MW_SNAPF_THREADS), 0, (hipStream_t)stream, a, d_envs, e->args.status, d_obs,
                       reinterpret_cast<const uint8_t *>(a.depth_bytes ? d_depth : nullptr), (const uint8_t *)(a.stack_depth ? e->stack.ring : nullptr),
                       (const uint8_t *)(a.stack_depth ? stack_flags(e, e->stack.cur) : nullptr), d_frames);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_snapshot_load_frames(mw_engine *e, const int32_t *d_envs, const int32_t *d_recs, int32_t count, const uint8_t *d_frames, int32_t n_recs,
                            int32_t capacity, int32_t flags, uint8_t *d_obs, float *d_depth, void *stream)
{
    if (!e) return MW_E_INVALID;
    MwSnapfArgs a;
    unsigned grid = 1;
    if (const int rc = snapf_args(e, "mw_snapshot_load_frames", d_frames, d_obs, d_depth, count, n_recs, capacity, flags, true, &a, &grid)) return rc;
    ON_DEVICE(e);
    invalidate(e, snapshot_load_frames_invalidation(false));        // (rows of d_obs are written; the frame cache stays: no state changed)
    hipLaunchKernelGGL(mw_snapshot_load_frames_kernel, dim3(grid), dim3(MW_SNAPF_THREADS), 0, (hipStream_t)stream, a, d_envs, e->args.status, d_recs, d_frames,
                       d_obs, reinterpret_cast<uint8_t *>(a.depth_bytes ? d_depth : nullptr), a.stack_depth ? e->stack.ring : nullptr,
                       a.stack_depth ? stack_flags(e, e->stack.cur) : nullptr);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_snapshot_save_frames_at(mw_engine *e, const int32_t *d_envs, const int32_t *d_recs, int32_t count, const uint8_t *d_obs, const float *d_depth,
                               uint8_t *d_frames, int32_t capacity, int32_t flags, void *stream)
{
    if (!e) return MW_E_INVALID;
    MwSnapfArgs a;
    unsigned grid = 1;
    if (const int rc = snapf_args(e, "mw_snapshot_save_frames_at", d_frames, d_obs, d_depth, count, capacity, capacity, flags, d_envs == nullptr, &a, &grid)) return rc;
    ON_DEVICE(e);
    hipLaunchKernelGGL(mw_snapshot_save_frames_at_kernel, dim3(grid), dim3(MW_SNAPF_THREADS), 0, (hipStream_t)stream, a, d_envs, e->args.status, d_obs,
                       reinterpret_cast<const uint8_t *>(a.depth_bytes ? d_depth : nullptr), (const uint8_t *)(a.stack_depth ? e->stack.ring : nullptr),
                       (const uint8_t *)(a.stack_depth ? stack_flags(e, e->stack.cur) : nullptr), d_frames, d_recs);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_snapshot_load_frames_where(mw_engine *e, const uint8_t *d_mask, const int32_t *d_recs, const uint8_t *d_frames, int32_t n_recs, int32_t capacity,
                                  int32_t flags, uint8_t *d_obs, float *d_depth, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (!d_mask) return fail(e, MW_E_INVALID, "mw_snapshot_load_frames_where: d_mask is null");
    if (!d_recs) return fail(e, MW_E_INVALID, "mw_snapshot_load_frames_where: d_recs is null (record i for env i: mw_snapshot_load_frames)");
    MwSnapfArgs a;
    unsigned grid = 1;
    if (const int rc = snapf_args(e, "mw_snapshot_load_frames_where", d_frames, d_obs, d_depth, e->cfg.num_envs, n_recs, capacity, flags, false, &a, &grid,
                                  ITEMS_MASKED))
        return rc;
    ON_DEVICE(e);
    invalidate(e, snapshot_load_frames_invalidation(true));
    hipLaunchKernelGGL(mw_snapshot_load_frames_where_kernel, dim3(grid), dim3(MW_SNAPF_THREADS), 0, (hipStream_t)stream, a, (const int32_t *)nullptr, e->args.status,
                       d_recs, d_frames, d_obs, reinterpret_cast<uint8_t *>(a.depth_bytes ? d_depth : nullptr), a.stack_depth ? e->stack.ring : nullptr,
                       a.stack_depth ? stack_flags(e, e->stack.cur) : nullptr, d_mask);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

}  // extern "C"
