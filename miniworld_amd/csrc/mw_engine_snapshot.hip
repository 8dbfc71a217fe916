// mwengine host runtime: snapshot records — states (mw_snapshot_save / mw_snapshot_load) and frames (mw_snapshot_save_frames /
// mw_snapshot_load_frames), their forms with chosen records (_at) and with a device mask over all envs (_where), their byte counts and
// their helpers.
#include "mw_engine.h"

using namespace mwhost;

namespace {

// The items of a call, as its entry point's contract names them (the kernels' rule: MW_SNAP_ITEMS, mw_kernels.h): a list of `count`
// of them, or — mask non-null, the _where forms — every env under a device mask; count is num_envs then, and the list form's limits on it
// do not apply: records repeat.
struct SnapItems {
    const int32_t *envs, *recs;
    const uint8_t *mask;
    int32_t count;
    bool whole_batch_limit;     // count may not exceed num_envs (item k is env k, or the envs must be distinct)
};

// the arguments all calls share, checked before anything is launched (n_recs: the valid records of a load; a save passes the capacity)
int snapshot_args(mw_engine *e, const char *what, const void *d_snap, const SnapItems &it, int32_t n_recs, int32_t capacity)
{
    if (!d_snap) return fail(e, MW_E_INVALID, "%s: the record buffer is null", what);
    if ((uintptr_t)d_snap & 15u) return fail(e, MW_E_INVALID, "%s: the record buffer is not 16-byte aligned", what);
    if (capacity < 0) return fail(e, MW_E_INVALID, "%s: capacity %d < 0", what, (int)capacity);
    if (!it.mask) {
        if (it.count < 0 || it.count > capacity) return fail(e, MW_E_INVALID, "%s: count %d outside 0 .. capacity %d", what, (int)it.count, (int)capacity);
        if (it.whole_batch_limit && it.count > e->cfg.num_envs) return fail(e, MW_E_INVALID, "%s: count %d > num_envs %d", what, (int)it.count, e->cfg.num_envs);
    }
    if (n_recs < 0 || n_recs > capacity) return fail(e, MW_E_INVALID, "%s: n_recs %d outside 0 .. capacity %d", what, (int)n_recs, (int)capacity);
    return MW_OK;
}

// What a save and a load of state records share: the arguments checked, the engine's device, the grid of the call over its items (MW_E_INVALID past the 1-D grid limit) and the order behind the refills (mw_engine.h: refill_order).
int snapshot_begin(mw_engine *e, const char *what, const void *d_snap, const SnapItems &it, int32_t n_recs, int32_t capacity, hipStream_t st, SnapshotGrid *g)
{
    if (const int rc = snapshot_args(e, what, d_snap, it, n_recs, capacity)) return rc;
    ON_DEVICE(e);
    *g = it.mask ? snapshot_where_grid(it.count, e->snap_layout.total_rows, e->snap_chunks_per_item)
                 : snapshot_grid(it.count, e->snap_layout.total_rows, e->snap_chunks_per_item);
    if (grid_too_large((unsigned long long)g->blocks))
        return fail(e, MW_E_INVALID, "%s: %d items need %lld workgroups, more than one launch holds: split the call", what, it.count, g->blocks);
    g->blocks = std::max<long long>(g->blocks, 1);
    return refill_order(e, st);
}

int save_states(mw_engine *e, const char *what, const SnapItems &it, uint8_t *d_snap, int32_t capacity, hipStream_t st)
{
    SnapshotGrid g;
    if (const int rc = snapshot_begin(e, what, d_snap, it, capacity, capacity, st, &g)) return rc;
    hipLaunchKernelGGL(mw_snapshot_save_kernel, dim3((unsigned)g.blocks), dim3(MW_SNAP_THREADS), 0, st, (const MwSnapTable *)e->d_snap_tab, mw_snap_key(e->snap_cfg, capacity),
                       e->cfg.num_envs, (int)capacity, (int)it.count, g.item_chunks, e->args.status, d_snap, it.envs, it.recs, it.mask);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int load_states(mw_engine *e, const char *what, const SnapItems &it, const uint8_t *d_snap, int32_t n_recs, int32_t capacity, hipStream_t st)
{
    SnapshotGrid g;
    if (const int rc = snapshot_begin(e, what, d_snap, it, n_recs, capacity, st, &g)) return rc;
    // The frames in the caller's buffers are those of the states that are about to go, and so are the cached ones: a loaded env's
    // epoch is not part of its record.  Masked: the held frame goes; the cached frames of the envs that are not written stay, and the
    // kernel sees to the others (mw_policy.h).
    const bool masked = it.mask != nullptr;
    invalidate(e, snapshot_load_invalidation(masked));
    hipLaunchKernelGGL(mw_snapshot_load_kernel, dim3((unsigned)g.blocks), dim3(MW_SNAP_THREADS), 0, st, (const MwSnapTable *)e->d_snap_tab, mw_snap_key(e->snap_cfg, capacity),
                       e->cfg.num_envs, (int)capacity, (int)it.count, g.item_chunks, e->args.status, d_snap, (int)n_recs, e->args.frame_clean,
                       e->cfg.shared_geometry ? nullptr : e->args.occ_valid, e->stack.depth ? stack_flags(e, e->stack.cur) : nullptr,
                       masked ? e->args.fc_epoch : nullptr, it.envs, it.recs, it.mask);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
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
int snapf_args(mw_engine *e, const char *what, const void *d_frames, const void *d_obs, const void *d_depth, const SnapItems &it, int32_t n_recs,
               int32_t capacity, int32_t flags, MwSnapfArgs *out, unsigned *grid)
{
    if (const int rc = snapshot_args(e, what, d_frames, it, n_recs, capacity)) return rc;
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
    a.N = e->cfg.num_envs; a.count = it.count; a.n_recs = n_recs;
    a.stack_depth = c.stack_depth;
    a.first_slot = c.stack_depth ? stack_phase_of(e) : 0;
    // 16-byte units: every base and every size a multiple of 16 (the sections always are: mw_snapframes.h)
    const uintptr_t bases = (uintptr_t)d_frames | (uintptr_t)d_obs | (uintptr_t)(a.depth_bytes ? d_depth : nullptr) | (uintptr_t)(c.stack_depth ? e->stack.ring : nullptr);
    const SnapfGrid g = it.mask ? snapf_where_grid(bases, a.frame_bytes, a.depth_bytes, c.stack_depth, it.count)
                                : snapf_grid(bases, a.frame_bytes, a.depth_bytes, c.stack_depth, it.count);
    if (grid_too_large(g.blocks))
        return fail(e, MW_E_INVALID, "%s: %d items need %llu workgroups, more than one launch holds: split the call", what, (int)it.count, (unsigned long long)g.blocks);
    a.wide = g.wide;
    a.frame_chunks = (int32_t)g.frame_chunks; a.depth_chunks = (int32_t)g.depth_chunks; a.chunks_per_item = (int32_t)g.per_item;
    *out = a;
    *grid = (unsigned)std::max<uint64_t>(g.blocks, 1);
    return MW_OK;
}

int save_frames(mw_engine *e, const char *what, const SnapItems &it, const uint8_t *d_obs, const float *d_depth, uint8_t *d_frames, int32_t capacity,
                int32_t flags, hipStream_t st)
{
    MwSnapfArgs a;
    unsigned grid = 1;
    if (const int rc = snapf_args(e, what, d_frames, d_obs, d_depth, it, capacity, capacity, flags, &a, &grid)) return rc;
    ON_DEVICE(e);
    hipLaunchKernelGGL(mw_snapshot_save_frames_kernel, dim3(grid), dim3(MW_SNAPF_THREADS), 0, st, a, e->args.status, d_obs,
                       reinterpret_cast<const uint8_t *>(a.depth_bytes ? d_depth : nullptr), (const uint8_t *)(a.stack_depth ? e->stack.ring : nullptr),
                       (const uint8_t *)(a.stack_depth ? stack_flags(e, e->stack.cur) : nullptr), d_frames, it.envs, it.recs, it.mask);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int load_frames(mw_engine *e, const char *what, const SnapItems &it, const uint8_t *d_frames, int32_t n_recs, int32_t capacity, int32_t flags,
                uint8_t *d_obs, float *d_depth, hipStream_t st)
{
    MwSnapfArgs a;
    unsigned grid = 1;
    if (const int rc = snapf_args(e, what, d_frames, d_obs, d_depth, it, n_recs, capacity, flags, &a, &grid)) return rc;
    ON_DEVICE(e);
    invalidate(e, snapshot_load_frames_invalidation(it.mask != nullptr));       // (rows of d_obs are written; the frame cache stays: no state changed)
    hipLaunchKernelGGL(mw_snapshot_load_frames_kernel, dim3(grid), dim3(MW_SNAPF_THREADS), 0, st, a, e->args.status, d_frames, d_obs,
                       reinterpret_cast<uint8_t *>(a.depth_bytes ? d_depth : nullptr), a.stack_depth ? e->stack.ring : nullptr,
                       a.stack_depth ? stack_flags(e, e->stack.cur) : nullptr, it.envs, it.recs, it.mask);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

}  // namespace

// The eight entry points: each fills the items its own contract names and makes one call.  A plain save writes record k whatever else
// (null recs); the _where forms are every env (null envs, count = num_envs) under the mask, through the records given.
extern "C" {

int64_t mw_snapshot_bytes(const mw_engine *e, int32_t capacity)
{
    if (!e || capacity < 0) return MW_E_INVALID;
    return mw_snap_bytes(e->snap_layout, capacity);
}

int mw_snapshot_save(mw_engine *e, const int32_t *d_envs, int32_t count, uint8_t *d_snap, int32_t capacity, void *stream)
{
    if (!e) return MW_E_INVALID;
    return save_states(e, "mw_snapshot_save", {d_envs, nullptr, nullptr, count, d_envs == nullptr}, d_snap, capacity, (hipStream_t)stream);
}

int mw_snapshot_load(mw_engine *e, const int32_t *d_envs, const int32_t *d_recs, int32_t count, const uint8_t *d_snap, int32_t n_recs,
                     int32_t capacity, void *stream)
{
    if (!e) return MW_E_INVALID;
    return load_states(e, "mw_snapshot_load", {d_envs, d_recs, nullptr, count, true}, d_snap, n_recs, capacity, (hipStream_t)stream);
}

int mw_snapshot_save_at(mw_engine *e, const int32_t *d_envs, const int32_t *d_recs, int32_t count, uint8_t *d_snap, int32_t capacity, void *stream)
{
    if (!e) return MW_E_INVALID;
    return save_states(e, "mw_snapshot_save_at", {d_envs, d_recs, nullptr, count, d_envs == nullptr}, d_snap, capacity, (hipStream_t)stream);
}

int mw_snapshot_load_where(mw_engine *e, const uint8_t *d_mask, const int32_t *d_recs, const uint8_t *d_snap, int32_t n_recs, int32_t capacity,
                           void *stream)
{
    if (!e) return MW_E_INVALID;
    if (!d_mask) return fail(e, MW_E_INVALID, "mw_snapshot_load_where: d_mask is null");
    if (!d_recs) return fail(e, MW_E_INVALID, "mw_snapshot_load_where: d_recs is null (record i for env i: mw_snapshot_load)");
    return load_states(e, "mw_snapshot_load_where", {nullptr, d_recs, d_mask, e->cfg.num_envs, false}, d_snap, n_recs, capacity, (hipStream_t)stream);
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
    return save_frames(e, "mw_snapshot_save_frames", {d_envs, nullptr, nullptr, count, d_envs == nullptr}, d_obs, d_depth, d_frames, capacity, flags,
                       (hipStream_t)stream);
}

int mw_snapshot_load_frames(mw_engine *e, const int32_t *d_envs, const int32_t *d_recs, int32_t count, const uint8_t *d_frames, int32_t n_recs,
                            int32_t capacity, int32_t flags, uint8_t *d_obs, float *d_depth, void *stream)
{
    if (!e) return MW_E_INVALID;
    return load_frames(e, "mw_snapshot_load_frames", {d_envs, d_recs, nullptr, count, true}, d_frames, n_recs, capacity, flags, d_obs, d_depth,
                       (hipStream_t)stream);
}

int mw_snapshot_save_frames_at(mw_engine *e, const int32_t *d_envs, const int32_t *d_recs, int32_t count, const uint8_t *d_obs, const float *d_depth,
                               uint8_t *d_frames, int32_t capacity, int32_t flags, void *stream)
{
    if (!e) return MW_E_INVALID;
    return save_frames(e, "mw_snapshot_save_frames_at", {d_envs, d_recs, nullptr, count, d_envs == nullptr}, d_obs, d_depth, d_frames, capacity, flags,
                       (hipStream_t)stream);
}

int mw_snapshot_load_frames_where(mw_engine *e, const uint8_t *d_mask, const int32_t *d_recs, const uint8_t *d_frames, int32_t n_recs, int32_t capacity,
                                  int32_t flags, uint8_t *d_obs, float *d_depth, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (!d_mask) return fail(e, MW_E_INVALID, "mw_snapshot_load_frames_where: d_mask is null");
    if (!d_recs) return fail(e, MW_E_INVALID, "mw_snapshot_load_frames_where: d_recs is null (record i for env i: mw_snapshot_load_frames)");
    return load_frames(e, "mw_snapshot_load_frames_where", {nullptr, d_recs, d_mask, e->cfg.num_envs, false}, d_frames, n_recs, capacity, flags, d_obs,
                       d_depth, (hipStream_t)stream);
}

}  // extern "C"
