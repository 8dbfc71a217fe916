// mwengine host runtime: everything that launches a frame or a step — the mesh path's buffers and chain, the launches, the three step
// entry points, the renders, final observations, the frame stack, frame reuse and the frame cache.
#include "mw_engine.h"

using namespace mwhost;

namespace {

// K1 out of the four kernels of a mode (mw_kernels.h: the K1 table): the dense form for lanes = k1_dense_lanes > 0, the wave-per-env form
// otherwise, then the engine's random stream
#define MW_K1(e, lanes, stem) ((lanes) ? MW_BY_STREAM(e, stem##_dense) : MW_BY_STREAM(e, stem))

// a kernel and its list form (mw_kernels.h: MW_KERNEL_PAIR)
template <typename... A>
struct KernelPair {
    void (*plain)(A...);
    void (*sub)(A..., const int32_t *);
};
template <typename... A>
KernelPair<A...> kernel_pair(void (*plain)(A...), void (*sub)(A..., const int32_t *)) { return {plain, sub}; }
#define MW_PAIR(stem) kernel_pair(stem##_kernel, stem##_sub_kernel)

// launches the list form over the envs of `list` (int32 [0] count, [1 + i] env) when there is one, the plain kernel otherwise
template <typename... A, typename... P>
void launch(const KernelPair<A...> &k, const int32_t *list, dim3 grid, dim3 block, size_t lds, hipStream_t st, P &&...args)
{
    if (list) hipLaunchKernelGGL(k.sub, grid, block, lds, st, std::forward<P>(args)..., list);
    else hipLaunchKernelGGL(k.plain, grid, block, lds, st, std::forward<P>(args)...);
}

// the geometry kernel: big scenes (one env per wavefront) or small, 8 samples per pixel (compiled in) or any
auto geom_kernel_of(int L, int msaa)
{
    const bool fixed8 = msaa == 8;
    if (L == 64) return fixed8 ? MW_PAIR(mw_geom_big) : MW_PAIR(mw_geom_big_any);
    return fixed8 ? MW_PAIR(mw_geom) : MW_PAIR(mw_geom_any);
}

// the tile kernel (mw_raster.hip).  big: a visiting order exists, records read in place; general: an output layout other than
// HWC or debug flags (the small-scene production kernels carry neither, nor a run-time depth switch); ragged: a frame off the
// 16 x 4 grid (no meshes: raster_path); first: K2's first part of a frame with meshes, which never enters a mesh tile — the
// plain tile code with the skip (the small-scene observation path only)
auto tile_kernel_of(bool big, bool depth, bool general, bool ragged, bool mesh, bool first)
{
    if (mesh) {
        if (big) return MW_PAIR(mw_raster_big_mesh_wrap);
        if (general) return MW_PAIR(mw_raster_mesh_wrap);
        if (first) return depth ? MW_PAIR(mw_raster_nomesh_depth) : MW_PAIR(mw_raster_nomesh);
        return depth ? MW_PAIR(mw_raster_mesh_depth) : MW_PAIR(mw_raster_mesh);
    }
    if (ragged) return big ? MW_PAIR(mw_raster_big_ragged) : MW_PAIR(mw_raster_ragged);
    if (general) return big ? MW_PAIR(mw_raster_big_wrap) : MW_PAIR(mw_raster_wrap);
    if (big) return depth ? MW_PAIR(mw_raster_big_depth) : MW_PAIR(mw_raster_big);
    return depth ? MW_PAIR(mw_raster_depth) : MW_PAIR(mw_raster);
}

// The buffers of one call, and which step kernels it runs: mw_step's (repeat = horizon = 0), mw_step_repeat's (repeat > 0: up to `repeat`
// sub-steps per env with its action, the executed count into nsteps) or mw_step_plan's (horizon > 0: `actions` is the plans,
// [horizon][N], and each sub-step's own reward goes to step_reward; with `trace`, mw_step_plan_trace's: the trace kernels store each
// sub-step's row of it) — the same launch shape for all of them.  A render has no actions
// and no outputs.  reward, term and trunc are never null behind resolve_outputs: everything downstream reads them as they stand.
struct Call {
    const int32_t *actions = nullptr;
    uint8_t *obs = nullptr; float *depth = nullptr;
    float *reward = nullptr; uint8_t *term = nullptr, *trunc = nullptr;
    hipStream_t st = nullptr;
    int repeat = 0; int32_t *nsteps = nullptr;
    int horizon = 0; float *step_reward = nullptr;
    const mw_plan_trace *trace = nullptr;
};
// the one place where the outputs a caller did not ask for get the engine's scratch (step_frames, the entry point of every step)
void resolve_outputs(const mw_engine *e, Call &c)
{
    if (!c.reward) c.reward = e->d_reward_scratch;
    if (!c.term) c.term = e->d_flag_scratch;
    if (!c.trunc) c.trunc = e->d_flag_scratch + e->cfg.num_envs;
}

// the push of the rows of `obs` behind a step's last raster kernel (step: its call — term, trunc: what the step kernel wrote), or the
// refresh (step = null)
int launch_stack(mw_engine *e, const uint8_t *obs, hipStream_t st, const Call *step)
{
    auto &s = e->stack;
    const bool push = step != nullptr;
    const int N = e->cfg.num_envs, phase = push ? (int)(s.pushes % s.depth) : stack_phase_of(e);
    const ResetMode r = reset_mode(e->cfg.generator, e->cfg.autoreset);
    const uint8_t *final_obs = push && r.same && s.final_stack ? e->final_obs : nullptr;
    uint8_t *final_stack = final_obs ? s.final_stack : nullptr;
    const StackLaunch l = stack_launch((uintptr_t)obs | (uintptr_t)s.ring | (uintptr_t)final_obs | (uintptr_t)final_stack, s.frame_bytes);
    const dim3 grid(N, l.chunks);
    const uint8_t *in = stack_flags(e, s.cur);
    uint8_t *out = stack_flags(e, s.cur ^ 1);
    if (push)
        hipLaunchKernelGGL(mw_stack_push_kernel, grid, dim3(MW_STACK_THREADS), 0, st, s.depth, s.pad, phase, (unsigned long long)s.frame_bytes, (int)l.wide,
                           obs, s.ring, in, out, r.same ? (const uint8_t *)step->term : nullptr, r.same ? (const uint8_t *)step->trunc : nullptr,
                           r.next ? (const uint8_t *)e->args.reset_pending : nullptr, final_obs, final_stack);
    else
        hipLaunchKernelGGL(mw_stack_refresh_kernel, grid, dim3(MW_STACK_THREADS), 0, st, s.depth, s.pad, phase, (unsigned long long)s.frame_bytes, (int)l.wide,
                           obs, s.ring, in, out);
    HIP_TRY(e, hipGetLastError());
    s.cur ^= 1;
    if (push) ++s.pushes;
    return MW_OK;
}

RasterPath raster_path_of(const mw_engine *e, bool depth)
{
    const MwArgs &a = e->args;
    return raster_path({e->cfg.msaa, a.W, a.H, e->have_meshes, a.rec_order != nullptr, e->use_k2q, e->generic_raster, e->k2q_ok, e->obs_layout, e->dbg_flags}, depth);
}

}  // namespace

// Fills mw_engine::MeshPath: everything a frame with mesh entities needs beyond the triangle records — the plane cache (one record
// per mesh triangle that can be in view: the geometry kernel admits 0xC000 per env), the sample keys of the tiles a mesh can touch,
// the slow-path lists, the mesh stream; for the generic-resolution path the view keys.  Called by mw_upload_mesh (a synchronous
// entry point): a frame never allocates, never synchronises.  Failure-atomic: either every buffer of a group is there or none.
int mwhost::ensure_mesh_buffers(mw_engine *e)
{
    const MwArgs &a = e->args; mw_engine::MeshPath &m = e->mp;
    const size_t N = (size_t)e->cfg.num_envs;
    // the stream of the raster kernel's first part in a frame with meshes: LOW priority — the mesh kernels on the caller's stream are the
    // critical path, the quad kernel fills the CUs around them
    if (!m.quad_stream) HIP_TRY(e, make_stream(m.quad_stream));
    for (Event *ev : {&m.ev_fork, &m.ev_join}) if (!*ev) HIP_TRY(e, make_event(*ev));
    if (raster_path_of(e, false).path == MW_PATH_GENERIC)
        return grow(e, m.view_keys, m.view_keys_bytes, N * a.W * a.H * e->cfg.msaa * 4, 1);
    if (a.W > 255 * MW_TILE_W || a.H > 255 * MW_TILE_H) return fail(e, MW_E_CAPACITY, "frame too large for the mesh tile rectangles");
    // the mesh tiles' work list (mw_geom.hip): a tile index in the 8 bits above the env, and one bit of a lane's 32-bit mask per tile
    // sub + k L.  tile_path_ok caps these frames at 192 tiles and the geometry kernel has at least 8 lanes per env, so
    // this holds today; a larger frame limit or fewer lanes must not leave mesh tiles undrawn (and their sample keys uncleared) in silence
    if (a.n_tiles > 255 || a.n_tiles > 32 * geom_lanes_of(e))
        return fail(e, MW_E_CAPACITY, "%d tiles per frame: the mesh tiles' work list holds 255 (8-bit tile index) and 32 per lane of the geometry kernel (%d lanes)", a.n_tiles, geom_lanes_of(e));
    const long long want = std::min<long long>(0xC000, (long long)e->cfg.max_ents * e->max_mesh_tris);
    int rc;
    if ((rc = grow(e, m.plane_cache, m.plane_cap, (int)want, N * (MW_PLANE_REC + MW_PLANE_XTRA) * 4))) return rc;
    if (!m.ent_list) {
        // (all three work lists or none)
        const int cap = (int)N * std::min(MW_MAX_MESH_ENTS, std::max(e->cfg.max_ents, 1));
        DevBuf<uint32_t> ents, slow, tiles;
        if ((rc = dev_alloc(e, ents, (size_t)cap * 16, false)) || (rc = dev_alloc(e, slow, N * 2, false)) ||
            (rc = dev_alloc(e, tiles, N * (size_t)a.n_tiles * 8, false)))
            return rc;
        m.ent_list_cap = cap;
        m.ent_list = std::move(ents); m.slow_envs = std::move(slow); m.tile_list = std::move(tiles);
    }
    if (!m.keys) {
        const size_t px = N * a.W * a.H;
        DevBuf<uint32_t> keys, tris, head; DevBuf<int32_t> cnt; DevBuf<float4> frags;
        // triangles that cross a frustum plane and their fragments (mw_mesh_slow_kernel): counts, 1024 / 2048 entries per env
        if ((rc = dev_alloc(e, keys, px * 8, false)) || (rc = dev_alloc(e, cnt, N * 4 + 2 * MW_CNT_WORDS)) ||
            (rc = dev_alloc(e, tris, N * MW_SLOW_TRIS, false)) || (rc = dev_alloc(e, frags, N * MW_SLOW_STRIDE, false)) ||
            (rc = dev_alloc(e, head, px)))
            return rc;
        HIP_TRY(e, hipMemset(keys.get(), 0xFF, px * 8 * 4));
        m.ent_counter = cnt.get() + N * 4;          // (behind the slow path's counts)
        m.keys = std::move(keys); m.slow_count = std::move(cnt); m.slow_tris = std::move(tris);
        m.slow_frags = std::move(frags); m.slow_head = std::move(head);
        // (the memsets above ran on the null stream, which a caller's non-blocking stream is not ordered against: finish them here)
        (void)hipDeviceSynchronize();
        m.keys_dirty = false;
    }
    return MW_OK;
}

namespace {

// This frame's side of the mesh path's double-buffered lists: the work lists' counters, the slow-path lists and the fragment stamps
// alternate between two sets from frame to frame (the entity kernel zeroes the next frame's counters).  Every parity offset is here.
struct MeshFrame {
    uint32_t stamp;                 // frame stamp of the slow-fragment chains: the sequence number's low 16 bits
    int parity;                     // (the slow kernel indexes slow_count itself)
    int32_t *cnt, *cnt_next, *slow_count;   // [MW_CNT_WORDS] this frame's lengths and cursors of the work lists, the next frame's; [2][N] this frame's listed triangles, fragments
    uint32_t *slow_envs;            // [N] this frame's envs with slow-path triangles: cnt[MW_CNT_SLOW_ENVS] of them
};
MeshFrame mesh_frame(mw_engine::MeshPath &m, size_t N)
{
    const uint32_t seq = m.frame_seq++;         // (the next frame through the lists)
    const int parity = (int)(seq & 1u);
    return {seq & 0xFFFFu, parity, m.ent_counter + parity * MW_CNT_WORDS, m.ent_counter + (parity ^ 1) * MW_CNT_WORDS,
            m.slow_count.get() + (size_t)parity * 2 * N, m.slow_envs.get() + (size_t)parity * N};
}

// what the stages of one frame share (launch_frame)
struct Frame {
    MwArgs a;
    int view_flags;
    const int32_t *list;        // CALL_LIST_PASS: the list forms draw the listed envs only
    uint8_t *obs; float *depth; hipStream_t st;
    FramePolicy pol;            // reuse; cache: the frame consults and fills the frame cache (both through the frame plan on the quad path: frame_plans)
    bool plans;                 // the plan kernel runs behind the geometry kernel (frame_plans)
    RasterPath p;
    MeshFrame mf;               // p.mesh only
};

// the Maze's spare worlds are refilled on the side stream behind a step (launch_side_refill), not by blocks of the step kernel
bool side_refills(const mw_engine *e) { return e->spare_mode && e->cfg.generator == MW_GEN_MAZE; }

// the step kernel (frameless: of an mw_step_plan that no frame follows)
void launch_k1(mw_engine *e, const MwArgs &ak, const Call &c, bool frameless)
{
    const int N = e->cfg.num_envs;
    // spare mode: blocks appended to the grid regenerate the spare worlds consumed in earlier steps, beside the step itself
    const int refill_blocks = (e->spare_mode && !side_refills(e)) ? (N + 63) / 64 : 0;
    const int lanes = dense_lanes_of(e);
    const dim3 grid(env_blocks(N, lanes) + refill_blocks);
    if (c.horizon > 0 && c.trace)
        hipLaunchKernelGGL(MW_K1(e, lanes, mw_step_trace), grid, dim3(64), 0, c.st, ak, lanes, c.actions, c.reward, c.term, c.trunc, c.horizon, c.nsteps, c.step_reward,
                           frameless ? 1 : 0, *c.trace);
    else if (c.horizon > 0)
        hipLaunchKernelGGL(MW_K1(e, lanes, mw_step_plan), grid, dim3(64), 0, c.st, ak, lanes, c.actions, c.reward, c.term, c.trunc, c.horizon, c.nsteps, c.step_reward,
                           frameless ? 1 : 0);
    else if (c.repeat > 0) hipLaunchKernelGGL(MW_K1(e, lanes, mw_step_repeat), grid, dim3(64), 0, c.st, ak, lanes, c.actions, c.reward, c.term, c.trunc, c.repeat, c.nsteps);
    else hipLaunchKernelGGL(MW_K1(e, lanes, mw_step_setup), grid, dim3(64), 0, c.st, ak, lanes, c.actions, c.reward, c.term, c.trunc);
}

// the step (a render or a list pass has none), the list of a terminal step's finished envs, the frame's vertex half, CollectHealth's respawns
void launch_step_and_geometry(mw_engine *e, const Frame &f, const Call &c, CallKind kind)
{
    const MwArgs &a = f.a; const int N = e->cfg.num_envs;
    if (call_steps(kind)) {
        MwArgs ak = a;          // the step kernel's arguments: the first pass of a final-observation step runs as a next-step terminal step
        if (kind == CALL_TERMINAL_STEP) ak.autoreset = MW_AUTORESET_NEXT_STEP;
        launch_k1(e, ak, c, false);
    }
    if (kind == CALL_TERMINAL_STEP)
        hipLaunchKernelGGL(mw_final_list_kernel, dim3(1), dim3(1024), 0, f.st, N, (const uint8_t *)a.reset_pending, a.pending_remove, e->d_final_list);
    // the frame's vertex half: camera, lighting, transform, clipping, triangle setup (mw_geom.hip)
    // ... of the envs the plan will have drawn only, dealt evenly over the wavefronts, where a plan kernel follows (mw_kernels.h: MW_GEOM_DEAL)
    const int L = geom_lanes_of(e);
    const bool deals = geom_deals(f.plans, e->geom_deal, L);
    const int flags = f.view_flags | (deals ? MW_GEOM_DEAL | (f.pol.reuse ? MW_GEOM_REUSE : 0) : 0);
    launch(geom_kernel_of(L, e->cfg.msaa), f.list, dim3(env_blocks(N, L)), dim3(64), 0, f.st, a, flags, e->cfg.msaa, L, N,
           deals && f.pol.cache ? (const uint64_t *)e->fc.meta.get() : nullptr, deals && f.pol.cache ? e->fc.slots : 0, e->d_geom_built);
    if (call_steps(kind) && e->cfg.task == MW_TASK_COLLECT)
        hipLaunchKernelGGL(MW_BY_STREAM(e, mw_collect_respawn), dim3((N + 63) / 64), dim3(64), 0, f.st, a);
}

// The Maze's spare worlds: regenerating one takes ~300 us on a single wave, four times a whole step of the batch, and any launch
// that carries such a block lasts that long.  Its refills go to a kernel of their own on the low-priority side stream, running
// beside this and the next steps; nothing waits for it but the entry points that touch the worlds from the host
// (ON_DEVICE_SYNC) — an env that needs its spare earlier follows the refill_mask protocol.
int launch_side_refill(mw_engine *e, hipStream_t st)
{
    if (!e->side_stream) HIP_TRY(e, make_stream(e->side_stream));
    if (!e->ev_fork) HIP_TRY(e, make_event(e->ev_fork));
    HIP_TRY(e, hipEventRecord(e->ev_fork.get(), st));
    HIP_TRY(e, hipStreamWaitEvent(e->side_stream.get(), e->ev_fork.get(), 0));
    hipLaunchKernelGGL(MW_BY_STREAM(e, mw_refill), dim3(e->cfg.num_envs), dim3(64), 0, e->side_stream.get(), e->args);
    e->side_refill_pending = true;
    return MW_OK;
}

// The generic-resolution path (mw_raster_mesh.hip) over `count` envs from first_env, or over the envs of a list, at a.W x a.H and
// S samples: with meshes resident the view keys are cleared and the mesh triangles scattered into them (mesh_grid), then the
// raster kernel — frames off the 16 x 4 grid and the wrapper layouts take its "any" form (mw_raster_view_any.hip).
int launch_generic(mw_engine *e, const MwArgs &a, int first_env, int count, int S, dim3 mesh_grid, uint8_t *out, float *depth,
                   int layout, const int32_t *list, hipStream_t st)
{
    uint32_t *keys = nullptr;
    if (e->have_meshes) {
        const size_t need = (size_t)count * a.W * a.H * S * 4;
        if (need > e->mp.view_keys_bytes) return fail(e, MW_E_INVALID, "view keys missing (mw_upload_mesh allocates them)");
        keys = e->mp.view_keys.get();
        HIP_TRY(e, hipMemsetAsync(keys, 0xFF, need, st));
        launch(MW_PAIR(mw_view_mesh), list, mesh_grid, dim3(256), 0, st, a.W, a.H, S, first_env, (const float *)a.envhdr, a.mesh_pos, keys);
    }
    const bool any = !frame_on_grid(a.W, a.H) || layout != MW_OBS_HWC_U8;
    launch(any ? MW_PAIR(mw_view_raster_any) : MW_PAIR(mw_view_raster), list, dim3(a.n_tiles, count), dim3(64), 0, st, first_env, a.W, a.H, S,
           a.max_vis, a.tiles_x, (const float *)a.rec_raster, (const float *)a.rec_shade, (const float *)a.rec_cull, (const int32_t *)a.nvis,
           (const float *)a.envhdr, a.tex, a.texels, a.mesh_pos, a.mesh_nrm, a.mesh_rgb, a.mesh_uv, keys, out, depth, e->texel_bytes, layout);
    return MW_OK;
}

// the quad kernel (mw_rasterq.hip); part: raster_flags.  plan: the block the plan kernel filled for this frame (launch_plan), or null —
// then every env is drawn, and the cache is neither consulted nor filled
void launch_quad(const mw_engine *e, const Frame &f, int part, hipStream_t st, const uint32_t *plan = nullptr)
{
    const MwArgs &a = f.a;
    const int lds = mw_rasterq_lds_bytes(e->cfg.msaa, a.W, a.H, a.n_tiles, f.depth ? 1 : 0);
    launch(f.p.quad4 ? MW_PAIR(mw_rasterq4) : MW_PAIR(mw_rasterq), f.list, dim3(e->cfg.num_envs), dim3(MWQ_THREADS), (size_t)lds, st, a.N, a.W, a.H, a.max_vis,
           a.tiles_x, a.n_tiles, (const float *)a.rec_raster, (const float *)a.rec_shade, (const float *)a.rec_cull,
           (const int32_t *)a.nvis, (const float *)a.envhdr, a.texels, f.obs, f.depth, raster_flags(e->dbg_flags, e->obs_layout, part, 0u, false), e->texel_bytes, e->d_k2q_prof,
           plan && f.pol.cache ? (const MwFcArgs *)e->fc.d_args.get() : nullptr, plan);
}

// The frame plan of a plain whole-batch step through the quad kernel (frame_plans), behind the geometry kernel on the caller's stream: which envs
// the quad kernel draws, which it copies from the cache, which it leaves.  Returns the block it filled.
const uint32_t *launch_plan(mw_engine *e, const Frame &f, hipStream_t st)
{
    const MwArgs &a = f.a; const int N = e->cfg.num_envs;
    uint32_t *plan = e->d_plan[e->plan_cur], *next = e->d_plan[e->plan_cur ^ 1];
    e->plan_cur ^= 1;
    e->plan_made = true;
    hipLaunchKernelGGL(mw_frame_plan_kernel, dim3((N + MW_PLAN_ENVS - 1) / MW_PLAN_ENVS), dim3(64), 0, st, N, f.pol.reuse ? 1 : 0, (const uint8_t *)a.frame_clean,
                       (const uint64_t *)a.fc_key, f.pol.cache ? (const uint64_t *)e->fc.meta.get() : nullptr, f.pol.cache ? e->fc.slots : 0,
                       frame_plan_ordered(N) ? (const int32_t *)a.nvis : nullptr, a.fc_source, plan, next);
    return plan;
}

// the tile kernels (mw_raster.hip); part: raster_flags
void launch_tiles(const mw_engine *e, const Frame &f, int part, hipStream_t st)
{
    const MwArgs &a = f.a; const mw_engine::MeshPath &m = e->mp;
    const TileLaunch t = tile_launch(part, a.tile_list != nullptr, f.p.big, a.max_vis, a.n_tiles, e->waves_per_env, e->cfg.num_envs, m.mesh_tile_waves);
    launch(tile_kernel_of(f.p.big, f.p.depth, f.p.general, f.p.ragged, f.p.mesh, t.part == 1), f.list, dim3(t.grid), dim3(64), t.lds, st,
           a.N, a.W, a.H, a.max_vis, a.tiles_x, a.n_tiles, t.waves_per_env, t.tiles_per_wave, (const float *)a.rec_raster, (const float *)a.rec_shade,
           (const float *)a.rec_cull, (const int32_t *)a.nvis, (const float *)a.envhdr, a.tex, a.texels, f.obs, f.depth, raster_flags(e->dbg_flags, e->obs_layout, t.part, f.mf.stamp, f.pol.reuse),
           e->texel_bytes, (const uint16_t *)a.rec_order, a.mesh_pos, a.mesh_nrm, a.mesh_rgb, a.mesh_uv, m.keys.get(),
           (const float *)m.plane_cache.get(), m.plane_cap, (const float4 *)m.slow_frags.get(), (const uint32_t *)m.slow_head.get(),
           (const uint32_t *)a.tile_list, a.ent_list_n, a.tile_list_cap, std::max(a.n_xcc, 1), (const uint8_t *)a.frame_clean);
}

// A frame with mesh entities through the tile / quad kernels, behind the geometry kernel: the mesh kernels, the raster kernel's
// first part beside them on the quad stream, its second part behind both.
int launch_mesh_chain(mw_engine *e, const Frame &f, hipStream_t st)
{
    const MwArgs &a = f.a; const MeshFrame &mf = f.mf;
    mw_engine::MeshPath &m = e->mp; const int N = e->cfg.num_envs;
    // (plane cache, sample keys — all-ones between frames, K2 clears what it reads —, slow-path lists, mesh stream:
    // ensure_mesh_buffers, at upload time)
    if (!m.keys || !m.plane_cache || !m.quad_stream) return fail(e, MW_E_INVALID, "mesh buffers missing (mw_upload_mesh allocates them)");
    if (m.keys_dirty) HIP_TRY(e, hipMemsetAsync(m.keys.get(), 0xFF, (size_t)N * a.W * a.H * 8 * 4, st));
    m.keys_dirty = true;        // until the raster kernel that clears them again has been enqueued
    // The stamp has 16 bits: a head that no frame has overwritten since frame F would read as valid again at frame F + 65536 (24 s
    // of PickupObjects), so the heads are wiped on the frame whose stamp is 0 — behind the previous frame's readers, before this
    // frame's slow-path kernel, in stream order (tests/test_gpu_env_api.py::test_slow_fragment_heads_survive_the_stamp_wrap)
    if (mf.stamp == 0u) HIP_TRY(e, hipMemsetAsync(m.slow_head.get(), 0, (size_t)N * a.W * a.H * 4, st));
    // The mesh kernels — the frame's critical path — stay on the caller's stream, right behind the geometry kernel; the quad
    // kernel, which draws every tile no mesh can touch, goes to the low-priority quad stream beside them.  (The other way
    // round — mesh kernels on a side stream — the quad kernel started a few microseconds EARLIER, its 2 048 workgroups
    // took the CUs, and the entity kernel's workgroups waited a quad-kernel workgroup's lifetime for room: 212 instead of
    // 133 us, PickupObjects 4.55 -> 5.3 M env-steps/s.)
    HIP_TRY(e, hipEventRecord(m.ev_fork.get(), st));
    HIP_TRY(e, hipStreamWaitEvent(m.quad_stream.get(), m.ev_fork.get(), 0));
    // persistent workgroups drawing entities from the geometry kernel's list (two sets of counters swapping places: the
    // kernel zeroes the next frame's)
    hipLaunchKernelGGL(mw_mesh_entity_kernel, dim3(std::max(a.n_xcc, std::min(m.ent_list_cap, m.ent_blocks))), dim3(MW_ENT_THREADS), (size_t)e->max_mesh_verts * 16, st, N, a.W, a.H,
                       (const float *)a.envhdr, a.mesh, (const float4 *)e->pools.vpos.get(), (const uint2 *)e->pools.idx.get(), (const float *)e->pools.stream.get(),
                       (const float *)e->pools.attr.get(), m.keys.get(), m.plane_cache.get(), m.plane_cap, mf.slow_count, m.slow_tris.get(),
                       (const uint32_t *)m.ent_list.get(), m.ent_list_cap, mf.cnt, mf.cnt_next, mf.slow_envs, e->args.n_xcc, e->d_ent_prof);
    hipLaunchKernelGGL(mw_mesh_slow_kernel, dim3(std::min(N * 16, m.slow_waves)), dim3(64), 0, st, a.W, a.H, (const float *)a.envhdr, a.mesh_pos, a.mesh_nrm, a.mesh_rgb,
                       a.mesh_uv, a.texels, e->texel_bytes, m.keys.get(), m.slow_count.get(), N, mf.parity, (const uint32_t *)m.slow_tris.get(),
                       m.slow_frags.get(), m.slow_head.get(), mf.stamp, a.status,
                       (const uint32_t *)mf.slow_envs, (const int32_t *)(mf.cnt + MW_CNT_SLOW_ENVS));
    // the first part — every tile no mesh can touch: it needs nothing of the mesh kernels — on the quad stream beside them
    // (forked above, behind the geometry kernel); the mesh tiles end the chain on the caller's stream
    if (f.p.path == MW_PATH_QUAD_MESH) launch_quad(e, f, 1, m.quad_stream.get()); else launch_tiles(e, f, 1, m.quad_stream.get());
    launch_tiles(e, f, 2, st);
    HIP_TRY(e, hipEventRecord(m.ev_join.get(), m.quad_stream.get()));
    HIP_TRY(e, hipStreamWaitEvent(st, m.ev_join.get(), 0));
    m.keys_dirty = false;
    return MW_OK;
}

// the three events of a timed frame
mw_engine::Ev get_events(mw_engine *e)
{
    if (!e->ev_free.empty()) {
        mw_engine::Ev ev = std::move(e->ev_free.back());
        e->ev_free.pop_back();
        return ev;
    }
    mw_engine::Ev ev;
    for (Event *x : {&ev.a, &ev.b, &ev.c}) (void)make_event(*x, hipEventDefault);
    return ev;
}

// One frame of the whole batch (or, CALL_LIST_PASS, of the listed envs) into c.obs / c.depth, behind the step kernel where the call
// has one.  What the frame may reuse, cache and hold: frame_policy (mw_policy.h).
int launch_frame(mw_engine *e, const Call &c, CallKind kind, int view_flags = 0)
{
    if (!c.obs) return fail(e, MW_E_INVALID, "d_obs is null");
    uint8_t *const d_obs = c.obs; float *const d_depth = c.depth; const hipStream_t st = c.st;
    const RasterPath path = raster_path_of(e, d_depth != nullptr);
    const bool held_match = e->held.valid && e->held.obs == d_obs && e->held.depth == d_depth && e->held.layout == e->obs_layout;
    const FramePolicy pol = frame_policy({kind, view_flags, e->frame_reuse, held_match, e->have_meshes, e->dbg_flags, e->obs_layout, e->cfg.task,
                                          e->fc.slots > 0 && e->fc.frames, path.path, e->reset_seeds != nullptr});
    frames_stale(e);
    const int N = e->cfg.num_envs;
    Frame f{e->args, view_flags, kind == CALL_LIST_PASS ? e->d_final_list : nullptr, d_obs, d_depth, st, pol, false, path, {}};
    f.plans = frame_plans(pol, path.path, f.list != nullptr, N);
    if (pol.cache) {
        if (d_depth && !e->fc.depth) {
            if (const int rc = dev_alloc(e, e->fc.depth, (size_t)N * e->fc.slots * f.a.W * f.a.H, false)) return rc;
            e->fc.args_stale = true;
        }
        if ((d_depth != nullptr) != e->fc.with_depth) { e->fc.with_depth = d_depth != nullptr; e->fc.dirty = true; }
        if (e->fc.args_stale) {
            // (the buffers are new: no frame that is still running reads the block)
            e->fc.args = MwFcArgs{f.a.fc_key, e->fc.meta.get(), e->fc.frames.get(), e->fc.depth.get(), e->fc.slots, 0};
            HIP_TRY(e, hipMemcpyAsync(e->fc.d_args.get(), &e->fc.args, sizeof(MwFcArgs), hipMemcpyHostToDevice, st));
            e->fc.args_stale = false;
            e->fc.dirty = true;
        }
        if (e->fc.dirty) {
            HIP_TRY(e, hipMemsetAsync(e->fc.meta.get(), 0, (size_t)N * MW_FC_META_WORDS(e->fc.slots) * 8, st));
            e->fc.dirty = false;
        }
    }
    f.a.step_override = e->use_step_override ? e->d_step_override : nullptr;
    // a frame with mesh entities through the tile / quad kernels: the geometry kernel lists the entities in view for the mesh
    // entity kernel and the tiles a mesh can touch for the raster kernel's second part
    if (f.p.mesh && e->mp.ent_list && e->mp.keys) {
        f.mf = mesh_frame(e->mp, (size_t)N);
        f.a.ent_list = e->mp.ent_list.get(); f.a.ent_list_n = f.mf.cnt; f.a.ent_list_cap = e->mp.ent_list_cap;
        f.a.tile_list = e->mp.tile_list.get(); f.a.tile_list_cap = N * f.a.n_tiles;
    }
    mw_engine::Ev ev{};
    // kernel durations are sampled: three event records on every launch cost ~4 % of the step rate,
    // on one launch in MW_TIMING_STRIDE they cost nothing measurable
    // (the second pass of a final-observation step is no frame of its own here)
    const bool timed = kind != CALL_LIST_PASS && e->timing && (e->frame_count++ % (uint64_t)e->timing_stride) == 0;
    if (timed) {
        ev = get_events(e);
        (void)hipEventRecord(ev.a.get(), st);
    }
    launch_step_and_geometry(e, f, c, kind);
    if (timed) (void)hipEventRecord(ev.b.get(), st);
    int rc = MW_OK;
    if (call_steps(kind) && side_refills(e) && (rc = launch_side_refill(e, st))) return rc;
    if (f.p.path == MW_PATH_GENERIC) rc = launch_generic(e, f.a, 0, N, e->cfg.msaa, dim3(32, N), d_obs, d_depth, e->obs_layout, f.list, st);
    else if (f.p.mesh) rc = launch_mesh_chain(e, f, st);
    else if (f.p.path == MW_PATH_QUAD) launch_quad(e, f, 0, st, f.plans ? launch_plan(e, f, st) : nullptr);
    else launch_tiles(e, f, 0, st);
    if (rc) return rc;
    e->last_raster_path = f.p.path;
    if (timed) {
        (void)hipEventRecord(ev.c.get(), st);
        e->ev_used.push_back(std::move(ev));
    }
    HIP_TRY(e, hipGetLastError());
    if (pol.hold) e->held = {d_obs, d_depth, e->obs_layout, true};
    return MW_OK;
}

}  // namespace

extern "C" {

// the frames of one call: one, or the two passes of a same-step step with final observations or reset seeds (mw_policy.h: step_passes_of)
static int step_passes(mw_engine *e, const Call &c, const StepPasses &p)
{
    if (p.shape == STEP_ONE_PASS) return launch_frame(e, c, CALL_STEP);
    // Same-step auto-reset in two passes.  1: the step as the next-step mode's terminal step — physics, rule, reward, flags, final
    // info, per-step draws; the finished envs keep their terminal state — and the frame of every env.  With final buffers the finished
    // envs' rows go there.  2: they install their next world — the same install code and stream order as the plain same-step step
    // (the step's draws, then the reset's), or with reset seeds the world of the env's seed on a stream seeded here —, and the frame
    // of those envs alone overwrites their rows.
    const int N = e->cfg.num_envs;
    if (const int rc = launch_frame(e, c, CALL_TERMINAL_STEP)) return rc;
    if (p.final_copy)
        hipLaunchKernelGGL(mw_final_copy_kernel, dim3(N), dim3(256), 0, c.st, (const int32_t *)e->d_final_list, (const uint8_t *)c.obs, e->final_obs,
                           (unsigned long long)frame_bytes_of(e), (const float *)c.depth, e->final_depth, e->cfg.obs_width * e->cfg.obs_height);
    if (p.seeded_install)
        hipLaunchKernelGGL(MW_BY_STREAM(e, mw_seed_install), dim3(N), dim3(64), 0, c.st, e->args, (const int32_t *)e->d_final_list,
                           e->reset_seeds);
    else
        hipLaunchKernelGGL(MW_BY_STREAM(e, mw_final_install), dim3(N), dim3(64), 0, c.st, e->args, (const int32_t *)e->d_final_list);
    return launch_frame(e, c, CALL_LIST_PASS);
}

// A frameless mw_step_plan: the step kernel in the engine's own auto-reset mode — it applies the frame's tail behind the last executed
// sub-step itself —, the Maze's side-stream refill where a drawn call has one, and the stack's flag bytes.  No geometry kernel, no
// raster, no respawn kernel, no push, no final-buffer pass; nothing is timed.  The buffers that frame reuse holds no longer show the
// envs' states; the frame cache is neither read nor filled and stays valid (the epochs part what the call changed).
static int step_frameless(mw_engine *e, const Call &c)
{
    frames_stale(e);
    const int N = e->cfg.num_envs;
    MwArgs a = e->args;
    a.step_override = e->use_step_override ? e->d_step_override : nullptr;
    launch_k1(e, a, c, true);
    if (side_refills(e))
        if (const int rc = launch_side_refill(e, c.st)) return rc;
    if (e->stack.depth) {
        const ResetMode r = reset_mode(e->cfg.generator, e->cfg.autoreset);
        hipLaunchKernelGGL(mw_stack_plan_kernel, dim3((N + 255) / 256), dim3(256), 0, c.st, N, r.same ? (const uint8_t *)c.term : nullptr,
                           r.same ? (const uint8_t *)c.trunc : nullptr, r.next ? (const uint8_t *)e->args.reset_pending : nullptr, stack_flags(e, e->stack.cur));
    }
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

// mw_step (the plain step kernels), mw_step_repeat (the repeat kernels), mw_step_plan and mw_step_plan_trace (the plan and the trace
// kernels; c.actions: the plans)
static int step_frames(mw_engine *e, const char *what, Call c)
{
    ON_DEVICE(e);
    if (!c.actions) return fail(e, MW_E_INVALID, "%s: %s is null", what, c.horizon ? "d_plans" : "d_actions");
    if ((e->cfg.generator == MW_GEN_PROGRAM || e->cfg.task >= MW_TASK_SIDEWALK) && !e->args.prog)
        return fail(e, MW_E_INVALID, "no placement program installed (mw_set_gen_program)");
    const StepPasses p = step_passes_of(e->reset_seeds != nullptr, e->final_obs != nullptr, c.horizon && !c.obs);
    if (p.shape == STEP_REFUSED)
        return fail(e, MW_E_INVALID, "%s: a frameless call while reset seeds are set (mw_set_reset_seeds): the step kernel cannot seed the finished envs", what);
    resolve_outputs(e, c);
    if (p.shape == STEP_FRAMELESS) return step_frameless(e, c);
    if (const int rc = stack_check(e, what)) return rc;
    const int rc = step_passes(e, c, p);
    if (rc != MW_OK || !e->stack.depth) return rc;
    return launch_stack(e, c.obs, c.st, &c);     // the call's one push, behind its last raster kernel
}

int mw_step(mw_engine *e, const int32_t *d_actions, uint8_t *d_obs, float *d_depth, float *d_reward,
            uint8_t *d_term, uint8_t *d_trunc, void *stream)
{
    if (!e) return MW_E_INVALID;
    return step_frames(e, "mw_step", Call{d_actions, d_obs, d_depth, d_reward, d_term, d_trunc, (hipStream_t)stream});
}

int mw_step_repeat(mw_engine *e, const int32_t *d_actions, int32_t repeat, uint8_t *d_obs, float *d_depth, float *d_reward,
                   uint8_t *d_term, uint8_t *d_trunc, int32_t *d_nsteps, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (repeat < 1 || repeat > MW_MAX_REPEAT) return fail(e, MW_E_INVALID, "mw_step_repeat: repeat %d outside 1 .. %d", (int)repeat, MW_MAX_REPEAT);
    return step_frames(e, "mw_step_repeat", Call{d_actions, d_obs, d_depth, d_reward, d_term, d_trunc, (hipStream_t)stream, repeat, d_nsteps});
}

int mw_step_plan(mw_engine *e, const int32_t *d_plans, int32_t horizon, uint8_t *d_obs, float *d_depth, float *d_reward,
                 float *d_step_reward, uint8_t *d_term, uint8_t *d_trunc, int32_t *d_nsteps, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (horizon < 1 || horizon > MW_MAX_PLAN) return fail(e, MW_E_INVALID, "mw_step_plan: horizon %d outside 1 .. %d", (int)horizon, MW_MAX_PLAN);
    if (d_depth && !d_obs) return fail(e, MW_E_INVALID, "mw_step_plan: d_depth without d_obs (a frameless call draws nothing)");
    return step_frames(e, "mw_step_plan", Call{d_plans, d_obs, d_depth, d_reward, d_term, d_trunc, (hipStream_t)stream, 0, d_nsteps, horizon, d_step_reward});
}

int mw_step_plan_trace(mw_engine *e, const int32_t *d_plans, int32_t horizon, uint8_t *d_obs, float *d_depth, float *d_reward,
                       float *d_step_reward, uint8_t *d_term, uint8_t *d_trunc, int32_t *d_nsteps, const mw_plan_trace *trace, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (horizon < 1 || horizon > MW_MAX_PLAN) return fail(e, MW_E_INVALID, "mw_step_plan_trace: horizon %d outside 1 .. %d", (int)horizon, MW_MAX_PLAN);
    if (d_depth && !d_obs) return fail(e, MW_E_INVALID, "mw_step_plan_trace: d_depth without d_obs (a frameless call draws nothing)");
    if (!trace || !(trace->agent_pos || trace->agent_dir || trace->carrying || trace->ent_pos))
        return fail(e, MW_E_INVALID, "mw_step_plan_trace: no trace field asked for (mw_step_plan is the call without a trace)");
    if (trace->ent_pos && (trace->ent_slot < 0 || trace->ent_slot >= e->cfg.max_ents))
        return fail(e, MW_E_INVALID, "mw_step_plan_trace: ent_slot %d outside 0 .. %d", (int)trace->ent_slot, (int)e->cfg.max_ents - 1);
    if (trace->ent_pos && e->cfg.task == MW_TASK_COLLECT)
        return fail(e, MW_E_INVALID, "mw_step_plan_trace: ent_pos on a MW_TASK_COLLECT engine (a kit's respawn belongs to the frame's tail: where it is "
                                     "after a sub-step depends on whether a frame follows)");
    Call c{d_plans, d_obs, d_depth, d_reward, d_term, d_trunc, (hipStream_t)stream, 0, d_nsteps, horizon, d_step_reward};
    c.trace = trace;
    return step_frames(e, "mw_step_plan_trace", c);
}

int mw_set_final_obs(mw_engine *e, uint8_t *d_final_obs, float *d_final_depth)
{
    if (!e) return MW_E_INVALID;
    if (e->cfg.autoreset != MW_AUTORESET_SAME_STEP)
        return fail(e, MW_E_INVALID, "mw_set_final_obs: final observations exist in MW_AUTORESET_SAME_STEP only (next-step returns the terminal frame itself)");
    if (e->cfg.generator == MW_GEN_NONE)
        return fail(e, MW_E_INVALID, "mw_set_final_obs: MW_GEN_NONE engines auto-reset nothing (the returned frame is the terminal one)");
    frames_stale(e);
    e->final_obs = d_final_obs;
    e->final_depth = d_final_obs ? d_final_depth : nullptr;
    return MW_OK;
}

int mw_set_reset_seeds(mw_engine *e, const uint64_t *d_next_seed)
{
    if (!e) return MW_E_INVALID;
    if (e->cfg.autoreset != MW_AUTORESET_SAME_STEP)
        return fail(e, MW_E_INVALID, "mw_set_reset_seeds: the seeded auto-reset exists in MW_AUTORESET_SAME_STEP only");
    if (e->cfg.generator == MW_GEN_NONE)
        return fail(e, MW_E_INVALID, "mw_set_reset_seeds: MW_GEN_NONE engines auto-reset nothing (there is no generator to seed)");
    frames_stale(e);        // (the step changes its shape: trust starts with the next whole frame, as for mw_set_final_obs)
    e->reset_seeds = d_next_seed;
    return MW_OK;
}

int mw_set_frame_stack(mw_engine *e, int32_t depth, int32_t pad, uint8_t *d_ring, uint8_t *d_final_stack)
{
    if (!e) return MW_E_INVALID;
    if (depth == 0 || !d_ring) {
        e->stack.depth = 0;
        e->stack.ring = e->stack.final_stack = nullptr;
        return MW_OK;
    }
    if (depth < 2 || depth > MW_MAX_STACK) return fail(e, MW_E_INVALID, "mw_set_frame_stack: depth %d outside 2 .. %d", (int)depth, MW_MAX_STACK);
    if (pad != MW_STACK_PAD_RESET && pad != MW_STACK_PAD_ZERO) return fail(e, MW_E_INVALID, "mw_set_frame_stack: unknown pad mode %d", (int)pad);
    if (d_final_stack && (e->cfg.autoreset != MW_AUTORESET_SAME_STEP || e->cfg.generator == MW_GEN_NONE))
        return fail(e, MW_E_INVALID, "mw_set_frame_stack: final stacks exist where final observations do (MW_AUTORESET_SAME_STEP with a generator)");
    ON_DEVICE(e);
    // every env "never pushed": written behind whatever still runs, and finished before the caller's stream can read it
    HIP_TRY(e, hipDeviceSynchronize());
    HIP_TRY(e, hipMemset(e->stack.flags, MW_STACK_FRESH, 2 * (size_t)e->cfg.num_envs));
    HIP_TRY(e, hipDeviceSynchronize());
    e->stack.depth = depth; e->stack.pad = pad; e->stack.layout = e->obs_layout; e->stack.cur = 0;
    e->stack.ring = d_ring; e->stack.final_stack = d_final_stack;
    e->stack.frame_bytes = frame_bytes_of(e);
    e->stack.pushes = 0;
    return MW_OK;
}

int mw_stack_refresh(mw_engine *e, const uint8_t *d_obs, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (!e->stack.depth) return fail(e, MW_E_INVALID, "mw_stack_refresh: no frame stack set (mw_set_frame_stack)");
    if (!d_obs) return fail(e, MW_E_INVALID, "mw_stack_refresh: d_obs is null");
    if (const int rc = stack_check(e, "mw_stack_refresh")) return rc;
    ON_DEVICE(e);
    return launch_stack(e, d_obs, (hipStream_t)stream, nullptr);
}

int mw_stack_window(const mw_engine *e, int32_t *first_slot, int64_t *pushes)
{
    if (!e || !e->stack.depth) return MW_E_INVALID;
    if (first_slot) *first_slot = stack_phase_of(e);
    if (pushes) *pushes = e->stack.pushes;
    return MW_OK;
}

int mw_render(mw_engine *e, uint8_t *d_obs, float *d_depth, void *stream)
{
    if (!e) return MW_E_INVALID;
    ON_DEVICE(e);
    return launch_frame(e, Call{nullptr, d_obs, d_depth, nullptr, nullptr, nullptr, (hipStream_t)stream}, CALL_RENDER);     // (no actions, no step outputs)
}

int mw_render_top(mw_engine *e, uint8_t *d_obs, float *d_depth, int32_t render_agent, void *stream)
{
    if (!e) return MW_E_INVALID;
    ON_DEVICE(e);
    return launch_frame(e, Call{nullptr, d_obs, d_depth, nullptr, nullptr, nullptr, (hipStream_t)stream}, CALL_RENDER, 1 | (render_agent ? 2 : 0));
}

int mw_render_view(mw_engine *e, int32_t env, int32_t view_flags, int32_t width, int32_t height, int32_t msaa,
                   uint8_t *d_out, float *d_depth, void *stream)
{
    if (!e || !d_out) return fail(e, MW_E_INVALID, "null argument");
    ON_DEVICE(e);
    if (env < 0 || env >= e->cfg.num_envs) return fail(e, MW_E_INVALID, "env %d out of range", env);
    if (msaa != 1 && msaa != 4 && msaa != 8 && msaa != 16) return fail(e, MW_E_INVALID, "msaa must be 1, 4, 8 or 16");
    if (!frame_size_ok(width, height))
        return fail(e, MW_E_INVALID, "frame buffer size %dx%d: 1 to %d x 1 to %d pixels", width, height, 255 * MW_TILE_W, 255 * MW_TILE_H);
    frames_stale(e);        // (d_out may lie inside the held buffers)
    hipStream_t st = (hipStream_t)stream;
    MwArgs b = e->args;
    b.step_override = nullptr;
    b.W = width; b.H = height;
    b.tiles_x = tiles_across(width); b.tiles_y = tiles_down(height); b.n_tiles = b.tiles_x * b.tiles_y;
    b.env_base = env;
    hipLaunchKernelGGL(geom_kernel_of(64, msaa).plain, dim3(1), dim3(64), 0, st, b, view_flags, msaa, 64, 1, (const uint64_t *)nullptr, 0, (uint8_t *)nullptr);
    if (const int rc = e->have_meshes ? grow(e, e->mp.view_keys, e->mp.view_keys_bytes, (size_t)width * height * msaa * 4, 1) : MW_OK) return rc;
    if (const int rc = launch_generic(e, b, env, 1, msaa, dim3(128), d_out, d_depth, MW_OBS_HWC_U8, nullptr, st)) return rc;
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_set_obs_layout(mw_engine *e, int32_t layout)
{
    if (!e) return MW_E_INVALID;
    if (layout != MW_OBS_HWC_U8 && layout != MW_OBS_CWH_U8 && layout != MW_OBS_GREY_F64) return fail(e, MW_E_INVALID, "unknown obs layout %d", layout);
    world_changed(e);
    e->obs_layout = layout;
    return MW_OK;
}

int mw_visible_ents(mw_engine *e, int32_t first_env, int32_t count, uint8_t *d_vis, void *stream)
{
    if (!e || !d_vis) return fail(e, MW_E_INVALID, "null argument");
    ON_DEVICE(e);
    if (first_env < 0 || count <= 0 || first_env + count > e->cfg.num_envs) return fail(e, MW_E_INVALID, "env range out of bounds");
    const size_t lds = (size_t)e->cfg.obs_width * e->cfg.obs_height * e->cfg.msaa * 4;
    if (lds + 1024 > 160 * 1024) return fail(e, MW_E_CAPACITY, "obs frame too large for the in-LDS depth buffer of mw_visible_ents");
    hipStream_t st = (hipStream_t)stream;
    MwArgs b = e->args;
    b.step_override = nullptr;
    b.env_base = first_env;
    // the geometry kernel in proxy mode (view_flags bit 2): room polygons + one tagged proxy box per entity
    {
        const int L = geom_lanes_of(e);
        hipLaunchKernelGGL(geom_kernel_of(L, e->cfg.msaa).plain, dim3(env_blocks(count, L)), dim3(64), 0, st, b, 4, e->cfg.msaa, L, count, (const uint64_t *)nullptr, 0, (uint8_t *)nullptr);
    }
    if (const int rc = allow_dynamic_lds(e, mw_visible_kernel, e->visible_lds_set, lds)) return rc;
    hipLaunchKernelGGL(mw_visible_kernel, dim3(count), dim3(256), lds, st, first_env, e->cfg.obs_width, e->cfg.obs_height,
                       e->cfg.msaa, b.max_vis, e->cfg.max_ents, (const float *)b.rec_raster, (const float *)b.rec_cull, (const int32_t *)b.nvis, d_vis);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_set_frame_reuse(mw_engine *e, int32_t on)
{
    if (!e) return MW_E_INVALID;
    frames_stale(e);        // (trust starts with the next whole frame)
    e->frame_reuse = on != 0;
    return MW_OK;
}

int mw_set_frame_cache(mw_engine *e, int32_t slots)
{
    if (!e) return MW_E_INVALID;
    if (slots < 0 || slots > MW_FC_MAX_SLOTS) return fail(e, MW_E_INVALID, "mw_set_frame_cache: %d slots outside 0 .. %d", (int)slots, MW_FC_MAX_SLOTS);
    ON_DEVICE(e);
    e->fc.dirty = true;     // (the cached frames go; the held frame stays: no state and no frame changed)
    if (slots == e->fc.slots) return MW_OK;
    // the frames that may still read or write the old buffers finish first
    HIP_TRY(e, hipDeviceSynchronize());
    e->fc.slots = 0;
    e->fc.frames.reset(); e->fc.depth.reset(); e->fc.meta.reset();
    // (only the quad kernel uses the cache: an engine whose frames take another path holds the setting and no memory)
    if (slots > 0 && e->use_k2q && e->k2q_ok) {
        const size_t N = (size_t)e->cfg.num_envs;
        DevBuf<uint8_t> frames; DevBuf<uint64_t> meta;
        int rc;
        if ((rc = dev_alloc(e, frames, N * slots * e->cfg.obs_width * e->cfg.obs_height * 3, false)) || (rc = dev_alloc(e, meta, N * MW_FC_META_WORDS(slots))) ||
            (!e->fc.d_args && (rc = dev_alloc(e, e->fc.d_args, 1))))
            return rc;
        e->fc.frames = std::move(frames); e->fc.meta = std::move(meta);
        e->fc.args_stale = true;
    }
    e->fc.slots = slots;
    return MW_OK;
}

// The launch shape for tests and measurements.  None of the three worker kinds waits for another — the entity kernel's workgroups draw
// items from a cursor, the listed tile wavefronts and the slow kernel's stride over their lists —, so any count draws the same frame as
// long as every class b % n_xcc of the entity and tile lists has a worker: 8, the most classes the engine knows.
int mw_debug_set_launch_shape(mw_engine *e, int waves_per_env, int mesh_tile_waves, int ent_blocks, int slow_waves)
{
    if (!e) return MW_E_INVALID;
    if (waves_per_env < 0 || mesh_tile_waves < 0 || ent_blocks < 0 || slow_waves < 0)
        return fail(e, MW_E_INVALID, "mw_debug_set_launch_shape: negative value (%d, %d, %d, %d)", waves_per_env, mesh_tile_waves, ent_blocks, slow_waves);
    if (waves_per_env && e->args.n_tiles % waves_per_env != 0)
        return fail(e, MW_E_INVALID, "mw_debug_set_launch_shape: waves_per_env %d does not divide the %d tiles of the frame", waves_per_env, e->args.n_tiles);
    if ((mesh_tile_waves && mesh_tile_waves < 8) || (ent_blocks && ent_blocks < 8))
        return fail(e, MW_E_INVALID, "mw_debug_set_launch_shape: mesh_tile_waves %d, ent_blocks %d: fewer than 8 leave whole lists undrawn", mesh_tile_waves, ent_blocks);
    frames_stale(e);
    if (waves_per_env) e->waves_per_env = waves_per_env;
    if (mesh_tile_waves) e->mp.mesh_tile_waves = mesh_tile_waves;
    if (ent_blocks) e->mp.ent_blocks = ent_blocks;
    if (slow_waves) e->mp.slow_waves = slow_waves;      // (0 keeps the value, so a value below 1 cannot be set)
    return MW_OK;
}

}  // extern "C"
