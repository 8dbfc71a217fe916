// mwengine host runtime: the C ABI of include/mwengine.h on top of the HIP kernels — creation, assets, state, resets, the getters
// (frames and steps: mw_engine_frame.hip; snapshot records: mw_engine_snapshot.hip).
#include <cmath>
#include <cstring>

#include "mw_engine.h"
#include "mw_rng.h"

namespace mwhost {
thread_local std::string g_create_error;
}
using namespace mwhost;

namespace {

// (re)seed env i in a host copy of the uint64[5][N] rng array
void seed_env(const mw_engine *e, uint64_t *rng, int i, uint64_t seed)
{
    const size_t N = (size_t)e->cfg.num_envs;
    uint64_t w[5];
    mw::rng_seed_words(e->cfg.rng_mode == MW_RNG_PCG64, seed, w);
    for (int k = 0; k < 5; ++k) rng[(size_t)k * N + i] = w[k];
}

// One device block holds the descriptor table followed by the texels of every level: the raster kernels reach
// both through a single buffer resource (4 SGPRs instead of 8), texel offsets count dwords from the block's start.
int upload_textures(mw_engine *e)
{
    const size_t table = (size_t)MW_MAX_TEX * sizeof(MwTexDesc) / 4;       // dwords
    size_t total = table;
    std::vector<MwTexDesc> descs = e->tex_desc;
    static_assert((MW_MAX_TEX * sizeof(MwTexDesc)) % 32 == 0, "footprint records are 32-byte aligned behind the table");
    for (size_t i = 0; i < descs.size(); ++i) {
        for (uint32_t l = 0; l < descs[i].nlevels; ++l) descs[i].lvl[l].off += (uint32_t)(total / 8);      // in 32-byte records
        total += e->tex_data[i].size();
    }
    if (total * 4 > 0xFFFFFFF0ull) return fail(e, MW_E_CAPACITY, "texture pool of %zu bytes exceeds one buffer resource", total * 4);
    // (the pool is rewritten in place unless it grows: the frames that may still read it finish first)
    HIP_TRY(e, hipDeviceSynchronize());
    if (const int rc = grow(e, e->d_texels, e->texel_cap, total, 4)) return rc;
    uint32_t *texels = e->d_texels.get();
    e->args.texels = texels; e->args.tex = reinterpret_cast<MwTexDesc *>(texels);
    size_t off = table;
    for (size_t i = 0; i < descs.size(); ++i) {
        if (!e->tex_data[i].empty())
            HIP_TRY(e, hipMemcpy(texels + off, e->tex_data[i].data(), e->tex_data[i].size() * 4, hipMemcpyHostToDevice));
        off += e->tex_data[i].size();
    }
    HIP_TRY(e, hipMemcpy(texels, descs.data(), descs.size() * sizeof(MwTexDesc), hipMemcpyHostToDevice));
    e->texel_bytes = (int)(total * 4);
    if (e->d_gen_live && sync_gen_args(e) != MW_OK) return MW_E_HIP;
    return MW_OK;
}

// copy host [count][slots][inner] <-> device, element type T: component k of slot s is an array over the envs at dev_of(k, s)
template <typename T, typename F>
int xfer(mw_engine *e, F dev_of, T *host, int first, int count, int slots, int inner, bool to_device)
{
    if (!host) return MW_OK;
    std::vector<T> tmp((size_t)count);
    for (int k = 0; k < inner; ++k)
        for (int s = 0; s < slots; ++s) {
            T *d = dev_of(k, s) + first;
            if (to_device) {
                for (int i = 0; i < count; ++i) tmp[i] = host[((size_t)i * slots + s) * inner + k];
                HIP_TRY(e, hipMemcpy(d, tmp.data(), sizeof(T) * count, hipMemcpyHostToDevice));
            } else {
                HIP_TRY(e, hipMemcpy(tmp.data(), d, sizeof(T) * count, hipMemcpyDeviceToHost));
                for (int i = 0; i < count; ++i) host[((size_t)i * slots + s) * inner + k] = tmp[i];
            }
        }
    return MW_OK;
}

int state_xfer(mw_engine *e, int first, int count, const mw_state_view *h, bool to_device)
{
    if (!e || !h) return fail(e, MW_E_INVALID, "null argument");
    if (first < 0 || count < 0 || first + count > e->cfg.num_envs) return fail(e, MW_E_INVALID, "env range out of bounds");
    MwArgs &a = e->args;
    const size_t N = (size_t)e->cfg.num_envs, E = (size_t)e->cfg.max_ents;
    // per env: host [count][inner], device SoA [inner][N] (component-major); per entity slot: host [count][E][inner], device [inner][E][N]
    auto env = [&](auto *dev, auto *host, int inner) { return xfer(e, [=](int k, int) { return dev + k * N; }, host, first, count, 1, inner, to_device); };
    auto ent = [&](auto *dev, auto *host, int inner) { return xfer(e, [=](int k, int s) { return dev + (k * E + s) * N; }, host, first, count, (int)E, inner, to_device); };
    // agent_pos is [count][3] on the host, three separate arrays on the device
    double *const pos[3] = {a.ax, a.ay, a.az};
    int rc = xfer(e, [&](int k, int) { return pos[k]; }, h->agent_pos, first, count, 1, 3, to_device);
    // ... and every other field of the view is a row of the table (mw_world_fields.h)
#define X(m, T, inner, slot, when, spare, view, vf) MW_WF_VIEWED_##view(if (!rc) rc = slot ? ent(a.m, h->vf, inner) : env(a.m, h->vf, inner);)
    MW_WORLD_FIELDS(X)
#undef X
    return rc;
}

// Device copies of the argument block for the generators (live state; spare state with the world pointers
// redirected): generate_world indexes the block dynamically, which a by-value kernarg would turn into a scratch copy.
}  // namespace
int mwhost::sync_gen_args(mw_engine *e)
{
    if (e->cfg.generator == MW_GEN_NONE) return MW_OK;
    MwArgs live = e->args;
    HIP_TRY(e, hipMemcpy(e->d_gen_live, &live, sizeof live, hipMemcpyHostToDevice));
    if (e->spare_mode) {
        // everything of the world goes to the spare arrays; the random stream (rng) and the status word stay the live ones
        MwArgs sa = e->args;
        const MwSpare &sp = e->spare_host;
#define X(m, T, inner, slot, when, spare, view, vf) MW_WF_SPARE_##spare(MW_WF_OWNED_##when(sa.m = sp.m;))
        MW_WORLD_FIELDS(X)
#undef X
        // (no spare copy: what the generator writes of them in spare mode goes nowhere)
        sa.carry = e->d_spare_dummy; sa.step = e->d_spare_dummy + e->cfg.num_envs; sa.picked = e->d_spare_dummy + 2 * (size_t)e->cfg.num_envs;
        if (!e->cfg.shared_geometry) { sa.polys = sp.polys; sa.npolys = sp.npolys; sa.segs = sp.segs; sa.nsegs = sp.nsegs; sa.occ_valid = nullptr; sa.occ_cache = nullptr; }
        sa.spare = nullptr;
        HIP_TRY(e, hipMemcpy(e->d_gen_spare, &sa, sizeof sa, hipMemcpyHostToDevice));
    }
    return MW_OK;
}
namespace {

// mw_create's engine for a checked configuration; on failure mw_create destroys it with whatever it holds
int init_engine(mw_engine *e, const mw_config *cfg)
{
    e->cfg = *cfg;
    const int N = cfg->num_envs, E = std::max(cfg->max_ents, 1);
    e->cfg.max_ents = E;
    e->n_sets = cfg->shared_geometry ? 1 : N;
    MwArgs &a = e->args;
    a.N = N; a.W = cfg->obs_width; a.H = cfg->obs_height; a.E = E;
    a.max_polys = cfg->max_polys; a.max_segs = cfg->max_segs;
    // triangle records per env: a polygon or box face is two triangles, clipping adds a few
    a.max_vis = cfg->max_visible * 6 < 60000 ? cfg->max_visible * 6 : 60000;
    a.shared_geom = cfg->shared_geometry ? 1 : 0;
    a.task = cfg->task; a.goal_ent = cfg->goal_ent; a.goal_ent2 = cfg->goal_ent2; a.num_objs = cfg->num_objs; a.max_steps = cfg->max_episode_steps;
    a.rng_mode = cfg->rng_mode;
    a.occlusion = 1;
    if (const char *s = getenv("MW_OCCLUSION")) a.occlusion = atoi(s) != 0;
    a.domain_rand = cfg->domain_rand; a.generator = cfg->generator; a.autoreset = cfg->autoreset;
    a.tiles_x = tiles_across(a.W); a.tiles_y = tiles_down(a.H); a.n_tiles = a.tiles_x * a.tiles_y;    // the raster grid
    a.agent_radius = cfg->agent_radius; a.max_forward_step = cfg->max_forward_step;
    a.agent_height = cfg->agent_height > 0.0 ? cfg->agent_height : 1.6;
    a.fwd = cfg->forward_step; a.drift = cfg->forward_drift; a.turn = cfg->turn_step;
    memcpy(a.gen_args, cfg->gen_args, sizeof a.gen_args);
    MwGenTables gt{};
    memcpy(gt.gen_tab, cfg->gen_tab, sizeof gt.gen_tab);
    memcpy(gt.gen_colors, cfg->gen_colors, sizeof gt.gen_colors);
    memcpy(gt.tex_nvar, cfg->tex_nvar, sizeof gt.tex_nvar);
    memcpy(gt.tex_var_id, cfg->tex_var_id, sizeof gt.tex_var_id);
    memcpy(gt.tex_var_scale, cfg->tex_var_scale, sizeof gt.tex_var_scale);
    gt.room_wall_height = cfg->room_wall_height; gt.room_no_ceiling = cfg->room_no_ceiling;
    for (int i = 0; i < 3; ++i) {
        a.sky[i] = cfg->sky_color[i]; a.light_pos[i] = cfg->light_pos[i]; a.light_color[i] = cfg->light_color[i];
        a.light_ambient[i] = cfg->light_ambient[i]; a.color_bias[i] = cfg->obj_color_bias[i];
    }
    a.cam_height = cfg->cam_height; a.cam_fwd_disp = cfg->cam_fwd_disp; a.cam_pitch = cfg->cam_pitch; a.cam_fov_y = cfg->cam_fov_y;
#define ALLOC(ptr, count) do { if (const int rc_ = fixed_alloc(e, &ptr, (size_t)(count))) return rc_; } while (0)
    // the world's arrays (mw_world_fields.h), zeroed: [rows][N] each, those the configuration has; the counts of the geometry sets
    // come with the sets below.  The rows `pick` chooses, in the table's order: extent, pending_remove and reset_pending keep the
    // places in the sequence of allocations that they had before there was a table (Hallway measured 0.1 % slower in the table's order)
    const auto rows = [&](int inner, int slot, int when) { return (size_t)mw_wf_rows(inner, slot, when, E, cfg->task == MW_TASK_COLLECT, !cfg->shared_geometry); };
#define LIVE_ALLOC(m, T, inner, slot, when, spare, view, vf) MW_WF_OWNED_##when(if (rows(inner, slot, MW_WF_##when) && pick(MW_SC_##m)) ALLOC(a.m, rows(inner, slot, MW_WF_##when) * N);)
    { const auto pick = [](int id) { return id != MW_SC_extent && id < MW_SC_pending_remove; }; MW_WORLD_FIELDS(LIVE_ALLOC) }
    { const auto pick = [](int id) { return id == MW_SC_extent; }; MW_WORLD_FIELDS(LIVE_ALLOC) }
    MwGenTables *d_gt = nullptr;
    ALLOC(d_gt, 1);
    HIP_TRY(e, hipMemcpy(d_gt, &gt, sizeof gt, hipMemcpyHostToDevice));
    a.gt = d_gt;
    mw_poly *polys = nullptr; int32_t *npolys = nullptr; double *segs = nullptr; int32_t *nsegs = nullptr;
    ALLOC(polys, (size_t)e->n_sets * cfg->max_polys); ALLOC(npolys, e->n_sets);
    ALLOC(segs, (size_t)e->n_sets * cfg->max_segs * 4); ALLOC(nsegs, e->n_sets);
    a.polys = polys; a.npolys = npolys; a.segs = segs; a.nsegs = nsegs;
    // spare mode: a pre-generated next world per env (mw_device.h::MwSpare)
    MwSpare sp{};
    // Spare worlds pay where the inline generator is the launch's tail: in the dense K1 of small scenes (a wave with a
    // finished env takes 26 us instead of 12, profiles/r02a) and in the Maze (a block regenerating its maze takes 300 us,
    // the launch with it; its refills run on the side stream, launch_side_refill); in the other wave-per-env scenes they bought
    // 2 us of 51 (Hallway) and stay off.  MW_SPARE=1 / 0 forces either.  Not with domain randomisation: the per-step draws
    // interleave with the worlds in the env's stream.
    {
        bool want = k1_dense_lanes(cfg->max_polys, E, cfg->max_visible, cfg->task) > 0 || cfg->generator == MW_GEN_MAZE;
        if (const char *s = getenv("MW_SPARE")) want = atoi(s) != 0;
        e->spare_mode = cfg->generator != MW_GEN_NONE && !cfg->domain_rand && want && cfg->task != MW_TASK_COLLECT;     // CollectHealth's respawns draw from the stream mid-episode
    }
    if (e->spare_mode) {
#define X(m, T, inner, slot, when, spare, view, vf) MW_WF_SPARE_##spare(MW_WF_OWNED_##when(if (rows(inner, slot, MW_WF_##when)) ALLOC(sp.m, rows(inner, slot, MW_WF_##when) * N);))
        MW_WORLD_FIELDS(X)
#undef X
        if (!cfg->shared_geometry) {
            ALLOC(sp.polys, (size_t)e->n_sets * cfg->max_polys); ALLOC(sp.npolys, e->n_sets);
            ALLOC(sp.segs, (size_t)e->n_sets * cfg->max_segs * 4); ALLOC(sp.nsegs, e->n_sets);
        }
        MwSpare *d_sp = nullptr;
        ALLOC(d_sp, 1);
        ALLOC(a.refill_mask, N);
        ALLOC(e->d_spare_dummy, 3 * (size_t)N);
        e->spare_host = sp;
        {       // every spare starts out consumed: the first reset generates it
            std::vector<uint32_t> ones((size_t)N, 1u);
            HIP_TRY(e, hipMemcpy(a.refill_mask, ones.data(), 4 * (size_t)N, hipMemcpyHostToDevice));
        }
        HIP_TRY(e, hipMemcpy(d_sp, &sp, sizeof sp, hipMemcpyHostToDevice));
        a.spare = d_sp;
    }
    if (cfg->generator != MW_GEN_NONE) {
        ALLOC(e->d_gen_live, 1); a.gen_live = e->d_gen_live;
        if (e->spare_mode) { ALLOC(e->d_gen_spare, 1); a.gen_spare = e->d_gen_spare; }
    }
    ALLOC(e->d_meshdesc, MW_MAX_MESH);
    a.mesh = e->d_meshdesc;      // a.tex / a.texels: upload_textures
    ALLOC(a.rec_raster, (size_t)N * a.max_vis * MW_RASTER_REC);
    ALLOC(a.rec_shade, (size_t)N * a.max_vis * MW_SHADE_REC);
    ALLOC(a.rec_cull, (size_t)N * a.max_vis * MW_CULL_REC);
    if (has_visiting_order(cfg->max_visible)) {
        // big scenes: the visiting order the geometry kernel leaves for K2 (mw_geom.hip), zeroed
        ALLOC(a.rec_order, (size_t)N * (a.max_vis + 1));
    }
    if (cfg->max_polys > 64 && !(getenv("MW_OCC_CACHE") && atoi(getenv("MW_OCC_CACHE")) == 0)) {
        // big scenes: the geometry kernel's per-world culling data (mw_geom.hip), zeroed = nothing cached
        ALLOC(a.occ_valid, e->n_sets);
        ALLOC(a.occ_cache, (size_t)e->n_sets * MW_OCC_CACHE_STRIDE(cfg->max_polys));
    }
    { const auto pick = [](int id) { return id >= MW_SC_pending_remove; }; MW_WORLD_FIELDS(LIVE_ALLOC) }      // (reset_pending zeroed: nothing pending)
    ALLOC(a.frame_clean, (size_t)N);        // (zeroed: nothing clean before the first step)
    ALLOC(a.fc_key, (size_t)MW_FC_KEY_WORDS * N); ALLOC(a.fc_epoch, (size_t)N); ALLOC(a.fc_source, (size_t)N);
    HIP_TRY(e, hipMemset(a.pending_remove, 0xFF, 4 * (size_t)N));
    ALLOC(a.nvis, N); ALLOC(a.envhdr, (size_t)MW_ENVHDR * N); ALLOC(a.status, 1);
    ALLOC(e->d_reward_scratch, N); ALLOC(e->d_flag_scratch, 2 * (size_t)N);
    ALLOC(e->d_final_list, 1 + (size_t)N);
    ALLOC(e->d_plan[0], MW_PLAN_WORDS(N, frame_plan_ordered(N))); ALLOC(e->d_plan[1], MW_PLAN_WORDS(N, frame_plan_ordered(N)));      // (zeroed: the first plan kernel counts from nothing)
    ALLOC(e->stack.flags, 2 * (size_t)N);
    ALLOC(e->d_geom_built, (size_t)N);
    ALLOC(e->d_mask, N); ALLOC(e->d_step_override, 3 * (size_t)N);
#ifdef MW_PERF_HOOKS        // (tools/perf: make EXTRA=-DMW_PERF_HOOKS — kernel phase stamps dumped by mw_destroy; not in the product build)
    if (getenv("MW_K1_PROF")) ALLOC(a.k1_prof, MW_K1_PROF_SLOTS * (size_t)N);     // per-env cycle stamps of the geometry kernel's phases (zeroed)
    if (getenv("MW_ENT_PROF")) ALLOC(e->d_ent_prof, (size_t)16 * 2 * N * MW_MAX_MESH_ENTS * 8);
    if (getenv("MW_K2Q_PROF")) ALLOC(e->d_k2q_prof, (size_t)N * 96);
#endif
#undef LIVE_ALLOC
#undef ALLOC
    // carrying = -1 everywhere; default seeds = env index
    {
        std::vector<int32_t> m1((size_t)N, -1);
        HIP_TRY(e, hipMemcpy(a.carry, m1.data(), 4 * (size_t)N, hipMemcpyHostToDevice));
        std::vector<uint64_t> seeds(5 * (size_t)N, 0);
        for (int i = 0; i < N; ++i) seed_env(e, seeds.data(), i, (uint64_t)i);
        HIP_TRY(e, hipMemcpy(a.rng, seeds.data(), 40 * (size_t)N, hipMemcpyHostToDevice));
    }
    e->meshes.assign(MW_MAX_MESH, {}); e->tex_desc.assign(MW_MAX_TEX, MwTexDesc{}); e->tex_data.assign(MW_MAX_TEX, {});
    if (const int rc = upload_textures(e)) return rc;
    e->waves_per_env = pick_waves_per_env(a.n_tiles, N);
#if defined(MW_PERF_HOOKS) || defined(MW_TUNE_HOOKS)
    if (const char *s = getenv("MW_WAVES_PER_ENV")) { const int v = atoi(s); if (v > 0 && a.n_tiles % v == 0) e->waves_per_env = v; }
#endif
    {
        // The XCDs of this device as workgroups see them (HW_REG_XCC_ID of 256 workgroups: 8, 4, 2 or one id per partition mode).
        // The mesh path files an env's entities and mesh tiles under class env % n_xcc and workgroup b of the entity / tile launches
        // draws from class b % n_xcc: where workgroup b runs on XCD b % n_xcc — every launch of a fresh process — an env's records,
        // keys and planes meet one L2 (the mesh tiles' fetch 50 -> 37 MB).  Locality only: nothing is wrong when the dispatcher's
        // round-robin starts elsewhere.
        uint32_t *p = nullptr, ids[256];
        a.n_xcc = 0;
        if (hipMalloc((void **)&p, sizeof ids) == hipSuccess) {
            const DevBuf<uint32_t> d_ids(p);
            hipLaunchKernelGGL(mw_xcc_probe_kernel, dim3(256), dim3(64), 0, 0, d_ids.get());
            if (hipMemcpy(ids, d_ids.get(), sizeof ids, hipMemcpyDeviceToHost) == hipSuccess) {
                uint32_t seen = 0u;
                for (uint32_t v : ids) seen |= 1u << (v & 15u);
                for (int n : {8, 4, 2}) if (seen == (1u << n) - 1u) a.n_xcc = n;
            }
        }
        if (a.n_xcc == 0) a.n_xcc = 1;      // (one id, or a set this code does not know: one class — the lists are about locality only)
    }
    if (const char *s = getenv("MW_DEBUG_FLAGS")) e->dbg_flags = atoi(s) & MW_DEBUG_BITS;
    if (const char *s = getenv("MW_K2Q")) e->use_k2q = atoi(s) != 0;
    if (const char *s = getenv("MW_GENERIC_RASTER")) e->generic_raster = atoi(s) != 0;
    if (const char *s = getenv("MW_GEOM_DEAL")) e->geom_deal = atoi(s) != 0;
    e->k2q_ok = k2q_ok(cfg->msaa, a.W, a.H, mw_rasterq_lds_bytes(cfg->msaa == 4 ? 4 : 8, a.W, a.H, a.n_tiles, 1));
    {
        // snapshot records: the components this engine has, each with its array and its place in a record (mw_snapshot.h)
        e->snap_cfg = {E, cfg->max_polys, cfg->max_segs, cfg->shared_geometry ? 1 : 0, cfg->task, cfg->generator, cfg->rng_mode, e->spare_mode ? 1 : 0,
                       cfg->task == MW_TASK_COLLECT ? 1 : 0};
        const MwSnapLayout &L = e->snap_layout = mw_snap_layout(e->snap_cfg);
        void *arr[MW_SC_COUNT] = {};
#define X(m, T, inner, slot, when, spare, view, vf) arr[MW_SC_##m] = (void *)a.m; MW_WF_SPARE_##spare(arr[MW_SC_SP_##m] = sp.m;)
        MW_WORLD_FIELDS(X)
#undef X
        arr[MW_SC_REFILL_MASK] = a.refill_mask;
        MwSnapTable t{};
        for (int id = 0; id < MW_SC_COUNT; ++id) {
            if (!L.comp_rows[id]) continue;
            if (!arr[id]) return fail(e, MW_E_INVALID, "snapshot layout: component %d has rows but no array", id);
            t.comp[t.n_comps++] = {arr[id], L.comp_unit[id], L.comp_row0[id], L.comp_rows[id], L.comp_elem[id], 0};
        }
        t.total_rows = L.total_rows; t.n_geo = L.n_geo; t.max_polys = cfg->max_polys; t.max_segs = cfg->max_segs;
        const int chunk = MW_SNAP_THREADS * MW_SNAP_UNROLL;
        t.poly_chunks = (cfg->max_polys * (MW_SNAP_POLY_BYTES / 16) + chunk - 1) / chunk;
        t.seg_chunks = (cfg->max_segs * (MW_SNAP_SEG_BYTES / 16) + chunk - 1) / chunk;
        t.eng_polys[0] = const_cast<mw_poly *>(a.polys); t.eng_segs[0] = const_cast<double *>(a.segs);
        t.eng_npolys[0] = const_cast<int32_t *>(a.npolys); t.eng_nsegs[0] = const_cast<int32_t *>(a.nsegs);
        t.eng_polys[1] = sp.polys; t.eng_segs[1] = sp.segs; t.eng_npolys[1] = sp.npolys; t.eng_nsegs[1] = sp.nsegs;
        t.polys_unit[0] = L.blob_unit[MW_SB_POLYS]; t.segs_unit[0] = L.blob_unit[MW_SB_SEGS];
        t.polys_unit[1] = L.blob_unit[MW_SB_SP_POLYS]; t.segs_unit[1] = L.blob_unit[MW_SB_SP_SEGS];
        t.npolys_unit[0] = L.comp_unit[MW_SC_npolys]; t.nsegs_unit[0] = L.comp_unit[MW_SC_nsegs];
        t.npolys_unit[1] = L.comp_unit[MW_SC_SP_npolys]; t.nsegs_unit[1] = L.comp_unit[MW_SC_SP_nsegs];
        t.reset_pending_unit = L.comp_unit[MW_SC_reset_pending];
        e->snap_chunks_per_item = t.n_geo * (t.poly_chunks + t.seg_chunks);
        {
            std::vector<uint16_t> row_comp((size_t)t.total_rows);
            for (int c = 0; c < t.n_comps; ++c)
                for (int r = 0; r < t.comp[c].rows; ++r) row_comp[(size_t)t.comp[c].row0 + r] = (uint16_t)c;
            uint16_t *d_row_comp = nullptr;
            if (const int rc = fixed_alloc(e, &d_row_comp, row_comp.size())) return rc;
            HIP_TRY(e, hipMemcpy(d_row_comp, row_comp.data(), row_comp.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
            t.row_comp = d_row_comp;
        }
        if (const int rc = fixed_alloc(e, &e->d_snap_tab, 1)) return rc;
        HIP_TRY(e, hipMemcpy(e->d_snap_tab, &t, sizeof t, hipMemcpyHostToDevice));
    }
    return sync_gen_args(e);
}

// mw_get_info / mw_get_final_info: slot `slot` of a component-major [3][E][N] table and the health array, gathered per env
int launch_info(mw_engine *e, int E, const int32_t *health, const double *pos, int slot, int32_t *d_health, double *d_pos, void *stream)
{
    ON_DEVICE(e);
    const int N = e->cfg.num_envs;
    hipLaunchKernelGGL(mw_info_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, E, health, pos, slot, d_health, d_pos);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

// the engine's arrays of mw_state_view's fields, for the state-view kernels (mw_state_view.h)
MwStateArrays state_arrays_of(const mw_engine *e)
{
#define X(m, T, inner, slot, when, spare, view, vf) MW_WF_INVIEW_##view(e->args.m,)
    return {MW_WORLD_FIELDS(X)};        // (MwStateArrays' members are the same rows in the same order)
#undef X
}

// mw_get_reset_pending / mw_get_frame_source / mw_get_frame_clean: one of the engine's uint8 [N] arrays, device to device
int get_env_bytes(mw_engine *e, const char *what, const uint8_t *src, uint8_t *d_out, void *stream)
{
    if (!d_out) return fail(e, MW_E_INVALID, "%s: d_out is null", what);
    ON_DEVICE(e);
    HIP_TRY(e, hipMemcpyAsync(d_out, src, (size_t)e->cfg.num_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MW_OK;
}

}  // namespace

extern "C" {

const char *mw_last_error(const mw_engine *e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int mw_create(const mw_config *cfg, mw_engine **out)
{
    if (!cfg || !out) return fail(nullptr, MW_E_INVALID, "null argument");
    if (cfg->abi_version != MW_ABI_VERSION) return fail(nullptr, MW_E_INVALID, "ABI version mismatch: header %d, caller %d", MW_ABI_VERSION, cfg->abi_version);
    if (cfg->num_envs <= 0 || cfg->max_ents < 0 || cfg->max_polys <= 0 || cfg->max_segs <= 0 || cfg->max_visible <= 0)
        return fail(nullptr, MW_E_INVALID, "bad capacities");
    if (cfg->rng_mode != MW_RNG_PHILOX && cfg->rng_mode != MW_RNG_PCG64) return fail(nullptr, MW_E_INVALID, "unknown rng_mode %d", cfg->rng_mode);
    if (cfg->autoreset != MW_AUTORESET_OFF && cfg->autoreset != MW_AUTORESET_SAME_STEP && cfg->autoreset != MW_AUTORESET_NEXT_STEP)
        return fail(nullptr, MW_E_INVALID, "unknown autoreset mode %d", cfg->autoreset);
    if (cfg->rng_mode == MW_RNG_PCG64 && cfg->generator == MW_GEN_NONE)
        return fail(nullptr, MW_E_INVALID, "MW_RNG_PCG64 (the reference's own numpy stream) needs a device generator");
    if (cfg->max_ents > 64) return fail(nullptr, MW_E_CAPACITY, "max_ents > 64 (one entity slot per lane of the env's wavefront)");
    if (cfg->msaa != 8 && cfg->msaa != 4 && cfg->msaa != 1) return fail(nullptr, MW_E_INVALID, "msaa must be 8, 4 or 1");
    if (!frame_size_ok(cfg->obs_width, cfg->obs_height))
        return fail(nullptr, MW_E_INVALID, "obs size %dx%d: 1 to %d x 1 to %d pixels", cfg->obs_width, cfg->obs_height, 255 * MW_TILE_W, 255 * MW_TILE_H);
    if (cfg->max_visible > 60000) return fail(nullptr, MW_E_CAPACITY, "max_visible too large (16-bit draw ids)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, MW_E_DEVICE, "no HIP device available");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(nullptr, MW_E_DEVICE, "device %d out of range (%d devices)", cfg->device_id, ndev);
    hipError_t st = hipSetDevice(cfg->device_id);
    if (st != hipSuccess) return fail(nullptr, MW_E_HIP, "hipSetDevice: %s", hipGetErrorString(st));

    mw_engine *e = new mw_engine();
    if (const int rc = init_engine(e, cfg)) { g_create_error = e->err; mw_destroy(e); return rc; }
    *out = e;
    return MW_OK;
}

void mw_destroy(mw_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->cfg.device_id);       // (the members release their buffers, streams and events on the engine's device)
    (void)hipDeviceSynchronize();
#ifdef MW_PERF_HOOKS
    auto dump = [](const unsigned long long *dev, size_t count, const char *var) {      // count stamps to the file the variable names
        std::vector<unsigned long long> h(count);
        if (dev && hipMemcpy(h.data(), dev, count * 8, hipMemcpyDeviceToHost) == hipSuccess)
            if (FILE *f = fopen(getenv(var), "wb")) { fwrite(h.data(), 8, count, f); fclose(f); }
    };
    dump(e->d_k2q_prof, (size_t)e->cfg.num_envs * 96, "MW_K2Q_PROF");
    dump(e->d_ent_prof, (size_t)16 * 2 * e->cfg.num_envs * MW_MAX_MESH_ENTS * 8, "MW_ENT_PROF");
    dump(e->args.k1_prof, (size_t)e->cfg.num_envs * MW_K1_PROF_SLOTS, "MW_K1_PROF");
    if (getenv("MW_SLOW_STATS") && e->mp.slow_count) {      // perf experiments only: the last frame's slow fragments per env
        std::vector<int32_t> h((size_t)e->cfg.num_envs * 4);
        if (hipMemcpy(h.data(), e->mp.slow_count.get(), h.size() * 4, hipMemcpyDeviceToHost) == hipSuccess) {
            long long tot = 0, nz = 0, mx = 0;
            for (int i = 0; i < e->cfg.num_envs; ++i) { const int v = h[(size_t)e->cfg.num_envs + i] + h[(size_t)e->cfg.num_envs * 3 + i]; tot += v; nz += v > 0; mx = std::max<long long>(mx, v); }
            fprintf(stderr, "slow fragments: total %lld, envs with any %lld of %d, max %lld\n", tot, nz, e->cfg.num_envs, mx);
            int32_t c[2 * MW_CNT_WORDS];
            if (e->mp.ent_counter && hipMemcpy(c, e->mp.ent_counter, sizeof c, hipMemcpyDeviceToHost) == hipSuccess)
                for (int p = 0; p < 2; ++p) {
                    int nl = 0, ns = 0, nt = 0;
                    for (int x = 0; x < 8; ++x) { nl += c[p * MW_CNT_WORDS + MW_CNT_LONG + x]; ns += c[p * MW_CNT_WORDS + MW_CNT_SHORT + x]; nt += c[p * MW_CNT_WORDS + MW_CNT_TILES + x]; }
                    fprintf(stderr, "work lists (parity %d): long meshes %d, short %d, mesh tiles %d, envs with slow-path triangles %d\n", p, nl, ns,
                            nt, c[p * MW_CNT_WORDS + MW_CNT_SLOW_ENVS]);
                }
        }
    }
#endif
    delete e;
}

int mw_upload_texture(mw_engine *e, int32_t tex_id, const uint8_t *rgb, int32_t w, int32_t h)
{
    if (!e || !rgb) return fail(e, MW_E_INVALID, "null argument");
    ON_DEVICE_SYNC(e);
    world_changed(e);
    if (tex_id < 0 || tex_id >= MW_MAX_TEX) return fail(e, MW_E_CAPACITY, "texture id %d out of range (max %d)", tex_id, MW_MAX_TEX);
    if (w <= 0 || h <= 0 || w > 16384 || h > 16384) return fail(e, MW_E_INVALID, "bad texture size %dx%d", w, h);
    mwasset::build_pyramid(rgb, w, h, e->tex_data[tex_id], e->tex_desc[tex_id]);
    return upload_textures(e);
}

int mw_upload_mesh(mw_engine *e, int32_t mesh_id, const float *pos, const float *nrm, const float *uv,
                   const float *rgb, int32_t ntris, int32_t tex_id)
{
    if (!e || !pos || !nrm || !rgb) return fail(e, MW_E_INVALID, "null argument");
    ON_DEVICE_SYNC(e);
    world_changed(e);
    if (tex_id >= MW_MAX_TEX || (tex_id >= 0 && !uv)) return fail(e, MW_E_INVALID, "textured mesh needs texcoords and a valid texture id");
    if (mesh_id < 0 || mesh_id >= MW_MAX_MESH) return fail(e, MW_E_CAPACITY, "mesh id %d out of range (max %d)", mesh_id, MW_MAX_MESH);
    if (ntris <= 0 || ntris > 60000) return fail(e, MW_E_CAPACITY, "mesh with %d triangles (1..60000 supported: 16-bit draw ids)", ntris);
    e->meshes[mesh_id] = mwasset::prepare_mesh(pos, nrm, uv, rgb, ntris, tex_id);
    // repack all pools (uploads are rare) into new ones: a failure leaves the installed pools, descriptors and MwArgs as they are
    std::vector<MwMeshDesc> descs(MW_MAX_MESH);
    size_t total = 0, total_v = 0, max_verts = 0;
    for (int i = 0; i < MW_MAX_MESH; ++i) {
        descs[i] = e->meshes[i].desc;
        descs[i].first = (uint32_t)total; total += descs[i].ntris;
        descs[i].vfirst = (uint32_t)total_v; total_v += descs[i].nverts;
        max_verts = std::max<size_t>(max_verts, descs[i].nverts);
    }
    mw_engine::MeshPools p;
    int rc;
    if ((rc = dev_alloc(e, p.vpos, total_v, false)) || (rc = dev_alloc(e, p.idx, total, false)) || (rc = dev_alloc(e, p.pos, total * MW_MESH_POS_STRIDE, false)) ||
        (rc = dev_alloc(e, p.nrm, total * 9, false)) || (rc = dev_alloc(e, p.rgb, total * 9, false)) || (rc = dev_alloc(e, p.uv, total * 6, false)) ||
        (rc = dev_alloc(e, p.stream, total * 12, false)) || (rc = dev_alloc(e, p.attr, total * 24, false)))
        return rc;
    for (int i = 0; i < MW_MAX_MESH; ++i) {
        const mwasset::HostMesh &m = e->meshes[i];
        const size_t n = descs[i].ntris, first = descs[i].first;
        if (!n) continue;
        HIP_TRY(e, hipMemcpy(p.pos.get() + first * MW_MESH_POS_STRIDE, m.pos.data(), n * 4 * MW_MESH_POS_STRIDE, hipMemcpyHostToDevice));
        HIP_TRY(e, hipMemcpy(p.nrm.get() + first * 9, m.nrm.data(), n * 36, hipMemcpyHostToDevice));
        HIP_TRY(e, hipMemcpy(p.rgb.get() + first * 9, m.rgb.data(), n * 36, hipMemcpyHostToDevice));
        HIP_TRY(e, hipMemcpy(p.uv.get() + first * 6, m.uv.data(), n * 24, hipMemcpyHostToDevice));
        if (descs[i].nverts)
            HIP_TRY(e, hipMemcpy(p.vpos.get() + descs[i].vfirst, m.vtab.data(), (size_t)descs[i].nverts * 16, hipMemcpyHostToDevice));
        HIP_TRY(e, hipMemcpy(p.idx.get() + first, m.itab.data(), n * 8, hipMemcpyHostToDevice));
        HIP_TRY(e, hipMemcpy(p.stream.get() + first * 12, m.stream.data(), n * 48, hipMemcpyHostToDevice));
        HIP_TRY(e, hipMemcpy(p.attr.get() + first * 24, m.attr.data(), n * 96, hipMemcpyHostToDevice));
    }
    // install: the frames that may still read the old pools and descriptors finish first
    HIP_TRY(e, hipDeviceSynchronize());
    HIP_TRY(e, hipMemcpy(e->d_meshdesc, descs.data(), sizeof(MwMeshDesc) * MW_MAX_MESH, hipMemcpyHostToDevice));
    e->args.mesh_pos = p.pos.get(); e->args.mesh_nrm = p.nrm.get(); e->args.mesh_rgb = p.rgb.get(); e->args.mesh_uv = p.uv.get();
    e->pools = std::move(p);
    e->max_mesh_verts = (int)max_verts;
    if (e->d_gen_live && sync_gen_args(e) != MW_OK) return MW_E_HIP;
    e->have_meshes = true;
    e->max_mesh_tris = std::max(e->max_mesh_tris, (int)ntris);
    return ensure_mesh_buffers(e);
}

int mw_set_geometry(mw_engine *e, int32_t env, const mw_poly *polys, int32_t n_polys, const double *segs, int32_t n_segs)
{
    if (!e || (n_polys > 0 && !polys) || (n_segs > 0 && !segs)) return fail(e, MW_E_INVALID, "null argument");
    ON_DEVICE_SYNC(e);
    world_changed(e);
    if (n_polys < 0 || n_polys > e->cfg.max_polys) return fail(e, MW_E_CAPACITY, "%d polygons > max_polys %d", n_polys, e->cfg.max_polys);
    if (n_segs < 0 || n_segs > e->cfg.max_segs) return fail(e, MW_E_CAPACITY, "%d segments > max_segs %d", n_segs, e->cfg.max_segs);
    int set = 0;
    if (e->cfg.shared_geometry) {
        if (env != -1) return fail(e, MW_E_INVALID, "engine uses one shared geometry set: pass env = -1");
    } else {
        if (env < 0 || env >= e->cfg.num_envs) return fail(e, MW_E_INVALID, "env %d out of range", env);
        set = env;
    }
    for (int i = 0; i < n_polys; ++i) {
        const int nv = polys[i].nv & 0xFF;
        if (nv != 3 && nv != 4) return fail(e, MW_E_INVALID, "polygon %d has %d vertices (3 or 4 supported)", i, nv);
        if (polys[i].tex >= MW_MAX_TEX) return fail(e, MW_E_INVALID, "polygon %d: bad texture id", i);
        if (polys[i].tex >= 0 && e->tex_desc[polys[i].tex].nlevels == 0) return fail(e, MW_E_INVALID, "polygon %d uses texture %d which was never uploaded", i, polys[i].tex);
    }
    HIP_TRY(e, hipMemcpy(const_cast<mw_poly *>(e->args.polys) + (size_t)set * e->cfg.max_polys, polys, sizeof(mw_poly) * (size_t)n_polys, hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(const_cast<int32_t *>(e->args.npolys) + set, &n_polys, 4, hipMemcpyHostToDevice));
    if (e->args.occ_valid) HIP_TRY(e, hipMemset(e->args.occ_valid + set, 0, 4));
    HIP_TRY(e, hipMemcpy(const_cast<double *>(e->args.segs) + (size_t)set * e->cfg.max_segs * 4, segs, 32 * (size_t)n_segs, hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(const_cast<int32_t *>(e->args.nsegs) + set, &n_segs, 4, hipMemcpyHostToDevice));
    return MW_OK;
}

int mw_get_geometry(mw_engine *e, int32_t env, mw_poly *polys, int32_t *n_polys, double *segs, int32_t *n_segs)
{
    if (!e || !polys || !n_polys || !segs || !n_segs) return fail(e, MW_E_INVALID, "null argument");
    ON_DEVICE_SYNC(e);
    const int set = e->cfg.shared_geometry ? 0 : env;
    if (set < 0 || set >= e->n_sets) return fail(e, MW_E_INVALID, "env out of range");
    HIP_TRY(e, hipDeviceSynchronize());
    HIP_TRY(e, hipMemcpy(n_polys, e->args.npolys + set, 4, hipMemcpyDeviceToHost));
    HIP_TRY(e, hipMemcpy(n_segs, e->args.nsegs + set, 4, hipMemcpyDeviceToHost));
    HIP_TRY(e, hipMemcpy(polys, e->args.polys + (size_t)set * e->cfg.max_polys, sizeof(mw_poly) * (size_t)e->cfg.max_polys, hipMemcpyDeviceToHost));
    HIP_TRY(e, hipMemcpy(segs, e->args.segs + (size_t)set * e->cfg.max_segs * 4, 32 * (size_t)e->cfg.max_segs, hipMemcpyDeviceToHost));
    return MW_OK;
}

int mw_set_state(mw_engine *e, int32_t first_env, int32_t count, const mw_state_view *host)
{
    if (!e) return MW_E_INVALID;
    ON_DEVICE_SYNC(e);
    world_changed(e);
    const int rc = state_xfer(e, first_env, count, host, true);
    if (rc != MW_OK) return rc;
    // a world written from the host replaces whatever a pending next-step auto-reset would have installed
    HIP_TRY(e, hipMemset(e->args.reset_pending + first_env, 0, (size_t)count));
    HIP_TRY(e, hipDeviceSynchronize());     // (a null-stream memset: the caller's stream is not ordered against it)
    if (e->stack.depth && count > 0) {
        // ... and with it the rebuild of the env's frame stack that reset would have caused; the stacks themselves stay
        std::vector<uint8_t> fl((size_t)count);
        uint8_t *d = stack_flags(e, e->stack.cur) + first_env;
        HIP_TRY(e, hipMemcpy(fl.data(), d, (size_t)count, hipMemcpyDeviceToHost));
        for (uint8_t &f : fl) f &= (uint8_t)~MW_STACK_PENDING;
        HIP_TRY(e, hipMemcpy(d, fl.data(), (size_t)count, hipMemcpyHostToDevice));
    }
    return MW_OK;
}

int mw_get_state(mw_engine *e, int32_t first_env, int32_t count, mw_state_view *host)
{
    if (!e) return MW_E_INVALID;
    ON_DEVICE_SYNC(e);
    (void)hipDeviceSynchronize();
    return state_xfer(e, first_env, count, host, false);
}

// The two device-side state views.  Neither waits for the Maze's side-stream refills (refill_order), which mw_snapshot_load and
// mw_reset_where do wait for: those calls read or write spares, refill_mask words or the envs' streams, the refill kernel's own data.
// The refill kernel generates into the spare arrays through the redirected argument block (sync_gen_args: everything of the world goes
// to the spares, carry / step / picked to a dummy) and touches the stream and refill_mask beside them — it neither reads nor writes a
// live array of mw_state_view's fields, and these two calls touch nothing else of the world (the write's reset_pending, frame_clean,
// fc_epoch and stack flags belong to the caller's stream alone).  So the order of either against a running refill does not matter.
int mw_get_state_device(mw_engine *e, int32_t first_env, int32_t count, const mw_state_view *d_view, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (!d_view) return fail(e, MW_E_INVALID, "mw_get_state_device: d_view is null");
    if (first_env < 0 || count < 0 || first_env > e->cfg.num_envs - count) return fail(e, MW_E_INVALID, "mw_get_state_device: env range out of bounds");
    if (!mwsv::any_field(*d_view)) return fail(e, MW_E_INVALID, "mw_get_state_device: every pointer of the view is null");
    if (count == 0) return MW_OK;
    ON_DEVICE(e);
    hipLaunchKernelGGL(mw_state_get_kernel, dim3((unsigned)((count + MW_SV_ENVS - 1) / MW_SV_ENVS)), dim3(MW_SV_THREADS), 0, (hipStream_t)stream,
                       state_arrays_of(e), *d_view, e->cfg.num_envs, e->args.E, (int)first_env, (int)count);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_set_state_where(mw_engine *e, const uint8_t *d_mask, const mw_state_view *d_view, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (!d_mask || !d_view) return fail(e, MW_E_INVALID, "mw_set_state_where: %s is null", d_mask ? "d_view" : "d_mask");
    if (!mwsv::any_field(*d_view)) return fail(e, MW_E_INVALID, "mw_set_state_where: every pointer of the view is null");
    ON_DEVICE(e);
    // the caller's buffers no longer show the masked envs; the other envs keep their cached frames (the kernel advances the epochs of the
    // envs it writes)
    invalidate(e, set_state_where_invalidation());
    const int N = e->cfg.num_envs;
    hipLaunchKernelGGL(mw_state_set_where_kernel, dim3((unsigned)((N + MW_SV_ENVS - 1) / MW_SV_ENVS)), dim3(MW_SV_THREADS), 0, (hipStream_t)stream,
                       state_arrays_of(e), *d_view, d_mask, N, e->args.E, e->args.status, e->args.reset_pending, e->args.frame_clean, e->args.fc_epoch,
                       e->stack.depth ? stack_flags(e, e->stack.cur) : nullptr);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_set_gen_program(mw_engine *e, const mw_gen_program *prog, const mw_poly *polys, const int32_t *poly_room,
                       const int32_t *poly_surf, const double *poly_m, int32_t n_polys, const double *segs, int32_t n_segs)
{
    if (!e || !prog) return fail(e, MW_E_INVALID, "null argument");
    ON_DEVICE_SYNC(e);
    world_changed(e);
    if (prog->n_rooms < 1 || prog->n_rooms > MW_PROG_MAX_ROOMS || prog->n_tex < 0 || prog->n_tex > MW_PROG_MAX_TEX ||
        prog->n_ops < 0 || prog->n_ops > MW_PROG_MAX_OPS || prog->n_ents < 0 || prog->n_ents > MW_PROG_MAX_ENTS ||
        prog->n_ents > e->cfg.max_ents || prog->sign_n < 0 || prog->sign_n > 8)
        return fail(e, MW_E_CAPACITY, "placement program exceeds the table sizes");
    if (n_polys < 0 || n_polys > e->cfg.max_polys || n_segs < 0 || n_segs > e->cfg.max_segs)
        return fail(e, MW_E_CAPACITY, "template geometry exceeds max_polys / max_segs");
    if (n_polys > 0 && (!polys || !poly_room || !poly_surf || !poly_m)) return fail(e, MW_E_INVALID, "null template geometry");
    for (int i = 0; i < prog->n_ops; ++i) {
        const mw_prog_op &op = prog->ops[i];
        const bool needs_slot = op.op == MW_OP_PLACE || op.op == MW_OP_FIXED || op.op == MW_OP_BOX_SIZE || op.op == MW_OP_COLOR || op.op == MW_OP_APPEND;
        if (op.op < MW_OP_COIN || op.op > MW_OP_APPEND) return fail(e, MW_E_INVALID, "op %d: unknown opcode %d", i, op.op);
        if (needs_slot && (op.slot >= prog->n_ents || (op.slot < 0 && !(op.op == MW_OP_PLACE || op.op == MW_OP_FIXED))))
            return fail(e, MW_E_INVALID, "op %d: bad entity slot %d", i, op.slot);
        if (op.op == MW_OP_PLACE && op.room >= prog->n_rooms) return fail(e, MW_E_INVALID, "op %d: bad room %d", i, op.room);
    }
    MwProgram hp{};
    hp.p = *prog;
    hp.n_polys = n_polys; hp.n_segs = n_segs;
    // the new tables are built beside the installed ones: a failure leaves those, the program block and MwArgs as they are
    DevBuf<mw_poly> d_polys; DevBuf<int32_t> d_room, d_surf; DevBuf<double> d_m, d_segs;
    int rc;
    if ((rc = dev_alloc(e, d_polys, (size_t)n_polys)) || (rc = dev_alloc(e, d_room, (size_t)n_polys)) || (rc = dev_alloc(e, d_surf, (size_t)n_polys)) ||
        (rc = dev_alloc(e, d_m, (size_t)n_polys * 8)) || (rc = dev_alloc(e, d_segs, (size_t)n_segs * 4)) || (!e->d_prog && (rc = dev_alloc(e, e->d_prog, 1))))
        return rc;
    if (n_polys > 0) {
        HIP_TRY(e, hipMemcpy(d_polys.get(), polys, sizeof(mw_poly) * (size_t)n_polys, hipMemcpyHostToDevice));
        HIP_TRY(e, hipMemcpy(d_room.get(), poly_room, 4 * (size_t)n_polys, hipMemcpyHostToDevice));
        HIP_TRY(e, hipMemcpy(d_surf.get(), poly_surf, 4 * (size_t)n_polys, hipMemcpyHostToDevice));
        HIP_TRY(e, hipMemcpy(d_m.get(), poly_m, 64 * (size_t)n_polys, hipMemcpyHostToDevice));
    }
    if (n_segs > 0) HIP_TRY(e, hipMemcpy(d_segs.get(), segs, 32 * (size_t)n_segs, hipMemcpyHostToDevice));
    hp.polys = d_polys.get(); hp.poly_room = d_room.get(); hp.poly_surf = d_surf.get(); hp.poly_m = d_m.get(); hp.segs = d_segs.get();
    // install: the device finishes whatever may still read the program block and the previous program's tables, which then go
    HIP_TRY(e, hipDeviceSynchronize());
    HIP_TRY(e, hipMemcpy(e->d_prog.get(), &hp, sizeof hp, hipMemcpyHostToDevice));
    e->d_prog_polys = std::move(d_polys); e->d_prog_room = std::move(d_room); e->d_prog_surf = std::move(d_surf);
    e->d_prog_m = std::move(d_m); e->d_prog_segs = std::move(d_segs);
    e->args.prog = e->d_prog.get();
    if (e->cfg.shared_geometry && n_polys > 0) {        // no texture randomisation: the template IS the geometry
        const int r2 = mw_set_geometry(e, -1, polys, n_polys, segs, n_segs);
        if (r2 != MW_OK) return r2;
    }
    return sync_gen_args(e);
}

int mw_set_step_params(mw_engine *e, const double *host_params)
{
    if (!e) return MW_E_INVALID;
    if (!host_params) { e->use_step_override = false; return MW_OK; }
    ON_DEVICE_SYNC(e);
    HIP_TRY(e, hipMemcpy(e->d_step_override, host_params, 24 * (size_t)e->cfg.num_envs, hipMemcpyHostToDevice));
    e->use_step_override = true;
    return MW_OK;
}

int mw_reset(mw_engine *e, const uint8_t *mask, const uint64_t *seeds, void *stream)
{
    if (!e) return MW_E_INVALID;
    ON_DEVICE_SYNC(e);
    world_changed(e);
    if (e->cfg.generator == MW_GEN_NONE && !seeds) return fail(e, MW_E_INVALID, "engine was created without a device-side generator");
    if (e->cfg.generator == MW_GEN_PROGRAM && !e->args.prog) return fail(e, MW_E_INVALID, "MW_GEN_PROGRAM: no placement program installed (mw_set_gen_program)");
    const int N = e->cfg.num_envs;
    hipStream_t st = (hipStream_t)stream;
    if (seeds) {
        std::vector<uint64_t> cur(5 * (size_t)N);
        HIP_TRY(e, hipStreamSynchronize(st));
        HIP_TRY(e, hipMemcpy(cur.data(), e->args.rng, 40 * (size_t)N, hipMemcpyDeviceToHost));
        for (int i = 0; i < N; ++i)
            if (!mask || mask[i]) seed_env(e, cur.data(), i, seeds[i]);
        HIP_TRY(e, hipMemcpy(e->args.rng, cur.data(), 40 * (size_t)N, hipMemcpyHostToDevice));
    }
    // host-generated worlds (MW_GEN_NONE): seeds only re-seed the env's device stream, which then serves the per-step
    // domain-randomisation draws (miniworld.py:677-680); the world itself comes through mw_set_state / mw_set_geometry
    if (e->cfg.generator == MW_GEN_NONE) return MW_OK;
    if (mask) HIP_TRY(e, hipMemcpyAsync(e->d_mask, mask, N, hipMemcpyHostToDevice, st));
    auto gen = MW_BY_STREAM(e, mw_reset);
    const dim3 grid(e->cfg.generator == MW_GEN_MAZE ? N : (N + 63) / 64);
    const int all = mask ? 0 : 1;
    if (!e->spare_mode) {
        hipLaunchKernelGGL(gen, grid, dim3(64), 0, st, e->args, (const uint8_t *)e->d_mask, all, 0);
    } else {
        // spare mode: a fresh seed generates the live world directly; without seeds the env's pre-generated world is
        // taken (what the same-step auto-reset does, after the pending refills have been run); either way the spare
        // of a reset env is then regenerated from its stream
        auto refill = MW_BY_STREAM(e, mw_refill);
        if (seeds) {
            hipLaunchKernelGGL(gen, grid, dim3(64), 0, st, e->args, (const uint8_t *)e->d_mask, all, 1);
        } else {
            hipLaunchKernelGGL(refill, grid, dim3(64), 0, st, e->args);
            hipLaunchKernelGGL(mw_take_spare_kernel, dim3(N), dim3(64), 0, st, e->args, (const uint8_t *)e->d_mask, all);
        }
        hipLaunchKernelGGL(refill, grid, dim3(64), 0, st, e->args);
    }
    // the envs whose world was just written start an episode: mw_stack_refresh or their next push rebuilds their frame stacks
    if (e->stack.depth)
        hipLaunchKernelGGL(mw_stack_mark_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, (const uint8_t *)e->d_mask, all, stack_flags(e, e->stack.cur));
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_reset_where(mw_engine *e, const uint8_t *d_mask, const uint64_t *d_seeds, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (!d_mask || !d_seeds) return fail(e, MW_E_INVALID, "mw_reset_where: %s is null", d_mask ? "d_seeds" : "d_mask");
    if (e->cfg.generator == MW_GEN_PROGRAM && !e->args.prog) return fail(e, MW_E_INVALID, "MW_GEN_PROGRAM: no placement program installed (mw_set_gen_program)");
    ON_DEVICE(e);
    const int N = e->cfg.num_envs;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = refill_order(e, st)) return rc;
    // the caller's buffers no longer show the masked envs; the other envs keep their cached frames (the kernel advances the epochs of the
    // envs it writes)
    invalidate(e, reset_where_invalidation());
    const dim3 grid(e->cfg.generator == MW_GEN_MAZE ? N : (N + 63) / 64);
    // spare mode: the live world comes directly from the fresh stream and the env's spare is marked stale (mw_reset's seeded path); the
    // refill blocks of the next step, or its side-stream refill, regenerate it
    hipLaunchKernelGGL(MW_BY_STREAM(e, mw_reset_where), grid, dim3(64), 0, st, e->args, d_mask, d_seeds);
    if (e->stack.depth && e->cfg.generator != MW_GEN_NONE)
        hipLaunchKernelGGL(mw_stack_mark_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, d_mask, 0, stack_flags(e, e->stack.cur));
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_pcg64_draws(uint64_t seed, int32_t n, const int32_t *bounds, double *out)
{
    if (!out || n < 0) return MW_E_INVALID;
    uint64_t s[4];
    mwasset::pcg64_seed(seed, s);
    mw::Rng r{s[0], s[1], s[2], s[3], 1, 0u, 0u};
    for (int i = 0; i < n; ++i)
        out[i] = (bounds && bounds[i] > 0) ? (double)mw::rng_below(r, (uint32_t)bounds[i]) : mw::rng_double(r);
    return MW_OK;
}

int mw_check(mw_engine *e, void *stream)
{
    if (!e) return MW_E_INVALID;
    ON_DEVICE_SYNC(e);
    HIP_TRY(e, hipStreamSynchronize((hipStream_t)stream));
    uint32_t st = 0;
    HIP_TRY(e, hipMemcpy(&st, e->args.status, 4, hipMemcpyDeviceToHost));
    if (st & MW_ST_STATE_BAD) {
        // reported once, and ahead of the sticky bits below, which return first on every check once they are set: the bit belongs to the
        // calls since the last check (the stream is idle here); the other bits stay as they are, for the next check to report
        const uint32_t rest = st & ~MW_ST_STATE_BAD;
        HIP_TRY(e, hipMemcpy(e->args.status, &rest, 4, hipMemcpyHostToDevice));
        return fail(e, MW_E_INVALID, "mw_set_state_where skipped an env: its carrying outside -1 .. %d or an ent_kind outside %d .. %d", e->args.E - 1, MW_ENT_NONE, MW_ENT_FRAME);
    }
    if (st & MW_ST_NAV_BAD) {       // the same rule: once, then forgotten
        const uint32_t rest = st & ~MW_ST_NAV_BAD;
        HIP_TRY(e, hipMemcpy(e->args.status, &rest, 4, hipMemcpyHostToDevice));
        return fail(e, MW_E_INVALID, "mw_nav_build refused an env (its row of the field is all 0xFFFF): the grid does not cover the env's extent, or a cost would reach 0xFFFE");
    }
    if (st & MW_ST_SEEN_BAD) {      // and again
        const uint32_t rest = st & ~MW_ST_SEEN_BAD;
        HIP_TRY(e, hipMemcpy(e->args.status, &rest, 4, hipMemcpyHostToDevice));
        return fail(e, MW_E_INVALID, "mw_seen_update refused an env (its row of the map is zeroed, its count 0): the grid does not cover the env's extent");
    }
    if (st & MW_ST_DEPTH_BAD) {     // and again
        const uint32_t rest = st & ~MW_ST_DEPTH_BAD;
        HIP_TRY(e, hipMemcpy(e->args.status, &rest, 4, hipMemcpyHostToDevice));
        return fail(e, MW_E_INVALID, "mw_depth_project refused an env (its rows of the map are zeroed, its counts 0): the grid does not cover the env's extent");
    }
    if (st & MW_ST_LABELMAP_BAD) {  // and again
        const uint32_t rest = st & ~MW_ST_LABELMAP_BAD;
        HIP_TRY(e, hipMemcpy(e->args.status, &rest, 4, hipMemcpyHostToDevice));
        return fail(e, MW_E_INVALID, "mw_label_project refused an env (its map is zeroed, its cells 0, its positions NaN): the grid does not cover the env's extent");
    }
    if (st & MW_ST_VIS_OVERFLOW) return fail(e, MW_E_OVERFLOW, "more than max_visible=%d visible primitives in some env", e->cfg.max_visible);
    if (st & MW_ST_PLACEMENT_FAIL) return fail(e, MW_E_OVERFLOW, "device-side placement did not converge in some env");
    if (st & MW_ST_SNAPSHOT_BAD)
        return fail(e, MW_E_INVALID, "mw_snapshot_save / mw_snapshot_load / mw_snapshot_save_frames / mw_snapshot_load_frames (or an _at / _where form of them) skipped an item: an env or record index out of range, or a record "
                    "buffer of another layout (key mismatch)");
    return MW_OK;
}

int mw_raster_path(const mw_engine *e) { return e ? e->last_raster_path : MW_E_INVALID; }

int mw_debug_set_mesh_frame_seq(mw_engine *e, uint32_t seq)
{
    if (!e) return MW_E_INVALID;
    // (the work lists and the slow-path counters alternate with the sequence number's parity: keep it)
    if ((seq & 1u) != (e->mp.frame_seq & 1u)) return fail(e, MW_E_INVALID, "mw_debug_set_mesh_frame_seq: the parity of the sequence number must stay");
    frames_stale(e);
    e->mp.frame_seq = seq;
    return MW_OK;
}

int mw_debug_get_slow_heads(mw_engine *e, uint32_t *host_out, void *stream)
{
    if (!e || !host_out) return fail(e, MW_E_INVALID, "null argument");
    if (!e->mp.slow_head) return fail(e, MW_E_INVALID, "mw_debug_get_slow_heads: this engine has no mesh path buffers");
    ON_DEVICE(e);
    HIP_TRY(e, hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(e, hipMemcpy(host_out, e->mp.slow_head.get(), sizeof(uint32_t) * (size_t)e->cfg.num_envs * e->args.W * e->args.H, hipMemcpyDeviceToHost));
    return MW_OK;
}

int mw_get_list_lengths(mw_engine *e, int32_t first_env, int32_t count, int32_t *host_out, void *stream)
{
    if (!e || !host_out) return fail(e, MW_E_INVALID, "null argument");
    if (first_env < 0 || count <= 0 || first_env + count > e->cfg.num_envs) return fail(e, MW_E_INVALID, "env range out of bounds");
    ON_DEVICE(e);
    HIP_TRY(e, hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(e, hipMemcpy(host_out, e->args.nvis + first_env, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost));
    return MW_OK;
}

int mw_get_info(mw_engine *e, int32_t *d_health, double *d_ent_pos, int32_t ent_slot, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (!d_health && !d_ent_pos) return fail(e, MW_E_INVALID, "mw_get_info: nothing asked for");
    if (d_ent_pos && (ent_slot < 0 || ent_slot >= e->args.E)) return fail(e, MW_E_INVALID, "mw_get_info: entity slot %d out of range", ent_slot);
    // (the health array exists for the CollectHealth rule only: collecthealth.py:79-100)
    if (d_health && !e->args.health) return fail(e, MW_E_INVALID, "mw_get_info: this engine's task keeps no health (MW_TASK_COLLECT only)");
    return launch_info(e, e->args.E, e->args.health, e->args.epos, d_ent_pos ? ent_slot : 0, d_health, d_ent_pos, stream);
}

int mw_get_final_info(mw_engine *e, int32_t *d_health, double *d_goal_pos, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (!d_health && !d_goal_pos) return fail(e, MW_E_INVALID, "mw_get_final_info: nothing asked for");
    if (d_health && !e->args.final_health) return fail(e, MW_E_INVALID, "mw_get_final_info: this engine's task keeps no health (MW_TASK_COLLECT only)");
    // (the arrays are component-major like the state: the gather kernel of mw_get_info with slot 0 of a one-slot table)
    return launch_info(e, 1, e->args.final_health, e->args.final_goal, 0, d_health, d_goal_pos, stream);
}

int mw_get_reset_pending(mw_engine *e, uint8_t *d_out, void *stream)
{
    return e ? get_env_bytes(e, "mw_get_reset_pending", e->args.reset_pending, d_out, stream) : MW_E_INVALID;
}

int mw_get_frame_source(mw_engine *e, uint8_t *d_out, void *stream)
{
    return e ? get_env_bytes(e, "mw_get_frame_source", e->args.fc_source, d_out, stream) : MW_E_INVALID;
}

int mw_get_frame_plan(mw_engine *e, uint32_t *host_plan, int64_t words, int32_t *host_lengths, void *stream)
{
    if (!e || !host_plan || !host_lengths) return fail(e, MW_E_INVALID, "mw_get_frame_plan: null argument");
    const int N = e->cfg.num_envs;
    const size_t want = MW_PLAN_WORDS(N, frame_plan_ordered(N));
    if (words != (int64_t)want) return fail(e, MW_E_INVALID, "mw_get_frame_plan: %lld words given, the block has %zu", (long long)words, want);
    if (!e->plan_made) return fail(e, MW_E_INVALID, "mw_get_frame_plan: no frame of this engine has been planned yet");
    ON_DEVICE(e);
    HIP_TRY(e, hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(e, hipMemcpy(host_plan, e->d_plan[e->plan_cur ^ 1], want * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(e, hipMemcpy(host_lengths, e->args.nvis, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost));
    return MW_OK;
}

int mw_get_geom_built(mw_engine *e, uint8_t *host_out, void *stream)
{
    if (!e || !host_out) return fail(e, MW_E_INVALID, "mw_get_geom_built: null argument");
    ON_DEVICE(e);
    HIP_TRY(e, hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(e, hipMemcpy(host_out, e->d_geom_built, (size_t)e->cfg.num_envs, hipMemcpyDeviceToHost));
    return MW_OK;
}

int mw_get_frame_clean(mw_engine *e, uint8_t *d_out, void *stream)
{
    return e ? get_env_bytes(e, "mw_get_frame_clean", e->args.frame_clean, d_out, stream) : MW_E_INVALID;
}

int mw_kernel_time_ms(mw_engine *e, int32_t reset, double *raster_ms, double *setup_ms, int64_t *launches)
{
    if (!e) return MW_E_INVALID;
    ON_DEVICE(e);
    double r = 0, s = 0;
    int64_t n = 0;
    for (auto &ev : e->ev_used) {
        (void)hipEventSynchronize(ev.c.get());
        float t1 = 0, t2 = 0;
        (void)hipEventElapsedTime(&t1, ev.a.get(), ev.b.get());
        (void)hipEventElapsedTime(&t2, ev.b.get(), ev.c.get());
        s += t1; r += t2; ++n;
        e->ev_free.push_back(std::move(ev));
    }
    e->ev_used.clear();
    if (raster_ms) *raster_ms = n ? r / n : 0.0;
    if (setup_ms) *setup_ms = n ? s / n : 0.0;
    if (launches) *launches = n;
    e->timing = true;
    e->frame_count = 0;
    e->timing_stride = reset > 0 ? reset : MW_TIMING_STRIDE;
    if (reset < 0) e->timing = false;
    return MW_OK;
}

int mw_abi_version(void) { return MW_ABI_VERSION; }

}  // extern "C"

