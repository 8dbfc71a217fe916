// mwengine host runtime: the C ABI of include/mwengine.h on top of the HIP kernels.
// Owns the device-resident Structure-of-Arrays world state of N environments, the texture /
// mesh pools and the per-step scratch; never touches torch (the caller hands raw device
// pointers and a hipStream_t).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "mw_assets.h"
#include "mw_device.h"
#include "mw_kernels.h"
#include "mw_rng.h"

#define MW_TIMING_STRIDE 8

// mw_get_info: what the envs' step() returns in `info` beside the observation (collecthealth.py:100, tmaze.py:89, ymaze.py:125)
extern "C" __global__ void mw_info_kernel(int N, int E, const int32_t *health, const double *epos, int slot, int32_t *out_health, double *out_pos)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (out_health) out_health[i] = health[i];
    if (out_pos)
        for (int c = 0; c < 3; ++c) out_pos[(size_t)i * 3 + c] = epos[((size_t)c * E + slot) * N + i];
}

// Same-step auto-reset with final observations (mw_set_final_obs), behind the first pass's step kernel: the envs whose episode
// ended with this step — reset_pending, set by the step kernel run as the next-step mode's terminal step — in ascending order, as
// list[0] = count, list[1 + i] = env.  One workgroup, ballot compaction, deterministic.  The finished worlds' pending removals go:
// the same-step install drops them (a picked object's world is replaced; CollectHealth's consumed kit does not respawn).
extern "C" __global__ __launch_bounds__(1024) void mw_final_list_kernel(int N, const uint8_t *__restrict__ pending, int32_t *__restrict__ pending_remove,
                                                                       int32_t *__restrict__ list)
{
    __shared__ int s_wave[16];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int i0 = 0; i0 < N; i0 += 1024) {
        const int i = i0 + tid;
        const bool p = i < N && pending[i] != 0;
        const unsigned long long m = __ballot(p);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = base, total = 0;
        for (int w = 0; w < 16; ++w) {
            const int c = s_wave[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (p) {
            list[1 + before + __popcll(m & ((1ull << lane) - 1ull))] = i;
            pending_remove[i] = -1;
        }
        base += total;
        __syncthreads();        // (s_wave is rewritten by the next round)
    }
    if (tid == 0) list[0] = base;
}

// ... behind the first pass's frame: the listed envs' rows of the observation (and depth) into the final buffers.  Grid N, one
// workgroup per list slot.
extern "C" __global__ __launch_bounds__(256) void mw_final_copy_kernel(const int32_t *__restrict__ list, const uint8_t *__restrict__ obs,
                                                                      uint8_t *__restrict__ final_obs, unsigned long long row_bytes,
                                                                      const float *__restrict__ depth, float *__restrict__ final_depth, int depth_row)
{
    if ((int)blockIdx.x >= list[0]) return;
    const size_t env = (size_t)list[1 + blockIdx.x];
    const uint8_t *src = obs + env * row_bytes;
    uint8_t *dst = final_obs + env * row_bytes;
    if ((((uintptr_t)obs | (uintptr_t)final_obs | (uintptr_t)row_bytes) & 15u) == 0) {
        for (size_t k = threadIdx.x; k < row_bytes / 16; k += blockDim.x)
            reinterpret_cast<uint4 *>(dst)[k] = reinterpret_cast<const uint4 *>(src)[k];
    } else {
        for (size_t k = threadIdx.x; k < row_bytes; k += blockDim.x) dst[k] = src[k];
    }
    if (depth && final_depth)
        for (int k = threadIdx.x; k < depth_row; k += blockDim.x) final_depth[env * depth_row + k] = depth[env * depth_row + k];
}

namespace {
thread_local std::string g_create_error;

// Owning handles: every device buffer, stream and event of an engine has exactly one, and is released with it (mw_destroy keeps
// the engine's device current while the members go).  The kernels keep taking raw pointers (MwArgs and the launches: .get()).
template <typename H, hipError_t (*destroy)(H)>
struct Destroy { void operator()(H h) const { (void)destroy(h); } };
template <typename T>
using DevBuf = std::unique_ptr<T, Destroy<void *, hipFree>>;
using Stream = std::unique_ptr<ihipStream_t, Destroy<hipStream_t, hipStreamDestroy>>;
using Event = std::unique_ptr<ihipEvent_t, Destroy<hipEvent_t, hipEventDestroy>>;
}

struct mw_engine {
    mw_config cfg{};
    MwArgs args{};
    MwArgs *d_gen_live = nullptr, *d_gen_spare = nullptr;   // device copies of the argument block for the generators
    bool spare_mode = false;
    bool side_refill_pending = false;   // Maze: spare worlds are regenerated by a kernel of their own on the side stream, across steps
    MwSpare spare_host{};
    int32_t *d_spare_dummy = nullptr;   // carry / step / picked written by the generator in spare mode go nowhere
    int n_sets = 1;
    std::string err;
    // the buffers mw_create makes for the engine's lifetime (world state, records, scratch); MwArgs and the members below point into them
    std::vector<DevBuf<void>> fixed;
    // textures
    std::vector<MwTexDesc> tex_desc;
    std::vector<std::vector<uint32_t>> tex_data;   // per texture: every level as 32-byte footprint records (build_pyramid)
    DevBuf<uint32_t> d_texels;          // the descriptor table, then the texels (upload_textures)
    size_t texel_cap = 0;               // dwords d_texels holds
    MwMeshDesc *d_meshdesc = nullptr;
    std::vector<mwasset::HostMesh> meshes;      // per mesh id (ntris = 0: none); the pools below are repacked from them (mw_upload_mesh)
    struct MeshPools {
        DevBuf<float> pos, nrm, rgb, uv;
        DevBuf<float> stream, attr;     // the entity kernel's triangle streams (rasterisation order): positions (meshes without a vertex table), vertex attributes
        DevBuf<float4> vpos;            // the meshes' distinct positions (MwMeshDesc::vfirst, nverts)
        DevBuf<uint2> idx;              // per triangle of the rasterisation order: three 16-bit indices into the mesh's table, the triangle's index
    } pools;
    int max_mesh_verts = 0, max_mesh_tris = 0;
    bool have_meshes = false, visible_attr_set = false;
    Stream side_stream;     // low priority: the Maze's spare-world refills beside the steps
    Event ev_fork;
    // The mesh path: what a frame with mesh entities uses beside the triangle records and the pools (ensure_mesh_buffers fills it)
    struct MeshPath {
        Stream quad_stream;     // low priority: the raster kernel's first part (every tile no mesh can touch) beside the mesh kernels
        Event ev_fork, ev_join;
        DevBuf<uint32_t> view_keys;     // sample keys of the generic-resolution path
        size_t view_keys_bytes = 0;
        DevBuf<uint32_t> keys;          // [N][H][W][8] sample keys of the mesh scatter kernel (all-ones between frames)
        bool keys_dirty = true;
        DevBuf<int32_t> slow_count;     // [2 parities][2][N] listed triangles, fragments; then ent_counter
        int32_t *ent_counter = nullptr; // [2][MW_CNT_WORDS] the work lists' lengths and cursors (mw_device.h: ent_list_n), this frame's and the next frame's
        DevBuf<uint32_t> slow_envs;     // [2][N] the envs with triangles across a frustum plane (written by the entity kernel: the slow kernel's work list)
        DevBuf<uint32_t> tile_list;     // [N * n_tiles] the mesh tiles' work list (written by the geometry kernel)
        DevBuf<uint32_t> ent_list;      // [2][N * slots] the work list itself (written by the geometry kernel)
        int ent_list_cap = 0;
        uint32_t frame_seq = 1;         // frames drawn through the lists: the parity picks their side, the low 16 bits stamp the slow fragments (mesh_frame)
        DevBuf<uint32_t> slow_tris; DevBuf<float4> slow_frags; DevBuf<uint32_t> slow_head;     // (mw_mesh_slow_kernel)
        DevBuf<float> plane_cache;      // [N][plane_cap][16] + [N][plane_cap][4] attribute planes of the mesh triangles that win samples (mw_raster_mesh.hip)
        int plane_cap = 0;
        static constexpr int mesh_tile_waves = 16384;   // wavefronts of the mesh tiles' launch, wavefront w taking the items w, w + 16384, ... of the list (4096: 139 us, 8192: 122, 16384: 112)
        static constexpr int ent_blocks = 512;          // the entity kernel's persistent workgroups: two of 512 lanes per CU (768 of them, or 256 of 1024 lanes: measured slower)
        static constexpr int slow_waves = 8192;         // wavefronts of the slow kernel's launch (4096: 59 us, 8192: 55)
    } mp;
    int obs_layout = MW_OBS_HWC_U8;
    // scratch for the step outputs when the caller passes none
    float *d_reward_scratch = nullptr;
    uint8_t *d_flag_scratch = nullptr;
    int32_t *d_action_scratch = nullptr;
    uint8_t *d_mask = nullptr;
    double *d_step_override = nullptr;
    bool use_step_override = false;
    // timing
    bool timing = false;
    int timing_stride = MW_TIMING_STRIDE;
    uint64_t frame_count = 0;
    struct Ev { Event a, b, c; };
    std::vector<Ev> ev_used, ev_free;
    int waves_per_env = 0;
    DevBuf<MwProgram> d_prog;           // placement program (mw_set_gen_program) and the tables it points at
    DevBuf<mw_poly> d_prog_polys;
    DevBuf<int32_t> d_prog_room, d_prog_surf;
    DevBuf<double> d_prog_m, d_prog_segs;
    int texel_bytes = 4;
    int dbg_flags = 0;       // MW_DEBUG_FLAGS & MW_DEBUG_BITS: perf experiments only (bit0: flat shading)
    int last_raster_path = -1;  // mw_raster_path
    // switches read once by mw_create (the launch path never touches the environment): the ones tests and A/B baselines use.
    // (The experiments that lost their A/B — the step fused into the geometry kernel, the quad kernel on big scenes, the stream
    // arrangements of the mesh kernels — are gone from the library: tools/experiments/ keeps the record and the patches.)
    bool use_k2q = true;        // MW_K2Q=0: the tile kernels of mw_raster.hip for small scenes too (the A/B baseline of the quad kernel)
    bool k2q_ok = false;        // the frame fits the quad kernel's LDS plan
    bool generic_raster = false;    // MW_GENERIC_RASTER=1: msaa = 4 frames through the generic-resolution kernel (tests run both)
    unsigned long long *d_ent_prof = nullptr;   // MW_ENT_PROF=<file>: the mesh entity kernel's per-env times and counts of the last frame, [N][8], dumped by mw_destroy
    unsigned long long *d_k2q_prof = nullptr;   // MW_K2Q_PROF=<file>: s_memtime stamps of the quad kernel's phases, [N][8 waves][8], dumped by mw_destroy
    // mw_set_final_obs: the terminal frames of the envs whose episode ends in a same-step step (null: off); the list of those envs
    uint8_t *final_obs = nullptr;
    float *final_depth = nullptr;
    int32_t *d_final_list = nullptr;    // [1 + N]: count, envs (mw_final_list_kernel)
    // mw_set_frame_reuse: the caller's buffers keep their frames from step to step, so a step need not redraw an env whose frame
    // did not change (MwArgs::frame_clean).  `held`: the buffers that hold every env's current agent-view frame, and their layout —
    // set by a whole plain frame (launch_frame), dropped by every other frame and by every entry point that writes something a
    // frame depends on (drop_held_frame).
    bool frame_reuse = false;
    struct { uint8_t *obs = nullptr; float *depth = nullptr; int layout = 0; bool valid = false; } held;
    // mw_set_frame_cache: per env the last `slots` distinct frames the quad kernel drew, with their keys (mw_kernels.h).  The engine's
    // own copies: unlike frame reuse it needs no promise about the caller's buffers.  `dirty`: an entry point wrote something a
    // frame depends on (drop_frame_cache) — the next frame that uses the cache clears the key table first, on its own stream.
    struct {
        int slots = 0;
        DevBuf<uint8_t> frames;         // [N][slots][H W 3]
        DevBuf<float> depth;            // [N][slots][H W], allocated by the first frame with a depth output
        DevBuf<uint64_t> meta;          // [N][MW_FC_META_WORDS(slots)]
        DevBuf<MwFcArgs> d_args;        // the quad kernel's view of the above (mw_device.h), rewritten with the clear when a buffer changed
        MwFcArgs args{};
        bool args_stale = true;
        bool with_depth = false;        // the cached frames were drawn with a depth output
        bool dirty = true;
    } fc;
    // mw_set_frame_stack: the caller's ring (depth = 0: off), the layout and frame size it was set under, the pushes so far — a host
    // counter, every launch gets its phase by value — and the engine's flag bytes, [2][N] (MW_STACK_*): a push or refresh reads
    // flags[cur] and writes the other half, which becomes the current one (mw_stack.hip); the host's marks go to flags[cur]
    struct {
        int depth = 0, pad = 0, layout = 0, cur = 0;
        uint8_t *ring = nullptr, *final_stack = nullptr;
        size_t frame_bytes = 0;
        int64_t pushes = 0;
        uint8_t *flags = nullptr;
    } stack;
    // mw_snapshot_*: what of the configuration shapes a record, the layout that follows from it (mw_snapshot.h), the copy kernels'
    // table of the engine's arrays, and the event that orders a call behind the side stream's refills
    MwSnapConfig snap_cfg{};
    MwSnapLayout snap_layout{};
    MwSnapTable *d_snap_tab = nullptr;
    int snap_chunks_per_item = 0;       // blob workgroups per item: geometry sets x (polygon chunks + segment chunks), as in the table
    Event ev_refill_done;
};

namespace {

int fail(mw_engine *e, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (e) e->err = buf; else g_create_error = buf;
    return code;
}

#define HIP_TRY(e, call)                                                                         \
    do {                                                                                         \
        hipError_t _st = (call);                                                                 \
        if (_st != hipSuccess)                                                                   \
            return fail(e, MW_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_st), __FILE__, __LINE__); \
    } while (0)

// count elements of T (at least one), zeroed unless asked otherwise; `out` is left as it was on failure
template <typename T>
int dev_alloc(mw_engine *e, DevBuf<T> &out, size_t count, bool zero = true)
{
    void *p = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    hipError_t st = hipMalloc(&p, bytes);
    if (st != hipSuccess) return fail(e, MW_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(st));
    DevBuf<T> buf(static_cast<T *>(p));
    if (zero) {
        st = hipMemset(p, 0, bytes);
        if (st != hipSuccess) return fail(e, MW_E_HIP, "hipMemset failed: %s", hipGetErrorString(st));
    }
    out = std::move(buf);
    return MW_OK;
}

// ... one of mw_create's buffers: *out points into it, the engine owns it until it is destroyed
template <typename T>
int fixed_alloc(mw_engine *e, T **out, size_t count)
{
    DevBuf<T> buf;
    if (const int rc = dev_alloc(e, buf, count)) return rc;
    *out = buf.get();
    e->fixed.emplace_back(std::move(buf));
    return MW_OK;
}

// Grows a buffer to `want` units of `unit` bytes (`have`: what it holds): the new buffer is allocated beside the old one, which stays
// in place if that fails; the device finishes whatever may still read the old one before it is released.
template <typename T, typename C>
int grow(mw_engine *e, DevBuf<T> &buf, C &have, C want, size_t unit)
{
    if (want <= have) return MW_OK;
    DevBuf<T> fresh;
    if (const int rc = dev_alloc(e, fresh, (size_t)want * unit / sizeof(T), false)) return rc;
    (void)hipDeviceSynchronize();
    buf = std::move(fresh);
    have = want;
    return MW_OK;
}

hipError_t make_event(Event &out, unsigned flags = hipEventDisableTiming)
{
    hipEvent_t ev = nullptr;
    const hipError_t st = hipEventCreateWithFlags(&ev, flags);
    if (st == hipSuccess) out.reset(ev);
    return st;
}

// a low-priority stream: the filler work beside the caller's stream must not keep the main kernels' workgroups out
hipError_t make_stream(Stream &out)
{
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    hipStream_t s = nullptr;
    const hipError_t st = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio_least);
    if (st == hipSuccess) out.reset(s);
    return st;
}

// K1 for the engine's random stream (the device code is compiled once per stream, mw_rng.h): the dense form for
// lanes = k1_dense_lanes(e) > 0, the wave-per-env form otherwise
auto k1_of(const mw_engine *e, int lanes) -> decltype(&mw_step_setup_kernel)
{
    const bool pcg = e->cfg.rng_mode == MW_RNG_PCG64;
    if (lanes) return pcg ? mw_step_setup_dense_pcg_kernel : mw_step_setup_dense_kernel;
    return pcg ? mw_step_setup_pcg_kernel : mw_step_setup_kernel;
}

// ... and mw_step_repeat's K1 (the same two forms around the sub-step loop)
auto k1_repeat_of(const mw_engine *e, int lanes) -> decltype(&mw_step_repeat_kernel)
{
    const bool pcg = e->cfg.rng_mode == MW_RNG_PCG64;
    if (lanes) return pcg ? mw_step_repeat_dense_pcg_kernel : mw_step_repeat_dense_kernel;
    return pcg ? mw_step_repeat_pcg_kernel : mw_step_repeat_kernel;
}

// ... and mw_step_plan's (the loop with one action per sub-step)
auto k1_plan_of(const mw_engine *e, int lanes) -> decltype(&mw_step_plan_kernel)
{
    const bool pcg = e->cfg.rng_mode == MW_RNG_PCG64;
    if (lanes) return pcg ? mw_step_plan_dense_pcg_kernel : mw_step_plan_dense_kernel;
    return pcg ? mw_step_plan_pcg_kernel : mw_step_plan_kernel;
}

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

// The tile and quad kernels' flag word (`dbg`): the MW_DEBUG_FLAGS experiment bits, the output layout (bits 8-9,
// mw_set_obs_layout), the part of a frame with mesh entities the launch draws (bits 4-5: 0 every tile, 1 those no mesh can touch,
// 2 those a mesh can, 3 the same from the geometry kernel's tile list) and the frame stamp of the slow-fragment chains (bits
// 16-31; 0 for the quad kernel, which reads bits 13-15 as experiment bits).  mw_create keeps only MW_DEBUG_BITS of MW_DEBUG_FLAGS,
// so that no experiment flag lands in the fields beside it.
#define MW_DEBUG_BITS 0xFCCF
// `reuse`: MW_RASTER_REUSE (mw_kernels.h), frames without mesh entities only — it shares the stamp's field.
int raster_flags(const mw_engine *e, int part, uint32_t stamp, bool reuse = false)
{
    return e->dbg_flags | e->obs_layout << 8 | part << 4 | (int)(stamp << 16) | (reuse && stamp == 0u ? MW_RASTER_REUSE : 0);
}
void drop_held_frame(mw_engine *e) { e->held.valid = false; }
// ... and the cached frames of every env: for the entry points that change what a state's frame looks like or the states themselves
// behind K1's back.  Not for frames (launch_frame): a render, a top view or a list pass leaves the state-to-frame function alone.
void drop_frame_cache(mw_engine *e) { e->fc.dirty = true; }

// bytes of one env's row of d_obs in the current output layout
size_t obs_row_bytes(const mw_engine *e)
{
    return (size_t)e->cfg.obs_width * e->cfg.obs_height * (e->obs_layout == MW_OBS_GREY_F64 ? 8 : 3);
}

// Frame stacking (mw_set_frame_stack; kernels: mw_stack.hip).  phase of the last push: the window starts there (before the first push
// every slot a refresh wrote is valid, and the same formula gives depth - 1).
int stack_phase(const mw_engine *e) { return (int)((e->stack.pushes + e->stack.depth - 1) % e->stack.depth); }
uint8_t *stack_flags(const mw_engine *e, int half) { return e->stack.flags + (size_t)half * e->cfg.num_envs; }
// a push or refresh draws from rows of the layout and size the stack was set under: checked before anything is launched
int stack_check(mw_engine *e, const char *what)
{
    if (e->stack.depth && (e->stack.layout != e->obs_layout || e->stack.frame_bytes != obs_row_bytes(e)))
        return fail(e, MW_E_INVALID, "%s: the frame stack was set under obs layout %d, the engine is in layout %d now (mw_set_frame_stack again, or switch back)",
                    what, e->stack.layout, e->obs_layout);
    return MW_OK;
}
// the push behind a step's last raster kernel (term, trunc: the buffers the step kernel wrote), or the refresh (push = false)
int launch_stack(mw_engine *e, bool push, const uint8_t *d_obs, const uint8_t *term, const uint8_t *trunc, hipStream_t st)
{
    auto &s = e->stack;
    const int N = e->cfg.num_envs, phase = push ? (int)(s.pushes % s.depth) : stack_phase(e);
    const bool installs = e->cfg.generator != MW_GEN_NONE;      // auto-reset installs worlds (none with MW_GEN_NONE)
    const bool same = installs && e->cfg.autoreset == MW_AUTORESET_SAME_STEP, next = installs && e->cfg.autoreset == MW_AUTORESET_NEXT_STEP;
    const uint8_t *final_obs = push && same && s.final_stack ? e->final_obs : nullptr;
    uint8_t *final_stack = final_obs ? s.final_stack : nullptr;
    const bool wide = (((uintptr_t)d_obs | (uintptr_t)s.ring | (uintptr_t)final_obs | (uintptr_t)final_stack | (uintptr_t)s.frame_bytes) & 15u) == 0;
    const size_t units = s.frame_bytes / (wide ? 16 : 1), chunk = (size_t)MW_STACK_THREADS * MW_STACK_UNROLL;
    const dim3 grid(N, (unsigned)((units + chunk - 1) / chunk));
    const uint8_t *in = stack_flags(e, s.cur);
    uint8_t *out = stack_flags(e, s.cur ^ 1);
    if (push)
        hipLaunchKernelGGL(mw_stack_push_kernel, grid, dim3(MW_STACK_THREADS), 0, st, s.depth, s.pad, phase, (unsigned long long)s.frame_bytes, (int)wide, d_obs, s.ring,
                           in, out, same ? term : nullptr, same ? trunc : nullptr, next ? (const uint8_t *)e->args.reset_pending : nullptr, final_obs, final_stack);
    else
        hipLaunchKernelGGL(mw_stack_refresh_kernel, grid, dim3(MW_STACK_THREADS), 0, st, s.depth, s.pad, phase, (unsigned long long)s.frame_bytes, (int)wide, d_obs, s.ring,
                           in, out);
    HIP_TRY(e, hipGetLastError());
    s.cur ^= 1;
    if (push) ++s.pushes;
    return MW_OK;
}

// The tile / quad / mesh-scatter kernels keep edge values in 32 bits: |c_k| = |dcdx X - dcdy Y| <= 2 W H 2^16 has to stay below
// 2^31, i.e. W H < 16384 — 128 x 96 passes, 128 x 128 does not (a wall across the whole frame lost its triangle there);
// larger frames take the generic-resolution kernels (64-bit edge values).
bool tile_kernels_exact(int W, int H) { return W <= 128 && H <= 128 && W * H <= 128 * 96; }

// The frame is W x H, the size the caller asked for: the viewport, the projection and every output stride.  The raster grid is
// the frame rounded up to whole 16 x 4 tiles, ceil16(W) x ceil4(H): tiles_x, tiles_y, n_tiles.  A frame that is not the grid
// ("ragged": padding pixels right of column W - 1 or below row H - 1) takes, at 8 samples without mesh entities, with an even H
// and a grid inside the tile kernels' edge bound, the ragged tile kernels (mw_raster.hip, FMT -2: padding masked, per-pixel stores); any
// other ragged frame the generic-resolution kernels, which mask the padding per pixel too.  The quad kernel and the fixed-layout
// tile kernels take frames on the grid only ("Frame sizes").
bool frame_on_grid(int W, int H) { return W % MW_TILE_W == 0 && H % MW_TILE_H == 0; }
bool tile_path_ok(int W, int H) { return frame_on_grid(W, H) && tile_kernels_exact(W, H); }
// sizes mw_create and mw_render_view accept: at least one pixel, at most 255 tiles of grid in each direction (8-bit tile
// coordinates of the records' bounding boxes)
bool frame_size_ok(int W, int H)
{
    return W >= 1 && H >= 1 && W <= 255 * MW_TILE_W && H <= 255 * MW_TILE_H;
}

// lanes per env of the geometry kernel: the power of two that holds an env's triangles (two per polygon and box face, the
// agent marker), 8 .. 64 — except that the smallest scenes get 16 lanes for their up to 32 triangles: an env's lanes go over
// its triangles in rounds, and four envs per wavefront fill the chip with half the wavefronts of this one-wave-per-SIMD kernel
// (measured, 4096 Hallway envs: 64 lanes 117 us, 32: 86, 16: 79, 8: 101)
int geom_lanes(const mw_engine *e)
{
    const int items = 2 * (e->cfg.max_polys + 6 * e->cfg.max_ents + 1);      // one triangle per lane
    int L = 8;
    while (L < items && L < 64) L <<= 1;
    if (L == 32) L = 16;
    // mid-sized scenes (PickupObjects: 6 polygons + 5 entity slots = 74 triangles; no visiting order, no sifting): two envs per
    // wavefront — 2 048 envs are ONE round of this one-wave-per-SIMD kernel instead of two (K1 + KG 103 -> 71 us)
    if (L == 64 && !e->args.rec_order && e->cfg.max_polys <= 64) L = 32;
#if defined(MW_PERF_HOOKS) || defined(MW_TUNE_HOOKS)
    if (const char *s = getenv("MW_GEOM_LANES")) { const int v = atoi(s); if ((v == 8 || v == 16 || v == 32 || v == 64) && v >= L) L = v; }
#endif
    return L;
}

// Lanes per env of the dense K1 (mw_setup_dense.hip), or 0 when the step has to go through the wave-per-env kernel: big
// scenes, CollectHealth, or too many slots to pack two envs into a wavefront.
int k1_dense_lanes(const mw_engine *e)
{
    if (e->args.rec_order || e->cfg.task == MW_TASK_COLLECT) return 0;
    // at least two envs per wavefront: with one, every lane repeats the env's scalar work for nothing and the wave-per-env
    // kernel's lane-cooperative collision tests win (PickupObjects, 35 slots: 62 us dense against 47 us)
    const int lanes = e->cfg.max_polys + 6 * e->cfg.max_ents;
    return lanes <= 32 ? lanes : 0;
}

// (re)seed env i in a host copy of the uint64[4][N] rng array
void seed_env(const mw_engine *e, uint64_t *rng, int i, uint64_t seed)
{
    const size_t N = (size_t)e->cfg.num_envs;
    if (e->cfg.rng_mode == MW_RNG_PCG64) {
        uint64_t s[4];
        mwasset::pcg64_seed(seed, s, mw::pcg64_step);
        for (int k = 0; k < 4; ++k) rng[(size_t)k * N + i] = s[k];
        rng[4 * N + i] = 0;
    } else {
        rng[i] = seed; rng[N + i] = 0; rng[2 * N + i] = 0; rng[3 * N + i] = 0; rng[4 * N + i] = 0;
    }
}

int sync_gen_args(mw_engine *e);

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

int pick_waves_per_env(const mw_engine *e)
{
    const int n_tiles = e->args.n_tiles;
    // enough wavefronts to fill 256 CUs x 4 SIMDs x 7 resident waves several times over (measured:
    // 15-25 waves per env beat 5 by ~7 % at 4096 envs), in divisors of n_tiles
    int best = n_tiles;
#if defined(MW_PERF_HOOKS) || defined(MW_TUNE_HOOKS)      // (MW_TUNE_HOOKS: the launch-shape overrides alone, without the perf build's counters)
    if (const char *s = getenv("MW_WAVES_PER_ENV")) { const int v = atoi(s); if (v > 0 && n_tiles % v == 0) return v; }
#endif
    for (int w = 1; w <= n_tiles; ++w) {
        if (n_tiles % w) continue;
        if ((long long)e->cfg.num_envs * w >= 49152) { best = w; break; }
    }
    return best;
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
    int rc;
    if ((rc = xfer(e, [&](int k, int) { return pos[k]; }, h->agent_pos, first, count, 1, 3, to_device)) || (rc = env(a.adir, h->agent_dir, 1)) || (rc = env(a.cam, h->cam, 4)) || (rc = env(a.light, h->light, 12)) ||
        (rc = env(a.carry, h->carrying, 1)) || (rc = env(a.step, h->step_count, 1)) || (rc = env(a.picked, h->num_picked_up, 1)) ||
        (rc = ent(a.ekind, h->ent_kind, 1)) || (rc = ent(a.emesh, h->ent_mesh, 1)) || (rc = ent(a.estatic, h->ent_static, 1)) ||
        (rc = ent(a.epos, h->ent_pos, 3)) || (rc = ent(a.edir, h->ent_dir, 1)) || (rc = ent(a.egeom, h->ent_geom, 9)) ||
        (rc = env(a.extent, h->extent, 4)))
        return rc;
    return MW_OK;
}

// every entry point runs on the engine's device, whatever the calling thread's current device is (two engines
// on different GPUs in one process; torch's current device != cfg.device_id)
#define ON_DEVICE(e) do { hipError_t sd_ = hipSetDevice((e)->cfg.device_id); \
        if (sd_ != hipSuccess) return fail((e), MW_E_HIP, "hipSetDevice(%d): %s", (e)->cfg.device_id, hipGetErrorString(sd_)); } while (0)

// ... and, for every entry point but the step / render ones, after the spare-world refills still running on the side stream
#define ON_DEVICE_SYNC(e) do { ON_DEVICE(e); if ((e)->side_refill_pending) { (void)hipStreamSynchronize((e)->side_stream.get()); \
        (e)->side_refill_pending = false; } } while (0)

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

// Device copies of the argument block for the generators (live state; spare state with the world pointers
// redirected): generate_world indexes the block dynamically, which a by-value kernarg would turn into a scratch copy.
int sync_gen_args(mw_engine *e)
{
    if (e->cfg.generator == MW_GEN_NONE) return MW_OK;
    MwArgs live = e->args;
    HIP_TRY(e, hipMemcpy(e->d_gen_live, &live, sizeof live, hipMemcpyHostToDevice));
    if (e->spare_mode) {
        // everything of the world goes to the spare arrays; the random stream (rng) and the status word stay the live ones
        MwArgs sa = e->args;
        const MwSpare &sp = e->spare_host;
        sa.ax = sp.ax; sa.ay = sp.ay; sa.az = sp.az; sa.adir = sp.adir; sa.cam = sp.cam; sa.light = sp.light; sa.extent = sp.extent;
        sa.ekind = sp.ekind; sa.emesh = sp.emesh; sa.estatic = sp.estatic; sa.epos = sp.epos; sa.edir = sp.edir; sa.egeom = sp.egeom;
        sa.carry = e->d_spare_dummy; sa.step = e->d_spare_dummy + e->cfg.num_envs; sa.picked = e->d_spare_dummy + 2 * (size_t)e->cfg.num_envs;
        if (!e->cfg.shared_geometry) { sa.polys = sp.polys; sa.npolys = sp.npolys; sa.segs = sp.segs; sa.nsegs = sp.nsegs; sa.occ_valid = nullptr; sa.occ_cache = nullptr; }
        sa.spare = nullptr;
        HIP_TRY(e, hipMemcpy(e->d_gen_spare, &sa, sizeof sa, hipMemcpyHostToDevice));
    }
    return MW_OK;
}

// Which kernels draw a frame of the engine's size (mw_raster_path), and the forms of them the launches pick: the one statement
// of these conditions — launch_frame, the frame's mesh lists and ensure_mesh_buffers take their answer from here.  Inputs: msaa,
// W x H, resident meshes, a visiting order, the MW_K2Q / MW_GENERIC_RASTER switches; the frame's layout, debug flags, depth.
struct RasterPath {
    int path;           // MW_PATH_TILE, MW_PATH_QUAD, MW_PATH_QUAD_MESH, MW_PATH_GENERIC
    bool mesh;          // mesh entities through the tile / quad kernels: the frame runs the mesh chain (launch_mesh_chain) on the mesh path's lists
    bool quad4;         // the quad kernel at 4 samples
    // big scene: a visiting order exists; an output layout other than HWC or debug flags; a frame off the 16 x 4 grid; depth asked for
    bool big, general, ragged, depth;
};
RasterPath raster_path(const mw_engine *e, bool depth)
{
    const MwArgs &a = e->args; const int S = e->cfg.msaa;
    RasterPath p{MW_PATH_GENERIC, false, false, a.rec_order != nullptr, e->obs_layout != MW_OBS_HWC_U8 || e->dbg_flags != 0, !frame_on_grid(a.W, a.H), depth};
    // the quad kernel (mw_rasterq.hip): small scenes without a visiting order, frames that fit its LDS plan — 8 samples (the
    // hot path) and 4 (llvmpipe's GL_MAX_SAMPLES: the reference's own frames run through the same code); with mesh entities
    // it draws the tiles no mesh can touch (8 samples only)
    // (big scenes — a visiting order exists — keep the tile kernels: their near-to-far order with its early exit is the better fit
    // for deep scenes; the quad kernel on the Maze was measured and lost, tools/experiments/README.md)
    const bool k2q = e->use_k2q && e->k2q_ok && !p.big && !(S == 4 && (e->have_meshes || e->generic_raster));
    // a ragged frame the ragged tile kernels draw (frame_on_grid).  The even H: the tile kernels' 2x2 quads (texture lod) pair image rows from
    // the top, GL pairs window rows from the bottom (mw_frag.h), and the two agree only then.  Odd heights take the generic-resolution kernels.
    const bool ragged_tiles = !e->have_meshes && p.ragged && a.H % 2 == 0 && tile_kernels_exact(a.tiles_x * MW_TILE_W, a.tiles_y * MW_TILE_H);
    p.quad4 = k2q && S == 4;
    // FrameBuffer's fallback sample counts (opengl.py:229-231: a driver that clamps GL_MAX_SAMPLES gets 4 or 1
    // samples), observations beyond 128 x 128 (the tile kernels' 24-bit edge arithmetic) and frames off the 16 x 4 grid:
    // the generic-resolution kernels, 64-bit edge values, exact packed-key resolution, every output layout, the whole
    // batch in one grid (blockIdx.y = env)
    const bool generic = S != 8 || (!tile_path_ok(a.W, a.H) && !ragged_tiles);
    p.mesh = !p.quad4 && !generic && e->have_meshes;
    p.path = p.quad4 ? MW_PATH_QUAD : generic ? MW_PATH_GENERIC : !k2q ? MW_PATH_TILE : p.mesh ? MW_PATH_QUAD_MESH : MW_PATH_QUAD;
    return p;
}

// Fills mw_engine::MeshPath: everything a frame with mesh entities needs beyond the triangle records — the plane cache (one record
// per mesh triangle that can be in view: the geometry kernel admits 0xC000 per env), the sample keys of the tiles a mesh can touch,
// the slow-path lists, the mesh stream; for the generic-resolution path the view keys.  Called by mw_upload_mesh (a synchronous
// entry point): a frame never allocates, never synchronises.  Failure-atomic: either every buffer of a group is there or none.
int ensure_mesh_buffers(mw_engine *e)
{
    const MwArgs &a = e->args; mw_engine::MeshPath &m = e->mp;
    const size_t N = (size_t)e->cfg.num_envs;
    // the stream of the raster kernel's first part in a frame with meshes: LOW priority — the mesh kernels on the caller's stream are the
    // critical path, the quad kernel fills the CUs around them
    if (!m.quad_stream) HIP_TRY(e, make_stream(m.quad_stream));
    for (Event *ev : {&m.ev_fork, &m.ev_join}) if (!*ev) HIP_TRY(e, make_event(*ev));
    if (raster_path(e, false).path == MW_PATH_GENERIC)
        return grow(e, m.view_keys, m.view_keys_bytes, N * a.W * a.H * e->cfg.msaa * 4, 1);
    if (a.W > 255 * MW_TILE_W || a.H > 255 * MW_TILE_H) return fail(e, MW_E_CAPACITY, "frame too large for the mesh tile rectangles");
    // the mesh tiles' work list (mw_geom.hip): a tile index in the 8 bits above the env, and one bit of a lane's 32-bit mask per tile
    // sub + k L.  tile_path_ok caps these frames at 192 tiles and the geometry kernel has at least 8 lanes per env, so
    // this holds today; a larger frame limit or fewer lanes must not leave mesh tiles undrawn (and their sample keys uncleared) in silence
    if (a.n_tiles > 255 || a.n_tiles > 32 * geom_lanes(e))
        return fail(e, MW_E_CAPACITY, "%d tiles per frame: the mesh tiles' work list holds 255 (8-bit tile index) and 32 per lane of the geometry kernel (%d lanes)", a.n_tiles, geom_lanes(e));
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

// The frames of a same-step step with final observations (mw_step): FRAME_TERMINAL — the step kernel runs as the next-step mode's
// terminal step (no install; reset_pending marks the finished envs), the list of those envs is built behind it, and the frame
// shows every env's state after the step (terminal states for the finished envs); FRAME_LIST — no step, the frame of the listed
// envs only (their new worlds), through the list forms of the geometry and raster kernels.
enum { FRAME_ALL = 0, FRAME_TERMINAL = 1, FRAME_LIST = 2 };

// what the stages of one frame share (launch_frame)
struct Frame {
    MwArgs a;
    int view_flags;
    const int32_t *list;        // FRAME_LIST: the list forms draw the listed envs only
    uint8_t *obs; float *depth; hipStream_t st; bool reuse;
    int fc_slots;               // > 0: the quad kernel consults and fills the frame cache
    uint8_t *source;            // the per-env source byte (a plain step), or null
    RasterPath p;
    MeshFrame mf;               // p.mesh only
};

// Which step kernels a call runs: mw_step's (repeat = horizon = 0), mw_step_repeat's (repeat > 0: up to `repeat` sub-steps per env with
// its action, the executed count into nsteps) or mw_step_plan's (horizon > 0: d_actions is the plans, [horizon][N], and each sub-step's
// own reward goes to step_reward) — the same launch shape for all three.
struct StepCall {
    int repeat = 0;
    int32_t *nsteps = nullptr;
    int horizon = 0;
    float *step_reward = nullptr;
};

// the step kernel (frameless: of an mw_step_plan that no frame follows)
void launch_k1(mw_engine *e, const MwArgs &ak, hipStream_t st, bool async_refill, const int32_t *d_actions, float *d_reward, uint8_t *d_term,
               uint8_t *d_trunc, const StepCall &c, bool frameless = false)
{
    const int N = e->cfg.num_envs;
    // spare mode: blocks appended to the grid regenerate the spare worlds consumed in earlier steps, beside the step itself
    // (the Maze's go to the side stream: launch_side_refill)
    const int refill_blocks = (e->spare_mode && !async_refill) ? (N + 63) / 64 : 0;
    const int lanes = k1_dense_lanes(e), epw = lanes ? 64 / lanes : 1;      // envs per workgroup
    const dim3 grid((N + epw - 1) / epw + refill_blocks);
    float *reward = d_reward ? d_reward : e->d_reward_scratch;
    uint8_t *term = d_term ? d_term : e->d_flag_scratch, *trunc = d_trunc ? d_trunc : e->d_flag_scratch + N;
    if (c.horizon > 0)
        hipLaunchKernelGGL(k1_plan_of(e, lanes), grid, dim3(64), 0, st, ak, lanes, d_actions, reward, term, trunc, c.horizon, c.nsteps, c.step_reward, frameless ? 1 : 0);
    else if (c.repeat > 0) hipLaunchKernelGGL(k1_repeat_of(e, lanes), grid, dim3(64), 0, st, ak, lanes, d_actions, reward, term, trunc, c.repeat, c.nsteps);
    else hipLaunchKernelGGL(k1_of(e, lanes), grid, dim3(64), 0, st, ak, lanes, d_actions, reward, term, trunc);
}

// the step (a render-only frame has none), the list of a FRAME_TERMINAL step's finished envs, the frame's vertex half, CollectHealth's respawns
void launch_step_and_geometry(mw_engine *e, const Frame &f, bool do_step, int frame, bool async_refill, const int32_t *d_actions,
                              float *d_reward, uint8_t *d_term, uint8_t *d_trunc, const StepCall &c)
{
    const MwArgs &a = f.a; const int N = e->cfg.num_envs;
    if (do_step) {
        MwArgs ak = a;          // the step kernel's arguments: the first pass of a final-observation step runs as a next-step terminal step
        if (frame == FRAME_TERMINAL) ak.autoreset = MW_AUTORESET_NEXT_STEP;
        launch_k1(e, ak, f.st, async_refill, d_actions, d_reward, d_term, d_trunc, c);
    }
    if (frame == FRAME_TERMINAL)
        hipLaunchKernelGGL(mw_final_list_kernel, dim3(1), dim3(1024), 0, f.st, N, (const uint8_t *)a.reset_pending, a.pending_remove, e->d_final_list);
    // the frame's vertex half: camera, lighting, transform, clipping, triangle setup (mw_geom.hip)
    const int L = geom_lanes(e), epw = 64 / L;
    launch(geom_kernel_of(L, e->cfg.msaa), f.list, dim3((N + epw - 1) / epw), dim3(64), 0, f.st, a, f.view_flags, e->cfg.msaa, L, N);
    if (do_step && e->cfg.task == MW_TASK_COLLECT)
        hipLaunchKernelGGL(e->cfg.rng_mode == MW_RNG_PCG64 ? mw_collect_respawn_pcg_kernel : mw_collect_respawn_kernel, dim3((N + 63) / 64), dim3(64), 0, f.st, a);
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
    hipLaunchKernelGGL(e->cfg.rng_mode == MW_RNG_PCG64 ? mw_refill_pcg_kernel : mw_refill_kernel, dim3(e->cfg.num_envs), dim3(64), 0, e->side_stream.get(), e->args);
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

// the quad kernel (mw_rasterq.hip); part: raster_flags
void launch_quad(const mw_engine *e, const Frame &f, int part, hipStream_t st)
{
    const MwArgs &a = f.a;
    const int lds = mw_rasterq_lds_bytes(e->cfg.msaa, a.W, a.H, a.n_tiles, f.depth ? 1 : 0);
    launch(f.p.quad4 ? MW_PAIR(mw_rasterq4) : MW_PAIR(mw_rasterq), f.list, dim3(e->cfg.num_envs), dim3(MWQ_THREADS), (size_t)lds, st, a.N, a.W, a.H, a.max_vis,
           a.tiles_x, a.n_tiles, (const float *)a.rec_raster, (const float *)a.rec_shade, (const float *)a.rec_cull,
           (const int32_t *)a.nvis, (const float *)a.envhdr, a.texels, f.obs, f.depth, raster_flags(e, part, 0u, f.reuse), e->texel_bytes, e->d_k2q_prof,
           (const uint8_t *)a.frame_clean, f.fc_slots ? (const MwFcArgs *)e->fc.d_args.get() : nullptr, f.source);
}

// the tile kernels (mw_raster.hip); part: raster_flags
void launch_tiles(const mw_engine *e, const Frame &f, int part, hipStream_t st)
{
    const MwArgs &a = f.a; const mw_engine::MeshPath &m = e->mp;
    const int N = e->cfg.num_envs, wpe = e->waves_per_env;
    // big scenes (a visiting order exists): records read in place, near to far; otherwise the env's records are staged
    // in LDS when there are at most MW_LDS_RECS of them (a wave whose env holds more reads them in place).
    const int lds_recs = a.max_vis < MW_LDS_RECS ? a.max_vis : MW_LDS_RECS;
    const size_t lds = f.p.big ? 192 : (size_t)lds_recs * (MW_LDS_SHADE_Q + MW_LDS_CULL_Q) * 16 + 192;
    // the second part (the tiles a mesh can touch: few, slow, clustered): persistent wavefronts over the geometry kernel's
    // tile list (part 3)
    const bool listed = part == 2 && a.tile_list != nullptr;
    if (listed) part = 3;
    const int wpe2 = part == 2 ? a.n_tiles : wpe;
    const int tpw2 = part == 2 ? 1 : (a.n_tiles + wpe - 1) / wpe;
    const int grid = listed ? std::min(m.mesh_tile_waves, N * (int)a.n_tiles) : (N + 7) / 8 * 8 * wpe2;
    launch(tile_kernel_of(f.p.big, f.p.depth, f.p.general, f.p.ragged, f.p.mesh, part == 1), f.list, dim3(grid), dim3(64), lds, st,
           a.N, a.W, a.H, a.max_vis, a.tiles_x, a.n_tiles, wpe2, tpw2, (const float *)a.rec_raster, (const float *)a.rec_shade,
           (const float *)a.rec_cull, (const int32_t *)a.nvis, (const float *)a.envhdr, a.tex, a.texels, f.obs, f.depth, raster_flags(e, part, f.mf.stamp, f.reuse),
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

int launch_frame(mw_engine *e, bool do_step, int view_flags, const int32_t *d_actions, uint8_t *d_obs, float *d_depth,
                 float *d_reward, uint8_t *d_term, uint8_t *d_trunc, hipStream_t st, int frame = FRAME_ALL, const StepCall &call = {})
{
    if (!d_obs) return fail(e, MW_E_INVALID, "d_obs is null");
    // Frame reuse: a plain step of the whole batch into the buffers that hold the frame before it leaves the envs K1 marks clean
    // undrawn.  Any other frame — the first one, a render, a top view, the passes of a final-observation step, frames with mesh
    // entities (their sample keys and fragment lists have a protocol of their own), other buffers or another layout, experiment
    // flags — draws every env; a whole plain agent-view frame then makes its buffers the held ones, anything else leaves none.
    const bool plain = frame == FRAME_ALL && view_flags == 0;
    const bool reuse = e->frame_reuse && plain && do_step && !e->have_meshes && e->dbg_flags == 0 && e->held.valid && e->held.obs == d_obs &&
                       e->held.depth == d_depth && e->held.layout == e->obs_layout;
    drop_held_frame(e);
    const int N = e->cfg.num_envs;
    Frame f{e->args, view_flags, frame == FRAME_LIST ? e->d_final_list : nullptr, d_obs, d_depth, st, reuse, 0, nullptr, raster_path(e, d_depth != nullptr), {}};
    // The frame cache: consulted and filled by a plain step of the whole batch through the quad kernel, in the layout it was
    // allocated for, without mesh entities or experiment flags; whose buffers the frame goes to does not matter.  Every other frame
    // neither reads nor writes it.  CollectHealth never: its respawn kernel moves entities behind K1's back (as for frame_clean).
    if (plain && do_step && f.p.path == MW_PATH_QUAD) {
        f.source = f.a.fc_source;
        if (e->fc.slots > 0 && e->fc.frames && !e->have_meshes && e->dbg_flags == 0 && e->obs_layout == MW_OBS_HWC_U8 && e->cfg.task != MW_TASK_COLLECT) {
            if (d_depth && !e->fc.depth) {
                if (const int rc = dev_alloc(e, e->fc.depth, (size_t)N * e->fc.slots * f.a.W * f.a.H, false)) return rc;
                e->fc.args_stale = true;
            }
            if ((d_depth != nullptr) != e->fc.with_depth) { e->fc.with_depth = d_depth != nullptr; drop_frame_cache(e); }
            if (e->fc.args_stale) {
                // (the buffers are new: no frame that is still running reads the block)
                e->fc.args = MwFcArgs{f.a.fc_key, e->fc.meta.get(), e->fc.frames.get(), e->fc.depth.get(), e->fc.slots, 0};
                HIP_TRY(e, hipMemcpyAsync(e->fc.d_args.get(), &e->fc.args, sizeof(MwFcArgs), hipMemcpyHostToDevice, st));
                e->fc.args_stale = false;
                drop_frame_cache(e);
            }
            if (e->fc.dirty) {
                HIP_TRY(e, hipMemsetAsync(e->fc.meta.get(), 0, (size_t)N * MW_FC_META_WORDS(e->fc.slots) * 8, st));
                e->fc.dirty = false;
            }
            f.fc_slots = e->fc.slots;
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
    const bool timed = frame != FRAME_LIST && e->timing && (e->frame_count++ % (uint64_t)e->timing_stride) == 0;
    if (timed) {
        ev = get_events(e);
        (void)hipEventRecord(ev.a.get(), st);
    }
    const bool async_refill = e->spare_mode && do_step && e->cfg.generator == MW_GEN_MAZE;
    launch_step_and_geometry(e, f, do_step, frame, async_refill, d_actions, d_reward, d_term, d_trunc, call);
    if (timed) (void)hipEventRecord(ev.b.get(), st);
    int rc = MW_OK;
    if (async_refill && (rc = launch_side_refill(e, st))) return rc;
    if (f.p.path == MW_PATH_GENERIC) rc = launch_generic(e, f.a, 0, N, e->cfg.msaa, dim3(32, N), d_obs, d_depth, e->obs_layout, f.list, st);
    else if (f.p.mesh) rc = launch_mesh_chain(e, f, st);
    else if (f.p.path == MW_PATH_QUAD) launch_quad(e, f, 0, st);
    else launch_tiles(e, f, 0, st);
    if (rc) return rc;
    e->last_raster_path = f.p.path;
    if (timed) {
        (void)hipEventRecord(ev.c.get(), st);
        e->ev_used.push_back(std::move(ev));
    }
    HIP_TRY(e, hipGetLastError());
    if (plain) e->held = {d_obs, d_depth, e->obs_layout, true};
    return MW_OK;
}

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
    a.tiles_x = (a.W + MW_TILE_W - 1) / MW_TILE_W; a.tiles_y = (a.H + MW_TILE_H - 1) / MW_TILE_H; a.n_tiles = a.tiles_x * a.tiles_y;    // the raster grid
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
    ALLOC(a.ax, N); ALLOC(a.ay, N); ALLOC(a.az, N); ALLOC(a.adir, N);
    ALLOC(a.cam, 4 * (size_t)N); ALLOC(a.light, 12 * (size_t)N);
    ALLOC(a.carry, N); ALLOC(a.step, N); ALLOC(a.picked, N);
    if (cfg->task == MW_TASK_COLLECT) { ALLOC(a.health, N); ALLOC(a.final_health, N); }
    ALLOC(a.final_goal, 3 * (size_t)N);
    ALLOC(a.ekind, (size_t)E * N); ALLOC(a.emesh, (size_t)E * N); ALLOC(a.estatic, (size_t)E * N);
    ALLOC(a.epos, 3 * (size_t)E * N); ALLOC(a.edir, (size_t)E * N); ALLOC(a.egeom, 9 * (size_t)E * N);
    ALLOC(a.rng, 5 * (size_t)N); ALLOC(a.extent, 4 * (size_t)N);
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
    // the launch with it; its refills run on the side stream, launch_frame); in the other wave-per-env scenes they bought
    // 2 us of 51 (Hallway) and stay off.  MW_SPARE=1 / 0 forces either.  Not with domain randomisation: the per-step draws
    // interleave with the worlds in the env's stream.
    {
        const bool small_scene = cfg->max_visible <= 64 && cfg->max_polys + 6 * std::max(cfg->max_ents, 1) <= 32;      // = the dense K1 (k1_dense_lanes)
        bool want = small_scene || cfg->generator == MW_GEN_MAZE;
        if (const char *s = getenv("MW_SPARE")) want = atoi(s) != 0;
        e->spare_mode = cfg->generator != MW_GEN_NONE && !cfg->domain_rand && want && cfg->task != MW_TASK_COLLECT;     // CollectHealth's respawns draw from the stream mid-episode
    }
    if (e->spare_mode) {
        ALLOC(sp.ax, N); ALLOC(sp.ay, N); ALLOC(sp.az, N); ALLOC(sp.adir, N);
        ALLOC(sp.cam, 4 * (size_t)N); ALLOC(sp.light, 12 * (size_t)N); ALLOC(sp.extent, 4 * (size_t)N);
        ALLOC(sp.ekind, (size_t)E * N); ALLOC(sp.emesh, (size_t)E * N); ALLOC(sp.estatic, (size_t)E * N);
        ALLOC(sp.epos, 3 * (size_t)E * N); ALLOC(sp.edir, (size_t)E * N); ALLOC(sp.egeom, 9 * (size_t)E * N);
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
    if (cfg->max_visible > 64) {
        // big scenes: the visiting order the geometry kernel leaves for K2 (mw_geom.hip), zeroed
        ALLOC(a.rec_order, (size_t)N * (a.max_vis + 1));
    }
    if (cfg->max_polys > 64 && !(getenv("MW_OCC_CACHE") && atoi(getenv("MW_OCC_CACHE")) == 0)) {
        // big scenes: the geometry kernel's per-world culling data (mw_geom.hip), zeroed = nothing cached
        ALLOC(a.occ_valid, e->n_sets);
        ALLOC(a.occ_cache, (size_t)e->n_sets * MW_OCC_CACHE_STRIDE(cfg->max_polys));
    }
    ALLOC(a.pending_remove, (size_t)N);
    ALLOC(a.reset_pending, (size_t)N);      // (zeroed: nothing pending)
    ALLOC(a.frame_clean, (size_t)N);        // (zeroed: nothing clean before the first step)
    ALLOC(a.fc_key, (size_t)MW_FC_KEY_WORDS * N); ALLOC(a.fc_epoch, (size_t)N); ALLOC(a.fc_source, (size_t)N);
    HIP_TRY(e, hipMemset(a.pending_remove, 0xFF, 4 * (size_t)N));
    ALLOC(a.nvis, N); ALLOC(a.envhdr, (size_t)MW_ENVHDR * N); ALLOC(a.status, 1);
    ALLOC(e->d_reward_scratch, N); ALLOC(e->d_flag_scratch, 2 * (size_t)N); ALLOC(e->d_action_scratch, N);
    ALLOC(e->d_final_list, 1 + (size_t)N);
    ALLOC(e->stack.flags, 2 * (size_t)N);
    ALLOC(e->d_mask, N); ALLOC(e->d_step_override, 3 * (size_t)N);
#ifdef MW_PERF_HOOKS        // (tools/perf: make EXTRA=-DMW_PERF_HOOKS — kernel phase stamps dumped by mw_destroy; not in the product build)
    if (getenv("MW_K1_PROF")) ALLOC(a.k1_prof, MW_K1_PROF_SLOTS * (size_t)N);     // per-env cycle stamps of the geometry kernel's phases (zeroed)
    if (getenv("MW_ENT_PROF")) ALLOC(e->d_ent_prof, (size_t)16 * 2 * N * MW_MAX_MESH_ENTS * 8);
    if (getenv("MW_K2Q_PROF")) ALLOC(e->d_k2q_prof, (size_t)N * 80);
#endif
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
    e->waves_per_env = pick_waves_per_env(e);
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
    {
        // the quad kernel (mw_rasterq.hip) keeps an env's frame, quad lists and triangle records in LDS: frames up to 8192 pixels
        const int S = cfg->msaa == 4 ? 4 : 8;
        const int lds = mw_rasterq_lds_bytes(S, a.W, a.H, a.n_tiles, 1);
        e->k2q_ok = (cfg->msaa == 8 || cfg->msaa == 4) && frame_on_grid(a.W, a.H) && a.W <= 128 && a.H <= 128 && a.W * a.H <= 8192 && lds <= 64 * 1024;
    }
    {
        // snapshot records: the components this engine has, each with its array and its place in a record (mw_snapshot.h)
        e->snap_cfg = {E, cfg->max_polys, cfg->max_segs, cfg->shared_geometry ? 1 : 0, cfg->task, cfg->generator, cfg->rng_mode, e->spare_mode ? 1 : 0,
                       cfg->task == MW_TASK_COLLECT ? 1 : 0};
        const MwSnapLayout &L = e->snap_layout = mw_snap_layout(e->snap_cfg);
        void *arr[MW_SC_COUNT] = {};
        arr[MW_SC_AX] = a.ax; arr[MW_SC_AY] = a.ay; arr[MW_SC_AZ] = a.az; arr[MW_SC_ADIR] = a.adir; arr[MW_SC_CAM] = a.cam; arr[MW_SC_LIGHT] = a.light;
        arr[MW_SC_EXTENT] = a.extent; arr[MW_SC_CARRY] = a.carry; arr[MW_SC_STEP] = a.step; arr[MW_SC_PICKED] = a.picked; arr[MW_SC_HEALTH] = a.health;
        arr[MW_SC_FINAL_HEALTH] = a.final_health; arr[MW_SC_FINAL_GOAL] = a.final_goal; arr[MW_SC_EKIND] = a.ekind; arr[MW_SC_EMESH] = a.emesh;
        arr[MW_SC_ESTATIC] = a.estatic; arr[MW_SC_EPOS] = a.epos; arr[MW_SC_EDIR] = a.edir; arr[MW_SC_EGEOM] = a.egeom; arr[MW_SC_RNG] = a.rng;
        arr[MW_SC_PENDING_REMOVE] = a.pending_remove; arr[MW_SC_RESET_PENDING] = a.reset_pending;
        arr[MW_SC_NPOLYS] = const_cast<int32_t *>(a.npolys); arr[MW_SC_NSEGS] = const_cast<int32_t *>(a.nsegs);
        arr[MW_SC_SP_AX] = sp.ax; arr[MW_SC_SP_AY] = sp.ay; arr[MW_SC_SP_AZ] = sp.az; arr[MW_SC_SP_ADIR] = sp.adir; arr[MW_SC_SP_CAM] = sp.cam;
        arr[MW_SC_SP_LIGHT] = sp.light; arr[MW_SC_SP_EXTENT] = sp.extent; arr[MW_SC_SP_EKIND] = sp.ekind; arr[MW_SC_SP_EMESH] = sp.emesh;
        arr[MW_SC_SP_ESTATIC] = sp.estatic; arr[MW_SC_SP_EPOS] = sp.epos; arr[MW_SC_SP_EDIR] = sp.edir; arr[MW_SC_SP_EGEOM] = sp.egeom;
        arr[MW_SC_SP_NPOLYS] = sp.npolys; arr[MW_SC_SP_NSEGS] = sp.nsegs; arr[MW_SC_REFILL_MASK] = a.refill_mask;
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
        t.npolys_unit[0] = L.comp_unit[MW_SC_NPOLYS]; t.nsegs_unit[0] = L.comp_unit[MW_SC_NSEGS];
        t.npolys_unit[1] = L.comp_unit[MW_SC_SP_NPOLYS]; t.nsegs_unit[1] = L.comp_unit[MW_SC_SP_NSEGS];
        t.reset_pending_unit = L.comp_unit[MW_SC_RESET_PENDING];
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

// the arguments both calls share, checked before anything is launched
int snapshot_args(mw_engine *e, const char *what, const void *d_snap, int32_t count, int32_t capacity, bool whole_batch_limit)
{
    if (!d_snap) return fail(e, MW_E_INVALID, "%s: the record buffer is null", what);
    if ((uintptr_t)d_snap & 15u) return fail(e, MW_E_INVALID, "%s: the record buffer is not 16-byte aligned", what);
    if (capacity < 0) return fail(e, MW_E_INVALID, "%s: capacity %d < 0", what, (int)capacity);
    if (count < 0 || count > capacity) return fail(e, MW_E_INVALID, "%s: count %d outside 0 .. capacity %d", what, (int)count, (int)capacity);
    if (whole_batch_limit && count > e->cfg.num_envs) return fail(e, MW_E_INVALID, "%s: count %d > num_envs %d", what, (int)count, e->cfg.num_envs);
    return MW_OK;
}

// the grid of a call over `count` items: component blocks, then blob blocks (mw_snapshot.hip); MW_E_INVALID past the 1-D grid limit
int snapshot_grid(mw_engine *e, const char *what, int count, int *item_chunks, unsigned *grid)
{
    *item_chunks = (count + MW_SNAP_THREADS - 1) / MW_SNAP_THREADS;
    const long long blocks = (long long)*item_chunks * e->snap_layout.total_rows + (long long)count * e->snap_chunks_per_item;
    if (blocks > 0x7FFFFFFFll) return fail(e, MW_E_INVALID, "%s: %d items need %lld workgroups, more than one launch holds: split the call", what, count, blocks);
    *grid = (unsigned)std::max<long long>(blocks, 1);
    return MW_OK;
}

// Frame records (mw_snapshot_save_frames / mw_snapshot_load_frames; mw_snapframes.h): what of the engine's frame configuration shapes
// one under `flags`
MwSnapfConfig snapf_config(const mw_engine *e, int32_t flags)
{
    MwSnapfConfig c{};
    c.W = e->cfg.obs_width; c.H = e->cfg.obs_height; c.layout = e->obs_layout; c.flags = flags;
    c.stack_depth = (flags & MW_SNAPF_STACK) ? e->stack.depth : 0;
    c.frame_bytes = obs_row_bytes(e);
    return c;
}

// the arguments both calls share, checked before anything is launched; then the kernel's view of the call
int snapf_args(mw_engine *e, const char *what, const void *d_frames, const void *d_obs, const void *d_depth, int32_t count, int32_t n_recs,
               int32_t capacity, int32_t flags, bool whole_batch_limit, MwSnapfArgs *out, unsigned *grid)
{
    if (const int rc = snapshot_args(e, what, d_frames, count, capacity, whole_batch_limit)) return rc;
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
    a.first_slot = c.stack_depth ? stack_phase(e) : 0;
    // 16-byte units: every base and every size a multiple of 16 (the sections always are: mw_snapframes.h)
    a.wide = (((uintptr_t)d_frames | (uintptr_t)d_obs | (uintptr_t)(a.depth_bytes ? d_depth : nullptr) | (uintptr_t)(c.stack_depth ? e->stack.ring : nullptr) |
               (uintptr_t)a.frame_bytes | (uintptr_t)a.depth_bytes) & 15u) == 0;
    const uint64_t unit = a.wide ? 16 : 1, chunk = (uint64_t)MW_SNAPF_THREADS * MW_SNAPF_UNROLL * unit;
    const uint64_t frame_chunks = (a.frame_bytes + chunk - 1) / chunk, depth_chunks = (a.depth_bytes + chunk - 1) / chunk;
    const uint64_t per_item = frame_chunks * (1 + (uint64_t)c.stack_depth) + depth_chunks, blocks = per_item * (uint64_t)count;
    if (blocks > 0x7FFFFFFFull)
        return fail(e, MW_E_INVALID, "%s: %d items need %llu workgroups, more than one launch holds: split the call", what, (int)count, (unsigned long long)blocks);
    a.frame_chunks = (int32_t)frame_chunks; a.depth_chunks = (int32_t)depth_chunks; a.chunks_per_item = (int32_t)per_item;
    *out = a;
    *grid = (unsigned)std::max<uint64_t>(blocks, 1);
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
    dump(e->d_k2q_prof, (size_t)e->cfg.num_envs * 80, "MW_K2Q_PROF");
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
    drop_held_frame(e);
    drop_frame_cache(e);
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
    drop_held_frame(e);
    drop_frame_cache(e);
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
    drop_held_frame(e);
    drop_frame_cache(e);
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
    drop_held_frame(e);
    drop_frame_cache(e);
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

int mw_set_gen_program(mw_engine *e, const mw_gen_program *prog, const mw_poly *polys, const int32_t *poly_room,
                       const int32_t *poly_surf, const double *poly_m, int32_t n_polys, const double *segs, int32_t n_segs)
{
    if (!e || !prog) return fail(e, MW_E_INVALID, "null argument");
    ON_DEVICE_SYNC(e);
    drop_held_frame(e);
    drop_frame_cache(e);
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
    drop_held_frame(e);
    drop_frame_cache(e);
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
    const bool pcg = e->cfg.rng_mode == MW_RNG_PCG64;
    auto gen = pcg ? mw_reset_pcg_kernel : mw_reset_kernel;
    const dim3 grid(e->cfg.generator == MW_GEN_MAZE ? N : (N + 63) / 64);
    const int all = mask ? 0 : 1;
    if (!e->spare_mode) {
        hipLaunchKernelGGL(gen, grid, dim3(64), 0, st, e->args, (const uint8_t *)e->d_mask, all, 0);
    } else {
        // spare mode: a fresh seed generates the live world directly; without seeds the env's pre-generated world is
        // taken (what the same-step auto-reset does, after the pending refills have been run); either way the spare
        // of a reset env is then regenerated from its stream
        auto refill = pcg ? mw_refill_pcg_kernel : mw_refill_kernel;
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

// the frames of one call: one, or the two passes of a same-step step with final observations
static int step_passes(mw_engine *e, const int32_t *d_actions, const StepCall &call, uint8_t *d_obs, float *d_depth, float *d_reward,
                       uint8_t *d_term, uint8_t *d_trunc, hipStream_t st)
{
    if (!e->final_obs)
        return launch_frame(e, true, 0, d_actions, d_obs, d_depth, d_reward, d_term, d_trunc, st, FRAME_ALL, call);
    // Same-step auto-reset with final observations, in two passes.  1: the step as the next-step mode's terminal step — physics,
    // rule, reward, flags, final info, per-step draws; the finished envs keep their terminal state — and the frame of every env.
    // The finished envs' rows go to the final buffers.  2: they install their next world (the same install code and stream order
    // as the plain same-step step: the step's draws, then the reset's), and the frame of those envs alone overwrites their rows.
    const int N = e->cfg.num_envs;
    int rc = launch_frame(e, true, 0, d_actions, d_obs, d_depth, d_reward, d_term, d_trunc, st, FRAME_TERMINAL, call);
    if (rc != MW_OK) return rc;
    const size_t row_bytes = obs_row_bytes(e);
    hipLaunchKernelGGL(mw_final_copy_kernel, dim3(N), dim3(256), 0, st, (const int32_t *)e->d_final_list, (const uint8_t *)d_obs, e->final_obs,
                       (unsigned long long)row_bytes, (const float *)d_depth, e->final_depth, e->cfg.obs_width * e->cfg.obs_height);
    hipLaunchKernelGGL(e->cfg.rng_mode == MW_RNG_PCG64 ? mw_final_install_pcg_kernel : mw_final_install_kernel, dim3(N), dim3(64), 0, st,
                       e->args, (const int32_t *)e->d_final_list);
    return launch_frame(e, false, 0, e->d_action_scratch, d_obs, d_depth, nullptr, nullptr, nullptr, st, FRAME_LIST);
}

// A frameless mw_step_plan: the step kernel in the engine's own auto-reset mode — it applies the frame's tail behind the last executed
// sub-step itself —, the Maze's side-stream refill where a drawn call has one, and the stack's flag bytes.  No geometry kernel, no
// raster, no respawn kernel, no push, no final-buffer pass; nothing is timed.  The buffers that frame reuse holds no longer show the
// envs' states; the frame cache is neither read nor filled and stays valid (the epochs part what the call changed).
static int step_frameless(mw_engine *e, const int32_t *d_plans, const StepCall &call, float *d_reward, uint8_t *d_term, uint8_t *d_trunc, hipStream_t st)
{
    drop_held_frame(e);
    const int N = e->cfg.num_envs;
    MwArgs a = e->args;
    a.step_override = e->use_step_override ? e->d_step_override : nullptr;
    uint8_t *term = d_term ? d_term : e->d_flag_scratch, *trunc = d_trunc ? d_trunc : e->d_flag_scratch + N;
    const bool async_refill = e->spare_mode && e->cfg.generator == MW_GEN_MAZE;
    launch_k1(e, a, st, async_refill, d_plans, d_reward, term, trunc, call, true);
    if (async_refill)
        if (const int rc = launch_side_refill(e, st)) return rc;
    if (e->stack.depth) {
        const bool installs = e->cfg.generator != MW_GEN_NONE;
        const bool same = installs && e->cfg.autoreset == MW_AUTORESET_SAME_STEP, next = installs && e->cfg.autoreset == MW_AUTORESET_NEXT_STEP;
        hipLaunchKernelGGL(mw_stack_plan_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, same ? (const uint8_t *)term : nullptr,
                           same ? (const uint8_t *)trunc : nullptr, next ? (const uint8_t *)e->args.reset_pending : nullptr, stack_flags(e, e->stack.cur));
    }
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

// mw_step (the plain step kernels), mw_step_repeat (the repeat kernels) and mw_step_plan (the plan kernels; d_actions: the plans)
static int step_frames(mw_engine *e, const char *what, const int32_t *d_actions, const StepCall &call, uint8_t *d_obs, float *d_depth, float *d_reward,
                uint8_t *d_term, uint8_t *d_trunc, void *stream)
{
    ON_DEVICE(e);
    if (!d_actions) return fail(e, MW_E_INVALID, "%s: %s is null", what, call.horizon ? "d_plans" : "d_actions");
    if ((e->cfg.generator == MW_GEN_PROGRAM || e->cfg.task >= MW_TASK_SIDEWALK) && !e->args.prog)
        return fail(e, MW_E_INVALID, "no placement program installed (mw_set_gen_program)");
    if (call.horizon && !d_obs) return step_frameless(e, d_actions, call, d_reward, d_term, d_trunc, (hipStream_t)stream);
    if (const int rc = stack_check(e, what)) return rc;
    const int rc = step_passes(e, d_actions, call, d_obs, d_depth, d_reward, d_term, d_trunc, (hipStream_t)stream);
    if (rc != MW_OK || !e->stack.depth) return rc;
    // the call's one push, behind its last raster kernel; the flags are where the step kernel wrote them (launch_step_and_geometry)
    return launch_stack(e, true, d_obs, d_term ? d_term : e->d_flag_scratch, d_trunc ? d_trunc : e->d_flag_scratch + e->cfg.num_envs, (hipStream_t)stream);
}

int mw_step(mw_engine *e, const int32_t *d_actions, uint8_t *d_obs, float *d_depth, float *d_reward,
            uint8_t *d_term, uint8_t *d_trunc, void *stream)
{
    if (!e) return MW_E_INVALID;
    return step_frames(e, "mw_step", d_actions, StepCall{}, d_obs, d_depth, d_reward, d_term, d_trunc, stream);
}

int mw_step_repeat(mw_engine *e, const int32_t *d_actions, int32_t repeat, uint8_t *d_obs, float *d_depth, float *d_reward,
                   uint8_t *d_term, uint8_t *d_trunc, int32_t *d_nsteps, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (repeat < 1 || repeat > MW_MAX_REPEAT) return fail(e, MW_E_INVALID, "mw_step_repeat: repeat %d outside 1 .. %d", (int)repeat, MW_MAX_REPEAT);
    return step_frames(e, "mw_step_repeat", d_actions, StepCall{repeat, d_nsteps}, d_obs, d_depth, d_reward, d_term, d_trunc, stream);
}

int mw_step_plan(mw_engine *e, const int32_t *d_plans, int32_t horizon, uint8_t *d_obs, float *d_depth, float *d_reward,
                 float *d_step_reward, uint8_t *d_term, uint8_t *d_trunc, int32_t *d_nsteps, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (horizon < 1 || horizon > MW_MAX_PLAN) return fail(e, MW_E_INVALID, "mw_step_plan: horizon %d outside 1 .. %d", (int)horizon, MW_MAX_PLAN);
    if (d_depth && !d_obs) return fail(e, MW_E_INVALID, "mw_step_plan: d_depth without d_obs (a frameless call draws nothing)");
    return step_frames(e, "mw_step_plan", d_plans, StepCall{0, d_nsteps, horizon, d_step_reward}, d_obs, d_depth, d_reward, d_term, d_trunc, stream);
}

int mw_set_final_obs(mw_engine *e, uint8_t *d_final_obs, float *d_final_depth)
{
    if (!e) return MW_E_INVALID;
    if (e->cfg.autoreset != MW_AUTORESET_SAME_STEP)
        return fail(e, MW_E_INVALID, "mw_set_final_obs: final observations exist in MW_AUTORESET_SAME_STEP only (next-step returns the terminal frame itself)");
    if (e->cfg.generator == MW_GEN_NONE)
        return fail(e, MW_E_INVALID, "mw_set_final_obs: MW_GEN_NONE engines auto-reset nothing (the returned frame is the terminal one)");
    drop_held_frame(e);
    e->final_obs = d_final_obs;
    e->final_depth = d_final_obs ? d_final_depth : nullptr;
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
    e->stack.frame_bytes = obs_row_bytes(e);
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
    return launch_stack(e, false, d_obs, nullptr, nullptr, (hipStream_t)stream);
}

int mw_stack_window(const mw_engine *e, int32_t *first_slot, int64_t *pushes)
{
    if (!e || !e->stack.depth) return MW_E_INVALID;
    if (first_slot) *first_slot = stack_phase(e);
    if (pushes) *pushes = e->stack.pushes;
    return MW_OK;
}

int mw_render(mw_engine *e, uint8_t *d_obs, float *d_depth, void *stream)
{
    if (!e) return MW_E_INVALID;
    ON_DEVICE(e);
    return launch_frame(e, false, 0, e->d_action_scratch, d_obs, d_depth, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

int mw_render_top(mw_engine *e, uint8_t *d_obs, float *d_depth, int32_t render_agent, void *stream)
{
    if (!e) return MW_E_INVALID;
    ON_DEVICE(e);
    return launch_frame(e, false, 1 | (render_agent ? 2 : 0), e->d_action_scratch, d_obs, d_depth, nullptr, nullptr, nullptr,
                        (hipStream_t)stream);
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
    drop_held_frame(e);     // (d_out may lie inside the held buffers)
    hipStream_t st = (hipStream_t)stream;
    MwArgs b = e->args;
    b.step_override = nullptr;
    b.W = width; b.H = height;
    b.tiles_x = (width + MW_TILE_W - 1) / MW_TILE_W; b.tiles_y = (height + MW_TILE_H - 1) / MW_TILE_H; b.n_tiles = b.tiles_x * b.tiles_y;
    b.env_base = env;
    hipLaunchKernelGGL(geom_kernel_of(64, msaa).plain, dim3(1), dim3(64), 0, st, b, view_flags, msaa, 64, 1);
    if (const int rc = e->have_meshes ? grow(e, e->mp.view_keys, e->mp.view_keys_bytes, (size_t)width * height * msaa * 4, 1) : MW_OK) return rc;
    if (const int rc = launch_generic(e, b, env, 1, msaa, dim3(128), d_out, d_depth, MW_OBS_HWC_U8, nullptr, st)) return rc;
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_pcg64_draws(uint64_t seed, int32_t n, const int32_t *bounds, double *out)
{
    if (!out || n < 0) return MW_E_INVALID;
    uint64_t s[4];
    mwasset::pcg64_seed(seed, s, mw::pcg64_step);
    mw::Rng r{s[0], s[1], s[2], s[3], 1, 0u, 0u};
    for (int i = 0; i < n; ++i)
        out[i] = (bounds && bounds[i] > 0) ? (double)mw::rng_below(r, (uint32_t)bounds[i]) : mw::rng_double(r);
    return MW_OK;
}

int mw_set_obs_layout(mw_engine *e, int32_t layout)
{
    if (!e) return MW_E_INVALID;
    if (layout != MW_OBS_HWC_U8 && layout != MW_OBS_CWH_U8 && layout != MW_OBS_GREY_F64) return fail(e, MW_E_INVALID, "unknown obs layout %d", layout);
    drop_held_frame(e);
    drop_frame_cache(e);
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
        const int L = geom_lanes(e), epw = 64 / L;
        hipLaunchKernelGGL(geom_kernel_of(L, e->cfg.msaa).plain, dim3((count + epw - 1) / epw), dim3(64), 0, st, b, 4, e->cfg.msaa, L, count);
    }
    if (!e->visible_attr_set) {
        HIP_TRY(e, hipFuncSetAttribute((const void *)mw_visible_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        e->visible_attr_set = true;
    }
    hipLaunchKernelGGL(mw_visible_kernel, dim3(count), dim3(256), lds, st, first_env, e->cfg.obs_width, e->cfg.obs_height,
                       e->cfg.msaa, b.max_vis, e->cfg.max_ents, (const float *)b.rec_raster, (const float *)b.rec_cull, (const int32_t *)b.nvis, d_vis);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int64_t mw_snapshot_bytes(const mw_engine *e, int32_t capacity)
{
    if (!e || capacity < 0) return MW_E_INVALID;
    return mw_snap_bytes(e->snap_layout, capacity);
}

int mw_snapshot_save(mw_engine *e, const int32_t *d_envs, int32_t count, uint8_t *d_snap, int32_t capacity, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (const int rc = snapshot_args(e, "mw_snapshot_save", d_snap, count, capacity, d_envs == nullptr)) return rc;
    ON_DEVICE(e);
    hipStream_t st = (hipStream_t)stream;
    int item_chunks = 0;
    unsigned grid = 1;
    if (const int rc = snapshot_grid(e, "mw_snapshot_save", count, &item_chunks, &grid)) return rc;
    if (const int rc = snapshot_order(e, st)) return rc;
    hipLaunchKernelGGL(mw_snapshot_save_kernel, dim3(grid), dim3(MW_SNAP_THREADS), 0, st, (const MwSnapTable *)e->d_snap_tab, mw_snap_key(e->snap_cfg, capacity),
                       e->cfg.num_envs, (int)capacity, (int)count, item_chunks, d_envs, e->args.status, d_snap);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_snapshot_load(mw_engine *e, const int32_t *d_envs, const int32_t *d_recs, int32_t count, const uint8_t *d_snap, int32_t n_recs,
                     int32_t capacity, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (const int rc = snapshot_args(e, "mw_snapshot_load", d_snap, count, capacity, true)) return rc;
    if (n_recs < 0 || n_recs > capacity) return fail(e, MW_E_INVALID, "mw_snapshot_load: n_recs %d outside 0 .. capacity %d", (int)n_recs, (int)capacity);
    ON_DEVICE(e);
    hipStream_t st = (hipStream_t)stream;
    int item_chunks = 0;
    unsigned grid = 1;
    if (const int rc = snapshot_grid(e, "mw_snapshot_load", count, &item_chunks, &grid)) return rc;
    if (const int rc = snapshot_order(e, st)) return rc;
    drop_held_frame(e);     // (the frames in the caller's buffers are those of the states that are about to go)
    drop_frame_cache(e);    // (... and so are the cached ones: a loaded env's epoch is not part of its record)
    hipLaunchKernelGGL(mw_snapshot_load_kernel, dim3(grid), dim3(MW_SNAP_THREADS), 0, st, (const MwSnapTable *)e->d_snap_tab, mw_snap_key(e->snap_cfg, capacity),
                       e->cfg.num_envs, (int)capacity, (int)count, item_chunks, d_envs, e->args.status, d_snap, d_recs, (int)n_recs, e->args.frame_clean,
                       e->cfg.shared_geometry ? nullptr : e->args.occ_valid, e->stack.depth ? stack_flags(e, e->stack.cur) : nullptr);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int64_t mw_snapshot_frames_bytes(const mw_engine *e, int32_t capacity, int32_t flags)
{
    if (!e || capacity < 0 || (flags & ~(MW_SNAPF_DEPTH | MW_SNAPF_STACK))) return MW_E_INVALID;
    // (stacked frames are those of the layout the stack was set under, as for the two calls: stack_check's own test, no message)
    if ((flags & MW_SNAPF_STACK) && (!e->stack.depth || e->stack.layout != e->obs_layout || e->stack.frame_bytes != obs_row_bytes(e))) return MW_E_INVALID;
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
    drop_held_frame(e);     // (rows of d_obs are written; the frame cache stays: no state changed)
    hipLaunchKernelGGL(mw_snapshot_load_frames_kernel, dim3(grid), dim3(MW_SNAPF_THREADS), 0, (hipStream_t)stream, a, d_envs, e->args.status, d_recs, d_frames,
                       d_obs, reinterpret_cast<uint8_t *>(a.depth_bytes ? d_depth : nullptr), a.stack_depth ? e->stack.ring : nullptr,
                       a.stack_depth ? stack_flags(e, e->stack.cur) : nullptr);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_check(mw_engine *e, void *stream)
{
    if (!e) return MW_E_INVALID;
    ON_DEVICE_SYNC(e);
    HIP_TRY(e, hipStreamSynchronize((hipStream_t)stream));
    uint32_t st = 0;
    HIP_TRY(e, hipMemcpy(&st, e->args.status, 4, hipMemcpyDeviceToHost));
    if (st & MW_ST_VIS_OVERFLOW) return fail(e, MW_E_OVERFLOW, "more than max_visible=%d visible primitives in some env", e->cfg.max_visible);
    if (st & MW_ST_PLACEMENT_FAIL) return fail(e, MW_E_OVERFLOW, "device-side placement did not converge in some env");
    if (st & MW_ST_SNAPSHOT_BAD)
        return fail(e, MW_E_INVALID, "mw_snapshot_save / mw_snapshot_load / mw_snapshot_save_frames / mw_snapshot_load_frames skipped an item: an env or record index out of range, or a record "
                    "buffer of another layout (key mismatch)");
    return MW_OK;
}

int mw_raster_path(const mw_engine *e) { return e ? e->last_raster_path : MW_E_INVALID; }

int mw_debug_set_mesh_frame_seq(mw_engine *e, uint32_t seq)
{
    if (!e) return MW_E_INVALID;
    // (the work lists and the slow-path counters alternate with the sequence number's parity: keep it)
    if ((seq & 1u) != (e->mp.frame_seq & 1u)) return fail(e, MW_E_INVALID, "mw_debug_set_mesh_frame_seq: the parity of the sequence number must stay");
    drop_held_frame(e);
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
    ON_DEVICE(e);
    const int N = e->cfg.num_envs;
    hipLaunchKernelGGL(mw_info_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, e->args.E, (const int32_t *)e->args.health,
                       (const double *)e->args.epos, d_ent_pos ? ent_slot : 0, d_health, d_ent_pos);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_get_final_info(mw_engine *e, int32_t *d_health, double *d_goal_pos, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (!d_health && !d_goal_pos) return fail(e, MW_E_INVALID, "mw_get_final_info: nothing asked for");
    if (d_health && !e->args.final_health) return fail(e, MW_E_INVALID, "mw_get_final_info: this engine's task keeps no health (MW_TASK_COLLECT only)");
    ON_DEVICE(e);
    const int N = e->cfg.num_envs;
    // (the arrays are component-major like the state: the gather kernel of mw_get_info with slot 0 of a one-slot table)
    hipLaunchKernelGGL(mw_info_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, 1, (const int32_t *)e->args.final_health,
                       (const double *)e->args.final_goal, 0, d_health, d_goal_pos);
    HIP_TRY(e, hipGetLastError());
    return MW_OK;
}

int mw_get_reset_pending(mw_engine *e, uint8_t *d_out, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (!d_out) return fail(e, MW_E_INVALID, "mw_get_reset_pending: d_out is null");
    ON_DEVICE(e);
    HIP_TRY(e, hipMemcpyAsync(d_out, e->args.reset_pending, (size_t)e->cfg.num_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MW_OK;
}

int mw_set_frame_reuse(mw_engine *e, int32_t on)
{
    if (!e) return MW_E_INVALID;
    drop_held_frame(e);     // (trust starts with the next whole frame)
    e->frame_reuse = on != 0;
    return MW_OK;
}

int mw_set_frame_cache(mw_engine *e, int32_t slots)
{
    if (!e) return MW_E_INVALID;
    if (slots < 0 || slots > MW_FC_MAX_SLOTS) return fail(e, MW_E_INVALID, "mw_set_frame_cache: %d slots outside 0 .. %d", (int)slots, MW_FC_MAX_SLOTS);
    ON_DEVICE(e);
    drop_frame_cache(e);
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

int mw_get_frame_source(mw_engine *e, uint8_t *d_out, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (!d_out) return fail(e, MW_E_INVALID, "mw_get_frame_source: d_out is null");
    ON_DEVICE(e);
    HIP_TRY(e, hipMemcpyAsync(d_out, e->args.fc_source, (size_t)e->cfg.num_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MW_OK;
}

int mw_get_frame_clean(mw_engine *e, uint8_t *d_out, void *stream)
{
    if (!e) return MW_E_INVALID;
    if (!d_out) return fail(e, MW_E_INVALID, "mw_get_frame_clean: d_out is null");
    ON_DEVICE(e);
    HIP_TRY(e, hipMemcpyAsync(d_out, e->args.frame_clean, (size_t)e->cfg.num_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MW_OK;
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
