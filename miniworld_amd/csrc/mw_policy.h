// The launch policy of the host runtime: which kernels draw a frame, with how many lanes, waves and workgroups, and what a frame may
// reuse, cache or hold.  Pure arithmetic over integers and switches — plain C++17, no HIP, no engine: the runtime (mw_engine*.hip)
// takes every such decision from here and keeps no second copy; tests/hostcheck/policy.cpp compiles it for the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mwengine.h"
#include "mw_ray.h"             // MW_RAY_THREADS, MW_RAY_WAVES, MW_RAY_WALL_BYTES, MW_RAY_DISC_BYTES
#include "mw_seen.h"            // MW_SEEN_THREADS, MW_SEEN_TAIL_BYTES
#include "mw_ego.h"             // MW_EGO_THREADS, mwego::staged_bytes
#include "mw_depth.h"           // MW_DEPTH_THREADS, MW_DEPTH_CELL_BYTES, MW_DEPTH_MAX_CELLS
#include "mw_nav_grid.h"        // MW_NAV_GRID_THREADS, mwnav::grid_field_bytes, mwnav::grid_extra_bytes
#include "mw_label.h"           // MW_LABEL_THREADS, MW_LABEL_CHUNK, MW_LABEL_MAX_POLYS, MW_LABEL_MAX_ENTS, mwlabel::plan_bytes
#include "mw_labelmap.h"        // MW_LABELMAP_THREADS, MW_LABELMAP_WORD_BYTES, MW_LABELMAP_MAX_CELLS, MW_LABELMAP_MAX_IDS
#include "mw_sight.h"           // MW_SIGHT_THREADS, mwsight::bits_bytes, weight_bytes, gain_bytes
#include "mw_regions.h"         // MW_REGIONS_THREADS, mwregions::label_bytes, table_bytes, scan_bytes
#include "mw_shape.h"
#include "mw_snapframes.h"     // MW_SNAPF_THREADS, MW_SNAPF_UNROLL
#include "mw_snapshot.h"        // MW_SNAP_THREADS

namespace mwpolicy {

// The tile / quad / mesh-scatter kernels evaluate an edge at a pixel as mul24(A_k, px) + mul24(B_k, gy) + C_k in 32 bits that wrap
// (mw_edge_rec.h).  Two bounds, both pinned at their boundary by tests/hostcheck/edge_limits.cpp against 64-bit edge functions:
//   edge_coeffs_fit   the multiply reads 24 signed bits of A_k = -256 dcdx_k and B_k = 256 dcdy_k.  Vertices are snapped inside
//                     [0, W] x [0, H] of the FRAME (the viewport: the vertex range), so |B| <= 2^16 W and |A| <= 2^16 H: W and H have
//                     to stay below 128 — at 128 an edge over the whole width (height) has B (A) = +2^23, which the multiply reads
//                     as -2^23.  This is the bound that binds first: 128 x 48 and 48 x 128 already draw wrong frames without it.
//   edge_sums_fit     the sum is compared as a signed 32-bit value.  The stated bound is the edge constant's, |c_k| = |dcdx X - dcdy Y| <=
//                     2 W H 2^16 < 2^31, i.e. W H <= 128 x 96, taken on the raster GRID (the frame rounded up to whole tiles: the
//                     padding pixels are evaluated too).  It is on the safe side: the sums wrap, so only the edge VALUE has to fit, and
//                     on the grid |E| <= W H 2^16 or little more (twice a triangle's area in 24.8 units) — the model finds the exact
//                     value inside 32 bits and, with exact multiplies, no wrong verdict up to 144 x 132.  The wall triangle that 128 x
//                     128 once lost was the multiply's operand, not this sum.  The bound stays as stated all the same.
// Larger frames take the generic-resolution kernels (64-bit edge values).
inline bool edge_coeffs_fit(int W, int H) { return W < 128 && H < 128; }
inline bool edge_sums_fit(int W, int H) { return W <= 128 && H <= 128 && W * H <= 128 * 96; }
// ... of a frame that is its own grid
inline bool tile_kernels_exact(int W, int H) { return edge_coeffs_fit(W, H) && edge_sums_fit(W, H); }

// The frame is W x H, the size the caller asked for: the viewport, the projection and every output stride.  The raster grid is
// the frame rounded up to whole 16 x 4 tiles, ceil16(W) x ceil4(H): tiles_x, tiles_y, n_tiles.  A frame that is not the grid
// ("ragged": padding pixels right of column W - 1 or below row H - 1) takes, at 8 samples without mesh entities, with an even H
// sides below 128 and a grid inside the edge sums' bound (above), the ragged tile kernels (mw_raster.hip, FMT -2: padding masked, per-pixel stores); any
// other ragged frame the generic-resolution kernels, which mask the padding per pixel too.  The quad kernel and the fixed-layout
// tile kernels take frames on the grid only ("Frame sizes").
inline int tiles_across(int W) { return (W + MW_TILE_W - 1) / MW_TILE_W; }
inline int tiles_down(int H) { return (H + MW_TILE_H - 1) / MW_TILE_H; }
inline bool frame_on_grid(int W, int H) { return W % MW_TILE_W == 0 && H % MW_TILE_H == 0; }
inline bool tile_path_ok(int W, int H) { return frame_on_grid(W, H) && tile_kernels_exact(W, H); }
// sizes mw_create and mw_render_view accept: at least one pixel, at most 255 tiles of grid in each direction (8-bit tile
// coordinates of the records' bounding boxes)
inline bool frame_size_ok(int W, int H) { return W >= 1 && H >= 1 && W <= 255 * MW_TILE_W && H <= 255 * MW_TILE_H; }

// big scenes: the geometry kernel leaves a visiting order for the tile kernels (MwArgs::rec_order) exactly then
inline bool has_visiting_order(int max_visible) { return max_visible > 64; }

// lanes per env of the geometry kernel: the power of two that holds an env's triangles (two per polygon and box face, the
// agent marker), 8 .. 64 — except that the smallest scenes get 16 lanes for their up to 32 triangles: an env's lanes go over
// its triangles in rounds, and four envs per wavefront fill the chip with half the wavefronts of this one-wave-per-SIMD kernel
// (measured, 4096 Hallway envs: 64 lanes 117 us, 32: 86, 16: 79, 8: 101)
inline int geom_lanes(int max_polys, int max_ents, bool order)
{
    const int items = 2 * (max_polys + 6 * max_ents + 1);      // one triangle per lane
    int L = 8;
    while (L < items && L < 64) L <<= 1;
    if (L == 32) L = 16;
    // mid-sized scenes (PickupObjects: 6 polygons + 5 entity slots = 74 triangles; no visiting order, no sifting): two envs per
    // wavefront — 2 048 envs are ONE round of this one-wave-per-SIMD kernel instead of two (K1 + KG 103 -> 71 us)
    if (L == 64 && !order && max_polys <= 64) L = 32;
    return L;
}

// Lanes per env of the dense K1 (mw_setup_dense.hip), or 0 when the step has to go through the wave-per-env kernel: big
// scenes, CollectHealth, or too many slots to pack two envs into a wavefront.  (max_ents: at least one, as the engine keeps it.)
inline int k1_dense_lanes(int max_polys, int max_ents, int max_visible, int task)
{
    if (has_visiting_order(max_visible) || task == MW_TASK_COLLECT) return 0;
    // at least two envs per wavefront: with one, every lane repeats the env's scalar work for nothing and the wave-per-env
    // kernel's lane-cooperative collision tests win (PickupObjects, 35 slots: 62 us dense against 47 us)
    const int lanes = max_polys + 6 * max_ents;
    return lanes <= 32 ? lanes : 0;
}

// workgroups of one wavefront over N envs at `lanes` lanes per env (0: a wavefront per env) — K1 and the geometry kernel
inline int env_blocks(int N, int lanes)
{
    const int epw = lanes ? 64 / lanes : 1;
    return (N + epw - 1) / epw;
}

// wavefronts per env of the tile kernels: enough to fill 256 CUs x 4 SIMDs x 7 resident waves several times over (measured:
// 15-25 waves per env beat 5 by ~7 % at 4096 envs), in divisors of n_tiles
inline int pick_waves_per_env(int n_tiles, int num_envs)
{
    for (int w = 1; w <= n_tiles; ++w)
        if (n_tiles % w == 0 && (long long)num_envs * w >= 49152) return w;
    return n_tiles;
}

// the quad kernel (mw_rasterq.hip) keeps an env's frame, quad lists and triangle records in LDS: frames up to 8192 pixels whose plan
// (lds_bytes: mw_rasterq_lds_bytes at 4 samples for msaa = 4, else 8, with depth) fits 64 KB
inline bool k2q_ok(int msaa, int W, int H, int lds_bytes)
{
    return (msaa == 8 || msaa == 4) && frame_on_grid(W, H) && edge_coeffs_fit(W, H) && W * H <= 8192 && lds_bytes <= 64 * 1024;
}

// Which kernels draw a frame of the engine's size (mw_raster_path), and the forms of them the launches pick: the one statement
// of these conditions — launch_frame, the frame's mesh lists and ensure_mesh_buffers take their answer from here.
struct RasterFacts {
    int msaa, W, H;
    bool meshes, order;             // meshes resident; a visiting order exists
    bool use_k2q, generic_raster;   // the MW_K2Q / MW_GENERIC_RASTER switches
    bool k2q_ok;                    // (k2q_ok above, worked out once by mw_create)
    int layout, dbg_flags;
};
struct RasterPath {
    int path;           // MW_PATH_TILE, MW_PATH_QUAD, MW_PATH_QUAD_MESH, MW_PATH_GENERIC
    bool mesh;          // mesh entities through the tile / quad kernels: the frame runs the mesh chain (launch_mesh_chain) on the mesh path's lists
    bool quad4;         // the quad kernel at 4 samples
    // big scene: a visiting order exists; an output layout other than HWC or debug flags; a frame off the 16 x 4 grid; depth asked for
    bool big, general, ragged, depth;
};
inline RasterPath raster_path(const RasterFacts &f, bool depth)
{
    const int S = f.msaa;
    RasterPath p{MW_PATH_GENERIC, false, false, f.order, f.layout != MW_OBS_HWC_U8 || f.dbg_flags != 0, !frame_on_grid(f.W, f.H), depth};
    // the quad kernel (mw_rasterq.hip): small scenes without a visiting order, frames that fit its LDS plan — 8 samples (the
    // hot path) and 4 (llvmpipe's GL_MAX_SAMPLES: the reference's own frames run through the same code); with mesh entities
    // it draws the tiles no mesh can touch (8 samples only)
    // (big scenes — a visiting order exists — keep the tile kernels: their near-to-far order with its early exit is the better fit
    // for deep scenes; the quad kernel on the Maze was measured and lost, tools/experiments/README.md)
    const bool k2q = f.use_k2q && f.k2q_ok && !p.big && !(S == 4 && (f.meshes || f.generic_raster));
    // a ragged frame the ragged tile kernels draw (frame_on_grid).  The even H: the tile kernels' 2x2 quads (texture lod) pair image rows from
    // the top, GL pairs window rows from the bottom (mw_frag.h), and the two agree only then.  Odd heights take the generic-resolution kernels.
    const bool ragged_tiles = !f.meshes && p.ragged && f.H % 2 == 0 && edge_coeffs_fit(f.W, f.H) && edge_sums_fit(tiles_across(f.W) * MW_TILE_W, tiles_down(f.H) * MW_TILE_H);
    p.quad4 = k2q && S == 4;
    // FrameBuffer's fallback sample counts (opengl.py:229-231: a driver that clamps GL_MAX_SAMPLES gets 4 or 1
    // samples), observations 128 pixels wide or high and beyond (the tile kernels' 24-bit edge coefficients) and frames off the 16 x 4 grid:
    // the generic-resolution kernels, 64-bit edge values, exact packed-key resolution, every output layout, the whole
    // batch in one grid (blockIdx.y = env)
    const bool generic = S != 8 || (!tile_path_ok(f.W, f.H) && !ragged_tiles);
    p.mesh = !p.quad4 && !generic && f.meshes;
    p.path = p.quad4 ? MW_PATH_QUAD : generic ? MW_PATH_GENERIC : !k2q ? MW_PATH_TILE : p.mesh ? MW_PATH_QUAD_MESH : MW_PATH_QUAD;
    return p;
}

// The tile and quad kernels' flag word (`dbg`): the MW_DEBUG_FLAGS experiment bits, the output layout (bits 8-9,
// mw_set_obs_layout), the part of a frame with mesh entities the launch draws (bits 4-5: 0 every tile, 1 those no mesh can touch,
// 2 those a mesh can, 3 the same from the geometry kernel's tile list) and the frame stamp of the slow-fragment chains (bits
// 16-31; 0 for the quad kernel, which reads bits 13-15 as experiment bits).  mw_create keeps only MW_DEBUG_BITS of MW_DEBUG_FLAGS,
// so that no experiment flag lands in the fields beside it.
#define MW_DEBUG_BITS 0xFCCF
// `reuse`: MW_RASTER_REUSE (mw_kernels.h), frames without mesh entities only — it shares the stamp's field.
inline int raster_flags(int dbg_flags, int layout, int part, uint32_t stamp, bool reuse)
{
    return dbg_flags | layout << 8 | part << 4 | (int)(stamp << 16) | (reuse && stamp == 0u ? MW_RASTER_REUSE : 0);
}

// bytes of one env's row of d_obs in an output layout
inline size_t obs_row_bytes(int W, int H, int layout) { return (size_t)W * H * (layout == MW_OBS_GREY_F64 ? 8 : 3); }

// Frame stacking (mw_set_frame_stack; kernels: mw_stack.hip).  phase of the last push: the window starts there (before the first push
// every slot a refresh wrote is valid, and the same formula gives depth - 1).
inline int stack_phase(int64_t pushes, int depth) { return (int)((pushes + depth - 1) % depth); }

// Auto-reset: does it install worlds (none with MW_GEN_NONE), and on the step that ends the episode or on the env's next call
struct ResetMode { bool installs, same, next; };
inline ResetMode reset_mode(int generator, int autoreset)
{
    const bool installs = generator != MW_GEN_NONE;
    return {installs, installs && autoreset == MW_AUTORESET_SAME_STEP, installs && autoreset == MW_AUTORESET_NEXT_STEP};
}

// What a launch_frame call is.  CALL_RENDER: no step, every env's frame.  CALL_STEP: the step kernel, then every env's frame.  The two
// passes of a same-step step with final observations (mw_set_final_obs): CALL_TERMINAL_STEP — the step kernel runs as the next-step
// mode's terminal step (no install; reset_pending marks the finished envs), the list of those envs is built behind it, and the frame
// shows every env's state after the step (terminal states for the finished envs); CALL_LIST_PASS — no step, the frame of the listed
// envs only (their new worlds), through the list forms of the geometry and raster kernels.
enum CallKind { CALL_RENDER = 0, CALL_STEP = 1, CALL_TERMINAL_STEP = 2, CALL_LIST_PASS = 3 };
inline bool call_steps(CallKind k) { return k == CALL_STEP || k == CALL_TERMINAL_STEP; }

// The passes of a step call (mw_step, mw_step_repeat, mw_step_plan) of a same-step engine.  One pass: CALL_STEP, the step kernel installs
// the next worlds itself.  Two passes — final buffers (mw_set_final_obs), reset seeds (mw_set_reset_seeds) or both: CALL_TERMINAL_STEP,
// with final buffers the copy of the finished envs' rows, the install of the listed envs — from their seeds where seeds are set, else the
// step kernel's own install code —, CALL_LIST_PASS.  A frameless mw_step_plan launches the step kernel alone and ignores final buffers;
// with seeds set it is refused: the step kernel cannot seed, and no list pass follows it.
enum StepShape { STEP_REFUSED = -1, STEP_FRAMELESS = 0, STEP_ONE_PASS = 1, STEP_TWO_PASS = 2 };
struct StepPasses { StepShape shape; bool final_copy, seeded_install; };
inline StepPasses step_passes_of(bool seeds, bool final_bufs, bool frameless)
{
    if (frameless) return {seeds ? STEP_REFUSED : STEP_FRAMELESS, false, false};
    if (!seeds && !final_bufs) return {STEP_ONE_PASS, false, false};
    return {STEP_TWO_PASS, final_bufs, seeds};
}

// The frame's policy.  Frame reuse: a plain step of the whole batch into the buffers that hold the frame before it leaves the envs K1
// marks clean undrawn.  Any other frame — the first one, a render, a top view, the passes of a final-observation step, frames with mesh
// entities (their sample keys and fragment lists have a protocol of their own), other buffers or another layout, experiment
// flags — draws every env; a whole plain agent-view frame then makes its buffers the held ones, anything else leaves none.
// The frame cache: consulted and filled by a plain step of the whole batch through the quad kernel, in the layout it was
// allocated for, without mesh entities or experiment flags; whose buffers the frame goes to does not matter.  Every other frame
// neither reads nor writes it.  CollectHealth never: its respawn kernel moves entities behind K1's back (as for frame_clean).
// With reset seeds set (mw_set_reset_seeds) EVERY step takes the two passes, so there the first pass counts as the plain step it is
// for all but the finished envs: K1 stored frame_clean and the key of every env, the frame shows every env's state after the step,
// a finished env's row may stay or come from the cache like any other (its terminal frame; the install advances its epoch), and the
// list pass redraws exactly the rows whose env got a new world — afterwards the call's buffers show every env and are the held ones.
struct FrameFacts {
    CallKind kind;
    int view_flags;
    bool frame_reuse, held_match;   // mw_set_frame_reuse is on; the held buffers are valid and are this call's, in this layout
    bool meshes;
    int dbg_flags, layout, task;
    bool cache_allocated;           // mw_set_frame_cache: slots > 0 and their frames exist
    int path;                       // RasterPath::path
    bool seeded = false;            // reset seeds are set: the call is a pass of a seeded step
};
struct FramePolicy {
    bool reuse;         // clean envs may stay undrawn
    bool source;        // a plain step through the quad kernel: the per-env source byte tells of this frame (K1's zeros; the plan kernel's verdicts, frame_plans)
    bool cache;         // ... and the frame consults and fills the frame cache
    bool hold;          // afterwards the call's buffers are the held ones
};
inline FramePolicy frame_policy(const FrameFacts &f)
{
    const bool plain = (f.kind == CALL_RENDER || f.kind == CALL_STEP) && f.view_flags == 0;
    const bool seeded_pass = f.seeded && (f.kind == CALL_TERMINAL_STEP || f.kind == CALL_LIST_PASS) && f.view_flags == 0;
    const bool plain_step = (plain && f.kind == CALL_STEP) || (seeded_pass && f.kind == CALL_TERMINAL_STEP), bare = !f.meshes && f.dbg_flags == 0;
    const bool source = plain_step && f.path == MW_PATH_QUAD;
    return {f.frame_reuse && plain_step && bare && f.held_match, source,
            source && f.cache_allocated && bare && f.layout == MW_OBS_HWC_U8 && f.task != MW_TASK_COLLECT, plain || seeded_pass};
}

// The frame plan (mw_frame_plan_kernel, behind the geometry kernel): made exactly for the frames whose quad kernel may leave an env
// undrawn — the whole batch (no list) through the quad kernel alone, with clean envs that may stay (reuse) or a cache to consult
// (cache).  Its entries keep the env in 24 bits (mw_frame_plan.h); a larger batch is drawn in full, which is always right.
inline bool frame_plans(const FramePolicy &pol, int path, bool listed, int N)
{
    return !listed && path == MW_PATH_QUAD && (pol.reuse || pol.cache) && N <= 0xFFFFFF;
}
// ... and the small-scene geometry kernel in front of it builds only the envs that plan will have drawn, dealt evenly over its wavefronts
// (mw_geom_deal.h), exactly then — unless the engine was created with MW_GEOM_DEAL=0 (enabled).  Big scenes (64 lanes: one env per
// wavefront) have nothing to deal.
inline bool geom_deals(bool plans, bool enabled, int lanes)
{
    return plans && enabled && lanes < 64;
}
// ... and its draw entries are filed by cost class (mw_frame_plan.h: an ordered plan, a segment of N entries per class and 16-bit
// class counts) for the batches whose counts fit, MW_PLAN_ORDERED_MAX_N; a larger batch gets one unordered draw list, which is always right.
inline bool frame_plan_ordered(int N)
{
    return N <= 0xFFFF;
}

// The tile kernels' launch (mw_raster.hip) for a part of the frame (raster_flags).  big scenes (a visiting order exists): records
// read in place, near to far; otherwise the env's records are staged in LDS when there are at most MW_LDS_RECS of them (a wave whose
// env holds more reads them in place).  The second part (the tiles a mesh can touch: few, slow, clustered) with a tile list:
// persistent wavefronts over the geometry kernel's list (part 3).
struct TileLaunch { int part, waves_per_env, tiles_per_wave, grid; size_t lds; };
inline TileLaunch tile_launch(int part, bool tile_list, bool big, int max_vis, int n_tiles, int wpe, int N, int mesh_tile_waves)
{
    const int lds_recs = max_vis < MW_LDS_RECS ? max_vis : MW_LDS_RECS;
    const size_t lds = big ? 192 : (size_t)lds_recs * (MW_LDS_SHADE_Q + MW_LDS_CULL_Q) * 16 + 192;
    const bool listed = part == 2 && tile_list;
    if (listed) part = 3;
    const int wpe2 = part == 2 ? n_tiles : wpe, tpw2 = part == 2 ? 1 : (n_tiles + wpe - 1) / wpe;
    const int all = N * n_tiles;
    return {part, wpe2, tpw2, listed ? (mesh_tile_waves < all ? mesh_tile_waves : all) : (N + 7) / 8 * 8 * wpe2, lds};
}

// 16-byte units where every base and size of a copy is a multiple of 16 (`bits`: the addresses and byte counts, or'ed), else bytes
inline bool wide_units(uintptr_t bits) { return (bits & 15u) == 0; }

// the frame stack's push / refresh: grid (N, chunks) over the units of one frame
struct StackLaunch { bool wide; unsigned chunks; };
inline StackLaunch stack_launch(uintptr_t address_bits, size_t frame_bytes)
{
    const bool wide = wide_units(address_bits | (uintptr_t)frame_bytes);
    const size_t units = frame_bytes / (wide ? 16 : 1), chunk = (size_t)MW_STACK_THREADS * MW_STACK_UNROLL;
    return {wide, (unsigned)((units + chunk - 1) / chunk)};
}

// more workgroups than one 1-D launch holds
inline bool grid_too_large(unsigned long long blocks) { return blocks > 0x7FFFFFFFull; }

// the grid of a state-record call over `count` items: component blocks, then blob blocks (mw_snapshot.hip)
struct SnapshotGrid { int item_chunks; long long blocks; };
inline SnapshotGrid snapshot_grid(int count, int total_rows, int chunks_per_item)
{
    const int item_chunks = (count + MW_SNAP_THREADS - 1) / MW_SNAP_THREADS;
    return {item_chunks, (long long)item_chunks * total_rows + (long long)count * chunks_per_item};
}

// The masked loads (mw_snapshot_load_where, mw_snapshot_load_frames_where): the grid is the list form's for count = N, whatever the mask
// holds and however few records the buffer has — records repeat, so N may exceed the capacity.
inline SnapshotGrid snapshot_where_grid(int N, int total_rows, int chunks_per_item) { return snapshot_grid(N, total_rows, chunks_per_item); }

// What a load of state records invalidates on the host.  The held frame (frame reuse) always: the caller's buffers no longer show the
// envs.  The frame cache of EVERY env only for the list form, whose kernel leaves the epochs alone; the masked form runs behind every
// step of a loop and must not cost the other envs their cached frames, so its kernel advances fc_epoch of each env it writes instead
// (the epoch is part of a frame's key and of no record: none of that env's cached frames can match again).
struct LoadInvalidation { bool held, cache; };
inline LoadInvalidation snapshot_load_invalidation(bool where) { return {true, !where}; }
// ... and mw_reset_where, the masked seeded reset on the device: as the masked load — its kernel advances the epochs of the envs it writes
inline LoadInvalidation reset_where_invalidation() { return snapshot_load_invalidation(true); }
// ... and mw_set_state_where, the masked state write on the device: the same again — where mw_set_state marks the whole cache dirty, its
// kernel advances the epochs of the envs it writes and every other env keeps its cached frames
inline LoadInvalidation set_state_where_invalidation() { return snapshot_load_invalidation(true); }
// ... and of frame records, either form: rows of d_obs are written, no state changes
inline LoadInvalidation snapshot_load_frames_invalidation(bool /*where*/) { return {true, false}; }

// ... and of a frame-record call (mw_snapframes.hip): per item the chunks of its obs row and of each window frame, then its depth row
struct SnapfGrid { bool wide; uint64_t frame_chunks, depth_chunks, per_item, blocks; };
inline SnapfGrid snapf_grid(uintptr_t address_bits, uint64_t frame_bytes, uint64_t depth_bytes, int stack_depth, int count)
{
    const bool wide = wide_units(address_bits | (uintptr_t)frame_bytes | (uintptr_t)depth_bytes);
    const uint64_t chunk = (uint64_t)MW_SNAPF_THREADS * MW_SNAPF_UNROLL * (wide ? 16 : 1);
    const uint64_t frame_chunks = (frame_bytes + chunk - 1) / chunk, depth_chunks = (depth_bytes + chunk - 1) / chunk;
    const uint64_t per_item = frame_chunks * (1 + (uint64_t)stack_depth) + depth_chunks;
    return {wide, frame_chunks, depth_chunks, per_item, per_item * (uint64_t)count};
}
inline SnapfGrid snapf_where_grid(uintptr_t address_bits, uint64_t frame_bytes, uint64_t depth_bytes, int stack_depth, int N)
{
    return snapf_grid(address_bits, frame_bytes, depth_bytes, stack_depth, N);
}

// The launch of a world query whose kernel takes a workgroup per env (seen_launch, ego_launch, depth_launch, labelmap_launch): the grid, the lanes of a
// workgroup, its dynamic LDS in bytes, and whether that fits.  (ray_launch and label_launch return more: RayLaunch, LabelLaunch.)
struct Launch { unsigned long long grid; int threads; size_t lds; bool fits; };
using SeenLaunch = Launch;      // (the names the three had while each declared the same four fields)
using EgoLaunch = Launch;
using DepthLaunch = Launch;

// Ray casts (mw_ray_cast; kernels: mw_ray.hip).  The form follows from the rays per env alone: from kRayPerLaneFrom rays on, a
// workgroup per env with a ray per lane and the obstacles staged in LDS; below it a wavefront per ray with an obstacle per lane.
// Both produce the same bits.  The ray-per-lane form takes as many whole wavefronts as hold the rays, MW_RAY_THREADS lanes at most;
// its LDS is sized from the engine's capacities (fits: at most 64 KiB — the caller refuses what does not).
// Measured (profiles/r24, us per call, a disc of the agent's radius, ray per lane / obstacle per lane): Maze x 1024, 256 segments:
// R = 16: 216 / 47, 64: 227 / 167, 256: 567 / 647; Hallway x 4096, 4 segments: R = 1: 16 / 11, 4: 16 / 17, 16: 13 / 55, 64: 14 / 207.
// The crossover moves with the segment count — below 4 rays in the Hallway, between 64 and 256 in the Maze —; 64 keeps the range
// sensor on the form that is flat in R and the few-ray queries on the one that is flat in the segment count.
constexpr int kRayPerLaneFrom = 64;
struct RayLaunch { bool per_lane; unsigned long long grid; int threads; size_t lds; bool fits; };
inline RayLaunch ray_launch(int N, int R, int max_segs, int max_ents, int forced = 0 /* measurements: 1 a ray per lane, 2 an obstacle per lane */)
{
    if (forced ? forced == 1 : R >= kRayPerLaneFrom) {
        const int waves = (R + 63) / 64;
        const size_t lds = ((size_t)max_segs * MW_RAY_WALL_BYTES + (size_t)max_ents * MW_RAY_DISC_BYTES + 15) / 16 * 16;
        return {true, (unsigned long long)N, 64 * (waves < MW_RAY_THREADS / 64 ? waves : MW_RAY_THREADS / 64), lds, lds <= 64 * 1024};
    }
    return {false, ((unsigned long long)N * (unsigned long long)R + MW_RAY_WAVES - 1) / MW_RAY_WAVES, MW_RAY_WAVES * 64, 0, true};
}

// Explored-area maps (mw_seen_update; kernel: mw_seen.hip): a workgroup of MW_SEEN_THREADS lanes per env.  Its LDS is the ray-per-lane
// form's staged obstacles, sized from the engine's capacities, and behind them the candidate list and its words (MW_SEEN_TAIL_BYTES);
// fits: at most 64 KiB, the rule of ray_launch — the caller refuses what does not.
inline Launch seen_launch(int N, int max_segs, int max_ents)
{
    const size_t lds = ((size_t)max_segs * MW_RAY_WALL_BYTES + (size_t)max_ents * MW_RAY_DISC_BYTES + 15) / 16 * 16 + MW_SEEN_TAIL_BYTES;
    return {(unsigned long long)N, MW_SEEN_THREADS, lds, lds <= 64 * 1024};
}

// Egocentric map windows (mw_ego_map; kernel: mw_ego.hip): a workgroup of MW_EGO_THREADS lanes per env.  Its LDS is the staged
// obstacles of the asked planes, sized from the engine's capacities (mwego::staged_bytes: 48 bytes per segment and 32 per slot for
// VISIBLE, 32 per segment for WALL, 32 per slot for ENTITY, rounded up to 16; nothing without planes); fits: at most 64 KiB — the caller
// refuses what does not.
inline Launch ego_launch(int N, int max_segs, int max_ents, int planes)
{
    const size_t lds = mwego::staged_bytes(max_segs, max_ents, planes);
    return {(unsigned long long)N, MW_EGO_THREADS, lds, lds <= 64 * 1024};
}

// Depth projection (mw_depth_project; kernel: mw_depth.hip): a workgroup of MW_DEPTH_THREADS lanes per env.  Its LDS is one uint32 per
// cell of the target — size * size of a window, gx * gz of a map —, never less than the two words per wavefront the map's reduction
// reuses, rounded up to 16; fits: at most 64 KiB, i.e. MW_DEPTH_MAX_CELLS = 16384 cells (a window of MW_EGO_MAX_SIZE = 128; the Maze at
// 0.25 m has 10 609) — the caller refuses what does not.
inline Launch depth_launch(int N, long long cells)
{
    const long long least = 2 * (MW_DEPTH_THREADS / 64);
    const size_t lds = ((size_t)(cells > least ? cells : least) * MW_DEPTH_CELL_BYTES + 15) / 16 * 16;
    return {(unsigned long long)N, MW_DEPTH_THREADS, lds, lds <= 64 * 1024};
}

// Grid navigation fields (mw_nav_build_grid; kernel: mw_nav_grid.hip): a workgroup of MW_NAV_GRID_THREADS lanes per env.  Its LDS is the
// uint16 cost grid, rounded up to 16 — mw_nav_build's —, and with extra costs a byte per cell behind it, rounded up to 16: at most
// 64 + 32 KiB at MW_NAV_MAX_CELLS, which one workgroup may hold (a CU has 160 KiB).  fits: no more cells than that, and a positive count.
inline Launch nav_grid_launch(int N, long long cells, bool weighted)
{
    const bool fits = cells >= 1 && cells <= MW_NAV_MAX_CELLS;
    const size_t lds = fits ? mwnav::grid_field_bytes(cells) + mwnav::grid_extra_bytes(cells, weighted) : 0;
    return {(unsigned long long)N, MW_NAV_GRID_THREADS, lds, fits};
}

// Label frames (mw_label_frame; kernel: mw_label.hip): a workgroup of MW_LABEL_THREADS lanes per env.  Its LDS (mwlabel::plan_bytes)
// holds the staged scene — min(max_polys, MW_LABEL_CHUNK) polygons of 160 bytes at a time, 72 + 20 bytes per entity slot — and 10 bytes
// per pixel of a band of whole rows, the bits of t and a 16-bit code; the frame is labelled band by band, band_rows rows at a time: as
// many as fit 64 KiB, the whole frame where it does (80 x 60: one band of 48 000 bytes; 84 x 84: two; 160 x 120: four).  fits: a row
// fits, and a 16-bit code can name every polygon and slot — the caller refuses what does not.
struct LabelLaunch { unsigned long long grid; int threads; size_t lds; int band_rows, chunk; bool fits; };
inline LabelLaunch label_launch(int N, int W, int H, int max_polys, int max_ents)
{
    const int chunk = max_polys < 1 ? 1 : (max_polys < MW_LABEL_CHUNK ? max_polys : MW_LABEL_CHUNK);
    LabelLaunch l{(unsigned long long)N, MW_LABEL_THREADS, 0, 0, chunk, false};
    if (W < 1 || H < 1 || max_polys > MW_LABEL_MAX_POLYS || max_ents < 0 || max_ents > MW_LABEL_MAX_ENTS) return l;
    const size_t scene = mwlabel::plan_bytes(0, chunk, max_ents) + 16;       // (+ 16: the sum is rounded up once more with the pixels)
    if (scene >= 64 * 1024) return l;
    const long long rows = (long long)((64 * 1024 - scene) / ((size_t)W * MW_LABEL_PIXEL_BYTES));
    l.band_rows = (int)(rows < (long long)H ? rows : (long long)H);
    l.fits = l.band_rows >= 1;
    l.lds = l.fits ? mwlabel::plan_bytes(l.band_rows * W, chunk, max_ents) : 0;
    return l;
}

// Object maps (mw_label_project; kernel: mw_labelmap.hip): a workgroup of MW_LABELMAP_THREADS lanes per env.  Its LDS is one uint32 key per
// cell of the target — size * size of a window, gx * gz of a map — and behind the keys three words per id (n, si, sj): 68 596 bytes at
// MW_LABELMAP_MAX_CELLS = 16384 cells and MW_LABELMAP_MAX_IDS = 255 ids, above 64 KiB, which one workgroup may hold (a CU has 160 KiB; the
// engine asks for it as for mw_nav_grid_kernel).  fits: a positive count of no more cells than that, and 0 .. 255 ids — the caller
// refuses what does not.
inline Launch labelmap_launch(int N, long long cells, int ids)
{
    const bool fits = cells >= 1 && cells <= MW_LABELMAP_MAX_CELLS && ids >= 0 && ids <= MW_LABELMAP_MAX_IDS;
    const size_t lds = fits ? ((size_t)cells + 3 * (size_t)ids) * MW_LABELMAP_WORD_BYTES : 0;
    return {(unsigned long long)N, MW_LABELMAP_THREADS, lds, fits};
}

// Grid sight (mw_grid_sight; kernel: mw_sight.hip): a workgroup of MW_SIGHT_THREADS lanes per env.  Its LDS is a bit per cell of the
// opaque row in 32-bit words, with weights a byte per cell behind it, then a gain word per viewpoint, each rounded up to 16: 4 + 32 + 1
// KiB at MW_NAV_MAX_CELLS and MW_SIGHT_MAX_VIEWS.  fits: a positive count of no more cells than that and 1 .. MW_SIGHT_MAX_VIEWS
// viewpoints — the caller refuses what does not.
inline Launch sight_launch(int N, long long cells, bool weighted, int views)
{
    const bool fits = cells >= 1 && cells <= MW_NAV_MAX_CELLS && views >= 1 && views <= MW_SIGHT_MAX_VIEWS;
    const size_t lds = fits ? mwsight::bits_bytes(cells) + mwsight::weight_bytes(cells, weighted) + mwsight::gain_bytes(views) : 0;
    return {(unsigned long long)N, MW_SIGHT_THREADS, lds, fits};
}

// Grid regions (mw_grid_regions; kernel: mw_regions.hip): a workgroup of MW_REGIONS_THREADS lanes per env.  Its LDS is a uint16 label and
// a uint16 size per cell, an entry of 24 bytes per listed region and a word per lane, each rounded up to 16: 64 + 64 + 6 + 1 KiB at
// MW_NAV_MAX_CELLS and MW_REGION_MAX, which one workgroup may hold (a CU has 160 KiB); sized by the actual cell count, so that the Maze's
// 103 x 103 cells take 48 KiB and three workgroups share a CU.  fits: a positive count of no more cells than that and 1 .. MW_REGION_MAX
// regions — the caller refuses what does not.
inline Launch regions_launch(int N, long long cells, int max_regions)
{
    const bool fits = cells >= 1 && cells <= MW_NAV_MAX_CELLS && max_regions >= 1 && max_regions <= MW_REGION_MAX;
    const size_t lds = fits ? 2 * mwregions::label_bytes(cells) + mwregions::table_bytes(max_regions) + mwregions::scan_bytes() : 0;
    return {(unsigned long long)N, MW_REGIONS_THREADS, lds, fits};
}

}  // namespace mwpolicy
