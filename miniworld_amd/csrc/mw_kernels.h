// The kernel interface: every kernel the host runtime (mw_engine*.hip) launches, declared once.  The engine includes this header to
// launch them and every translation unit that defines one includes it too, so a definition that drifts from its declaration does
// not compile.
#pragma once
#include "mw_device.h"
#include "mw_frame_plan.h"
#include "mw_snapshot.h"
#include "mw_snapframes.h"
#include "mw_state_view.h"
#include "mw_nav.h"
#include "mw_nav_grid.h"
#include "mw_ray.h"
#include "mw_seen.h"
#include "mw_ego.h"
#include "mw_depth.h"
#include "mw_label.h"
#include "mw_labelmap.h"
#include "mw_sight.h"
#include "mw_regions.h"

// a kernel and its list form: the same arguments, then the envs of a list (int32 [0] count, [1 + i] env) it draws instead of the
// whole batch — the second pass of a same-step auto-reset step with final observations (mw_engine_frame.hip)
#define MW_KERNEL_PAIR(stem, ...)                          \
    extern "C" __global__ void stem##_kernel(__VA_ARGS__); \
    extern "C" __global__ void stem##_sub_kernel(__VA_ARGS__, const int32_t *list)

// a kernel compiled once per random stream (mw_rng.h: MW_RNG_KIND): the Philox form and the PCG64 form
#define MW_RNG_PAIR(stem, ...)                             \
    extern "C" __global__ void stem##_kernel(__VA_ARGS__); \
    extern "C" __global__ void stem##_pcg_kernel(__VA_ARGS__)
// ... and the name of the one a unit defines: the form of the stream the unit is compiled for
#define MW_CAT_(a, b) a##b
#define MW_CAT(a, b) MW_CAT_(a, b)
#define MW_STREAM_SUFFIX_0
#define MW_STREAM_SUFFIX_1 _pcg
#define MW_KERNEL_NAME(stem) MW_CAT(MW_CAT(stem, MW_CAT(MW_STREAM_SUFFIX_, MW_RNG_KIND)), _kernel)

// K1, the step: one row per mode, MW_K1_ROW_<mode>(X) = X(stem, parameters), and four kernels per row: the wave-per-env form
// (mw_setup.hip) and the dense form, several envs per wavefront (mw_setup_dense.hip), each per random stream.  The Makefile compiles
// each of the two sources once per mode and stream, with MW_K1_MODE and MW_RNG_KIND; a unit takes its kernel's name and parameters
// from the row of its mode, and mw_setup_common.h has the mode's call of the step body.
#define MW_K1_DECLARE(stem, ...) MW_RNG_PAIR(stem, __VA_ARGS__); MW_RNG_PAIR(stem##_dense, __VA_ARGS__)
#define MW_K1_STEM(stem, ...) stem
#define MW_K1_PARAMS_OF(stem, ...) __VA_ARGS__
// mode 0, mw_step's
#define MW_K1_ARGS MwArgs a, int lanes_per_env, const int32_t *__restrict__ actions, float *__restrict__ reward, \
                   uint8_t *__restrict__ term, uint8_t *__restrict__ trunc
#define MW_K1_ROW_0(X) X(mw_step_setup, MW_K1_ARGS)
MW_K1_ROW_0(MW_K1_DECLARE);
// mode 1, mw_step_repeat's: the same sources around the sub-step loop (mw_setup_common.h: step_env_repeat), up to `repeat` sub-steps
// per env, the executed count into nsteps (may be null)
#define MW_K1_REPEAT_ARGS MW_K1_ARGS, int repeat, int32_t *__restrict__ nsteps
#define MW_K1_ROW_1(X) X(mw_step_repeat, MW_K1_REPEAT_ARGS)
MW_K1_ROW_1(MW_K1_DECLARE);
// mode 2, mw_step_plan's (step_env_repeat with PLAN): `actions` is the plans, int32 [horizon][N], sub-step k of
// every env reads row k; step_reward, float [horizon][N] or null, gets each sub-step's own reward; frameless != 0: no frame follows,
// the kernel applies the frame's tail behind the last executed sub-step itself
#define MW_K1_PLAN_ARGS MW_K1_ARGS, int horizon, int32_t *__restrict__ nsteps, float *__restrict__ step_reward, int frameless
#define MW_K1_ROW_2(X) X(mw_step_plan, MW_K1_PLAN_ARGS)
MW_K1_ROW_2(MW_K1_DECLARE);
// mode 3, mw_step_plan_trace's (step_env_repeat with PLAN and TRACE): the plan kernels' arguments and the caller's
// trace by value — device pointers, [horizon][N] rows, null = field not asked for; row k of env i := the state sub-step k left
#define MW_K1_TRACE_ARGS MW_K1_PLAN_ARGS, mw_plan_trace trace
#define MW_K1_ROW_3(X) X(mw_step_trace, MW_K1_TRACE_ARGS)
MW_K1_ROW_3(MW_K1_DECLARE);

// reset, spare refill, CollectHealth respawn, same-step install, spare take-over (mw_reset.hip, compiled once per stream)
MW_RNG_PAIR(mw_reset, MwArgs a, const uint8_t *__restrict__ mask, int force_all, int mark_refill);
MW_RNG_PAIR(mw_refill, MwArgs a);
MW_RNG_PAIR(mw_collect_respawn, MwArgs a);
MW_RNG_PAIR(mw_final_install, MwArgs a, const int32_t *__restrict__ list);
extern "C" __global__ void mw_take_spare_kernel(MwArgs a, const uint8_t *__restrict__ mask, int force_all);
// ... and with seeds the device holds: mw_reset_where's masked seeded reset, the seeded same-step install (mw_set_reset_seeds)
MW_RNG_PAIR(mw_reset_where, MwArgs a, const uint8_t *__restrict__ mask, const uint64_t *__restrict__ seeds);
MW_RNG_PAIR(mw_seed_install, MwArgs a, const int32_t *__restrict__ list, const uint64_t *__restrict__ next_seed);

// the geometry kernel (mw_geom.hip): small / big scenes, 8 samples per pixel compiled in or any
// view_flags beyond the view's own bits 0-2 (mw_geom.hip), small scenes' plain kernels only — set exactly where the plan kernel runs
// behind the launch (mw_policy.h: geom_deals): MW_GEOM_DEAL — the kernel builds only the envs the plan will have drawn, or whose
// pending removal it must still apply, and deals them evenly over the wavefronts (mw_geom_deal.h); every wavefront of a group takes
// each env's verdict from the plan kernel's functions (mw_frame_plan.h) on the bytes the plan kernel reads — K1's frame_clean and
// fc_key, the cache's key table fc_meta with fc_slots slots (the plan kernel's own arguments; null: no cache) —, and nothing writes
// them between the two, so built is a superset of drawn.  MW_GEOM_REUSE: the plan kernel's `reuse`.  built: uint8 [N], 1 where the launch built env's list, 0
// where it left the list, nvis and the header of an earlier frame (mw_get_geom_built); written in deal mode only.
#define MW_GEOM_DEAL 8
#define MW_GEOM_REUSE 16
#define MW_GEOM_ARGS MwArgs a, int view_flags, int S, int L, int n_env, const uint64_t *fc_meta, int fc_slots, uint8_t *built
MW_KERNEL_PAIR(mw_geom, MW_GEOM_ARGS);
MW_KERNEL_PAIR(mw_geom_big, MW_GEOM_ARGS);
MW_KERNEL_PAIR(mw_geom_any, MW_GEOM_ARGS);
MW_KERNEL_PAIR(mw_geom_big_any, MW_GEOM_ARGS);

// MW_RASTER_REUSE (mw_shape.h), a bit of the raster kernels' flag word (mw_policy.h::raster_flags): the observation buffer still
// holds every env's last frame, so an env whose frame_clean byte is set (MwArgs) is not drawn — the plain tile kernels' wavefronts of
// that env leave at once; for the quad kernel the frame plan (below) leaves the env out of its lists, and the kernel itself never
// reads the bit or the byte.  Only frames without mesh entities carry it: the bit is the lowest of the field that holds the
// slow-fragment stamp of a frame with meshes, and such a frame is always drawn in full.  The list forms never honour it.

// the tile kernels (mw_raster.hip)
// (the frame kernels take parameter lists, not one struct: only __restrict__ on a kernel parameter tells the compiler that the
// buffers do not overlap, and a by-value struct's pointers lose it — measured, tools/experiments/README.md)
// (texd == texels: the descriptor table is the head of the texel block, mw_engine.hip: upload_textures; the kernels
// use `texels` for both)
#define MW_RASTER_ARGS \
    int N, int W, int H, int max_vis, int tiles_x, int n_tiles, int waves_per_env, int tiles_per_wave, \
    const float *__restrict__ rec_raster, const float *__restrict__ rec_shade, const float *__restrict__ rec_cull, \
    const int32_t *__restrict__ nvis_arr, const float *__restrict__ envhdr, const MwTexDesc *__restrict__ texd, \
    const uint32_t *__restrict__ texels, uint8_t *__restrict__ obs, float *__restrict__ depth, int dbg, int texel_bytes, \
    const uint16_t *__restrict__ rec_order, const float *__restrict__ mesh_pos, const float *__restrict__ mesh_nrm, \
    const float *__restrict__ mesh_rgb, const float *__restrict__ mesh_uv, uint32_t *__restrict__ mesh_keys, \
    const float *__restrict__ plane_cache, int plane_cap, const float4 *__restrict__ slow_frags, const uint32_t *__restrict__ slow_head, \
    const uint32_t *__restrict__ tile_list, int32_t *__restrict__ tile_n, int tile_list_cap, int n_xcc, \
    const uint8_t *__restrict__ frame_clean
MW_KERNEL_PAIR(mw_raster, MW_RASTER_ARGS);
MW_KERNEL_PAIR(mw_raster_depth, MW_RASTER_ARGS);
MW_KERNEL_PAIR(mw_raster_big, MW_RASTER_ARGS);
MW_KERNEL_PAIR(mw_raster_big_depth, MW_RASTER_ARGS);
MW_KERNEL_PAIR(mw_raster_wrap, MW_RASTER_ARGS);
MW_KERNEL_PAIR(mw_raster_big_wrap, MW_RASTER_ARGS);
MW_KERNEL_PAIR(mw_raster_ragged, MW_RASTER_ARGS);
MW_KERNEL_PAIR(mw_raster_big_ragged, MW_RASTER_ARGS);
MW_KERNEL_PAIR(mw_raster_nomesh, MW_RASTER_ARGS);
MW_KERNEL_PAIR(mw_raster_nomesh_depth, MW_RASTER_ARGS);
MW_KERNEL_PAIR(mw_raster_mesh, MW_RASTER_ARGS);
MW_KERNEL_PAIR(mw_raster_mesh_depth, MW_RASTER_ARGS);
MW_KERNEL_PAIR(mw_raster_mesh_wrap, MW_RASTER_ARGS);
MW_KERNEL_PAIR(mw_raster_big_mesh_wrap, MW_RASTER_ARGS);

// the quad kernel (mw_rasterq.hip): one workgroup of MWQ_THREADS lanes per env, 8 or 4 samples per pixel
// plan == null: workgroup b draws env b (the list forms: env list[1 + b] while b < list[0]).
// plan != null (mw_frame_plan.h: the block mw_frame_plan_kernel filled behind the geometry kernel; plain whole-batch steps only,
// mw_policy.h: frame_plans): the kernel decides nothing about an env itself.  Workgroup b < n_draw draws the env of draw entry b — in
// an ordered plan the entry mw_plan_slot names: the cost classes from the highest down, so the longest frames start first —;
// workgroup n_draw <= b < n_draw + n_copy copies the frame, and the depth map, of the slot its copy entry names from the frame cache
// into the caller's buffers — 16-, 4- or 1-byte stores by the buffer's alignment — and leaves before any barrier; every other
// workgroup leaves at once.  So the drawing workgroups are the first the launch dispatches and the copies fill its tail; nothing
// waits on another workgroup, and no result depends on the order of dispatch or of the entries.
// The frame cache (mw_set_frame_cache), fc != null (MwFcArgs, mw_device.h; only with a plan) — uint8 HWC frames without mesh entities
// only, never the list forms: a frame the kernel draws also goes to the slot its draw entry names (the plan kernel read it from the
// env's header: round-robin), with the key K1 stored for it (MwArgs::fc_key), and the header advances; a copy changes nothing.
// The source byte (MwArgs::fc_source; mw_get_frame_source) — 0 drawn, 1 left alone as clean, 2 + j copied from slot j — is K1's 0
// for every env, overwritten for every env by the plan kernel where one runs.
#define MWQ_THREADS 512
#define MWQ_ARGS \
    int N, int W, int H, int max_vis, int tiles_x, int n_tiles, \
    const float *__restrict__ rec_raster, const float *__restrict__ rec_shade, const float *__restrict__ rec_cull, \
    const int32_t *__restrict__ nvis_arr, const float *__restrict__ envhdr, const uint32_t *__restrict__ texels, \
    uint8_t *__restrict__ obs, float *__restrict__ depth, int dbg, int texel_bytes, unsigned long long *__restrict__ prof, \
    const MwFcArgs *__restrict__ fc, const uint32_t *__restrict__ plan
MW_KERNEL_PAIR(mw_rasterq, MWQ_ARGS);
MW_KERNEL_PAIR(mw_rasterq4, MWQ_ARGS);
// bytes of dynamic LDS a launch needs; the longest display list the quad path draws (longer ones: the tile code)
extern "C" int mw_rasterq_lds_bytes(int S, int W, int H, int n_tiles, int depth);
extern "C" int mw_rasterq_cap(int depth);

// the mesh entity and slow-path kernels, the XCD probe (mw_raster_mesh.hip)
extern "C" __global__ void mw_mesh_entity_kernel(
    int N, int W, int H, const float *__restrict__ envhdr, const MwMeshDesc *__restrict__ meshes, const float4 *__restrict__ mesh_vpos,
    const uint2 *__restrict__ mesh_idx, const float *__restrict__ mesh_stream, const float *__restrict__ mesh_attr, uint32_t *__restrict__ keys_all,
    float *__restrict__ plane_cache, int plane_cap, int32_t *__restrict__ slow_count, uint32_t *__restrict__ slow_tris, const uint32_t *__restrict__ ent_list,
    int ent_list_cap, int32_t *ent_n, int32_t *ent_n_after, uint32_t *__restrict__ slow_envs, int n_xcc, unsigned long long *prof);
extern "C" __global__ void mw_mesh_slow_kernel(int W, int H, const float *envhdr, const float *mesh_pos, const float *mesh_nrm, const float *mesh_rgb,
                                               const float *mesh_uv, const uint32_t *texels, int texel_bytes, uint32_t *keys, int32_t *counts, int N,
                                               int parity, const uint32_t *slow_tris, float4 *frags, uint32_t *heads, uint32_t stamp, uint32_t *status,
                                               const uint32_t *slow_envs, const int32_t *slow_env_n);
extern "C" __global__ void mw_xcc_probe_kernel(uint32_t *out);

// the generic-resolution kernels (mw_raster_mesh.hip; the list forms in mw_raster_view_list.hip, the raster kernel for frames off
// the grid and wrapper layouts in mw_raster_view_any.hip)
MW_KERNEL_PAIR(mw_view_mesh, int W, int H, int S, int first_env, const float *__restrict__ envhdr, const float *__restrict__ mesh_pos, uint32_t *keys);
#define MW_VIEW_RASTER_ARGS \
    int first_env, int W, int H, int S, int max_vis, int tiles_x, const float *__restrict__ rec_raster, \
    const float *__restrict__ rec_shade, const float *__restrict__ rec_cull, const int32_t *__restrict__ nvis_arr, const float *__restrict__ envhdr, \
    const MwTexDesc *__restrict__ texd, const uint32_t *__restrict__ texels, const float *__restrict__ mesh_pos, \
    const float *__restrict__ mesh_nrm, const float *__restrict__ mesh_rgb, const float *__restrict__ mesh_uv, const uint32_t *mesh_keys, \
    uint8_t *__restrict__ out, float *__restrict__ depth, int texel_bytes, int layout
MW_KERNEL_PAIR(mw_view_raster, MW_VIEW_RASTER_ARGS);
MW_KERNEL_PAIR(mw_view_raster_any, MW_VIEW_RASTER_ARGS);

// frame stacking (mw_stack.hip): the push behind a step's last raster kernel, mw_stack_refresh's form of the same body, mw_reset's marks.
// Grid (N, chunks of MW_STACK_THREADS * MW_STACK_UNROLL units: mw_shape.h); a unit is 16 bytes (`wide`: obs, ring, the final buffers and the frame
// size are all multiples of 16) or one byte.  The per-env flag byte: MW_STACK_FRESH — reset by the host or never pushed, the stack is
// rebuilt by mw_stack_refresh or the next push; MW_STACK_PENDING — the env's next call installs a world (next-step auto-reset), the
// push of that call rebuilds.
#define MW_STACK_FRESH 1
#define MW_STACK_PENDING 2
#define MW_STACK_ARGS \
    int depth, int pad, int phase, unsigned long long frame_bytes, int wide, const uint8_t *__restrict__ obs, uint8_t *ring, \
    const uint8_t *__restrict__ flags_in, uint8_t *__restrict__ flags_out
extern "C" __global__ void mw_stack_push_kernel(MW_STACK_ARGS, const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc,
                                                const uint8_t *__restrict__ pending, const uint8_t *__restrict__ final_obs,
                                                uint8_t *__restrict__ final_stack);
extern "C" __global__ void mw_stack_refresh_kernel(MW_STACK_ARGS);
extern "C" __global__ void mw_stack_mark_kernel(int N, const uint8_t *__restrict__ mask, int force_all, uint8_t *__restrict__ flags);
// behind the step kernel of a frameless mw_step_plan, which pushes nothing: the current flag bytes follow the episodes that began and
// ended inside the call (term, trunc: the call's flags where it installs worlds on the sub-step that ends an episode, else null;
// pending: reset_pending where the env's next call installs one, else null).  One thread per env.
extern "C" __global__ void mw_stack_plan_kernel(int N, const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc,
                                                const uint8_t *__restrict__ pending, uint8_t *__restrict__ flags);

// snapshot records (mw_snapshot.hip; the layout: mw_snapshot.h): one launch per save, one per load.  A 1-D grid of MW_SNAP_THREADS
// lanes: first the component blocks — (row of a component, 256 consecutive items), a lane per item —, then, with per-env geometry
// sets, the blob blocks — (item, geometry set, chunk of its polygons or segments), 16-byte units.
//
// The items of a call, the last arguments of all four kernels.  Item k is present when k < count and (mask is null or mask[k] != 0);
// its env is d_envs ? d_envs[k] : k, its record d_recs ? d_recs[k] : k, and neither array is read for an absent item.  Every index is
// tested against its limit; an offending item is skipped and sets MW_ST_SNAPSHOT_BAD.  So the plain calls, the saves into chosen records
// (_at) and the masked loads (_where: count = N, d_envs null; a workgroup whose items are all unmasked leaves after reading the mask)
// are the same kernels.  (Separate parameters, not a struct: the note at MW_RASTER_ARGS.)
#define MW_SNAP_ITEMS const int32_t *__restrict__ d_envs, const int32_t *__restrict__ d_recs, const uint8_t *__restrict__ mask
#define MW_SNAP_ARGS \
    const MwSnapTable *__restrict__ tab, MwSnapKey key, int N, int capacity, int count, int item_chunks, uint32_t *__restrict__ status
extern "C" __global__ void mw_snapshot_save_kernel(MW_SNAP_ARGS, uint8_t *__restrict__ snap, MW_SNAP_ITEMS);
//   n_recs               the records of the buffer that are valid
//   frame_clean, occ_valid, stack_flags  what a load resets for every env it writes (the last two may be null)
//   fc_epoch             null, or advanced for every env written (MwArgs::fc_epoch): the masked form, where it stands in for the host's
//                        cache-wide invalidation
extern "C" __global__ void mw_snapshot_load_kernel(MW_SNAP_ARGS, const uint8_t *__restrict__ snap, int n_recs, uint8_t *__restrict__ frame_clean,
                                                   int32_t *__restrict__ occ_valid, uint8_t *__restrict__ stack_flags, uint32_t *__restrict__ fc_epoch,
                                                   MW_SNAP_ITEMS);

// frame records (mw_snapframes.hip; the layout and MwSnapfArgs: mw_snapframes.h): one launch per call, a 1-D grid of MW_SNAPF_THREADS
// lanes, workgroup (item, chunk of the record: its obs row, its depth row, its K window frames).  Items (MW_SNAP_ITEMS; a.count, a.N,
// a.n_recs) and their index tests as for the state records; a load compares the key first.  The frame buffer does not alias obs, depth
// or the ring (the caller's contract).
//   obs, depth, ring, stack_flags  the caller's rows, the stack's ring and the CURRENT half of its flag bytes (depth / the last two:
//                                  null without MW_SNAPF_DEPTH / MW_SNAPF_STACK)
#define MW_SNAPF_ARGS MwSnapfArgs a, uint32_t *__restrict__ status
extern "C" __global__ void mw_snapshot_save_frames_kernel(MW_SNAPF_ARGS, const uint8_t *__restrict__ obs, const uint8_t *__restrict__ depth,
                                                          const uint8_t *__restrict__ ring, const uint8_t *__restrict__ stack_flags,
                                                          uint8_t *__restrict__ frames, MW_SNAP_ITEMS);
extern "C" __global__ void mw_snapshot_load_frames_kernel(MW_SNAPF_ARGS, const uint8_t *__restrict__ frames, uint8_t *__restrict__ obs,
                                                          uint8_t *__restrict__ depth, uint8_t *__restrict__ ring, uint8_t *__restrict__ stack_flags,
                                                          MW_SNAP_ITEMS);

// the host runtime's own small kernels (mw_engine_kernels.hip): mw_get_info's gather; behind the first pass of a same-step step with
// final observations, the list of the envs that finished and the copy of their rows into the final buffers
extern "C" __global__ void mw_info_kernel(int N, int E, const int32_t *health, const double *epos, int slot, int32_t *out_health, double *out_pos);
extern "C" __global__ void mw_final_list_kernel(int N, const uint8_t *__restrict__ pending, int32_t *__restrict__ pending_remove, int32_t *__restrict__ list);
extern "C" __global__ void mw_final_copy_kernel(const int32_t *__restrict__ list, const uint8_t *__restrict__ obs, uint8_t *__restrict__ final_obs,
                                                unsigned long long row_bytes, const float *__restrict__ depth, float *__restrict__ final_depth, int depth_row);
// ... and the frame plan of a plain whole-batch step through the quad kernel (mw_frame_plan.h), behind the geometry kernel: a lane per
// env; grid ceil(N / MW_PLAN_ENVS) x 64 lanes
#define MW_PLAN_ENVS 64
extern "C" __global__ void mw_frame_plan_kernel(int N, int reuse, const uint8_t *__restrict__ frame_clean, const uint64_t *__restrict__ key,
                                                const uint64_t *__restrict__ meta, int slots, const int32_t *__restrict__ nvis,
                                                uint8_t *__restrict__ frame_source, uint32_t *__restrict__ plan, uint32_t *__restrict__ next);

// state views (mw_state_view.hip; the index arithmetic and MwStateArrays: mw_state_view.h): one launch per call, a wavefront per env,
// MW_SV_ENVS envs per workgroup.  The view is the caller's mw_state_view by value: device pointers, null = field not asked for.
//   get        item k < count is env first_env + k, row k of every non-null field := its state
//   set_where  grid over all N envs; env i with mask[i] != 0: row i of every non-null field into the engine, then reset_pending,
//              frame_clean, fc_epoch and the MW_STACK_PENDING bit of stack_flags (the current half; null without a stack) as
//              mw_set_state_where owes them; an env whose carrying or ent_kind row is out of range writes nothing and sets MW_ST_STATE_BAD
#define MW_SV_THREADS 256
#define MW_SV_ENVS (MW_SV_THREADS / 64)
extern "C" __global__ void mw_state_get_kernel(MwStateArrays a, mw_state_view v, int N, int E, int first_env, int count);
extern "C" __global__ void mw_state_set_where_kernel(MwStateArrays a, mw_state_view v, const uint8_t *__restrict__ mask, int N, int E,
                                                     uint32_t *__restrict__ status, uint8_t *__restrict__ reset_pending,
                                                     uint8_t *__restrict__ frame_clean, uint32_t *__restrict__ fc_epoch,
                                                     uint8_t *__restrict__ stack_flags);

// navigation fields (mw_nav.hip; the arithmetic, the phases and MwNavArgs: mw_nav.h).  The parameters are the caller's mw_nav_params by
// value; d_target null = the slot target.
//   build  grid N workgroups of MW_NAV_THREADS lanes, 2 * gx * gz bytes of dynamic LDS; env b's row of `field` where mask is null or
//          mask[b] != 0; passes: null, or int32[N] that gets the env's count of relaxation rounds (measurements)
//   query  a lane per env; pos null = the agents; cost, next, waypoint: any may be null
#define MW_NAV_THREADS 512
#define MW_NAV_QUERY_THREADS 256
extern "C" __global__ void mw_nav_build_kernel(MwNavArgs a, mw_nav_params p, const uint8_t *__restrict__ mask, const double *__restrict__ d_target,
                                               uint16_t *__restrict__ field, int32_t *__restrict__ passes);
extern "C" __global__ void mw_nav_query_kernel(MwNavArgs a, mw_nav_params p, const double *__restrict__ d_target, const uint16_t *__restrict__ field,
                                               const double *__restrict__ pos, int32_t *__restrict__ cost, int32_t *__restrict__ next,
                                               double *__restrict__ waypoint);
// grid navigation fields (mw_nav_grid.hip; the phases: mw_nav_grid.h): the build over the caller's own rows — blocked, and sources,
// d_target (at least one of the two) and extra, each uint8[N][gz][gx] or null.  R: mwnav::inflate_radius of the parameters.  Grid,
// lanes, mask and passes as for the build above; mwpolicy::nav_grid_launch gives the dynamic LDS.
extern "C" __global__ void mw_nav_grid_kernel(MwNavArgs a, mw_nav_params p, int R, const uint8_t *__restrict__ mask, const uint8_t *__restrict__ blocked,
                                              const uint8_t *__restrict__ sources, const double *__restrict__ d_target, const uint8_t *__restrict__ extra,
                                              uint16_t *__restrict__ field, int32_t *__restrict__ passes);

// ray casts (mw_ray.hip; the arithmetic, MwRayArgs and the launch constants: mw_ray.h; the choice of form: mwpolicy::ray_launch).  The
// parameters are the caller's mw_ray_params by value; origin null = the agents, exactly one of dir / offsets (the fan) non-null; hit
// and dir_out may be null; an env under a zero mask byte is skipped.
//   lanes  grid N workgroups of 64 .. MW_RAY_THREADS lanes, a ray per lane, max_segs * MW_RAY_WALL_BYTES + E * MW_RAY_DISC_BYTES bytes
//          of dynamic LDS
//   waves  grid ceil(N * R / MW_RAY_WAVES) workgroups of MW_RAY_WAVES wavefronts, a wavefront per ray, an obstacle per lane
extern "C" __global__ void mw_ray_lanes_kernel(MwRayArgs a, mw_ray_params p, const uint8_t *__restrict__ mask, const double *__restrict__ origin,
                                               const double *__restrict__ dir, const double *__restrict__ offsets, double *__restrict__ t_out,
                                               int32_t *__restrict__ hit_out, double *__restrict__ dir_out);
extern "C" __global__ void mw_ray_waves_kernel(MwRayArgs a, mw_ray_params p, const uint8_t *__restrict__ mask, const double *__restrict__ origin,
                                               const double *__restrict__ dir, const double *__restrict__ offsets, double *__restrict__ t_out,
                                               int32_t *__restrict__ hit_out, double *__restrict__ dir_out);

// explored-area maps (mw_seen.hip; the tests, the phases and the launch constants: mw_seen.h; the launch: mwpolicy::seen_launch).  The
// grid is the caller's mw_nav_params by value (cell, gx, gz are read), the sight its range, cos(fov / 2) and flags.  Grid N workgroups
// of MW_SEEN_THREADS lanes, max_segs * MW_RAY_WALL_BYTES + E * MW_RAY_DISC_BYTES (rounded up to 16) + MW_SEEN_TAIL_BYTES bytes of
// dynamic LDS; env b's row of `seen`, count[b] and newly[b] where mask is null or mask[b] != 0; clear and newly may be null.
extern "C" __global__ void mw_seen_kernel(MwRayArgs a, mw_nav_params p, mwseen::Sight s, const uint8_t *__restrict__ mask, const uint8_t *__restrict__ clear,
                                          uint8_t *seen, int32_t *__restrict__ count, int32_t *__restrict__ newly);

// egocentric map windows (mw_ego.hip; the point, the tests, the phases and the launch constant: mw_ego.h; the launch: mwpolicy::ego_launch).
// The window, the sight (range, cos(fov / 2), flags) and the sampled grid travel by value.  Grid N workgroups of MW_EGO_THREADS lanes,
// mwego::staged_bytes(max_segs, E, planes) bytes of dynamic LDS; env b's [P][size][size] bytes of `planes` and its row of `sample` where
// mask is null or mask[b] != 0; pos null = the agents; planes null iff no plane is asked for; src and sample both null = no sample.
extern "C" __global__ void mw_ego_kernel(MwRayArgs a, mwego::Window w, mwseen::Sight s, mwego::Source q, const uint8_t *__restrict__ mask,
                                         const double *__restrict__ pos, uint8_t *__restrict__ planes, const void *__restrict__ src,
                                         void *__restrict__ sample);

// depth projection (mw_depth.hip; the arithmetic, the phases and the launch constants: mw_depth.h; the launch: mwpolicy::depth_launch).  The
// sensor, the window and the grid (cell, gx, gz are read) travel by value; cam is the world's [4][N] camera rows.  Grid N workgroups of
// MW_DEPTH_THREADS lanes, MW_DEPTH_CELL_BYTES of dynamic LDS per cell of the target; exactly one of planes ([N][2][size][size]) and map
// ([N][2][gz][gx], with count [N][2]) is non-null; env b's rows where mask is null or mask[b] != 0; clear and newly may be null; wide != 0:
// W * H is a multiple of 4 and depth 16-byte aligned.
extern "C" __global__ void mw_depth_kernel(MwRayArgs a, const double *__restrict__ cam, mwdepth::Sensor s, mwdepth::Window w, mw_nav_params p, int min_points,
                                           int wide, const float *__restrict__ depth, const uint8_t *__restrict__ mask, const uint8_t *__restrict__ clear,
                                           uint8_t *__restrict__ planes, uint8_t *__restrict__ map, int32_t *__restrict__ count, int32_t *__restrict__ newly);

// label frames (mw_label.hip; the arithmetic, the phases, MwLabelArgs and the launch constants: mw_label.h; the launch: mwpolicy::label_launch).
// The parameters are the caller's mw_label_params by value.  Grid N workgroups of MW_LABEL_THREADS lanes, mwlabel::plan_bytes(band_rows * W,
// chunk, E) bytes of dynamic LDS; env b's rows of the outputs where mask is null or mask[b] != 0; every output but cls may be null;
// prune == 0: the mesh phase without its pruning rectangle (MW_LABEL_UNPRUNED).
extern "C" __global__ void mw_label_kernel(MwLabelArgs a, mw_label_params p, int band_rows, int chunk, int prune, const uint8_t *__restrict__ mask,
                                           uint8_t *__restrict__ cls, int32_t *__restrict__ code, float *__restrict__ depth,
                                           int32_t *__restrict__ ent_pixels, int32_t *__restrict__ ent_box);

// object maps (mw_labelmap.hip; the arithmetic, the phases and the launch constants: mw_labelmap.h; the launch: mwpolicy::labelmap_launch).
// The sensor, the window and the grid travel by value as for mw_depth_kernel, whose cam it reads too.  Grid N workgroups of
// MW_LABELMAP_THREADS lanes, MW_LABELMAP_WORD_BYTES of dynamic LDS per cell of the target and three times that per id; exactly one of plane
// ([N][size][size]) and map ([N][gz][gx]) is non-null; env b's rows where mask is null or mask[b] != 0; clear may be null; K ids (0 with a
// plane) with obj_cells ([N][K]) and obj_pos ([N][K][3]), either of which may be null; wide != 0: W * H is a multiple of 4 and depth and
// code 16-byte aligned.
extern "C" __global__ void mw_labelmap_kernel(MwRayArgs a, const double *__restrict__ cam, mwdepth::Sensor s, mwdepth::Window w, mw_nav_params p, int wide,
                                              const float *__restrict__ depth, const int32_t *__restrict__ code, int32_t base, const uint8_t *__restrict__ mask,
                                              const uint8_t *__restrict__ clear, uint8_t *__restrict__ plane, uint8_t *__restrict__ map, int K,
                                              int32_t *__restrict__ obj_cells, double *__restrict__ obj_pos);

// grid sight (mw_sight.hip; the rule, the walk, the phases and the launch constant: mw_sight.h; the launch: mwpolicy::sight_launch).  The grid
// (cell, gx, gz are read) and the sight (range, cos(fov / 2); no flags) travel by value; R = mwsight::reach_cells, chunks =
// mwsight::chunks_of of them.  Grid N workgroups of MW_SIGHT_THREADS lanes; opaque and weight (or null) uint8[N][gz][gx]; cells
// int32[N][views] with dirs float64[N][views] or null, or cells null (views = 1): the agents; env b's row of gain ([N][views]) and its
// cells of seen (or null) where mask is null or mask[b] != 0.
extern "C" __global__ void mw_sight_kernel(MwRayArgs a, mw_nav_params p, mwseen::Sight s, int views, int R, int chunks, const uint8_t *__restrict__ mask,
                                           const uint8_t *__restrict__ opaque, const uint8_t *__restrict__ weight, const int32_t *__restrict__ cells,
                                           const double *__restrict__ dirs, int32_t *__restrict__ gain, uint8_t *seen);

// grid regions (mw_regions.hip; the rule, the arrays, the phases and the launch constant: mw_regions.h; the launch: mwpolicy::regions_launch).
// The view is not read.  Grid N workgroups of MW_REGIONS_THREADS lanes; member uint8[N][gz][gx]; diag != 0: connectivity 8; K listed
// regions at most; env b's element of count ([N]), its rows of size and cell ([N][K]), of sum
// ([N][K][2], or null) and of out (int16[N][gz][gx], or null) where mask is null or mask[b] != 0.
extern "C" __global__ void mw_regions_kernel(MwNavArgs a, int gx, int gz, int diag, int min_cells, int K, const uint8_t *__restrict__ mask,
                                             const uint8_t *__restrict__ member, int32_t *__restrict__ count, int32_t *__restrict__ size,
                                             int32_t *__restrict__ cell, int32_t *__restrict__ sum, int16_t *__restrict__ out);

// the occlusion queries of mw_visible_ents (mw_visible.hip)
extern "C" __global__ void mw_visible_kernel(int env_base, int W, int H, int S, int max_vis, int E, const float *__restrict__ rec_raster,
                                             const float *__restrict__ rec_cull, const int32_t *__restrict__ nvis, uint8_t *__restrict__ vis);
