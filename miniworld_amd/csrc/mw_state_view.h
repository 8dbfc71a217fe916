// State views on the device (mw_get_state_device / mw_set_state_where; kernels: mw_state_view.hip): which element of the engine's
// component-major arrays belongs to which element of a caller's row.  The caller's side is mw_state_view's, row-major per env:
// a per-env field of `inner` components is [envs][inner], a per-slot field [envs][E][inner].  The engine's side (MwArgs, mw_device.h) is
// component-major over all N envs: [inner][N] and [inner][E][N] — except the agent's position, three arrays of [N].  With `slots` = 1
// for a per-env field and E for a per-slot one both are the same rule: row element r is slot r / inner, component r % inner, and lives
// at ((r % inner) * slots + r / inner) * N + env.  The transposition mw_get_state / mw_set_state perform on the host (mw_engine.hip:
// state_xfer) is this arithmetic; tests/hostcheck/state_view_index.cpp runs the functions below against it on the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mwengine.h"
#include "mw_hd.h"

// The engine's arrays of the fields of mw_state_view, by name (a kernel argument: indexing a by-value struct at run time would
// cost a private copy in scratch — the note at MwGenTables, mw_device.h).
struct MwStateArrays {
    double *ax, *ay, *az, *adir, *cam, *light;
    int32_t *carry, *step, *picked;
    int32_t *ekind, *emesh, *estatic;
    double *epos, *edir, *egeom, *extent;
};

// components per env (or per slot) of the fields: mw_state_view's comments
#define MW_SV_POS 3
#define MW_SV_CAM 4
#define MW_SV_LIGHT 12
#define MW_SV_EPOS 3
#define MW_SV_EGEOM 9
#define MW_SV_EXTENT 4

namespace mwsv {

// row element of (slot s, component k) of a field of INNER components
template <int INNER>
MW_HD int row_index(int s, int k) { return s * INNER + k; }

// the engine's element of row element r of env `env`
template <int INNER>
MW_HD size_t dev_index(int r, int slots, size_t N, size_t env)
{
    const int s = r / INNER, k = r % INNER;
    return ((size_t)k * (size_t)slots + (size_t)s) * N + env;
}

// One env's row of one field, engine -> row; `lane` of `stride` workers take elements lane, lane + stride, ... (the kernels: a lane of
// the env's wavefront; the host: 0 of 1).
template <typename T, int INNER>
MW_HD void gather_row(T *row, const T *dev, int slots, size_t N, size_t env, int lane, int stride)
{
    for (int r = lane; r < slots * INNER; r += stride) row[r] = dev[dev_index<INNER>(r, slots, N, env)];
}
// ... and row -> engine
template <typename T, int INNER>
MW_HD void scatter_row(const T *row, T *dev, int slots, size_t N, size_t env, int lane, int stride)
{
    for (int r = lane; r < slots * INNER; r += stride) dev[dev_index<INNER>(r, slots, N, env)] = row[r];
}

// the agent's position: [3] in the row, three arrays in the engine
MW_HD void gather_pos(double *row, const double *ax, const double *ay, const double *az, size_t env, int lane, int stride)
{
    for (int r = lane; r < MW_SV_POS; r += stride) row[r] = r == 0 ? ax[env] : r == 1 ? ay[env] : az[env];
}
MW_HD void scatter_pos(const double *row, double *ax, double *ay, double *az, size_t env, int lane, int stride)
{
    for (int r = lane; r < MW_SV_POS; r += stride) (r == 0 ? ax : r == 1 ? ay : az)[env] = row[r];
}

// Every non-null field of the view, for one env: `item` is the env's row in the caller's buffers (env - first_env for a read of a
// range, the env itself for the masked write).  The fields are written out by name.
MW_HD void gather_env(const MwStateArrays &a, const mw_state_view &v, int E, size_t N, size_t env, size_t item, int lane, int stride)
{
    const size_t e = (size_t)E;
    if (v.agent_pos) gather_pos(v.agent_pos + item * MW_SV_POS, a.ax, a.ay, a.az, env, lane, stride);
    if (v.agent_dir) gather_row<double, 1>(v.agent_dir + item, a.adir, 1, N, env, lane, stride);
    if (v.cam) gather_row<double, MW_SV_CAM>(v.cam + item * MW_SV_CAM, a.cam, 1, N, env, lane, stride);
    if (v.light) gather_row<double, MW_SV_LIGHT>(v.light + item * MW_SV_LIGHT, a.light, 1, N, env, lane, stride);
    if (v.carrying) gather_row<int32_t, 1>(v.carrying + item, a.carry, 1, N, env, lane, stride);
    if (v.step_count) gather_row<int32_t, 1>(v.step_count + item, a.step, 1, N, env, lane, stride);
    if (v.num_picked_up) gather_row<int32_t, 1>(v.num_picked_up + item, a.picked, 1, N, env, lane, stride);
    if (v.ent_kind) gather_row<int32_t, 1>(v.ent_kind + item * e, a.ekind, E, N, env, lane, stride);
    if (v.ent_mesh) gather_row<int32_t, 1>(v.ent_mesh + item * e, a.emesh, E, N, env, lane, stride);
    if (v.ent_static) gather_row<int32_t, 1>(v.ent_static + item * e, a.estatic, E, N, env, lane, stride);
    if (v.ent_pos) gather_row<double, MW_SV_EPOS>(v.ent_pos + item * e * MW_SV_EPOS, a.epos, E, N, env, lane, stride);
    if (v.ent_dir) gather_row<double, 1>(v.ent_dir + item * e, a.edir, E, N, env, lane, stride);
    if (v.ent_geom) gather_row<double, MW_SV_EGEOM>(v.ent_geom + item * e * MW_SV_EGEOM, a.egeom, E, N, env, lane, stride);
    if (v.extent) gather_row<double, MW_SV_EXTENT>(v.extent + item * MW_SV_EXTENT, a.extent, 1, N, env, lane, stride);
}
MW_HD void scatter_env(const MwStateArrays &a, const mw_state_view &v, int E, size_t N, size_t env, size_t item, int lane, int stride)
{
    const size_t e = (size_t)E;
    if (v.agent_pos) scatter_pos(v.agent_pos + item * MW_SV_POS, a.ax, a.ay, a.az, env, lane, stride);
    if (v.agent_dir) scatter_row<double, 1>(v.agent_dir + item, a.adir, 1, N, env, lane, stride);
    if (v.cam) scatter_row<double, MW_SV_CAM>(v.cam + item * MW_SV_CAM, a.cam, 1, N, env, lane, stride);
    if (v.light) scatter_row<double, MW_SV_LIGHT>(v.light + item * MW_SV_LIGHT, a.light, 1, N, env, lane, stride);
    if (v.carrying) scatter_row<int32_t, 1>(v.carrying + item, a.carry, 1, N, env, lane, stride);
    if (v.step_count) scatter_row<int32_t, 1>(v.step_count + item, a.step, 1, N, env, lane, stride);
    if (v.num_picked_up) scatter_row<int32_t, 1>(v.num_picked_up + item, a.picked, 1, N, env, lane, stride);
    if (v.ent_kind) scatter_row<int32_t, 1>(v.ent_kind + item * e, a.ekind, E, N, env, lane, stride);
    if (v.ent_mesh) scatter_row<int32_t, 1>(v.ent_mesh + item * e, a.emesh, E, N, env, lane, stride);
    if (v.ent_static) scatter_row<int32_t, 1>(v.ent_static + item * e, a.estatic, E, N, env, lane, stride);
    if (v.ent_pos) scatter_row<double, MW_SV_EPOS>(v.ent_pos + item * e * MW_SV_EPOS, a.epos, E, N, env, lane, stride);
    if (v.ent_dir) scatter_row<double, 1>(v.ent_dir + item * e, a.edir, E, N, env, lane, stride);
    if (v.ent_geom) scatter_row<double, MW_SV_EGEOM>(v.ent_geom + item * e * MW_SV_EGEOM, a.egeom, E, N, env, lane, stride);
    if (v.extent) scatter_row<double, MW_SV_EXTENT>(v.extent + item * MW_SV_EXTENT, a.extent, 1, N, env, lane, stride);
}

// does the view name any field at all
MW_HD bool any_field(const mw_state_view &v)
{
    return v.agent_pos || v.agent_dir || v.cam || v.light || v.carrying || v.step_count || v.num_picked_up || v.ent_kind || v.ent_mesh ||
           v.ent_static || v.ent_pos || v.ent_dir || v.ent_geom || v.extent;
}

// what the masked write tests of an env before it writes anything of it: the carried slot and every entity kind
MW_HD bool carrying_ok(int32_t c, int E) { return c >= -1 && c < E; }
MW_HD bool kind_ok(int32_t k) { return k >= MW_ENT_NONE && k <= MW_ENT_FRAME; }

}  // namespace mwsv
