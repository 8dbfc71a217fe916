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
#include "mw_world_fields.h"

// The engine's arrays of the fields of mw_state_view, by name (a kernel argument: indexing a by-value struct at run time would
// cost a private copy in scratch — the note at MwGenTables, mw_device.h): the rows of MW_WORLD_FIELDS that a view reaches, so that a
// view field cannot exist without its array.
struct MwStateArrays {
#define X(m, T, inner, slot, when, spare, view, vf) MW_WF_INVIEW_##view(T *m;)
    MW_WORLD_FIELDS(X)
#undef X
};

// components of agent_pos, the one field that is no row of the table: [3] in a row, the arrays ax, ay, az in the engine
#define MW_SV_POS 3
// every other field of mw_state_view is a VIEW row (of the row's element type: gather_row / scatter_row take row and array as T * alike)
#define X(m, T, inner, slot, when, spare, view, vf) MW_WF_VIEWED_##view(+1)
static_assert(sizeof(mw_state_view) == (1 MW_WORLD_FIELDS(X)) * sizeof(void *), "mw_state_view has a field that is no row of MW_WORLD_FIELDS");
#undef X

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

// Every non-null field of the view, for one env, engine -> rows (GATHER) or rows -> engine: `item` is the env's row in the caller's
// buffers (env - first_env for a read of a range, the env itself for the masked write).  One statement per VIEW row of the table: the
// field's and the array's names reach the compiler as names.
template <bool GATHER>
MW_HD void copy_env(const MwStateArrays &a, const mw_state_view &v, int E, size_t N, size_t env, size_t item, int lane, int stride)
{
    if (v.agent_pos && GATHER) gather_pos(v.agent_pos + item * MW_SV_POS, a.ax, a.ay, a.az, env, lane, stride);
    if (v.agent_pos && !GATHER) scatter_pos(v.agent_pos + item * MW_SV_POS, a.ax, a.ay, a.az, env, lane, stride);
#define X(m, T, inner, slot, when, spare, view, vf)                                                                                                   \
    MW_WF_VIEWED_##view(if (v.vf && GATHER) gather_row<T, inner>(v.vf + item * (size_t)((slot ? E : 1) * inner), a.m, slot ? E : 1, N, env, lane, stride); \
                        if (v.vf && !GATHER) scatter_row<T, inner>(v.vf + item * (size_t)((slot ? E : 1) * inner), a.m, slot ? E : 1, N, env, lane, stride);)
    MW_WORLD_FIELDS(X)
#undef X
}
MW_HD void gather_env(const MwStateArrays &a, const mw_state_view &v, int E, size_t N, size_t env, size_t item, int lane, int stride) { copy_env<true>(a, v, E, N, env, item, lane, stride); }
MW_HD void scatter_env(const MwStateArrays &a, const mw_state_view &v, int E, size_t N, size_t env, size_t item, int lane, int stride) { copy_env<false>(a, v, E, N, env, item, lane, stride); }

// does the view name any field at all
MW_HD bool any_field(const mw_state_view &v)
{
#define X(m, T, inner, slot, when, spare, view, vf) MW_WF_VIEWED_##view(|| v.vf)
    return v.agent_pos MW_WORLD_FIELDS(X);
#undef X
}

// what the masked write tests of an env before it writes anything of it: the carried slot and every entity kind
MW_HD bool carrying_ok(int32_t c, int E) { return c >= -1 && c < E; }
MW_HD bool kind_ok(int32_t k) { return k >= MW_ENT_NONE && k <= MW_ENT_FRAME; }

}  // namespace mwsv
