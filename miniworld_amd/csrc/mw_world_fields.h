// The per-env arrays that make up a world, ONCE: every list of them is an expansion of MW_WORLD_FIELDS — the engine's allocations,
// the spare world's, the generators' redirection to the spare and the host's mw_get_state / mw_set_state (mw_engine.hip), the
// components of a snapshot record (mw_snapshot.h), the state views (mw_state_view.h).  MwArgs, MwSpare (mw_device.h) and
// mw_state_view (include/mwengine.h) stay written out member by member: a row NAMES their members, and a row that names one they
// lack does not compile.  Not derived, because they are hand-scheduled code on the step's critical path: take_spare /
// take_spare_lane (mw_gen.h).  Plain C++: the host checks compile it without HIP.
//
// A row X(member, type, inner, per_slot, when, spare, view, view_field):
//   member      the array's name in MwArgs, and in MwSpare where the spare world has a copy
//   type        of an element
//   inner       components per env (per_slot 0: the array is [inner][N]) or per entity slot (per_slot 1: [inner][E][N])
//   when        the engine has the array ALWAYS, with MW_TASK_COLLECT alone (COLLECT), with per-env geometry sets alone (GEO: the
//               counts of the sets, which are allocated with the sets' blobs and not by the expansion — MW_WF_OWNED_*)
//   spare       SP: the spare world has a copy; NOSP
//   view        VIEW: mw_state_view's field `view_field` exposes the array; POS: one of the three arrays behind agent_pos, the view
//               code's one special case (gather_pos / scatter_pos); NOVIEW (view_field: none)
// THE ROW ORDER IS THE RECORD FORMAT: the live components of a snapshot record are the rows in this order, the spare's the SP rows
// in this order (mw_snapshot.h): a row added, removed or moved is a new MW_SNAP_FORMAT.
#pragma once
#include <stdint.h>

#include "mw_hd.h"

#define MW_WORLD_FIELDS(X) \
    X(ax,             double,    1, 0, ALWAYS,  SP,   POS,    agent_pos) \
    X(ay,             double,    1, 0, ALWAYS,  SP,   POS,    agent_pos) \
    X(az,             double,    1, 0, ALWAYS,  SP,   POS,    agent_pos) \
    X(adir,           double,    1, 0, ALWAYS,  SP,   VIEW,   agent_dir) \
    X(cam,            double,    4, 0, ALWAYS,  SP,   VIEW,   cam) \
    X(light,          double,   12, 0, ALWAYS,  SP,   VIEW,   light) \
    X(extent,         double,    4, 0, ALWAYS,  SP,   VIEW,   extent) \
    X(carry,          int32_t,   1, 0, ALWAYS,  NOSP, VIEW,   carrying) \
    X(step,           int32_t,   1, 0, ALWAYS,  NOSP, VIEW,   step_count) \
    X(picked,         int32_t,   1, 0, ALWAYS,  NOSP, VIEW,   num_picked_up) \
    X(health,         int32_t,   1, 0, COLLECT, NOSP, NOVIEW, none) \
    X(final_health,   int32_t,   1, 0, COLLECT, NOSP, NOVIEW, none) \
    X(final_goal,     double,    3, 0, ALWAYS,  NOSP, NOVIEW, none) \
    X(ekind,          int32_t,   1, 1, ALWAYS,  SP,   VIEW,   ent_kind) \
    X(emesh,          int32_t,   1, 1, ALWAYS,  SP,   VIEW,   ent_mesh) \
    X(estatic,        int32_t,   1, 1, ALWAYS,  SP,   VIEW,   ent_static) \
    X(epos,           double,    3, 1, ALWAYS,  SP,   VIEW,   ent_pos) \
    X(edir,           double,    1, 1, ALWAYS,  SP,   VIEW,   ent_dir) \
    X(egeom,          double,    9, 1, ALWAYS,  SP,   VIEW,   ent_geom) \
    X(rng,            uint64_t,  5, 0, ALWAYS,  NOSP, NOVIEW, none) \
    X(pending_remove, int32_t,   1, 0, ALWAYS,  NOSP, NOVIEW, none) \
    X(reset_pending,  uint8_t,   1, 0, ALWAYS,  NOSP, NOVIEW, none) \
    X(npolys,         int32_t,   1, 0, GEO,     SP,   NOVIEW, none) \
    X(nsegs,          int32_t,   1, 0, GEO,     SP,   NOVIEW, none)

// Filters: MW_WF_<what>_##column(code) leaves `code` for the rows that qualify and nothing for the others.
#define MW_WF_ON(...) __VA_ARGS__
#define MW_WF_OFF(...)
#define MW_WF_SPARE_SP MW_WF_ON             // the spare world has a copy
#define MW_WF_SPARE_NOSP MW_WF_OFF
#define MW_WF_VIEWED_VIEW MW_WF_ON          // a field of mw_state_view of its own
#define MW_WF_VIEWED_POS MW_WF_OFF
#define MW_WF_VIEWED_NOVIEW MW_WF_OFF
#define MW_WF_INVIEW_VIEW MW_WF_ON          // reachable through mw_state_view at all (a member of MwStateArrays)
#define MW_WF_INVIEW_POS MW_WF_ON
#define MW_WF_INVIEW_NOVIEW MW_WF_OFF
#define MW_WF_OWNED_ALWAYS MW_WF_ON         // allocated (and redirected to the spare) by the expansions in mw_engine.hip
#define MW_WF_OWNED_COLLECT MW_WF_ON
#define MW_WF_OWNED_GEO MW_WF_OFF

enum { MW_WF_ALWAYS = 0, MW_WF_COLLECT, MW_WF_GEO };

// rows of an array ([rows][N]) in an engine of E entity slots; 0: the engine has no such array
MW_HD int32_t mw_wf_rows(int32_t inner, int per_slot, int when, int32_t E, bool collect, bool own_geom)
{
    return when == MW_WF_ALWAYS || (when == MW_WF_COLLECT ? collect : own_geom) ? inner * (per_slot ? E : 1) : 0;
}
