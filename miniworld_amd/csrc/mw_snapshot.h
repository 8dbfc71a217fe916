// Snapshot records (mw_snapshot_save / mw_snapshot_load): where everything lies in the caller's buffer.  Shared by the host runtime
// (mw_engine.hip, mw_engine_snapshot.hip), the copy kernels (mw_snapshot.hip) and the CPU check of the layout (tests/hostcheck/snapshot_layout.cpp).
//
// A buffer for `capacity` records is a 64-byte header and then sections, each Structure-of-Arrays over the records like the engine's
// state is over the envs, so that consecutive lanes of the copy kernels take consecutive records of one component:
//   header     the layout key (MwSnapKey): format number, E, max_polys, max_segs, shared_geometry, task, generator, rng_mode,
//              spares on / off, capacity.  A load compares all of it.
//   blobs      per-env geometry sets only: [capacity][max_polys] mw_poly and [capacity][max_segs][4] double of the live world, then
//              the same of the spare world (spare mode) — contiguous per record, moved in 16-byte units
//   8-byte components, then 4-byte ones, then 1-byte ones: per component [rows][capacity], in the order of the MW_SC_* list (mw_world_fields.h)
// Every section starts at header + capacity * (bytes of one record in front of it): sections of one element size follow each other
// and the blobs are multiples of 16 bytes, so every section is aligned to its element and the blobs to 16 bytes, whatever capacity is.
//
// A record is everything that decides the env's future and is not configuration: agent pose, cam, light, extent, carry, step,
// picked, health, final_health, final_goal, the entity slabs, rng[5], pending_remove, reset_pending; with per-env geometry sets the
// env's polys / npolys / segs / nsegs; in spare mode the env's whole spare world and its refill_mask word.
// NOT part of a record: textures, meshes, the placement program and the shared geometry set (configuration: the key guards what it
// can); the mw_set_step_params override; rendered frames and the frame-stack ring; all per-frame scratch (display lists, the
// occlusion cache, work lists, frame_clean).
#pragma once
#include <stdint.h>

#include "mw_hd.h"
#include "mw_world_fields.h"

#define MW_SNAP_MAGIC 0x50414E53u       // "SNAP"
#define MW_SNAP_FORMAT 1u
#define MW_SNAP_HEADER_BYTES 64
#define MW_SNAP_KEY_WORDS 12
#define MW_SNAP_THREADS 256
#define MW_SNAP_UNROLL 4                // 16-byte units per lane and blob chunk

struct MwSnapKey { uint32_t w[MW_SNAP_KEY_WORDS]; };

// what of an engine's configuration shapes a record
struct MwSnapConfig {
    int32_t E, max_polys, max_segs, shared_geom, task, generator, rng_mode, spares;
    int32_t health;     // the task keeps health / final_health (MW_TASK_COLLECT)
};

// the components: the rows of MW_WORLD_FIELDS (MW_SC_<member>), then the spare world's — the rows it has a copy of, in the same
// order (MW_SC_SP_<member>) — and its state word
enum {
#define X(m, T, inner, slot, when, spare, view, vf) MW_SC_##m,
    MW_WORLD_FIELDS(X)
#undef X
#define X(m, T, inner, slot, when, spare, view, vf) MW_WF_SPARE_##spare(MW_SC_SP_##m,)
    MW_WORLD_FIELDS(X)
#undef X
    MW_SC_REFILL_MASK, MW_SC_COUNT
};
enum { MW_SB_POLYS = 0, MW_SB_SEGS, MW_SB_SP_POLYS, MW_SB_SP_SEGS, MW_SB_COUNT };
#define MW_SNAP_POLY_BYTES 128          // sizeof(mw_poly)
#define MW_SNAP_SEG_BYTES 32            // double[4]

// rows ([rows][N] in the engine, [rows][capacity] in the buffer; 0: the engine has no such array) and element size of a component
MW_HD void mw_snap_shape(const MwSnapConfig &c, int id, int32_t *rows, int32_t *elem)
{
    const int32_t sp = c.spares ? 1 : 0;
    *rows = id == MW_SC_REFILL_MASK ? sp : 0; *elem = 4;
#define X(m, T, inner, slot, when, spare, view, vf)                                                                          \
    if (id == MW_SC_##m MW_WF_SPARE_##spare(|| id == MW_SC_SP_##m)) {                                                        \
        *rows = mw_wf_rows(inner, slot, MW_WF_##when, c.E, c.health != 0, !c.shared_geom) * (id == MW_SC_##m ? 1 : sp);     \
        *elem = (int32_t)sizeof(T);                                                                                          \
    }
    MW_WORLD_FIELDS(X)
#undef X
}

// Capacity-independent form of the layout: `unit` = the bytes of ONE record that lie in front of a section, so that the section of a
// buffer of `capacity` records starts at MW_SNAP_HEADER_BYTES + capacity * unit (mw_snap_offset).
struct MwSnapLayout {
    uint64_t blob_unit[MW_SB_COUNT], blob_bytes[MW_SB_COUNT];       // blob_bytes: of one record's blob, 0 = absent
    uint64_t comp_unit[MW_SC_COUNT];
    int32_t comp_rows[MW_SC_COUNT], comp_elem[MW_SC_COUNT], comp_row0[MW_SC_COUNT];     // row0: the component's first row among all rows
    int32_t total_rows, n_geo;      // n_geo: geometry sets per record (0 shared geometry, 1 live, 2 live + spare)
    uint64_t record_bytes;
};

MW_HD MwSnapLayout mw_snap_layout(const MwSnapConfig &c)
{
    MwSnapLayout L{};
    uint64_t unit = 0;
    L.n_geo = c.shared_geom ? 0 : (c.spares ? 2 : 1);
    for (int b = 0; b < MW_SB_COUNT; ++b) {
        const bool have = b / 2 < L.n_geo;
        const bool polys = b % 2 == 0;
        L.blob_bytes[b] = have ? (polys ? (uint64_t)c.max_polys * MW_SNAP_POLY_BYTES : (uint64_t)c.max_segs * MW_SNAP_SEG_BYTES) : 0;
        L.blob_unit[b] = unit;
        unit += L.blob_bytes[b];
    }
    int32_t row = 0;
    for (int id = 0; id < MW_SC_COUNT; ++id) {
        mw_snap_shape(c, id, &L.comp_rows[id], &L.comp_elem[id]);
        L.comp_row0[id] = row;
        row += L.comp_rows[id];
    }
    L.total_rows = row;
    for (int32_t size = 8; size >= 1; size = size == 8 ? 4 : size == 4 ? 1 : 0)
        for (int id = 0; id < MW_SC_COUNT; ++id)
            if (L.comp_elem[id] == size) {
                L.comp_unit[id] = unit;
                unit += (uint64_t)L.comp_rows[id] * (uint64_t)size;
            }
    L.record_bytes = unit;
    return L;
}

MW_HD uint64_t mw_snap_offset(uint64_t unit, int64_t capacity) { return MW_SNAP_HEADER_BYTES + (uint64_t)capacity * unit; }
// bytes of a buffer for `capacity` records: whole 16-byte units
MW_HD int64_t mw_snap_bytes(const MwSnapLayout &L, int64_t capacity)
{
    return (int64_t)((mw_snap_offset(L.record_bytes, capacity) + 15u) & ~(uint64_t)15u);
}

MW_HD MwSnapKey mw_snap_key(const MwSnapConfig &c, int32_t capacity)
{
    MwSnapKey k{};
    k.w[0] = MW_SNAP_MAGIC; k.w[1] = MW_SNAP_FORMAT;
    k.w[2] = (uint32_t)c.E; k.w[3] = (uint32_t)c.max_polys; k.w[4] = (uint32_t)c.max_segs; k.w[5] = (uint32_t)(c.shared_geom != 0);
    k.w[6] = (uint32_t)c.task; k.w[7] = (uint32_t)c.generator; k.w[8] = (uint32_t)c.rng_mode; k.w[9] = (uint32_t)(c.spares != 0);
    k.w[10] = (uint32_t)capacity; k.w[11] = 0u;
    return k;
}

// What the copy kernels read, in device memory (one per engine, written once by mw_create): a component's array in the engine and
// its place in a record; the geometry sets.
struct MwSnapRow {
    void *eng;              // the engine's array, [rows][N]
    uint64_t unit;          // MwSnapLayout::comp_unit
    int32_t row0, rows, elem, pad;
};
struct MwSnapTable {
    int32_t n_comps, total_rows, n_geo, poly_chunks, seg_chunks, max_polys, max_segs, pad;
    MwSnapRow comp[MW_SC_COUNT];        // the components the engine has, n_comps of them, by ascending row0
    // per geometry set (0 live, 1 spare): the engine's blobs and counts, the records' blobs and the rows of their counts
    void *eng_polys[2], *eng_segs[2];
    int32_t *eng_npolys[2], *eng_nsegs[2];
    uint64_t polys_unit[2], segs_unit[2], npolys_unit[2], nsegs_unit[2];
    uint64_t reset_pending_unit;        // the records' reset_pending bytes (a load marks the frame stack from them)
    const uint16_t *row_comp;           // [total_rows] the entry of comp[] a row belongs to: one scalar load per workgroup, no search
};
