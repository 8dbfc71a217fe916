// Frame records (mw_snapshot_save_frames / mw_snapshot_load_frames): where everything lies in the caller's second buffer, the companion
// of the state records (mw_snapshot.h).  Shared by the host runtime (mw_engine_snapshot.hip), the copy kernels (mw_snapframes.hip) and the CPU
// check of the layout (tests/hostcheck/snapframes_layout.cpp).
//
// A buffer for `capacity` records is a 64-byte header and then up to four sections.  Unlike the state records they are RECORD-major: a
// frame is contiguous in d_obs and stays contiguous here, record after record, so that a workgroup moves a run of 16-byte units.
//   header     the layout key (MwSnapfKey): format number, W, H, obs layout, bytes of a frame, flags, stack depth, capacity.  A load
//              compares all of it.
//   obs        [capacity][frame bytes]                 the env's row of d_obs, in the layout of mw_set_obs_layout
//   depth      [capacity][W H 4]                       MW_SNAPF_DEPTH: its row of d_depth
//   stack      [capacity][K][frame bytes]              MW_SNAPF_STACK: its K stacked frames in WINDOW order, oldest first — not the
//                                                      2K - 1 slots of the ring, so a record does not depend on the ring phase
//   stack flag [capacity] bytes                        MW_SNAPF_STACK: the env's MW_STACK_FRESH / MW_STACK_PENDING byte
// Every section is padded to whole 16-byte units, so every section starts 16-byte aligned whatever capacity and the frame size are;
// a record inside a section is 16-byte aligned when the bytes of one are a multiple of 16 (80 x 60 x 3, every grey frame; not
// 81 x 61 x 3), which is when the copy kernels move 16-byte units.
#pragma once
#include <stdint.h>

#include "mw_hd.h"

#define MW_SNAPF_MAGIC 0x46504E53u      // "SNPF"
#define MW_SNAPF_FORMAT 1u
#define MW_SNAPF_HEADER_BYTES 64
#define MW_SNAPF_KEY_WORDS 12
#define MW_SNAPF_THREADS 256
#define MW_SNAPF_UNROLL 4               // units per lane and chunk
#define MW_SNAPF_FLAG_DEPTH 1           // MW_SNAPF_DEPTH, MW_SNAPF_STACK of include/mwengine.h
#define MW_SNAPF_FLAG_STACK 2

struct MwSnapfKey { uint32_t w[MW_SNAPF_KEY_WORDS]; };

// what of an engine's frame configuration shapes a record.  stack_depth counts with MW_SNAPF_FLAG_STACK alone.
struct MwSnapfConfig {
    int32_t W, H, layout, flags, stack_depth;
    uint64_t frame_bytes;       // of one env's row of d_obs in `layout`
};

enum { MW_SF_OBS = 0, MW_SF_DEPTH, MW_SF_STACK, MW_SF_STACK_FLAG, MW_SF_COUNT };

struct MwSnapfLayout {
    uint64_t rec_bytes[MW_SF_COUNT];    // of one record's part of a section, 0 = the section is absent
    uint64_t off[MW_SF_COUNT];          // where the section starts
    uint64_t bytes[MW_SF_COUNT];        // of the section, whole 16-byte units
    uint64_t total;                     // of the buffer
};

MW_HD uint64_t mw_snapf_round16(uint64_t b) { return (b + 15u) & ~(uint64_t)15u; }

MW_HD MwSnapfLayout mw_snapf_layout(const MwSnapfConfig &c, int64_t capacity)
{
    MwSnapfLayout L{};
    const bool depth = (c.flags & MW_SNAPF_FLAG_DEPTH) != 0, stack = (c.flags & MW_SNAPF_FLAG_STACK) != 0;
    L.rec_bytes[MW_SF_OBS] = c.frame_bytes;
    L.rec_bytes[MW_SF_DEPTH] = depth ? (uint64_t)c.W * (uint64_t)c.H * 4u : 0;
    L.rec_bytes[MW_SF_STACK] = stack ? (uint64_t)c.stack_depth * c.frame_bytes : 0;
    L.rec_bytes[MW_SF_STACK_FLAG] = stack ? 1 : 0;
    uint64_t at = MW_SNAPF_HEADER_BYTES;
    for (int s = 0; s < MW_SF_COUNT; ++s) {
        L.off[s] = at;
        L.bytes[s] = mw_snapf_round16(L.rec_bytes[s] * (uint64_t)capacity);
        at += L.bytes[s];
    }
    L.total = at;
    return L;
}

MW_HD MwSnapfKey mw_snapf_key(const MwSnapfConfig &c, int32_t capacity)
{
    MwSnapfKey k{};
    k.w[0] = MW_SNAPF_MAGIC; k.w[1] = MW_SNAPF_FORMAT;
    k.w[2] = (uint32_t)c.W; k.w[3] = (uint32_t)c.H; k.w[4] = (uint32_t)c.layout;
    k.w[5] = (uint32_t)c.frame_bytes; k.w[6] = (uint32_t)(c.frame_bytes >> 32);
    k.w[7] = (uint32_t)c.flags; k.w[8] = (c.flags & MW_SNAPF_FLAG_STACK) ? (uint32_t)c.stack_depth : 0u;
    k.w[9] = (uint32_t)capacity;
    return k;
}

// What a copy kernel gets by value: the key, the sections, and how its 1-D grid is cut.  A workgroup is (item, chunk of the record);
// the chunks of an item are those of its obs row, then of its depth row, then of its K window frames, MW_SNAPF_THREADS *
// MW_SNAPF_UNROLL units each (a unit: 16 bytes when `wide`, else one byte).
struct MwSnapfArgs {
    MwSnapfKey key;
    uint64_t off[MW_SF_COUNT];
    uint64_t frame_bytes, depth_bytes;      // depth_bytes: 0 without MW_SNAPF_DEPTH
    int32_t N, count, n_recs;               // envs of the engine, items of the call, valid records (a save: the capacity)
    int32_t stack_depth, first_slot;        // K (0 without MW_SNAPF_STACK) and where the window starts (mw_stack_window)
    int32_t wide;
    int32_t frame_chunks, depth_chunks, chunks_per_item;
};
