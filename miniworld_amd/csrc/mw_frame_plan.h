// The frame plan (mw_frame_plan_kernel, mw_kernels.h): what becomes of one env's frame in a plain whole-batch step through the quad
// kernel — left alone, copied from a slot of the frame cache, or drawn — and the block in device memory that carries the verdicts of
// a batch to the quad kernel.  The decision is MW_HD: the plan kernel runs it per lane, tests/hostcheck/frame_plan.cpp on the host.
#pragma once
#include <stdint.h>

#include "mw_hd.h"

// (as mw_device.h, which the host tests do not include)
#ifndef MW_FC_KEY_WORDS
#define MW_FC_KEY_WORDS 10
#define MW_FC_META_WORDS(slots) (2 + MW_FC_KEY_WORDS * (slots))
#define MW_FC_MAX_SLOTS 8
#endif

// The source byte of an env's frame (mw_get_frame_source): drawn, left alone as clean, copied from slot j
#define MW_SRC_DRAWN 0
#define MW_SRC_CLEAN 1
#define MW_SRC_SLOT(j) (2 + (j))

// The plan block, uint32 words.  The head, its counters a 128-byte line apart (the wavefronts' atomics on one line queue up behind
// each other): [0] draw entries, [1] copy entries, [2] MW_PLAN_CLASSES where the draw entries are filed by cost class (an ordered
// plan), 0 where they are one list; [32..33] the entries of cost classes 0..3 and [64..65] of classes 4..7, 16 bits each, the lowest
// class in the lowest bits (ordered plans only).  Behind the head N copy entries env | slot << 24, then the draw entries env | victim
// slot << 24 (the low 24 bits hold the env: plans are made for batches below 2^24 envs, mw_policy.h) — one list of N, or in an
// ordered plan a segment of N per cost class, class c's at MW_PLAN_DRAW(N, c).  Workgroup b of the quad kernel takes the entry
// mw_plan_slot names: the draw entries from the highest class down, dense, then the copies — the frames that take longest start
// first, so the launch does not end on them (profiles/r22).  The order of the entries inside a list or a segment is whatever the
// wavefronts' atomics made it; no result depends on any of it.  The engine keeps two blocks and alternates: the plan kernel of one
// frame zeroes the counters of the other block, which the frame before it has finished reading.
#define MW_PLAN_HEAD 96
#define MW_PLAN_CLS_LO 32
#define MW_PLAN_CLS_HI 64
#define MW_PLAN_CLASSES 8
#define MW_PLAN_COPY(N) ((size_t)MW_PLAN_HEAD)
#define MW_PLAN_DRAW(N, c) (MW_PLAN_HEAD + (size_t)(N) * (1u + (size_t)(c)))
#define MW_PLAN_WORDS(N, ordered) (MW_PLAN_HEAD + (size_t)(N) * ((ordered) ? 1u + MW_PLAN_CLASSES : 2u))
#define MW_PLAN_ENV_BITS 24
#define MW_PLAN_ENV_MASK 0xFFFFFFu
// an ordered plan counts a class in 16 bits, and a class may hold every env (mw_policy.h: frame_plan_ordered)
#define MW_PLAN_ORDERED_MAX_N 0xFFFF

// The cost class of a drawn env, from the length of its display list (MwArgs::nvis, which the geometry kernel has written by the time
// the plan kernel runs): monotone, 0 .. MW_PLAN_CLASSES - 1, the highest the most expensive.  Of the deterministic predictors measured
// against the drawing workgroups' residencies — this one, a weighted sum of the quad classes of the env's last drawn frame, both — the
// list length ranked best (Spearman 0.82 in Hallway x 4096, 0.60 in OneRoom with depth) and eight classes of four records lose nothing
// against the unquantised order in the list-scheduling simulation (profiles/r22, tools/perf/plan_order_sim.py).
MW_HD uint32_t mw_plan_cost_class(int32_t nvis)
{
    if (nvis <= 0) return 0u;
    const uint32_t c = (uint32_t)nvis >> 2;
    return c < MW_PLAN_CLASSES - 1u ? c : MW_PLAN_CLASSES - 1u;
}

// the count of class c in the head's two 64-bit words (lo: classes 0..3, hi: 4..7)
MW_HD uint32_t mw_plan_class_count(uint64_t lo, uint64_t hi, uint32_t c)
{
    return (uint32_t)((c < 4u ? lo : hi) >> (16u * (c & 3u))) & 0xFFFFu;
}

// The slot lookup of an ordered plan: what workgroup b of the quad kernel's launch takes, from the MW_PLAN_CLASSES class counts.  The
// draw entries go to workgroups 0 .. n_draw - 1 (n_draw: the sum of the counts) in non-increasing class order: true, with the class
// and the entry's rank inside the class's segment.  Past them: false, and *rank is b - n_draw, the index into the copy list.
MW_HD bool mw_plan_slot(uint32_t b, const uint32_t *count, uint32_t *cls, uint32_t *rank)
{
    uint32_t first = 0u;
    for (int c = MW_PLAN_CLASSES - 1; c >= 0; --c) {
        if (b - first < count[c]) { *cls = (uint32_t)c; *rank = b - first; return true; }       // (b >= first here)
        first += count[c];
    }
    *cls = 0u; *rank = b - first;
    return false;
}

// One env's verdict.  clean: K1's frame_clean byte, counted only where the caller's buffers hold the last frame (reuse: MW_RASTER_REUSE).
// match: bit j set = the key of the cache's slot j equals the key K1 stored for this frame in every word (0 without a cache); header:
// word 0 of the env's row of the key table, the slot the next drawn frame replaces.  Clean wins; else the lowest-numbered matching
// slot; else the frame is drawn into min(header, slots - 1) (0 without a cache).  Returns the source byte | that slot << 8.
MW_HD uint32_t mw_frame_verdict(bool clean, bool reuse, uint32_t match, uint32_t header, int slots)
{
    if (reuse && clean) return MW_SRC_CLEAN;
    if (slots <= 0) return MW_SRC_DRAWN;
    match &= (1u << slots) - 1u;
    if (match) {
        uint32_t hit = 0;
        while (!((match >> hit) & 1u)) ++hit;
        return (uint32_t)MW_SRC_SLOT(hit) | hit << 8;
    }
    const uint32_t last = (uint32_t)(slots - 1);
    return MW_SRC_DRAWN | (header < last ? header : last) << 8;
}

// two keys of MW_FC_KEY_WORDS words
MW_HD bool mw_fc_key_equal(const uint64_t *a, const uint64_t *b)
{
    bool eq = true;
    for (int w = 0; w < MW_FC_KEY_WORDS; ++w) eq &= a[w] == b[w];
    return eq;
}

// ... and the verdict from the tables themselves.  key: the env's MW_FC_KEY_WORDS words; meta: the env's row of the cache's key table —
// the header, then the slots' keys — or null without a cache.  (The plan kernel loads every slot's key before it compares any and
// calls the two functions above; this is the same decision with the loads in program order.)
MW_HD uint32_t mw_frame_verdict_of(bool clean, bool reuse, const uint64_t *key, const uint64_t *meta, int slots)
{
    if (!meta) return mw_frame_verdict(clean, reuse, 0u, 0u, 0);
    uint32_t match = 0u;
    for (int j = 0; j < slots; ++j) match |= mw_fc_key_equal(meta + 2 + MW_FC_KEY_WORDS * j, key) ? 1u << j : 0u;
    return mw_frame_verdict(clean, reuse, match, (uint32_t)meta[0], slots);
}
