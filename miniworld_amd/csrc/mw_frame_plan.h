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

// The plan block, uint32 words: [0] draw entries, [1] copy entries, [2..3] unused, then N draw entries env | victim slot << 24 and N
// copy entries env | slot << 24 (the low 24 bits hold the env: plans are made for batches below 2^24 envs, mw_policy.h).  The order
// of the entries inside a list is whatever the wavefronts' atomics made it; no result depends on it.  The engine keeps two blocks
// and alternates: the plan kernel of one frame zeroes the counts of the other block, which the frame before it has finished reading.
#define MW_PLAN_HEAD 4
#define MW_PLAN_WORDS(N) (MW_PLAN_HEAD + 2 * (size_t)(N))
#define MW_PLAN_ENV_BITS 24
#define MW_PLAN_ENV_MASK 0xFFFFFFu

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
