// The dealing rule of the small-scene geometry kernel (mw_geom.hip, geom_body<BIG = false>): which env a slot of a wavefront builds.
// A group is 64 consecutive envs of a launch and the wavefronts that serve them — L of them, 64 / L slots of L lanes each; the last
// group of a batch that is no multiple of 64 has as many wavefronts as hold its envs.  Every wavefront of the group knows the group's
// 64-bit mask of the envs to build and deals from it: the envs in ascending order, one to every wavefront in turn.  So each set bit
// goes to exactly one slot, no clear bit to any, and the wavefronts' slot counts differ by at most one — the launch lasts as long as
// its slowest wavefront, and that one gets no more envs than any other.  MW_HD: the kernel runs it per lane,
// tests/hostcheck/geom_deal.cpp on the host.
#pragma once
#include <stdint.h>

#include "mw_hd.h"

// the position of the set bit of rank r in mask (rank 0: the lowest), or -1 where mask has no such bit
MW_HD int mw_deal_select(uint64_t mask, int r)
{
    if (r < 0 || r >= __builtin_popcountll((unsigned long long)mask)) return -1;
    int pos = 0;
    for (int w = 32; w > 0; w >>= 1) {
        const uint64_t lo = mask & ((1ull << w) - 1ull);
        const int c = __builtin_popcountll((unsigned long long)lo);
        if (r >= c) { r -= c; mask >>= w; pos += w; } else mask = lo;
    }
    return pos;
}

// The env (its bit in mask) that slot j of the group's wavefront i builds, or -1: an empty slot.  waves: the wavefronts that serve the
// group (L, fewer for a ragged last group); a wavefront has 64 / L slots, and the caller asks for no slot beyond them.
MW_HD int mw_geom_deal(uint64_t mask, int waves, int i, int j)
{
    if (waves <= 0 || i < 0 || i >= waves || j < 0) return -1;
    return mw_deal_select(mask, i + j * waves);
}
