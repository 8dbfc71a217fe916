// The level-set decisions of the launch policy (miniworld_amd/csrc/mw_policy.h) compiled for the host: tests/test_levels_cpu.py asks what a
// load of state or frame records invalidates in either form, and for the grids of the masked forms beside the list forms'.
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace mwpolicy;

// what: the question; in / out: its integers.  Returns the number of answers, -1 for an unknown question.
extern "C" int mwpol(int what, const long long *in, long long *out)
{
    const auto I = [&](int k) { return (int)in[k]; };
    switch (what) {
    case 0: {   // where (0 / 1): a state-record load, then a frame-record load
        const LoadInvalidation s = snapshot_load_invalidation(in[0] != 0), f = snapshot_load_frames_invalidation(in[0] != 0);
        out[0] = s.held; out[1] = s.cache; out[2] = f.held; out[3] = f.cache;
        return 4;
    }
    case 1: {   // N, total_rows, chunks_per_item: the masked grid, then the list form's for count = N
        const SnapshotGrid w = snapshot_where_grid(I(0), I(1), I(2)), l = snapshot_grid(I(0), I(1), I(2));
        out[0] = w.item_chunks; out[1] = w.blocks; out[2] = l.item_chunks; out[3] = l.blocks;
        return 4;
    }
    case 2: {   // the addresses or'ed, frame_bytes, depth_bytes, stack_depth, N
        const SnapfGrid w = snapf_where_grid((uintptr_t)in[0], (uint64_t)in[1], (uint64_t)in[2], I(3), I(4));
        const SnapfGrid l = snapf_grid((uintptr_t)in[0], (uint64_t)in[1], (uint64_t)in[2], I(3), I(4));
        out[0] = w.wide; out[1] = (long long)w.per_item; out[2] = (long long)w.blocks; out[3] = l.wide; out[4] = (long long)l.per_item; out[5] = (long long)l.blocks;
        return 6;
    }
    }
    return -1;
}
