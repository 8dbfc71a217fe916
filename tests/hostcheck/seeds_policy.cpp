// The seeded auto-reset's decisions of the launch policy (miniworld_amd/csrc/mw_policy.h) compiled for the host: tests/test_seeds_cpu.py
// asks for the passes of a step call, for the frame policy of those passes, and for what mw_reset_where invalidates.
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace mwpolicy;

// what: the question; in / out: its integers.  Returns the number of answers, -1 for an unknown question.
extern "C" int mwpol(int what, const long long *in, long long *out)
{
    const auto I = [&](int k) { return (int)in[k]; };
    const auto B = [&](int k) { return in[k] != 0; };
    switch (what) {
    case 0: {   // seeds set, final buffers set, frameless
        const StepPasses p = step_passes_of(B(0), B(1), B(2));
        out[0] = p.shape; out[1] = p.final_copy; out[2] = p.seeded_install;
        return 3;
    }
    case 1: {   // kind, view_flags, frame_reuse, held_match, meshes, dbg_flags, layout, task, cache_allocated, path, seeded
        FrameFacts f{(CallKind)I(0), I(1), B(2), B(3), B(4), I(5), I(6), I(7), B(8), I(9)};
        f.seeded = B(10);
        const FramePolicy p = frame_policy(f);
        out[0] = p.reuse; out[1] = p.source; out[2] = p.cache; out[3] = p.hold;
        return 4;
    }
    case 2: {
        const LoadInvalidation v = reset_where_invalidation();
        out[0] = v.held; out[1] = v.cache;
        return 2;
    }
    }
    return -1;
}
