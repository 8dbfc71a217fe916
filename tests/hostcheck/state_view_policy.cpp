// What mw_set_state_where invalidates on the host (miniworld_amd/csrc/mw_policy.h) compiled for the host: tests/test_state_view_cpu.py
// asks for it beside the invalidations of the calls it is modelled on.
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace mwpolicy;

// what: the question; in / out: its integers.  Returns the number of answers, -1 for an unknown question.
extern "C" int mwpol(int what, const long long *in, long long *out)
{
    (void)in;
    LoadInvalidation v{};
    switch (what) {
    case 0: v = set_state_where_invalidation(); break;
    case 1: v = reset_where_invalidation(); break;
    case 2: v = snapshot_load_invalidation(false); break;       // (the list form, which mw_set_state's world_changed equals)
    default: return -1;
    }
    out[0] = v.held; out[1] = v.cache;
    return 2;
}
