// The table of a world's per-env arrays (miniworld_amd/csrc/mw_world_fields.h) compiled for the host: tests/test_world_fields_cpu.py
// compares the rows that mw_state_view exposes with the Python binding's mirrors of that struct.
#include <type_traits>

#include "../../miniworld_amd/csrc/mw_state_view.h"

extern "C" {

// Per field of mw_state_view — agent_pos (three arrays behind one field), then the table's VIEW rows in their order —: the field's
// name, the bytes of an element, whether it is a floating-point type, the components per env or per slot, whether it is per entity
// slot.  Returns the fields.
int mwwf_view_rows(const char **name, int *elem, int *is_float, int *inner, int *per_slot, int max)
{
    int n = 0;
    if (n < max) { name[n] = "agent_pos"; elem[n] = (int)sizeof(double); is_float[n] = 1; inner[n] = MW_SV_POS; per_slot[n] = 0; ++n; }
#define X(m, T, inner_, slot, when, spare, view, vf)                                                                                       \
    MW_WF_VIEWED_##view(if (n < max) { name[n] = #vf; elem[n] = (int)sizeof(T); is_float[n] = std::is_floating_point<T>::value; inner[n] = inner_; per_slot[n] = slot; ++n; })
    MW_WORLD_FIELDS(X)
#undef X
    return n;
}

}
