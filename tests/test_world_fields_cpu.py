"""The table of a world's per-env arrays (miniworld_amd/csrc/mw_world_fields.h), without a GPU: the snapshot record layout derived from
it is, byte for byte, the one recorded from the hand-written lists it replaced (tests/golden/snapshot_layout.json), and the rows that
mw_state_view exposes agree with the struct in include/mwengine.h and with the Python binding's mirrors of it (engine.MwStateView,
engine.STATE_FIELDS), which stay hand-written because ctypes mirrors the public header."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np

from test_snapshot_cpu import CONFIGS, layout_lib, sections

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "miniworld_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "snapshot_layout.json")
CAPACITIES = [0, 1, 3, 70, 1023, 4096]


def layout_dump(lib, configs=CONFIGS, sections=sections):
    """everything the layout says about every configuration: per capacity the sections (id, offset, bytes, alignment), the buffer's
    bytes and the key's words; per configuration the rows of a record"""
    out = {}
    for name in sorted(configs):
        cfg = configs[name]
        per = {"total_rows": int(lib.mwsnap_total_rows(cfg.ctypes.data)), "capacities": {}}
        for capacity in CAPACITIES:
            off, size, align, ident = sections(lib, cfg, capacity)
            key = np.zeros(12, np.uint32)
            lib.mwsnap_key(cfg.ctypes.data, capacity, key.ctypes.data)
            per["capacities"][str(capacity)] = {
                "sections": [[int(i), int(o), int(s), int(a)] for i, o, s, a in zip(ident, off, size, align)],
                "bytes": int(lib.mwsnap_bytes(cfg.ctypes.data, capacity)),
                "key": [int(w) for w in key],
            }
        out[name] = per
    return out


def test_the_record_layout_is_the_recorded_one():
    """MW_SNAP_FORMAT 1: every section's id, offset, size and alignment, the buffer sizes, the row counts and the keys of every
    configuration and capacity of tests/test_snapshot_cpu.py, as the hand-written MW_SC_* enum and mw_snap_shape gave them."""
    want = json.load(open(GOLDEN))
    got = layout_dump(layout_lib())
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name]["total_rows"] == want[name]["total_rows"], name
        for capacity in map(str, CAPACITIES):
            assert got[name]["capacities"][capacity] == want[name]["capacities"][capacity], (name, capacity)
    assert got == want


def view_rows():
    """the fields of mw_state_view as the table has them: name -> (element bytes, is float, components, per entity slot), in the
    table's order (tests/hostcheck/world_fields.cpp)"""
    src, lib = os.path.join(HERE, "hostcheck", "world_fields.cpp"), os.path.join(HERE, "hostcheck", "libmwworldfields.so")
    deps = [src, os.path.join(ROOT, "include", "mwengine.h")] + [os.path.join(CSRC, h) for h in ("mw_world_fields.h", "mw_state_view.h", "mw_hd.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-Wall", "-Werror", "-shared", src, "-o", lib])
    L = C.CDLL(lib)
    name = (C.c_char_p * 32)()
    elem, is_float, inner, per_slot = ((C.c_int * 32)() for _ in range(4))
    n = L.mwwf_view_rows(name, elem, is_float, inner, per_slot, 32)
    assert 0 < n < 32
    return {name[i].decode(): (elem[i], bool(is_float[i]), inner[i], bool(per_slot[i])) for i in range(n)}


def test_the_python_mirrors_agree_with_the_table_and_the_header():
    from miniworld_amd import engine
    rows = view_rows()
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    struct = header[header.index("typedef struct {\n    double *agent_pos;"):header.index("} mw_state_view;")]
    members = re.findall(r"^\s*(double|int32_t) \*(\w+);", struct, re.M)
    assert len(members) == len(re.findall(r";", re.sub(r"/\*.*?\*/", "", struct, flags=re.S)))     # every member was understood
    # the binding's struct is the header's, member for member and in its order; the table has the same fields, no more and no fewer
    assert [n for n, _ in engine.MwStateView._fields_] == [n for _, n in members] == list(engine.STATE_FIELDS)
    assert all(t is C.c_void_p for _, t in engine.MwStateView._fields_)
    assert sorted(rows) == sorted(n for _, n in members)
    E = 7
    for ctype, name in members:
        elem, is_float, inner, per_slot = rows[name]
        dt, shape = engine.STATE_FIELDS[name]
        dt = np.dtype(dt)
        # element type: the header's, the table's and the binding's
        assert (ctype == "double") == is_float == (dt.kind == "f"), name
        assert elem == dt.itemsize == {"double": 8, "int32_t": 4}[ctype], name
        # per-env shape: [E] for a per-slot field, [inner] where a field has more than one component
        assert tuple(shape(E)) == ((E,) if per_slot else ()) + ((inner,) if inner > 1 else ()), name
    # a rollout trace's fields are rows of state views (mw_plan_trace): the same types and component counts; ent_pos is ONE slot's
    for name, (dt, shape) in engine.TRACE_FIELDS.items():
        elem, is_float, inner, _ = rows[name]
        assert np.dtype(dt).itemsize == elem and (np.dtype(dt).kind == "f") == is_float and tuple(shape) == ((inner,) if inner > 1 else ()), name
