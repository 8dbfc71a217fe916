"""The launch policy (miniworld_amd/csrc/mw_policy.h), without a GPU: compiled for the host from tests/hostcheck/policy.cpp and compared,
case by case, with tests/golden/launch_policy_table.json.gz — the answers of the host runtime's own functions as they stood before the policy
was split out of it (recorded once from that text; never produced by the code under test), amended by one written rule where the policy
has since moved a size on purpose (`amended`: 128 x 96).  The raster path also has to agree with
tests/test_gpu_obs_sizes.py::expected_path on that file's sizes."""
import ctypes as C
import gzip
import itertools
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck", "policy.cpp")
LIB = os.path.join(HERE, "hostcheck", "libmwpolicy.so")
TABLE = os.path.join(HERE, "golden", "launch_policy_table.json.gz")

RASTER_PATH, LANES, FRAME_POLICY, STACK_PHASE, STACK_GRID, SNAPSHOT_GRID, SNAPF_GRID, TILE_LAUNCH, RESET_MODE, FLAGS_ROWS, SIZES = range(11)
HWC, CWH, GREY = 0, 1, 2
TASK_GOTO, TASK_PICKUP, TASK_COLLECT = 1, 2, 6
GRID_SIZES = [(80, 60), (64, 64), (128, 96), (128, 128), (160, 120), (84, 84), (81, 61), (100, 75), (17, 5), (1, 1)]
OBS_SIZES = [(84, 84), (81, 62), (81, 61), (100, 75), (17, 5), (1, 1), (130, 97)]       # tests/test_gpu_obs_sizes.py
# (max_polys, max_ents, max_visible, task) as MiniWorldVecEnv configures them
SCENES = {"hallway": (6, 1, 16, TASK_GOTO), "pickupobjects": (6, 5, 48, TASK_PICKUP), "maze": (510, 1, 528, TASK_GOTO)}


def policy_lib(src=SRC, lib=LIB):
    """tests/hostcheck/libmwpolicy.so, (re)built when a source is newer"""
    csrc = os.path.join(ROOT, "miniworld_amd", "csrc")
    deps = [src] + [os.path.join(csrc, h) for h in ("mw_policy.h", "mw_shape.h", "mw_snapshot.h", "mw_world_fields.h", "mw_snapframes.h")] + [os.path.join(ROOT, "include", "mwengine.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-Wall", "-shared", src, "-o", lib])
    L = C.CDLL(lib)
    L.mwpol.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    return L


def ask(lib, what, args):
    a = (C.c_longlong * 16)(*args)
    out = (C.c_longlong * 8)()
    n = lib.mwpol(what, a, out)
    assert n > 0, (what, args)
    return list(out[:n])


def lds_key(msaa, w, h):
    return "%d,%d,%d" % (4 if msaa == 4 else 8, w, h)


def cases(lds):
    """name -> (question, [argument lists]); `lds`: the quad kernel's LDS bytes per "samples,W,H" (an input: mw_rasterq_lds_bytes)"""
    t = {}
    t["raster_path"] = (RASTER_PATH, [[msaa, w, h, meshes, order, k2q, generic, layout, 0, depth, lds[lds_key(msaa, w, h)]]
                                      for (w, h), msaa, meshes, order, k2q, generic, layout, depth in
                                      itertools.product(GRID_SIZES, (8, 4, 1), (0, 1), (0, 1), (1, 0), (0, 1), (HWC, CWH), (0, 1))])
    t["raster_path_debug_flags"] = (RASTER_PATH, [[msaa, w, h, meshes, 0, 1, 0, HWC, 1, 0, lds[lds_key(msaa, w, h)]]
                                                  for (w, h), msaa, meshes in itertools.product(GRID_SIZES, (8, 4, 1), (0, 1))])
    t["raster_path_obs_sizes"] = (RASTER_PATH, [[msaa, w, h, meshes, order, 1, 0, HWC, 0, 0, lds[lds_key(msaa, w, h)]]
                                                for (w, h), msaa, meshes, order in itertools.product(OBS_SIZES, (8, 4, 1), (0, 1), (0, 1))])
    t["lanes"] = (LANES, [[p, e, v, task, n, 75] for (p, e, v, task), n in itertools.product(SCENES.values(), (16, 2048, 4096))] +
                  [[p, e, 16 * -(-(p + 6 * e) // 16), task, 1024, tiles] for p, e, task, tiles in
                   itertools.product((1, 6, 20, 26, 27, 64, 65), (0, 1, 2, 4, 5, 10), (TASK_GOTO, TASK_COLLECT), (1, 6, 75, 192))])
    t["frame_policy"] = (FRAME_POLICY, [list(c) for c in itertools.product(range(4), (0, 1, 3), (0, 1), (0, 1), (0, 1), (0, 1), (HWC, CWH, GREY),
                                                                            (TASK_GOTO, TASK_COLLECT), (0, 1), range(4))])
    t["stack_phase"] = (STACK_PHASE, [[d, p] for d in (2, 3, 4) for p in range(10)])
    base, hwc = 0x7F0000000000, 80 * 60 * 3
    t["stack_grid"] = (STACK_GRID, [[base + a, 2 * base + b, c and 3 * base + c - 1, d and 4 * base + d - 1, nbytes]
                                    for a, b, c, d, nbytes in itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1, 2), (hwc, hwc + 1, 84 * 84 * 3, 1 * 1 * 3, 80 * 60 * 8))])
    t["snapshot_grid"] = (SNAPSHOT_GRID, [[count, rows, chunks] for count, (rows, chunks) in
                                          itertools.product((0, 1, 255, 256, 257, 4096, 1 << 20, (1 << 31) - 256), ((37, 0), (64, 2), (120, 17)))])
    t["snapf_grid"] = (SNAPF_GRID, [[base + a, fb, db, k, count] for a, (fb, db), k, count in
                                    itertools.product((0, 1, 16), ((hwc, 0), (hwc, 80 * 60 * 4), (hwc + 1, 0), (84 * 84 * 3, 84 * 84 * 4), (3, 4)), (0, 2, 4),
                                                      (0, 1, 8, 4096, (1 << 31) - 1))])
    t["tile_launch"] = (TILE_LAUNCH, [list(c) + [16384] for c in itertools.product((0, 1, 2), (0, 1), (0, 1), (16, 96, 3168), (75, 192), (5, 15, 25), (1, 16, 4096))])
    t["reset_mode"] = (RESET_MODE, [[g, a] for g in range(6) for a in range(3)])
    t["flags_rows"] = (FLAGS_ROWS, [[dbg, layout, part, stamp, reuse, w, h] for dbg, layout, part, stamp, reuse, (w, h) in
                                    itertools.product((0, 1, 0xFFFF), (HWC, CWH, GREY), range(4), (0, 1, 0x7FFF), (0, 1), ((80, 60), (84, 84)))])
    t["sizes"] = (SIZES, [[w, h] for w, h in GRID_SIZES + OBS_SIZES + [(0, 60), (80, 0), (4080, 1020), (4081, 60), (80, 1021), (128, 100), (144, 64)]])
    return t


PATH_TILE, PATH_GENERIC = 0, 3


def amended(name, args, answer):
    """The recorded answer as the policy states it since it asks for the edge coefficients' range (mw_policy.h, edge_coeffs_fit): a frame
    128 pixels wide or high can hold a coefficient one past the 24 bits the tile and quad kernels multiply (tests/test_edge_limits_cpu.py),
    so it takes the generic-resolution kernels.  Of the table's sizes that moves 128 x 96 alone — the runtime gave it the tile kernels at 8
    samples, with the mesh chain where meshes are resident —, by this rule, written here and not taken from the code under test:
    [path, mesh, ...] becomes [generic, no mesh chain, ...] and of the size's facts [exact, on grid, tile path, accepted] the first and
    third become false.  Every other entry stays as recorded."""
    if name.startswith("raster_path") and (args[1], args[2]) == (128, 96) and answer[0] == PATH_TILE:
        return [PATH_GENERIC, 0] + answer[2:]
    if name == "sizes" and tuple(args) == (128, 96):
        return [0, answer[1], 0, answer[3]]
    return answer


with gzip.open(TABLE, "rt") as _f:
    _TABLE = json.load(_f)
_CASES = cases(_TABLE["lds"])


def test_the_table_covers_what_it_should():
    assert set(_CASES) == set(_TABLE["answers"])
    assert len(_CASES["raster_path"][1]) == 10 * 3 * 2 ** 4 * 2 * 2
    assert len(_CASES["frame_policy"][1]) == 4 * 3 * 2 ** 4 * 3 * 2 * 2 * 4
    for name, (_, args) in _CASES.items():
        assert len(args) == len(_TABLE["answers"][name]), name


@pytest.mark.parametrize("name", sorted(_CASES))
def test_policy_answers_what_the_runtime_answered(name):
    lib = policy_lib()
    what, args = _CASES[name]
    expected = [amended(name, a, exp) for a, exp in zip(args, _TABLE["answers"][name])]
    wrong = [(a, got, exp) for a, exp in zip(args, expected) for got in [ask(lib, what, a)] if got != exp]
    assert not wrong, (name, len(wrong), wrong[:5])


def test_raster_path_agrees_with_the_gpu_size_tests():
    from test_gpu_obs_sizes import expected_path
    lib = policy_lib()
    for (w, h), msaa, meshes, order, k2q, generic in itertools.product(OBS_SIZES, (8, 4, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        path = ask(lib, RASTER_PATH, [msaa, w, h, meshes, order, k2q, generic, HWC, 0, 0, _TABLE["lds"][lds_key(msaa, w, h)]])[0]
        assert path == expected_path(w, h, msaa, bool(meshes)), (w, h, msaa, meshes, order, k2q, generic, path)
