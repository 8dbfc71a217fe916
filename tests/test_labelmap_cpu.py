"""Object maps (mw_label_project; MiniWorldVecEnv.object_window / object_update / object_map / object_map_update) without a GPU.

The phases the kernel runs (miniworld_amd/csrc/mw_labelmap.h) run on the host with (lane, stride) = (0, 1) in a program of its own
(tests/hostcheck/label_project.cpp), built with the address and undefined-behaviour sanitizers, on the label frames of
tests/label_reference.py — their codes with their own depth, and with the oracle's 16-bit depth frames of the same states — over short
walks in worlds the host classes generate; plane, map, cell counts and positions are compared, exactly, with the restatement of
tests/objectmap_reference.py.  Beside that: the semantics on synthetic frames (the last observation wins, the lowest id wins, ids from K
on), the geometry (a sensed cell lies on its object), the launch arithmetic, the ABI names, the refusals of the binding over a stub
engine and the adapter's key."""
import math
import os
import re

import numpy as np
import pytest

import label_reference as label
import objectmap_reference as ref
from helpers import golden_meshes, stub_engine
from query_checks import (CSRC, ROOT, build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, launch_of, run,
                          pose_walk, scene as _scene)
from test_depth_cpu import CAMERAS

CELL = 0.25
NORTH = 2
SENSOR = ref.SENSOR
BASE = ref.RAY_ENT
FAMILIES = ["Hallway", "OneRoom", "Sign", "PickupObjects", "CollectHealth"]
# (samples, W, H): 80 x 60 at every sample count, and a frame of 273 pixels — no multiple of 4: the scalar loads
FRAMES = [(8, 80, 60), (4, 80, 60), (1, 80, 60), (8, 21, 13)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("label_project", tmp_path_factory.mktemp("label_project"))


_labels, _frames = {}, {}


def _label(cls_name, pose, cam, msaa, W, H):
    """label_reference's frame of the world from pose (x, z, dir) under cam, mesh objects as their cylinders: (code int32[H, W], depth
    float32[H, W]); computed once, never changed"""
    key = (cls_name, pose, cam, msaa, W, H)
    if key not in _labels:
        sc = _scene(cls_name)
        out = label.label_frame(sc, W, H, msaa, mode="bounds", pose=(pose[0], float(sc["agent_pos"][1]), pose[1], pose[2]), cam=cam)
        code, depth = out["code"].copy(), out["depth"].copy()
        code.setflags(write=False)
        depth.setflags(write=False)
        _labels[key] = (code, depth)
    return _labels[key]


def _oracle_depth(cls_name, pose, cam, msaa, W, H):
    """the oracle's depth frame of the same state, through its 16-bit depth values"""
    key = (cls_name, pose, cam, msaa, W, H)
    if key not in _frames:
        import pyoracle
        sc = dict(_scene(cls_name))
        pos = np.array(sc["agent_pos"], np.float64)
        pos[0], pos[2] = pose[0], pose[1]
        sc["agent_pos"], sc["agent_dir"] = pos, pose[2]
        sc["cam_height"], sc["cam_fwd_disp"], sc["cam_pitch"], sc["cam_fov_y"] = cam
        depth = pyoracle.render(sc, W, H, msaa, meshes=golden_meshes(sc))["depth"].reshape(H, W).copy()
        depth.setflags(write=False)
        _frames[key] = depth
    return _frames[key]


def _poses(cls_name, steps):
    """poses (x, z, dir) of a short walk — turns of 15 degrees and forward moves, kept well inside the extent — that starts 2.5 m from
    slot 0, facing it: the world's own first pose need not show any object"""
    sc = _scene(cls_name)
    return pose_walk([float(v) for v in sc["extent"]], facing(sc, 0, 2.5), np.random.default_rng(3600), steps, 15, 0.15, 0.5)


def facing(sc, slot, distance=1.5):
    """a pose (x, z, dir) `distance` metres from the slot, facing it, inside the extent: the first of eight directions that is at least
    half a metre inside"""
    ex, ez = float(sc["ents_pos"][slot][0]), float(sc["ents_pos"][slot][2])
    x0, x1, z0, z1 = (float(v) for v in sc["extent"])
    for k in range(8):
        d = k * math.pi / 4
        x, z = ex - distance * math.cos(d), ez + distance * math.sin(d)
        if x0 + 0.5 <= x <= x1 - 0.5 and z0 + 0.5 <= z <= z1 - 0.5:
            return (x, z, d)
    raise AssertionError("no place to stand")


def _bits(depth):
    return " ".join(f"{v:x}" for v in np.ascontiguousarray(depth, np.float32).ravel().view(np.uint32).tolist())


def _run(program, tmp_path, msaa, W, H, target, extent, steps, base=BASE, sensor=SENSOR, garbage=0):
    """target: dict(size, cell, back, north) or dict(cell, gx, gz, ids); steps: (pose, cam, mask, clear, depth[H, W], code[H, W]) -> per
    step the host build's uint8[S, S], or (uint8[gz, gx], cells int32[K], pos float64[K, 3])"""
    to_map = "gx" in target
    lines = [f"{W} {H} {msaa}", " ".join(repr(float(sensor[k])) for k in ("min_range", "max_range", "floor_tol", "top")), str(int(base))]
    if to_map:
        lines.append(f"1 {float(target['cell'])!r} {target['gx']} {target['gz']} {target['ids']}")
        shape = (target["gz"], target["gx"])
    else:
        lines.append(f"0 {target['size']} {float(target['cell'])!r} {float(target['back'])!r} {NORTH if target['north'] else 0}")
        shape = (target["size"], target["size"])
    lines += [str(garbage), " ".join(repr(float(v)) for v in extent), str(len(steps))]
    for pose, cam, mask, clear, depth, code in steps:
        lines.append(" ".join(repr(float(v)) for v in tuple(pose) + tuple(cam)) + f" {int(mask)} {int(clear)}")
        lines.append(_bits(depth))
        lines.append(" ".join(str(int(v)) for v in np.asarray(code).ravel().tolist()))
    rows = run(program, tmp_path / "walk.txt", lines, blank=True)
    per = 3 if to_map else 1
    assert len(rows) == per * len(steps)
    out = []
    for k in range(len(steps)):
        cells = np.array(rows[per * k].split(), np.uint8).reshape(shape)
        if to_map:
            K = target["ids"]
            n = np.array(rows[per * k + 1].split(), np.int64).astype(np.int32)
            pos = np.array([int(v, 16) for v in rows[per * k + 2].split()], np.uint64).view(np.float64).reshape(K, 3)
            out.append((cells, n, pos))
        else:
            out.append(cells)
    return out


def _reference(msaa, target, extent, steps, base=BASE, sensor=SENSOR, garbage=0):
    """the same walk through the restatement; a masked-off step keeps what the buffers held"""
    out = []
    if "gx" in target:
        m = ref.Map(target["gx"], target["gz"], target["ids"], garbage)
        for pose, cam, mask, clear, depth, code in steps:
            if mask:
                ref.map_update(m, depth, code, base, pose, cam, msaa, extent, target["cell"], clear, **sensor)
            out.append((m.map.copy(), m.cells.copy(), m.pos.copy()))
        return out
    plane = np.full((target["size"], target["size"]), garbage, np.uint8)
    for pose, cam, mask, clear, depth, code in steps:
        if mask:
            plane = ref.window(depth, code, base, pose, cam, msaa, target["size"], target["cell"], target["back"], target["north"], **sensor)
        out.append(plane.copy())
    return out


def _same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(g, tuple):
            assert np.array_equal(g[0], w[0]), (what, k, "map", np.argwhere(g[0] != w[0])[:8].tolist())
            assert g[1].dtype == w[1].dtype and np.array_equal(g[1], w[1]), (what, k, "cells", g[1], w[1])
            assert ref.same_bits(g[2], w[2]), (what, k, "pos", g[2], w[2])
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, k, np.argwhere(g != w)[:8].tolist())


def _both(program, tmp_path, msaa, W, H, target, extent, steps, what, **kw):
    got, want = _run(program, tmp_path, msaa, W, H, target, extent, steps, **kw), _reference(msaa, target, extent, steps, **kw)
    _same(got, want, what)
    return want


def _window(size=33, cell=CELL, anchor="centre", north=False):
    return dict(size=size, cell=cell, back=size / 2 if anchor == "bottom" else 0.0, north=north)


def _grid(extent, cell=CELL, ids=None):
    gx = max(1, math.ceil((float(extent[1]) - float(extent[0])) / cell))
    gz = max(1, math.ceil((float(extent[3]) - float(extent[2])) / cell))
    return dict(cell=cell, gx=int(gx), gz=int(gz), ids=ids)


SHAPES = [_window(33), _window(9, anchor="bottom", north=True), _window(2, north=True), _window(1), _window(33, anchor="bottom"), _window(128, cell=0.1)]


@pytest.mark.parametrize("cls_name", FAMILIES)
def test_walk_equals_the_restatement(program, tmp_path, cls_name):
    sc = _scene(cls_name)
    extent = [float(v) for v in sc["extent"]]
    E = len(sc["ents_kind"])
    poses = _poses(cls_name, 4)
    object_cells = counted = 0
    for f, (msaa, W, H) in enumerate(FRAMES):
        for source in (_label, _oracle_depth):
            # a camera per step, another start per frame format; the first step clears the map's garbage, the third is masked off, the last clears again
            steps = []
            for k, p in enumerate(poses):
                cam = CAMERAS[(f + k) % len(CAMERAS)]
                code, depth = _label(cls_name, p, cam, msaa, W, H)
                if source is _oracle_depth:
                    depth = _oracle_depth(cls_name, p, cam, msaa, W, H)
                steps.append((p, cam, 0 if k == 2 else 1, 1 if k in (0, 3) else 0, depth, code))
            sensor = dict(SENSOR, max_range=3.0) if f % 2 else SENSOR
            for target in [SHAPES[(2 * f + j) % len(SHAPES)] for j in range(2)] + [_grid(extent, ids=E), _grid(extent, 0.5, ids=max(E - 1, 0))]:
                want = _both(program, tmp_path, msaa, W, H, target, extent, steps, (cls_name, msaa, W, H, source.__name__, target), sensor=sensor, garbage=0xAB)
                if "gx" in target:
                    assert np.array_equal(want[1][0], want[2][0]) and np.array_equal(want[1][1], want[2][1]) and ref.same_bits(want[1][2], want[2][2])
                    counted += sum(int(w[1].sum()) for w in (want[0], want[1], want[3]))
                else:
                    object_cells += sum(int((w != 0).sum()) for w in want)
    # what makes the comparison above worth something, asserted on the restatement alone
    assert object_cells > 0 and counted > 0, (cls_name, object_cells, counted)


# ---------------------------------------------------------------------------------------------------------------- the semantics

W0, H0 = 80, 60
POSE, CAM = (2.0, 0.1, 0.3), CAMERAS[0]
EXTENT = [-1.0, 13.0, -3.0, 3.0]
WALL = 5            # a code below BASE: a static polygon, no object


def _flat(value):
    return np.full((H0, W0), value, np.float32)


def _codes(fill, **regions):
    """a label image of `fill` with BASE + id in columns lo .. hi - 1: _codes(WALL, id3=(30, 50))"""
    code = np.full((H0, W0), fill, np.int32)
    for name, (lo, hi) in regions.items():
        code[:, lo:hi] = BASE + int(name[2:])
    return code


def test_the_last_observation_wins(program, tmp_path):
    depth = _flat(2.0)
    back = (POSE[0], POSE[1], POSE[2] + math.pi)
    a, b = _codes(WALL, id3=(30, 50)), _codes(WALL)
    grid = _grid(EXTENT, ids=5)
    # A puts id 3 into some cells; C, looking the other way, leaves them; B, from A's pose, sees them as non-object; A again; clear with C
    steps = [(POSE, CAM, 1, 1, depth, a), (back, CAM, 1, 0, depth, b), (POSE, CAM, 1, 0, depth, b), (POSE, CAM, 1, 0, depth, a), (back, CAM, 1, 1, depth, b)]
    want = _both(program, tmp_path, 8, W0, H0, grid, EXTENT, steps, "A C B A clear", garbage=0xAB)
    (ma, na, pa), (mc, nc, pc), (mb, nb, pb), (ma2, na2, _), (mz, nz, pz) = want
    held = ma == 4
    assert held.sum() >= 2 and na.tolist() == [0, 0, 0, int(held.sum()), 0] and set(np.unique(ma).tolist()) == {0, 4}
    assert np.isnan(pa[[0, 1, 2, 4]]).all() and not np.isnan(pa[3]).any() and pa[3, 1] == 0.0
    jj, ii = np.nonzero(held)
    assert pa[3, 0] == EXTENT[0] + (ii.sum() / len(ii) + 0.5) * CELL and pa[3, 2] == EXTENT[2] + (jj.sum() / len(jj) + 0.5) * CELL
    assert np.array_equal(mc, ma) and np.array_equal(nc, na) and ref.same_bits(pc, pa)           # C saw elsewhere: the bytes stay
    assert not mb[held].any() and not mb.any() and not nb.any() and np.isnan(pb).all()              # B saw the same cells empty
    assert np.array_equal(ma2, ma) and np.array_equal(na2, na)
    assert not mz.any() and not nz.any() and np.isnan(pz).all()                                    # clear rewrites everything
    # uncleared, garbage survives where the frame does not look, and is counted as what it reads: 0xAB = 1 + 170
    wild = _both(program, tmp_path, 8, W0, H0, _grid(EXTENT, ids=255), EXTENT, [(POSE, CAM, 1, 0, depth, a)], "garbage", garbage=0xAB)[0]
    assert wild[1][170] == (wild[0] == 0xAB).sum() > 0 and wild[1][3] == held.sum()
    # the window is written in full by every call
    for target in (_window(33), _window(33, north=True)):
        got = _both(program, tmp_path, 8, W0, H0, target, EXTENT, [(POSE, CAM, 1, 0, depth, a), (POSE, CAM, 1, 0, depth, b), (POSE, CAM, 0, 0, depth, a)],
                    target, garbage=0xAB)
        assert set(np.unique(got[0]).tolist()) == {0, 4} and not got[1].any() and not got[2].any()


def test_the_lowest_id_wins_and_invalid_codes_are_no_object(program, tmp_path):
    one = _window(1, cell=20.0)
    depth = _flat(2.0)
    invalid = [BASE + 255, BASE + 300, -1, BASE - 1]
    mixed = np.resize(np.array([BASE + 7, BASE + 2, BASE + 200, BASE + 254] + invalid, np.int32), (H0, W0))
    for base, shift in ((BASE, 0), (0, -BASE)):          # a label frame's codes, and the caller's own category image
        codes = (mixed.astype(np.int64) + shift).astype(np.int32)
        if base == 0:
            codes[mixed == -1] = -1
            codes[mixed == BASE - 1] = np.iinfo(np.int32).min          # (code - base would overflow below base: compared first)
        want = _both(program, tmp_path, 8, W0, H0, one, EXTENT, [(POSE, CAM, 1, 0, depth, codes)], ("conflict", base), base=base)
        assert want[0].tolist() == [[1 + 2]]
        for k, only in enumerate((invalid, [BASE + 254] + invalid, [BASE + 200, BASE + 254])):
            codes = (np.resize(np.array(only, np.int32), (H0, W0)).astype(np.int64) + shift).astype(np.int32)
            want = _both(program, tmp_path, 8, W0, H0, one, EXTENT, [(POSE, CAM, 1, 0, depth, codes)], ("conflict", base, k), base=base)
            assert want[0].tolist() == [[(0, 255, 201)[k]]]
    # int32's extremes as codes
    for base, code, byte in ((0, np.iinfo(np.int32).max, 0), (np.iinfo(np.int32).max, np.iinfo(np.int32).max, 1), (np.iinfo(np.int32).max, np.iinfo(np.int32).min, 0)):
        want = _both(program, tmp_path, 8, W0, H0, one, EXTENT, [(POSE, CAM, 1, 0, depth, np.full((H0, W0), code, np.int32))], ("extreme", base, code), base=base)
        assert want[0].tolist() == [[byte]]
    # an id from K on is mapped, not counted; no id: nothing to write
    a = _codes(WALL, id3=(30, 50), id1=(50, 60))
    for K, counted in ((3, [1]), (4, [1, 3]), (0, [])):
        m, n, pos = _both(program, tmp_path, 8, W0, H0, _grid(EXTENT, ids=K), EXTENT, [(POSE, CAM, 1, 1, depth, a)], ("ids", K))[0]
        assert (m == 4).any() and (m == 2).any() and len(n) == K
        assert [q for q in range(K) if n[q]] == counted and all(np.isnan(pos[q]).all() == (q not in counted) for q in range(K))


def test_depths_that_are_no_point_and_uncovered_extents(program, tmp_path):
    nan, inf = float("nan"), float("inf")
    a = _codes(WALL, id3=(0, 80))
    for target in (_window(33), _window(9, cell=0.5, north=True), _grid(EXTENT, ids=5)):
        for bad in (nan, inf, -inf, 0.0, -0.0, -3.0, 100.0, np.float32(SENSOR["min_range"]) - np.float32(1e-6), 8.000001):
            want = _both(program, tmp_path, 8, W0, H0, target, EXTENT, [(POSE, CAM, 1, 0, _flat(bad), a)], (target, bad), garbage=0x11)[0]
            if "gx" in target:
                assert (want[0] == 0x11).all() and want[1].tolist() == [0] * 5
            else:
                assert not want.any()
        for edge in (0.5, 2.0):             # exactly at the bounds a pixel counts
            sensor = dict(SENSOR, min_range=0.5, max_range=2.0, top=3.0)
            want = _both(program, tmp_path, 8, W0, H0, target, EXTENT, [(POSE, CAM, 1, 1, _flat(edge), a)], (target, edge), sensor=sensor)[0]
            assert ((want[0] if "gx" in target else want) == 4).any()
    # a NaN pose puts nothing into a map
    want = _both(program, tmp_path, 8, W0, H0, _grid(EXTENT, ids=5), EXTENT, [((nan, 0.1, 0.3), CAM, 1, 1, _flat(2.0), a)], "nan pose")[0]
    assert not want[0].any() and np.isnan(want[2]).all()
    # a grid that does not cover the extent: a zeroed map, cells 0 and NaN positions, whatever they held
    short = dict(cell=CELL, gx=3, gz=3, ids=4)
    want = _both(program, tmp_path, 8, W0, H0, short, EXTENT, [(POSE, CAM, 1, 0, _flat(2.0), a)], "uncovered", garbage=0xCD)[0]
    assert not want[0].any() and not want[1].any() and np.isnan(want[2]).all()


# ---------------------------------------------------------------------------------------------------------------- the geometry

def lies_on_its_object(cells, pos, ents_xz, ents_radius, extent, cell):
    """cells uint8[gz, gx] and pos float64[K, 3] of one env: every cell of slot s has its centre within radius_s + cell * sqrt(2) / 2 +
    1e-6 of the slot — a hit lies on the slot's box or cylinder, a cell's centre within half its diagonal of its point —, and so has the
    slot's sensed position.  Returns the cells per slot."""
    bound = cell * math.sqrt(2) / 2 + 1e-6
    out = {}
    for s in sorted(set(np.unique(cells).tolist()) - {0}):
        s -= 1
        jj, ii = np.nonzero(cells == s + 1)
        cx, cz = extent[0] + (ii + 0.5) * cell, extent[2] + (jj + 0.5) * cell
        far = np.hypot(cx - ents_xz[s][0], cz - ents_xz[s][1])
        assert (far <= ents_radius[s] + bound).all(), (s, float(far.max()), ents_radius[s] + bound)
        if s < len(pos):
            assert math.hypot(pos[s][0] - ents_xz[s][0], pos[s][2] - ents_xz[s][1]) <= ents_radius[s] + bound, (s, pos[s])
        out[s] = len(ii)
    return out


@pytest.mark.parametrize("cls_name", ["Hallway", "OneRoom", "PickupObjects"])
def test_a_sensed_cell_lies_on_its_object(program, tmp_path, cls_name):
    sc = _scene(cls_name)
    extent = [float(v) for v in sc["extent"]]
    E = len(sc["ents_kind"])
    xz = [(float(p[0]), float(p[2])) for p in sc["ents_pos"]]
    radius = [float(r) for r in sc["ents_radius"]]
    # (a camera 1.5 m up with 30 degrees below its axis sees nothing lower than 0.63 m at 1.5 m: the objects that reach into its view)
    tall = [s for s in range(E) if float(sc["ents_height"][s]) >= 0.8]
    assert tall and (len(tall) >= 2 or cls_name != "PickupObjects")
    for slot in tall:
        pose = facing(sc, slot)
        code, depth = _label(cls_name, pose, CAMERAS[0], 8, 80, 60)
        grid = _grid(extent, ids=E)
        m, n, pos = _both(program, tmp_path, 8, 80, 60, grid, extent, [(pose, CAMERAS[0], 1, 1, depth, code)], (cls_name, slot))[0]
        found = lies_on_its_object(m, pos, xz, radius, extent, CELL)
        # the condition that keeps the statement from passing empty, on the restatement alone
        assert found.get(slot, 0) >= 1 and n[slot] == found[slot], (cls_name, slot, found)


# ---------------------------------------------------------------------------------------------------------------- the interface

def test_launch_arithmetic(program):
    for N, cells, ids in ((1, 1, 0), (4, 33 * 33, 0), (4096, 16384, 255), (7, 16384, 0), (2, 768, 18), (3, 128 * 128, 1)):
        assert launch_of(program, N, cells, ids) == dict(grid=N, threads=256, lds=4 * cells + 12 * ids, fits=1), (N, cells, ids)
    assert launch_of(program, 4096, 16384, 255)["lds"] == 68596 > 64 * 1024
    for N, cells, ids in ((1, 16385, 255), (1, 16385, 0), (1, 0, 0), (1, 100, 256), (1, 100, -1)):
        assert launch_of(program, N, cells, ids)["fits"] == 0, (N, cells, ids)


def test_header_declares_the_entry_point_and_the_build_has_the_units():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    text = " ".join(re.sub(r"/\*.*?\*/", "", header, flags=re.S).split())
    proto = ("int mw_label_project(mw_engine *e, const double *host_params , const float *d_depth , const int32_t *d_code , int32_t base, const uint8_t *d_mask, "
             "int32_t size, int32_t flags, uint8_t *d_plane , const mw_nav_params *grid , const uint8_t *d_clear, uint8_t *d_map , int32_t ids , "
             "int32_t *d_obj_cells , double *d_obj_pos , void *stream);")
    assert proto in text
    assert header.index("---- label frames") < header.index("---- object maps") < header.index("int mw_label_project(")
    assert re.search(r"#define MW_ABI_VERSION 4\b", header)
    assert "mw_label_project" in engine.SIGNATURES and engine.EXPORTS == list(engine.SIGNATURES)
    assert engine.LABELMAP_MAX_CELLS == 16384 and engine.LABELMAP_MAX_IDS == 255
    check_units_built("mw_labelmap.hip", "mw_engine_labelmap.hip")
    check_kernel("mw_labelmap_kernel", "mw_labelmap.hip")
    check_does_not_wait("mw_engine_labelmap.hip")
    # the projection is mw_depth.h's, called: the header restates none of it
    labelmap_h = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "mw_labelmap.h")).read())
    for shared in ("mwdepth::camera_of", "mwdepth::point_of", "mwdepth::window_bin", "mwdepth::map_bin", "mwnav::grid_of", "mwnav::covers"):
        assert shared in labelmap_h, shared
    for own in ("floor(", "sincos", "sub_x", "min_range", "floor_tol"):
        assert own not in labelmap_h, own
    kernel = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "mw_labelmap.hip")).read())
    assert "asm" not in kernel


def test_library_exports_the_entry_point_and_refuses_a_null_engine():
    check_refuses_null_engine("mw_label_project", None, None, None, 0, None, 9, 0, None, None, None, None, 0, None, None, None)


def test_vec_env_refusals_and_the_recorded_call(monkeypatch):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import MiniWorldVecEnv, ObjectMap, ObjectWindow
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5, want_depth=True)
    bare = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    many = MiniWorldVecEnv("MiniWorld-CollectHealth-v0", 2, want_depth=True)
    n0 = len(lib.calls)
    w, m = vec.object_window(), vec.object_map()
    assert len(lib.calls) == n0         # both are made without the library
    assert isinstance(w, ObjectWindow) and (w.size, w.cell, w.back, w.frame) == (33, 0.25, 0.0, "heading")
    assert (w.min_range, w.max_range, w.floor_tol, w.top) == (0.05, 8.0, 0.1, 1.6)
    assert w.plane.dtype == torch.uint8 and tuple(w.plane.shape) == (5, 33, 33) and not w.plane.any()
    field = vec.nav_field()
    K = min(int(vec.engine.cfg.max_ents), 255)
    assert isinstance(m, ObjectMap) and (m.cell, m.gx, m.gz, m.ids) == (0.25, field.gx, field.gz, K) and K >= 1
    assert m.map.dtype == torch.uint8 and tuple(m.map.shape) == (5, m.gz, m.gx) and not m.map.any()
    assert m.cells.dtype == torch.int32 and tuple(m.cells.shape) == (5, K) and not m.cells.any()
    assert m.pos.dtype == torch.float64 and tuple(m.pos.shape) == (5, K, 3) and m.pos.isnan().all()
    assert many.object_map().ids == int(many.engine.cfg.max_ents) == 18
    # the one library call of an object_update: a label frame's codes with base RAY_ENT; its own depth where it has one, else the env's
    labels, with_depth = vec.label_frame(), vec.label_frame(depth=True)
    n0 = len(lib.calls)
    assert vec.object_update(w, labels) is w.plane
    assert [c[0] for c in lib.calls[n0:]] == ["mw_label_project"]
    args = lib.calls[-1][1]
    assert list(args[1]) == [0.05, 8.0, 0.1, 1.6, 0.25, 0.0] and args[2].value == vec.depth.data_ptr() and args[3].value == labels.code.data_ptr()
    assert args[4] == engine.RAY_ENT and args[5] is None and tuple(args[6:8]) == (33, 0) and args[8].value == w.plane.data_ptr()
    assert args[9] is None and args[10] is None and args[11] is None and args[12] == 0 and args[13] is None and args[14] is None
    vec.object_update(w, with_depth)
    assert lib.calls[-1][1][2].value == with_depth.depth.data_ptr()
    assert bare.object_update(bare.object_window(), bare.label_frame(depth=True)) is not None        # no env depth needed then
    # the caller's own category image with base 0, the caller's depth, a mask, the bottom anchor and the north frame
    w2 = vec.object_window(size=8, cell=0.5, anchor="bottom", frame="north", min_range=0.2, max_range=4.0, floor_tol=0.0, top=2.0)
    mask = torch.tensor([1, 1, 0, 1, 0], dtype=torch.uint8)
    mine, cats = torch.ones((5, 60, 80), dtype=torch.float32), torch.zeros((5, 60, 80), dtype=torch.int32)
    vec.object_update(w2, cats, depth=mine, mask=mask)
    args = lib.calls[-1][1]
    assert list(args[1]) == [0.2, 4.0, 0.0, 2.0, 0.5, 4.0] and args[2].value == mine.data_ptr() and args[3].value == cats.data_ptr() and args[4] == 0
    assert args[5].value == mask.data_ptr() and tuple(args[6:8]) == (8, engine.EGO_NORTH) and args[8].value == w2.plane.data_ptr()
    # ... and of an object_map_update
    like = vec.object_map(like=vec.depth_map(cell=0.5), ids=7, top=1.0)
    clear = torch.tensor([0, 1, 0, 0, 1], dtype=torch.bool)
    assert vec.object_map_update(like, labels, clear=clear, mask=mask) is like.cells
    args = lib.calls[-1][1]
    p = args[9]._obj
    assert (p.cell, p.gx, p.gz) == (0.5, like.gx, like.gz) and list(args[1])[:4] == [0.05, 8.0, 0.1, 1.0] and args[8] is None and tuple(args[6:8]) == (0, 0)
    assert args[10].value == clear.data_ptr() and args[11].value == like.map.data_ptr() and args[12] == 7
    assert args[13].value == like.cells.data_ptr() and args[14].value == like.pos.data_ptr() and args[5].value == mask.data_ptr()
    none = vec.object_map(ids=0)
    vec.object_map_update(none, cats)
    args = lib.calls[-1][1]
    assert args[12] == 0 and args[13] is None and args[14] is None and tuple(none.cells.shape) == (5, 0) and tuple(none.pos.shape) == (5, 0, 3)
    # like= takes the four kinds of map, and the other maps take an ObjectMap
    for other in (field, vec.seen_map(), vec.depth_map(), m):
        assert (vec.object_map(like=other).gx, vec.object_map(like=other).gz) == (other.gx, other.gz)
    assert (vec.depth_map(like=m).gx, vec.seen_map(like=m).gz) == (m.gx, m.gz)
    blocked = torch.zeros((5, m.gz, m.gx), dtype=torch.uint8)
    grid_field = vec.grid_field(blocked, target=m.pos[:, 0].contiguous(), reach=0.5, like=m)
    assert (grid_field.gx, grid_field.gz) == (m.gx, m.gz)
    # refusals: every argument of object_window and object_map ...
    four = MiniWorldVecEnv("MiniWorld-FourRooms-v0", 2, want_depth=True)
    large = MiniWorldVecEnv("MiniWorld-Hallway-v0", 2, want_depth=True, obs_width=320, obs_height=240)
    n0 = len(lib.calls)
    nan, inf = float("nan"), float("inf")
    sensor = (dict(min_range=0.0), dict(min_range=nan), dict(max_range=inf), dict(min_range=3.0, max_range=2.0), dict(floor_tol=-0.1), dict(floor_tol=nan),
              dict(top=-1.0), dict(top=inf), dict(floor_tol=0.5, top=0.4), dict(top="high"))
    for kw in (dict(size=0), dict(size=129), dict(size=9.0), dict(cell=0.0), dict(cell=nan), dict(cell="a"), dict(anchor="top"), dict(frame="east")) + sensor:
        with pytest.raises(ValueError):
            vec.object_window(**kw)
    for kw in (dict(cell=0.0), dict(cell=nan), dict(cell=0.01), dict(like=w), dict(like=field, cell=0.5), dict(ids=-1), dict(ids=256), dict(ids=1.0),
               dict(ids=True)) + sensor:
        with pytest.raises(ValueError):
            vec.object_map(**kw)
    with pytest.raises(ValueError, match="use a larger cell"):
        four.object_map(cell=0.1)
    for make in (large.object_window, large.object_map):
        with pytest.raises(ValueError, match="65535"):
            make()
    # ... and of the updates
    no_code = vec.label_frame(code=False)
    for kw in (dict(labels=None), dict(labels=no_code), dict(labels=cats[:4]), dict(labels=cats.long()), dict(labels=cats.numpy()), dict(labels=labels.cls),
               dict(labels=torch.zeros((5, 60, 160), dtype=torch.int32)[:, :, ::2]), dict(labels=cats, depth=mine[:4]), dict(labels=cats, depth=mine.double()),
               dict(labels=labels, mask=[1, 0, 0, 1, 0]), dict(labels=labels, mask=mask[:4]), dict(labels=cats, mask=mask.float())):
        with pytest.raises(ValueError):
            vec.object_update(w, **kw)
        with pytest.raises(ValueError):
            vec.object_map_update(m, **kw)
    with pytest.raises(ValueError, match="want_depth=True"):
        bare.object_update(bare.object_window(), bare.label_frame())
    with pytest.raises(ValueError):
        vec.object_map_update(m, labels, clear=mask.float())
    for bad in (None, w.plane, m, vec.depth_window()):
        with pytest.raises(ValueError):
            vec.object_update(bad, labels)
    for bad in (None, m.map, w, vec.depth_map()):
        with pytest.raises(ValueError):
            vec.object_map_update(bad, labels)
    sensor4 = (0.05, 8.0, 0.1, 1.6)
    wide = torch.zeros((5, 33, 34), dtype=torch.uint8)
    for plane, size in ((w.plane.to(torch.int8), 33), (w.plane[:4], 33), (wide[:, :, :33], 33), (None, 33), (w.plane, 32)):
        with pytest.raises(engine.EngineError):
            vec.object_update(ObjectWindow(plane, size, 0.25, 0.0, "heading", *sensor4), labels)
    for name, value in (("map", m.map[:, :, :-1]), ("map", m.map.to(torch.int8)), ("map", None), ("cells", m.cells[:, :0]), ("cells", m.cells.long()),
                        ("pos", m.pos[:4]), ("pos", m.pos.float()), ("ids", K + 1)):
        b = ObjectMap(m.map, m.cells, m.pos, m.params, m.ids, *sensor4)
        setattr(b, name, value)
        with pytest.raises(engine.EngineError):
            vec.object_map_update(b, labels)
    assert len(lib.calls) == n0         # nothing reached the library


def test_adapter_is_off_by_default_and_needs_the_label_frame(monkeypatch):
    import torch
    from miniworld_amd.vector import MiniWorldVectorEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    plain = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, label_frame={})
    _, info = plain.reset(seed=0)
    _, _, _, _, info2 = plain.step(torch.zeros(2, dtype=torch.int32))
    assert plain.object_win is None and "object_map" not in info and "object_map" not in info2
    assert "mw_label_project" not in [c[0] for c in lib.calls]
    for bad in (True, 9, [("size", 9)]):
        with pytest.raises(ValueError):
            MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, object_map=bad, label_frame={})
    for frame in (None, dict(code=False)):
        with pytest.raises(ValueError, match="label_frame"):
            MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, object_map={}, label_frame=frame)
    with pytest.raises(ValueError, match="want_depth"):
        MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, object_map={}, label_frame={}, want_depth=False)
    n0 = len(lib.calls)
    envs = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, object_map=dict(size=9, max_range=4.0), label_frame=dict(meshes="bounds"))
    assert envs.vec.want_depth and envs.vec.depth is not None
    _, info = envs.reset(seed=0)
    assert envs.object_win.size == 9 and set(info) == {"label", "object_map"}
    _, _, _, _, info = envs.step(torch.zeros(2, dtype=torch.int32))
    assert info["object_map"].dtype == torch.uint8 and tuple(info["object_map"].shape) == (2, 9, 9) and info["object_map"] is not envs.object_win.plane
    names = [c[0] for c in lib.calls[n0:] if c[0] in ("mw_label_frame", "mw_label_project")]
    assert names == ["mw_label_frame", "mw_label_project"] * 2          # behind the label update, on the reset and on the step
    assert [c for c in lib.calls if c[0] == "mw_label_project"][-1][1][2].value == envs.vec.depth.data_ptr()
    own = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, object_map={}, label_frame=dict(depth=True), want_depth=False)
    own.reset(seed=0)
    assert [c for c in lib.calls if c[0] == "mw_label_project"][-1][1][2].value == own.label.depth.data_ptr() and own.vec.depth is None
