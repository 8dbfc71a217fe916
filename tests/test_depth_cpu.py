"""Depth projection (mw_depth_project; MiniWorldVecEnv.depth_window / depth_update / depth_map / depth_map_update) without a GPU.

The phases the kernel runs (miniworld_amd/csrc/mw_depth.h) run on the host with (lane, stride) = (0, 1) in a program of its own
(tests/hostcheck/depth_project.cpp), built with the address and undefined-behaviour sanitizers, on the oracle's own CPU depth frames
of worlds the host classes generate; its planes, maps, counts and new cells over a short walk are compared, exactly, with the
restatement of tests/depth_reference.py.  The geometry itself is checked against the renderer: every pixel of a frame, unprojected by
the restatement, lies on the floor, the ceiling, a collision segment or a Box, within the depth value's own quantisation.  Beside that:
synthetic depth for the edges, the ABI names, the sample table against the rasteriser's, the refusals of the binding over a stub engine
and the adapter's key."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import depth_reference as ref
import nav_reference as nav
import ray_reference as ray
from helpers import stub_engine
from query_checks import (CSRC, ROOT, build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, pose_of as _pose_of, run,
                          scene as _scene, scene_walk)

CELL = 0.25
NORTH = 2
SENSOR = ref.SENSOR
NEAR, FAR = 0.04, 100.0
# cameras at corners of the domain-randomisation ranges (height, fwd_disp, pitch, fov_y), and the default one
CAMERAS = [(1.5, 0.0, 0.0, 60.0), (1.45, -0.05, -5.0, 55.0), (1.55, 0.10, 5.0, 65.0), (1.45, 0.10, 5.0, 55.0), (1.55, -0.05, -5.0, 65.0)]
# the oracle's frames: (samples, W, H) — 80 x 60 at every sample count, and an odd size
FRAMES = [(8, 80, 60), (4, 80, 60), (1, 80, 60), (8, 21, 13), (1, 21, 13)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("depth_project", tmp_path_factory.mktemp("depth_project"))


_frames = {}


def _render(cls_name, pose, cam, msaa, W, H, seed=0):
    """the oracle's frame of the world from `pose` under `cam`: (depth float32[H, W], z16 uint16[H, W]); computed once, never changed"""
    key = (cls_name, seed, pose, cam, msaa, W, H)
    if key not in _frames:
        import pyoracle
        sc = dict(_scene(cls_name, seed))
        pos = np.array(sc["agent_pos"], np.float64)
        pos[0], pos[2] = pose[0], pose[1]
        sc["agent_pos"], sc["agent_dir"] = pos, pose[2]
        sc["cam_height"], sc["cam_fwd_disp"], sc["cam_pitch"], sc["cam_fov_y"] = cam
        out = pyoracle.render(sc, W, H, msaa)
        depth, z16 = out["depth"].reshape(H, W).copy(), out["z16"].copy()
        depth.setflags(write=False)
        z16.setflags(write=False)
        _frames[key] = (depth, z16)
    return _frames[key]


def _poses(cls_name, steps, seed=0):
    """poses (x, z, dir) from the world's own first one: turns and forward moves of the env's sizes, kept inside the extent"""
    return scene_walk(cls_name, steps, seed, 3400 + seed, 15)


def _bits(depth):
    return " ".join(f"{v:x}" for v in np.ascontiguousarray(depth, np.float32).ravel().view(np.uint32).tolist())


def _run(program, tmp_path, msaa, W, H, target, extent, steps, sensor=SENSOR, garbage=0):
    """target: dict(size, cell, back, north) or dict(cell, gx, gz, min_points); steps: (pose, cam, mask, clear, depth[H, W]) -> per
    step the host build's uint8[2, S, S], or (uint8[2, gz, gx], count int32[2], new int32[2])"""
    to_map = "gx" in target
    lines = [f"{W} {H} {msaa}", " ".join(repr(float(sensor[k])) for k in ("min_range", "max_range", "floor_tol", "top"))]
    if to_map:
        lines.append(f"1 {float(target['cell'])!r} {target['gx']} {target['gz']} {target['min_points']}")
        shape = (2, target["gz"], target["gx"])
    else:
        lines.append(f"0 {target['size']} {float(target['cell'])!r} {float(target['back'])!r} {NORTH if target['north'] else 0}")
        shape = (2, target["size"], target["size"])
    lines += [str(garbage), " ".join(repr(float(v)) for v in extent), str(len(steps))]
    for pose, cam, mask, clear, depth in steps:
        lines.append(" ".join(repr(float(v)) for v in tuple(pose) + tuple(cam)) + f" {int(mask)} {int(clear)}")
        lines.append(_bits(depth))
    rows = run(program, tmp_path / "walk.txt", lines, blank=True)
    per = 2 if to_map else 1
    assert len(rows) == per * len(steps)
    out = []
    for k in range(len(steps)):
        cells = np.array(rows[per * k].split(), np.uint8).reshape(shape)
        if to_map:
            c = np.array(rows[per * k + 1].split(), np.int64).astype(np.int32)
            out.append((cells, c[:2], c[2:]))
        else:
            out.append(cells)
    return out


def _reference(msaa, target, extent, steps, sensor=SENSOR, garbage=0):
    """the same walk through the restatement; a masked-off step keeps what the buffers held"""
    out = []
    if "gx" in target:
        m = ref.Map(target["gx"], target["gz"], garbage)
        for pose, cam, mask, clear, depth in steps:
            if mask:
                ref.map_update(m, depth, pose, cam, msaa, extent, target["cell"], target["min_points"], clear, **sensor)
            out.append((m.map.copy(), m.count.copy(), m.new.copy()))
        return out
    planes = np.full((2, target["size"], target["size"]), garbage, np.uint8)
    for pose, cam, mask, clear, depth in steps:
        if mask:
            planes = ref.window(depth, pose, cam, msaa, target["size"], target["cell"], target["back"], target["north"], **sensor)
        out.append(planes.copy())
    return out


def _same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(g, tuple):
            assert np.array_equal(g[0], w[0]), (what, k, "map", np.argwhere(g[0] != w[0])[:8].tolist())
            assert np.array_equal(g[1], w[1]) and np.array_equal(g[2], w[2]), (what, k, "count / new", g[1:], w[1:])
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, k, np.argwhere(g != w)[:8].tolist())


def _window(size=33, cell=CELL, anchor="centre", north=False):
    return dict(size=size, cell=cell, back=size / 2 if anchor == "bottom" else 0.0, north=north)


def _grid(extent, cell=CELL, min_points=1):
    gx, gz = nav.grid_shape(extent, cell)
    return dict(cell=cell, gx=int(gx), gz=int(gz), min_points=min_points)


ALL_SHAPES = [_window(S, anchor=a, north=n) for S in (1, 2, 9, 33) for a in ("centre", "bottom") for n in (False, True)]
FEW_SHAPES = [_window(33), _window(9, anchor="bottom", north=True), _window(2, north=True), _window(128, cell=0.1, anchor="bottom")]


@pytest.mark.parametrize("cls_name", ["Hallway", "OneRoom", "FourRooms", "MazeS3"])
def test_walk_equals_the_restatement(program, tmp_path, cls_name):
    extent = [float(v) for v in _scene(cls_name)["extent"]]
    poses = _poses(cls_name, 4)
    seen = {"floor": 0, "obstacle": 0, "clamped": 0, "new_later": 0, "dropped_far": 0}
    for f, (msaa, W, H) in enumerate(FRAMES):
        # a camera per step, another start per frame format; the first step clears the map's garbage, the third is masked off, the last clears again
        steps = [(p, CAMERAS[(f + k) % len(CAMERAS)], 0 if k == 2 else 1, 1 if k in (0, 3) else 0, None) for k, p in enumerate(poses)]
        steps = [(p, c, m, cl, _render(cls_name, p, c, msaa, W, H)[0]) for p, c, m, cl, _ in steps]
        sensor = dict(SENSOR, max_range=3.0) if f % 2 else SENSOR          # (every other format with a range that cuts the rooms)
        for target in (ALL_SHAPES if f == 0 else FEW_SHAPES) + [_grid(extent), _grid(extent, 0.5, min_points=3)]:
            got = _run(program, tmp_path, msaa, W, H, target, extent, steps, sensor=sensor, garbage=0xAB)
            want = _reference(msaa, target, extent, steps, sensor=sensor, garbage=0xAB)
            _same(got, want, (cls_name, msaa, W, H, target))
            if "gx" in target:
                assert all(np.array_equal(a, b) for a, b in zip(want[1], want[2]))        # the masked step kept every byte
                seen["new_later"] += int(want[1][2].sum())
            else:
                seen["floor"] += int(want[0][0].astype(np.int64).sum())
                seen["obstacle"] += int(want[0][1].astype(np.int64).sum())
                seen["clamped"] += int((want[0] == 255).sum())
        seen["dropped_far"] += int(sum((st[4] > sensor["max_range"]).sum() for st in steps))
    # what makes the comparison above worth something, asserted on the restatement alone
    assert seen["obstacle"] > 0 and seen["new_later"] > 0
    if cls_name in ("Hallway", "OneRoom"):
        assert seen["floor"] > 0 and seen["dropped_far"] > 0


def _flat(value, W=80, H=60):
    return np.full((H, W), value, np.float32)


def test_synthetic_depth_edges(program, tmp_path):
    extent = [-1.0, 13.0, -3.0, 3.0]
    pose, cam = (0.5, 0.1, 0.3), CAMERAS[0]
    nan, inf = float("nan"), float("inf")
    for target in (_window(33), _window(33, north=True), _grid(extent)):
        # nothing of these is a point: NaN, infinities, zero, negative values, the sky
        for bad in (nan, inf, -inf, 0.0, -0.0, -3.0, 100.0, np.float32(SENSOR["min_range"]) - np.float32(1e-6), 8.000001):
            for who, run in (("host", _run(program, tmp_path, 8, 80, 60, target, extent, [(pose, cam, 1, 0, _flat(bad))], garbage=0x11)),
                             ("restatement", _reference(8, target, extent, [(pose, cam, 1, 0, _flat(bad))], garbage=0x11))):
                cells = run[0][0] if "gx" in target else run[0]
                assert (cells == (0x11 if "gx" in target else 0)).all(), (who, target, bad)
                if "gx" in target:
                    assert run[0][2].tolist() == [0, 0]
        # exactly at the bounds a pixel counts
        sensor = dict(SENSOR, min_range=0.5, max_range=2.0, floor_tol=0.1, top=3.0)
        for edge in (0.5, 2.0):
            both = {"host": _run(program, tmp_path, 8, 80, 60, target, extent, [(pose, cam, 1, 1, _flat(edge))], sensor=sensor),
                    "restatement": _reference(8, target, extent, [(pose, cam, 1, 1, _flat(edge))], sensor=sensor)}
            _same(both["host"], both["restatement"], (target, edge))
            cells = both["restatement"][0][0] if "gx" in target else both["restatement"][0]
            assert cells.any(), (target, edge)
    # facing a wall at half a metre: thousands of points in a handful of cells, clamped to 255
    target = _window(9, cell=0.5)
    both = {"host": _run(program, tmp_path, 8, 80, 60, target, extent, [(pose, cam, 1, 0, _flat(0.5))]),
            "restatement": _reference(8, target, extent, [(pose, cam, 1, 0, _flat(0.5))])}
    _same(both["host"], both["restatement"], "pile-up")
    p = ref.unproject(_flat(0.5), pose, cam, 8, **SENSOR)
    most = int(ref.window_counts(p, 9, 0.5, 0.0, False).max())
    assert most > 1000 and both["restatement"][0].max() == 255 and (both["restatement"][0] == 255).sum() >= 1
    # a window of one cell, and one wholly outside the view (behind the agent)
    for target, empty in ((_window(1, cell=20.0), False), (dict(size=5, cell=0.25, back=-40.0, north=False), True)):
        depth = _render("OneRoom", _pose_of(_scene("OneRoom")), cam, 8, 80, 60)[0]
        steps = [(_pose_of(_scene("OneRoom")), cam, 1, 0, depth)]
        ext = [float(v) for v in _scene("OneRoom")["extent"]]
        both = {"host": _run(program, tmp_path, 8, 80, 60, target, ext, steps, garbage=0x77), "restatement": _reference(8, target, ext, steps, garbage=0x77)}
        _same(both["host"], both["restatement"], target)
        assert both["restatement"][0].any() != empty, target
    # a NaN pose puts nothing into a map or a north window
    for target in (_window(9, north=True), _grid(extent)):
        for who, run in (("host", _run(program, tmp_path, 8, 80, 60, target, extent, [((nan, 0.1, 0.3), cam, 1, 1, _flat(1.0))])),
                         ("restatement", _reference(8, target, extent, [((nan, 0.1, 0.3), cam, 1, 1, _flat(1.0))]))):
            cells = run[0][0] if "gx" in target else run[0]
            assert not cells.any(), (who, target)


def test_map_accumulates_clears_and_obeys_the_mask(program, tmp_path):
    sc = _scene("OneRoom")
    extent = [float(v) for v in sc["extent"]]
    poses = _poses("OneRoom", 6)
    cam = CAMERAS[0]
    frames = [_render("OneRoom", p, cam, 8, 80, 60)[0] for p in poses]
    for min_points in (1, 3):
        target = _grid(extent, min_points=min_points)
        # steps 0 - 2 accumulate; 3 is masked off with clear set (the mask wins); 4 clears; 5 repeats 4's frame: nothing new
        steps = [(poses[0], cam, 1, 1, frames[0]), (poses[1], cam, 1, 0, frames[1]), (poses[2], cam, 1, 0, frames[2]), (poses[3], cam, 0, 1, frames[3]),
                 (poses[4], cam, 1, 1, frames[4]), (poses[4], cam, 1, 0, frames[4])]
        got, want = _run(program, tmp_path, 8, 80, 60, target, extent, steps, garbage=0xCD), _reference(8, target, extent, steps, garbage=0xCD)
        _same(got, want, min_points)
        maps, counts, news = zip(*want)
        assert set(np.unique(maps[2]).tolist()) == {0, 1}
        assert (maps[1] >= maps[0]).all() and (maps[2] >= maps[1]).all()         # no call clears a byte
        assert counts[2].tolist() == maps[2].reshape(2, -1).sum(1).tolist() == (news[0] + news[1] + news[2]).tolist()
        assert np.array_equal(maps[3], maps[2]) and np.array_equal(counts[3], counts[2]) and np.array_equal(news[3], news[2])
        assert counts[4].tolist() == news[4].tolist() == maps[4].reshape(2, -1).sum(1).tolist()
        assert news[5].tolist() == [0, 0] and np.array_equal(maps[5], maps[4])
    one = _reference(8, _grid(extent), extent, [(poses[0], cam, 1, 1, frames[0])])[0][0]
    three = _reference(8, _grid(extent, min_points=3), extent, [(poses[0], cam, 1, 1, frames[0])])[0][0]
    assert (three <= one).all() and three.sum() < one.sum()
    # a grid that does not cover the extent: zeroed rows and counts, whatever they held
    short = dict(cell=CELL, gx=3, gz=3, min_points=1)
    got, want = _run(program, tmp_path, 8, 80, 60, short, extent, steps[:1], garbage=0xCD), _reference(8, short, extent, steps[:1], garbage=0xCD)
    _same(got, want, "uncovered")
    assert not want[0][0].any() and want[0][1].tolist() == want[0][2].tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------------------- the geometry

def _geometry_poses(cls_name):
    """The walk's poses.  In FourRooms turned by 270 degrees: a doorway's lintel (the wall between 2.2 m and the ceiling) is drawn but
    is no collision segment, and from the world's own first heading it fills more than the cap allows of a 21 x 13 frame."""
    turn = math.radians(270) if cls_name == "FourRooms" else 0.0
    return [(x, z, d + turn) for x, z, d in _poses(cls_name, 3)]


GEOMETRY = [(c, m, W, H) for c in ("Hallway", "OneRoom", "FourRooms", "MazeS3") for (m, W, H) in ((8, 80, 60), (4, 80, 60), (1, 80, 60), (8, 21, 13))]


@pytest.mark.parametrize("cls_name,msaa,W,H", GEOMETRY)
def test_every_pixel_lies_on_the_world_the_renderer_drew(cls_name, msaa, W, H):
    from miniworld_amd import engine
    assert all(int(k) == engine.ENT_BOX for k in _scene(cls_name)["ents_kind"])       # walls, floor, ceiling and Boxes only
    for k, pose in enumerate(_geometry_poses(cls_name)):
        for cam in (CAMERAS[0], CAMERAS[1 + (k % 4)]):
            depth, z16 = _render(cls_name, pose, cam, msaa, W, H)
            bad, inside = ref.unclassified(depth, z16, pose, cam, msaa, ref.solids_of_scene(_scene(cls_name)))
            print(f"{cls_name} {msaa} {W}x{H} pose {k} cam {cam}: {bad} of {inside} pixels within 5 m unclassified")
            assert inside > W * H // 10
            assert bad <= 0.02 * W * H, (cls_name, msaa, W, H, pose, cam, bad)


def test_a_wrong_sample_offset_or_sign_fails_the_geometry():
    """the check above is sharp: the pixel's centre in the place of sample 0, or a flipped pitch, leaves far more pixels off the world"""
    pose, cam = _poses("OneRoom", 1)[0], CAMERAS[2]
    depth, z16 = _render("OneRoom", pose, cam, 8, 80, 60)
    good, _ = ref.unclassified(depth, z16, pose, cam, 8, ref.solids_of_scene(_scene("OneRoom")))
    centre, _ = ref.unclassified(depth, z16, pose, cam, 1, ref.solids_of_scene(_scene("OneRoom")))         # (1 sample: the centre)
    flipped, _ = ref.unclassified(depth, z16, pose, (cam[0], cam[1], -cam[2], cam[3]), 8, ref.solids_of_scene(_scene("OneRoom")))
    assert good <= 96 < centre and flipped > 96, (good, centre, flipped)


# ---------------------------------------------------------------------------------------------------------------- the interface

def test_the_sample_table_is_the_rasterisers(program):
    text = open(os.path.join(CSRC, "mw_records.h")).read()
    body = re.search(r"kPat\[4\]\[16\]\[2\] = \{(.*?)\};", text, re.S).group(1)
    rows = [re.findall(r"\{(\d+), (\d+)\}", row) for row in body.split("\n") if row.strip()]
    first = {1: rows[0][0], 4: rows[1][0], 8: rows[2][0]}
    for msaa, (sx, sy) in first.items():
        out = subprocess.run([program, "--pattern", str(msaa)], capture_output=True, text=True, check=True).stdout.split()
        assert (int(sx), int(sy)) == tuple(map(int, out)) == ref.SAMPLE0[msaa], msaa
    assert ref.subpixel(8) == (9 / 16, 1 - 5 / 16) and ref.subpixel(1) == (0.5, 0.5)


def test_header_declares_the_entry_point_and_the_build_has_the_units():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    text = " ".join(re.sub(r"/\*.*?\*/", "", header, flags=re.S).split())
    proto = ("int mw_depth_project(mw_engine *e, const double *host_params , const float *d_depth , const uint8_t *d_mask, int32_t size, int32_t flags, "
             "uint8_t *d_planes , const mw_nav_params *grid , int32_t min_points, const uint8_t *d_clear , uint8_t *d_map , int32_t *d_count , "
             "int32_t *d_new , void *stream);")
    assert proto in text
    assert re.search(r"#define MW_DEPTH_MAX_PIXELS 65535\b", header) and engine.DEPTH_MAX_PIXELS == 65535
    assert re.search(r"#define MW_ABI_VERSION 4\b", header)
    assert header.index("---- egocentric map windows") < header.index("---- depth projection") < header.index("int mw_depth_project(")
    for cited in ("opengl.py:400-435", "miniworld.py:1200-1222", "entity.py:477-503", "z * z * (far - near) / (far * near * 65535)"):
        assert cited in header, cited
    assert "mw_depth_project" in engine.SIGNATURES and engine.EXPORTS == list(engine.SIGNATURES)
    check_units_built("mw_depth.hip", "mw_engine_depth.hip")
    check_kernel("mw_depth_kernel", "mw_depth.hip")
    depth_h = open(os.path.join(CSRC, "mw_depth.h")).read()
    for shared in ("mwego::frame_of", "mwnav::grid_of", "mwnav::covers", "mw::sincos_det"):
        assert shared in depth_h, shared
    code = re.sub(r"//[^\n]*", "", depth_h)
    for own in ("sqrt", "sin(", "cos(", "tan(", "atan"):
        assert own not in code.replace("sincos_det(", ""), own
    check_does_not_wait("mw_engine_depth.hip")


def test_library_exports_the_entry_point_and_refuses_a_null_engine():
    check_refuses_null_engine("mw_depth_project", None, None, None, 9, 0, None, None, 1, None, None, None, None, None)


def test_vec_env_refusals_and_the_recorded_call(monkeypatch):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import DepthMap, DepthWindow, MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    bare = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    with pytest.raises(ValueError, match="want_depth=True"):
        bare.depth_update(bare.depth_window())
    with pytest.raises(ValueError, match="want_depth=True"):
        bare.depth_map_update(bare.depth_map())
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5, want_depth=True)
    n0 = len(lib.calls)
    w, m = vec.depth_window(), vec.depth_map()
    assert len(lib.calls) == n0         # both are made without the library
    assert isinstance(w, DepthWindow) and (w.size, w.cell, w.back, w.frame) == (33, 0.25, 0.0, "heading")
    assert (w.min_range, w.max_range, w.floor_tol, w.top) == (0.05, 8.0, 0.1, float(vec.engine.cfg.agent_height)) and w.top == 1.6
    assert w.planes.dtype == torch.uint8 and tuple(w.planes.shape) == (5, 2, 33, 33) and not w.planes.any()
    assert w.floor.data_ptr() == w.planes[:, 0].data_ptr() and w.obstacle.data_ptr() == w.planes[:, 1].data_ptr() and tuple(w.floor.shape) == (5, 33, 33)
    field = vec.nav_field()
    assert isinstance(m, DepthMap) and (m.cell, m.gx, m.gz, m.min_points) == (0.25, field.gx, field.gz, 1)
    assert tuple(m.map.shape) == (5, 2, m.gz, m.gx) and m.free.data_ptr() == m.map[:, 0].data_ptr() and m.obstacle.data_ptr() == m.map[:, 1].data_ptr()
    assert m.count.dtype == m.new.dtype == torch.int32 and tuple(m.count.shape) == tuple(m.new.shape) == (5, 2)
    # the one library call of a depth_update
    n0 = len(lib.calls)
    assert vec.depth_update(w) is w.planes
    assert [c[0] for c in lib.calls[n0:]] == ["mw_depth_project"]
    args = lib.calls[-1][1]
    assert list(args[1]) == [0.05, 8.0, 0.1, 1.6, 0.25, 0.0] and args[2].value == vec.depth.data_ptr() and args[3] is None
    assert tuple(args[4:6]) == (33, 0) and args[6].value == w.planes.data_ptr() and args[7] is None and all(a is None for a in args[9:13])
    # the bottom anchor, the north frame, the caller's depth without the last axis, a mask
    w2 = vec.depth_window(size=8, cell=0.5, anchor="bottom", frame="north", min_range=0.2, max_range=4.0, floor_tol=0.0, top=2.0)
    mask = torch.tensor([1, 1, 0, 1, 0], dtype=torch.uint8)
    mine = torch.ones((5, 60, 80), dtype=torch.float32)
    vec.depth_update(w2, depth=mine, mask=mask)
    args = lib.calls[-1][1]
    assert list(args[1]) == [0.2, 4.0, 0.0, 2.0, 0.5, 4.0] and args[2].value == mine.data_ptr() and args[3].value == mask.data_ptr()
    assert tuple(args[4:6]) == (8, engine.EGO_NORTH) and args[6].value == w2.planes.data_ptr()
    # ... and of a depth_map_update
    like = vec.depth_map(like=vec.seen_map(cell=0.5), min_points=3, top=1.0)
    clear = torch.tensor([0, 1, 0, 0, 1], dtype=torch.bool)
    assert vec.depth_map_update(like, clear=clear, mask=mask) is like.new
    args = lib.calls[-1][1]
    p = args[7]._obj
    assert (p.cell, p.gx, p.gz) == (0.5, like.gx, like.gz) and list(args[1])[:4] == [0.05, 8.0, 0.1, 1.0] and args[6] is None and args[8] == 3
    assert args[9].value == clear.data_ptr() and args[10].value == like.map.data_ptr() and args[11].value == like.count.data_ptr()
    assert args[12].value == like.new.data_ptr() and args[3].value == mask.data_ptr()
    assert (vec.depth_map(like=field).gx, vec.depth_map(like=field).gz) == (field.gx, field.gz)
    # refusals: every argument of depth_window and depth_map ...
    four = MiniWorldVecEnv("MiniWorld-FourRooms-v0", 2, want_depth=True)
    large = MiniWorldVecEnv("MiniWorld-Hallway-v0", 2, want_depth=True, obs_width=320, obs_height=240)
    n0 = len(lib.calls)
    nan, inf = float("nan"), float("inf")
    sensor = (dict(min_range=0.0), dict(min_range=-1.0), dict(min_range=nan), dict(min_range=inf), dict(max_range=0.0), dict(max_range=inf), dict(max_range=nan),
              dict(max_range=True), dict(min_range=3.0, max_range=2.0), dict(floor_tol=-0.1), dict(floor_tol=nan), dict(floor_tol=inf), dict(top=-1.0),
              dict(top=nan), dict(top=inf), dict(floor_tol=0.5, top=0.4), dict(top="high"))
    for kw in (dict(size=0), dict(size=129), dict(size=9.0), dict(size=True), dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(cell=inf), dict(cell="a"),
               dict(anchor="top"), dict(frame="east"), dict(frame=None)) + sensor:
        with pytest.raises(ValueError):
            vec.depth_window(**kw)
    for kw in (dict(cell=0.0), dict(cell=nan), dict(cell=0.01), dict(like=w), dict(like=field, cell=0.5), dict(min_points=0), dict(min_points=256),
               dict(min_points=1.0), dict(min_points=True)) + sensor:
        with pytest.raises(ValueError):
            vec.depth_map(**kw)
    with pytest.raises(ValueError, match="use a larger cell"):
        four.depth_map(cell=0.1)         # 28 900 cells: a nav grid, too many here
    # a frame of more than 65535 pixels: a cell's two counts share a 32-bit word in the kernel
    for make in (large.depth_window, large.depth_map):
        with pytest.raises(ValueError, match="65535"):
            make()
    # ... and of the updates
    for kw in (dict(depth=mine[:4]), dict(depth=mine.double()), dict(depth=mine.numpy()), dict(depth=torch.ones((5, 60, 160))[:, :, ::2]),
               dict(depth=torch.ones((5, 80, 60))), dict(mask=[1, 0, 0, 1, 0]), dict(mask=mask[:4]), dict(mask=mask.float())):
        with pytest.raises(ValueError):
            vec.depth_update(w, **kw)
        with pytest.raises(ValueError):
            vec.depth_map_update(m, **kw)
    with pytest.raises(ValueError):
        vec.depth_map_update(m, clear=mask.float())
    for bad in (None, w.planes, m):
        with pytest.raises(ValueError):
            vec.depth_update(bad)
    for bad in (None, m.map, w):
        with pytest.raises(ValueError):
            vec.depth_map_update(bad)

    def broken(of, **kw):
        b = DepthWindow(of.planes, of.size, of.cell, of.back, of.frame, of.min_range, of.max_range, of.floor_tol, of.top)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    wide = torch.zeros((5, 2, 33, 34), dtype=torch.uint8)
    for b in (broken(w, planes=w.planes.to(torch.int8)), broken(w, planes=w.planes[:4]), broken(w, planes=w.planes[:, :1]), broken(w, planes=wide[:, :, :, :33]),
              broken(w, planes=None), broken(w, size=32)):
        with pytest.raises(engine.EngineError):
            vec.depth_update(b)
    for name, value in (("map", m.map[:, :, :-1]), ("map", m.map.to(torch.int8)), ("count", m.count[:, :1]), ("count", m.count.long()), ("new", m.new[:4])):
        b = DepthMap(m.map, m.count, m.new, m.params, 1, 0.05, 8.0, 0.1, 1.6)
        setattr(b, name, value)
        with pytest.raises(engine.EngineError):
            vec.depth_map_update(b)
    assert len(lib.calls) == n0         # nothing reached the library


def test_adapter_is_off_by_default_and_reports_the_window_when_asked(monkeypatch):
    import torch
    from miniworld_amd.vector import MiniWorldVectorEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    plain = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2)
    _, info = plain.reset(seed=0)
    _, _, _, _, info2 = plain.step(torch.zeros(2, dtype=torch.int32))
    assert plain.depth_win is None and "depth_map" not in info and "depth_map" not in info2 and plain.vec.depth is None
    assert "mw_depth_project" not in [c[0] for c in lib.calls]
    for bad in (True, 9, [("size", 9)]):
        with pytest.raises(ValueError):
            MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, depth_map=bad)
    with pytest.raises(ValueError, match="want_depth"):
        MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, depth_map={}, want_depth=False)
    n0 = len(lib.calls)
    envs = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, depth_map=dict(size=9, max_range=4.0))
    assert envs.vec.want_depth and envs.vec.depth is not None
    _, info = envs.reset(seed=0)
    assert envs.depth_win.size == 9 and set(info) == {"depth_map"}
    _, _, _, _, info = envs.step(torch.zeros(2, dtype=torch.int32))
    assert info["depth_map"].dtype == torch.uint8 and tuple(info["depth_map"].shape) == (2, 2, 9, 9) and info["depth_map"] is not envs.depth_win.planes
    assert len([c for c in lib.calls[n0:] if c[0] == "mw_depth_project"]) == 2        # one behind the reset, one behind the step
