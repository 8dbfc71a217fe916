"""Egocentric map windows (mw_ego_map; MiniWorldVecEnv.ego_window / ego_update) without a GPU.

The phases the kernel runs (miniworld_amd/csrc/mw_ego.h) run on the host with (lane, stride) = (0, 1) in a program of its own
(tests/hostcheck/ego_map.cpp), built with the address and undefined-behaviour sanitizers, on worlds the host classes generate; its
planes and samples over a short scripted walk are compared, exactly, with the restatement of tests/ego_reference.py.  The properties
of the definition are asserted on both alike.  Beside that: the ABI names, the launch arithmetic, the refusals of the binding over a
stub engine and the library call of one ego_update."""
import math
import os
import re

import numpy as np
import pytest

import ego_reference as ref
import nav_reference as nav
import seen_reference as seen_ref
from helpers import stub_engine
from query_checks import (CSRC, ROOT, build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, host_world, launch_of as _policy,
                          run, walk as _walk, world_lines)

CELL = 0.25
FOV = 2.0 * math.atan(math.tan(math.radians(60.0) / 2.0) * 80.0 / 60.0)        # the default camera's horizontal field of view
ENTITIES, NORTH = 1, 2
ALL = ref.WALL | ref.ENTITY | ref.VISIBLE


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("ego_map", tmp_path_factory.mktemp("ego_map"))


def _window(size=9, cell=CELL, anchor="centre", north=False, planes=ALL, wall_radius=CELL / 2, entity_pad=CELL / 2, max_range=10.0, cos_half=None,
            entities=False):
    return dict(size=size, cell=cell, back=size / 2 if anchor == "bottom" else 0.0, north=north, planes=planes, wall_radius=wall_radius,
                entity_pad=entity_pad, max_range=max_range, cos_half=math.cos(FOV / 2) if cos_half is None else cos_half, entities=entities)


def _step(pose, carry=-1, mask=1, origin=None):
    return (pose[0], pose[1], pose[2], carry, mask, origin)


def _run(program, tmp_path, w, win, steps, src=None, src_cell=CELL, fill=0, garbage=0):
    """steps: (x, z, dir, carry, mask, origin or None) -> per step (uint8[P, S, S], the sample [S, S] or None) of the host build"""
    S, P = win["size"], bin(win["planes"]).count("1")
    flags = (ENTITIES if win["entities"] else 0) | (NORTH if win["north"] else 0)
    lines = [f"{S} {float(win['cell'])!r} {float(win['back'])!r} {float(win['wall_radius'])!r} {float(win['entity_pad'])!r} {win['planes']} {flags}",
             f"{float(win['max_range'])!r} {float(win['cos_half'])!r}"]
    if src is None:
        lines.append("0 1.0 1 1 0")
    else:
        lines.append(f"{src.dtype.itemsize} {float(src_cell)!r} {src.shape[1]} {src.shape[0]} {int(fill)}")
        lines.append(" ".join(str(int(v)) for v in src.ravel()))
    lines += [str(garbage)] + world_lines(w)
    lines.append(str(len(steps)))
    for x, z, d, carry, mask, origin in steps:
        ox, oz = origin if origin is not None else (0.0, 0.0)
        lines.append(f"{float(x)!r} {float(z)!r} {float(d)!r} {int(carry)} {int(mask)} {int(origin is not None)} {float(ox)!r} {float(oz)!r}")
    rows = run(program, tmp_path / "world.txt", lines, blank=True)
    assert len(rows) == 2 * len(steps)
    out = []
    for k in range(len(steps)):
        planes = np.zeros((0, S, S), np.uint8) if P == 0 else np.array(rows[2 * k].split(), np.uint8).reshape(P, S, S)
        out.append((planes, None if src is None else np.array(rows[2 * k + 1].split(), np.int64).astype(src.dtype).reshape(S, S)))
    return out


def _reference(w, win, steps, src=None, src_cell=CELL, fill=0, garbage=0):
    """the same walk through the restatement; a masked-off step keeps what the buffers held"""
    S, P = win["size"], bin(win["planes"]).count("1")
    planes = np.full((P, S, S), garbage, np.uint8)
    sample = None if src is None else np.full((S, S), garbage * (0x101 if src.dtype == np.uint16 else 1), src.dtype)
    out = []
    for x, z, d, carry, mask, origin in steps:
        if mask:
            planes, sample = ref.window(dict(w, carry=carry), (x, z, d), S, win["cell"], win["back"], win["north"], win["planes"], win["wall_radius"],
                                        win["entity_pad"], win["max_range"], win["cos_half"], win["entities"], origin=origin, src=src, src_cell=src_cell,
                                        fill=fill)
        out.append((planes.copy(), None if sample is None else sample.copy()))
    return out


def _both(program, tmp_path, w, win, steps, **kw):
    return {"host": _run(program, tmp_path, w, win, steps, **kw), "restatement": _reference(w, win, steps, **kw)}


def _source(w, rng, dtype):
    """a grid of CELL metres over the extent with a different value in (nearly) every cell: a wrong index shows"""
    gx, gz = nav.grid_shape(w["extent"], CELL)
    return rng.integers(0, 0xFFFE if dtype == np.uint16 else 0xFF, (gz, gx)).astype(dtype)


# (class, seeds, entities): MazeS3's seeds are different floor plans; PickupObjects has entities, one of them carried for part of the walk
WORLDS = [("Hallway", (0,), False), ("FourRooms", (0,), False), ("MazeS3", (0, 1), False), ("PickupObjects", (0,), True)]
# S x anchor x frame in full; the source's dtype and the wall radius alternate so that every S meets all four pairs of them
SHAPES = [(S, anchor, north, (np.uint8, np.uint16)[k % 2], (0.0, CELL / 2)[(k // 2 + k) % 2])
          for S in (1, 2, 9, 33) for k, (anchor, north) in enumerate((a, n) for a in ("centre", "bottom") for n in (False, True))]


def test_the_shapes_cover_every_pairing():
    for S in (1, 2, 9, 33):
        mine = [s for s in SHAPES if s[0] == S]
        assert {(a, n) for _, a, n, _, _ in mine} == {(a, n) for a in ("centre", "bottom") for n in (False, True)}
        assert {(t, r) for _, _, _, t, r in mine} == {(t, r) for t in (np.uint8, np.uint16) for r in (0.0, CELL / 2)}


@pytest.mark.parametrize("cls_name,seeds,entities", WORLDS)
def test_walk_equals_the_restatement(program, tmp_path, cls_name, seeds, entities):
    rng = np.random.default_rng(3300)
    seen = {"wall": set(), "visible": set(), "outside_wall": 0, "fill": 0, "entity": 0, "carried": 0, "entity_blocks": 0}
    for seed in seeds:
        w = host_world(cls_name, seed)[2]
        ext = w["extent"]
        poses = _walk(w, rng, 11)
        # one slot carried for part of the walk, a masked-off step, an origin that is not the agent's, a pose in the extent's corner
        steps = [_step(p, carry=(0 if entities and 3 <= k < 8 else -1)) for k, p in enumerate(poses)]
        steps[6] = steps[6][:4] + (0, None)
        steps[9] = steps[9][:5] + ((poses[2][0] + 0.37, poses[2][1] - 0.21),)
        steps.append(_step((ext[0] + 0.3, ext[2] + 0.3, 2.2)))
        for S, anchor, north, dtype, wall_radius in SHAPES:
            win = _window(size=S, anchor=anchor, north=north, wall_radius=wall_radius, entities=entities)
            src = _source(w, rng, dtype)
            fill = 0xAB if dtype == np.uint8 else 0xFFFF
            got = _run(program, tmp_path, w, win, steps, src=src, fill=fill, garbage=0xCD)
            want = _reference(w, win, steps, src=src, fill=fill, garbage=0xCD)
            px_out = 0
            for k, ((planes, sample), (wplanes, wsample)) in enumerate(zip(got, want)):
                for p, name in enumerate(("wall", "entity", "visible")):
                    assert np.array_equal(planes[p], wplanes[p]), (seed, S, anchor, north, k, name, np.argwhere(planes[p] != wplanes[p])[:8].tolist())
                assert sample.dtype == wsample.dtype and np.array_equal(sample, wsample), (seed, S, anchor, north, k, "sample",
                                                                                           np.argwhere(sample != wsample)[:8].tolist())
                if steps[k][4]:
                    x, z, d, carry, _, origin = steps[k]
                    px, pz = ref.points((x, z, d), S, CELL, win["back"], north, origin)
                    outside = ~((px >= ext[0]) & (px <= ext[1]) & (pz >= ext[2]) & (pz <= ext[3]))
                    px_out += int(outside.sum())
                    assert (wplanes[0][outside] == 1).all()
                    seen["outside_wall"] += int(outside.sum())
                    seen["fill"] += int((wsample[outside] == fill).sum())
                    if carry >= 0:
                        seen["carried"] += 1
                        assert not (wplanes[1] == 1 + carry).any(), (seed, S, k, "the carried slot shows")
                seen["wall"] |= set(np.unique(wplanes[0]).tolist())
                seen["visible"] |= set(np.unique(wplanes[2]).tolist())
                seen["entity"] += int((wplanes[1] != 0).sum())
            if entities:
                walls_only = _reference(w, dict(win, entities=False), steps, src=src, fill=fill, garbage=0xCD)
                seen["entity_blocks"] += int(sum((a[0][2] != b[0][2]).sum() for a, b in zip(want, walls_only)))
            if S == 33:
                assert px_out > 0, "no window reached outside the extent"
    # what makes the comparison above worth something, asserted on the restatement alone
    assert seen["wall"] == {0, 1}, "the wall plane holds one value only"
    assert seen["outside_wall"] > 0 and seen["fill"] > 0
    if entities:
        assert seen["entity"] > 0 and seen["carried"] > 0, "no entity in any window"
        assert seen["entity_blocks"] > 0, "no entity ever stood in a line of sight"
    if cls_name == "MazeS3":
        assert seen["visible"] == {0, 1}


def test_a_nan_pose_and_a_masked_env(program, tmp_path):
    w = host_world("PickupObjects", 0)[2]
    rng = np.random.default_rng(3301)
    nan = float("nan")
    for dtype, fill in ((np.uint8, 0x5A), (np.uint16, 0xFFFF)):
        src = _source(w, rng, dtype)
        for north in (False, True):
            win = _window(size=9, north=north, entities=True)
            for bad in ((nan, 1.0, 0.0), (1.0, nan, 0.0), (nan, nan, nan)):
                for who, run in _both(program, tmp_path, w, win, [_step(bad)], src=src, fill=fill, garbage=0x77).items():
                    planes, sample = run[0]
                    assert (planes[0] == 1).all() and not planes[1].any() and not planes[2].any() and (sample == fill).all(), (who, north, bad)
            # ... and an origin of NaN under a sound agent
            for who, run in _both(program, tmp_path, w, win, [_step(w["agent"], origin=(nan, 0.5))], src=src, fill=fill, garbage=0x77).items():
                planes, sample = run[0]
                assert (planes[0] == 1).all() and not planes[1].any() and not planes[2].any() and (sample == fill).all(), (who, north)
            # a masked-off env's rows keep every byte, whatever they held
            for who, run in _both(program, tmp_path, w, win, [_step(w["agent"], mask=0)], src=src, fill=fill, garbage=0xAB).items():
                planes, sample = run[0]
                assert (planes == 0xAB).all() and (sample == (0xABAB if dtype == np.uint16 else 0xAB)).all(), (who, north)


@pytest.mark.parametrize("S", [9, 8])
def test_a_north_window_on_the_grid_is_the_plain_crop(program, tmp_path, S):
    """cell == the source's cell, the origin on a cell's centre (odd S) or corner (even S): the window's points are cell centres"""
    w = host_world("FourRooms", 0)[2]
    rng = np.random.default_rng(3302)
    ext = w["extent"]
    gx, gz = nav.grid_shape(ext, CELL)
    cx, cz = nav.centres(ext, CELL, gx, gz)
    max_range, cos_half = 3.0, -1.0
    for i0, j0, d in ((2, 3, 0.4), (gx - 2, gz - 3, 2.0), (gx // 2 + 3, gz // 2 - 5, -1.0)):      # two near the extent's corners: the crop is padded
        off = 0.5 if S % 2 else 0.0
        pose = (float(ext[0] + (i0 + off) * CELL), float(ext[2] + (j0 + off) * CELL), d)
        first_i, first_j = i0 - S // 2, j0 - S // 2         # the cell under point (0, 0)
        px, pz = ref.points(pose, S, CELL, 0.0, True)
        want_x = ext[0] + (np.arange(first_i, first_i + S, dtype=np.float64) + 0.5) * CELL
        want_z = ext[2] + (np.arange(first_j, first_j + S, dtype=np.float64) + 0.5) * CELL
        assert np.array_equal(px, want_x[None, :].repeat(S, 0)) and np.array_equal(pz, want_z[:, None].repeat(S, 1))       # exactly cell centres
        in_x, in_z = (want_x > ext[0]) & (np.arange(first_i, first_i + S) < gx), (want_z > ext[2]) & (np.arange(first_j, first_j + S) < gz)
        assert np.array_equal(want_x[in_x], cx[max(first_i, 0):first_i + S]) and np.array_equal(want_z[in_z], cz[max(first_j, 0):first_j + S])
        fresh = seen_ref.Map(gx, gz)
        seen_ref.update(fresh, dict(w, carry=-1), CELL, pose, max_range, cos_half, False)
        assert fresh.seen.any()
        for src, fill in ((_source(w, rng, np.uint16), 0xFFFF), (_source(w, rng, np.uint8), 0xEE), (fresh.seen, 0)):
            pad = S
            padded = np.full((gz + 2 * pad, gx + 2 * pad), fill, src.dtype)
            padded[pad:pad + gz, pad:pad + gx] = src
            crop = padded[first_j + pad:first_j + pad + S, first_i + pad:first_i + pad + S]
            assert (crop == fill).any() or (i0, j0) == (gx // 2 + 3, gz // 2 - 5)
            win = _window(size=S, north=True, planes=ref.VISIBLE, max_range=max_range, cos_half=cos_half)
            for who, run in _both(program, tmp_path, w, win, [_step(pose)], src=src, fill=fill).items():
                planes, sample = run[0]
                assert np.array_equal(sample, crop), (who, S, i0, j0, src.dtype)
                if src is fresh.seen:
                    # ... and what is visible now is the crop of a fresh seen map of the same range, fov and obstacles
                    assert np.array_equal(planes[0], crop), (who, S, i0, j0, np.argwhere(planes[0] != crop)[:8].tolist())
                    assert planes[0].any()


def test_heading_zero_is_the_north_window_turned(program, tmp_path):
    import pyoracle
    s, c = pyoracle.sincos(0.0)
    assert (c, s) == (1.0, 0.0)         # the engine's deterministic sin / cos at 0: the heading is exactly (1, -0)
    w = host_world("PickupObjects", 0)[2]
    x, z, _ = w["agent"]
    for S in (17, 8):          # (half a metre between points: the window reaches past the range and the cone)
        steps = [_step((x, z, 0.0)), _step((x + 0.3, z - 0.7, 0.0))]
        head = _both(program, tmp_path, w, _window(size=S, cell=0.5, entities=True, max_range=3.0), steps)
        north = _both(program, tmp_path, w, _window(size=S, cell=0.5, north=True, entities=True, max_range=3.0), steps)
        for who in head:
            for (h, _), (n, _) in zip(head[who], north[who]):
                for p in range(3):
                    assert all(h[p][r][c] == n[p][c][S - 1 - r] for r in range(S) for c in range(S)), (who, S, p)
                assert h[2].any() and not h[2].all()


# ---------------------------------------------------------------------------------------------------------------- the interface

def test_header_declares_the_entry_point_and_the_build_has_the_units():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    text = " ".join(re.sub(r"/\*.*?\*/", "", header, flags=re.S).split())
    proto = ("int mw_ego_map(mw_engine *e, const double *host_window , int32_t size, int32_t planes, int32_t flags, const uint8_t *d_mask, "
             "const double *d_pos , uint8_t *d_planes , const mw_nav_params *src_grid , const void *d_src , int32_t src_bytes , uint32_t fill, "
             "void *d_sample , void *stream);")
    assert proto in text
    for name, value in (("ENTITIES", 1), ("NORTH", 2), ("WALL", 1), ("ENTITY", 2), ("VISIBLE", 4), ("MAX_SIZE", 128)):
        assert re.search(rf"#define MW_EGO_{name} {value}\b", header) and getattr(engine, "EGO_" + name) == value, name
    assert re.search(r"#define MW_ABI_VERSION 4\b", header)
    assert header.index("---- explored-area maps") < header.index("---- egocentric map windows") < header.index("int mw_ego_map(")
    assert "mw_ego_map" in engine.SIGNATURES
    check_units_built("mw_ego.hip", "mw_engine_ego.hip")
    check_kernel("mw_ego_kernel", "mw_ego.hip")
    # the arithmetic is the shared one: the ego header defines no ray, wall or cone formula of its own
    ego_h = open(os.path.join(CSRC, "mw_ego.h")).read()
    for shared in ("mwnav::grid_of", "mwnav::seg_dist", "mwnav::segs_of", "mwnav::nsegs_of", "mwray::disc_of", "mwray::ray_of", "mwray::wall_of",
                   "mwseen::view_of", "mwseen::stage", "mwseen::free_line", "mwseen::in_cone"):
        assert shared in ego_h, shared
    code = re.sub(r"//[^\n]*", "", ego_h)
    for own in ("ray_seg", "ray_circle", "sincos", "cos_half *"):
        assert own not in code, own
    check_does_not_wait("mw_engine_ego.hip")


def test_library_exports_the_entry_point_and_refuses_a_null_engine():
    check_refuses_null_engine("mw_ego_map", None, 9, 1, 0, None, None, None, None, None, 0, 0, None, None)


def test_ego_launch_is_a_workgroup_per_env_and_refuses_what_lds_does_not_hold(program):
    src = open(os.path.join(CSRC, "mw_ego.h")).read()
    threads = int(re.search(r"#define MW_EGO_THREADS (\d+)", src).group(1))
    assert threads % 64 == 0

    def lds(segs, ents, planes):
        n = (48 * segs + 32 * ents if planes & ref.VISIBLE else 0) + (32 * segs if planes & ref.WALL else 0) + (32 * ents if planes & ref.ENTITY else 0)
        return -(-n // 16) * 16
    for n, segs, ents in ((1, 1, 1), (8, 4, 1), (1024, 256, 1), (67, 64, 35), (4096, 8, 8)):
        for planes in range(8):
            p = _policy(program, n, segs, ents, planes)
            assert p == {"grid": n, "threads": threads, "lds": lds(segs, ents, planes), "fits": 1}, (n, segs, ents, planes, p)
    assert _policy(program, 5, 256, 35, 0)["lds"] == 0
    # the boundary, per plane set: the bytes per segment against 64 KiB
    for planes, per_seg, per_ent in ((ref.WALL, 32, 0), (ref.VISIBLE, 48, 32), (ALL, 80, 64)):
        most = (64 * 1024 - per_ent) // per_seg
        assert _policy(program, 3, most, 1, planes)["fits"] == 1 and _policy(program, 3, most, 1, planes)["lds"] <= 64 * 1024
        assert _policy(program, 3, most + 1, 1, planes)["fits"] == 0 and _policy(program, 3, most + 1, 1, planes)["lds"] > 64 * 1024


def test_vec_env_refusals_and_the_recorded_call(monkeypatch):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import EgoWindow, MiniWorldVecEnv, NavField
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    n0 = len(lib.calls)
    w = vec.ego_window()
    m = vec.seen_map()
    assert len(lib.calls) == n0         # a window is made without the library
    assert isinstance(w, EgoWindow) and (w.size, w.cell, w.back, w.frame, w.names) == (33, 0.25, 0.0, "heading", ("wall", "entity", "visible"))
    assert (w.wall_radius, w.entity_pad, w.max_range, w.cos_half, w.obstacles) == (0.125, 0.125, 10.0, math.cos(FOV / 2), "walls")
    assert w.planes.dtype == torch.uint8 and tuple(w.planes.shape) == (5, 3, 33, 33) and not w.planes.any()
    assert w.wall.data_ptr() == w.planes[:, 0].data_ptr() and w.entity.data_ptr() == w.planes[:, 1].data_ptr() and tuple(w.visible.shape) == (5, 33, 33)
    # the one library call of an ego_update
    assert vec.ego_update(w) is w.planes
    assert [c[0] for c in lib.calls[n0:]] == ["mw_ego_map"]
    args = lib.calls[-1][1]
    assert list(args[1]) == [0.25, 0.0, 0.125, 0.125, 10.0, math.cos(FOV / 2)] and tuple(args[2:5]) == (33, 7, 0)
    assert args[5] is None and args[6] is None and args[7].value == w.planes.data_ptr()
    assert args[8] is None and args[9] is None and tuple(args[10:12]) == (0, 0) and args[12] is None
    # a source, a mask, an origin; the bottom anchor, the north frame, two planes out of order, entities in the way
    w2 = vec.ego_window(size=8, cell=0.5, anchor="bottom", frame="north", planes=("visible", "wall"), wall_radius=0.0, entity_pad=0.3, max_range=3.0,
                        fov=2 * math.pi, obstacles="walls+entities")
    assert w2.names == ("wall", "visible") and w2.entity is None and w2.back == 4.0 and tuple(w2.planes.shape) == (5, 2, 8, 8)
    mask = torch.tensor([1, 1, 0, 1, 0], dtype=torch.uint8)
    pos = torch.zeros((5, 3), dtype=torch.float64)
    planes, sample = vec.ego_update(w2, source=m, mask=mask, pos=pos)
    assert planes is w2.planes and sample.dtype == torch.uint8 and tuple(sample.shape) == (5, 8, 8)
    args = lib.calls[-1][1]
    assert list(args[1]) == [0.5, 4.0, 0.0, 0.3, 3.0, -1.0] and tuple(args[2:5]) == (8, 5, engine.EGO_ENTITIES | engine.EGO_NORTH)
    assert args[5].value == mask.data_ptr() and args[6].value == pos.data_ptr() and args[7].value == w2.planes.data_ptr()
    p = args[8]._obj
    assert (p.cell, p.gx, p.gz) == (m.cell, m.gx, m.gz) and args[9].value == m.seen.data_ptr() and tuple(args[10:12]) == (1, 0)
    assert args[12].value == sample.data_ptr()
    assert vec.ego_update(w2, source=m)[1] is sample         # the sample is the env's own, reused
    # a nav field: two bytes, blocked outside; planes=() samples only
    field = NavField(torch.zeros((5, 7, 9), dtype=torch.uint16), engine.MwNavParams(0.4, 0.2, 0.0, 9, 7, 0, 0), 0, "walls")
    w3 = vec.ego_window(size=5, planes=())
    assert w3.planes is None and w3.names == () and w3.wall is None
    planes, sample = vec.ego_update(w3, source=field)
    args = lib.calls[-1][1]
    assert planes is None and sample.dtype == torch.uint16 and tuple(sample.shape) == (5, 5, 5)
    assert args[3] == 0 and args[7] is None and args[9].value == field.field.data_ptr() and tuple(args[10:12]) == (2, 0xFFFF)
    vec.ego_update(w3, source=field, fill=7)
    assert lib.calls[-1][1][11] == 7
    # refusals: every argument of ego_window ...
    n0 = len(lib.calls)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(size=0), dict(size=129), dict(size=9.0), dict(size=True), dict(size="9"), dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(cell=inf),
               dict(cell="a"), dict(cell=True), dict(anchor="top"), dict(anchor=0), dict(frame="east"), dict(frame=None), dict(planes="wall"),
               dict(planes=("wall", "wall")), dict(planes=("walls",)), dict(planes=(1,)), dict(planes=None), dict(wall_radius=-0.1), dict(wall_radius=nan),
               dict(wall_radius=inf), dict(wall_radius="r"), dict(entity_pad=-0.1), dict(entity_pad=nan), dict(entity_pad=inf), dict(max_range=0.0),
               dict(max_range=-1.0), dict(max_range=inf), dict(max_range=nan), dict(max_range=True), dict(fov=0.0), dict(fov=-1.0), dict(fov=7.0),
               dict(fov=nan), dict(fov="wide"), dict(obstacles="entities")):
        with pytest.raises(ValueError):
            vec.ego_window(**kw)
    # ... and of ego_update
    for kw in (dict(source=m.seen), dict(source="seen"), dict(fill=3), dict(source=m, fill=256), dict(source=m, fill=-1), dict(source=m, fill=1.0),
               dict(source=field, fill=0x10000), dict(source=m, fill=True), dict(mask=[1, 0, 0, 1, 0]), dict(mask=mask[:4]), dict(mask=mask.float()),
               dict(mask=torch.zeros((5, 1), dtype=torch.uint8)), dict(pos=pos[:4]), dict(pos=pos.float()), dict(pos=[[0.0] * 3] * 5),
               dict(pos=torch.zeros((5, 6), dtype=torch.float64)[:, ::2])):
        with pytest.raises(ValueError):
            vec.ego_update(w, **kw)
    for bad in (None, w.planes, m, {"planes": w.planes}):
        with pytest.raises(ValueError):
            vec.ego_update(bad)
    with pytest.raises(ValueError):
        vec.ego_update(w3)              # neither a plane nor a source

    def broken(of, **kw):
        b = EgoWindow(of.planes, of.names, of.size, of.cell, of.back, of.frame, of.wall_radius, of.entity_pad, of.max_range, of.cos_half, of.obstacles)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    wide = torch.zeros((5, 3, 33, 34), dtype=torch.uint8)
    for b in (broken(w, planes=w.planes.to(torch.int8)), broken(w, planes=w.planes[:4]), broken(w, planes=w.planes[:, :2]), broken(w, planes=w.planes.reshape(5, 3, -1)),
              broken(w, planes=wide[:, :, :, :33]), broken(w, planes=None), broken(w, size=32)):
        with pytest.raises(engine.EngineError):
            vec.ego_update(b)
    with pytest.raises(engine.EngineError):
        vec.ego_update(broken(w3, planes=w.planes), source=field)        # a tensor without planes to write
    small = vec.seen_map()
    small.seen = small.seen[:, :-1]
    other = vec.seen_map()
    other.seen = other.seen.to(torch.int16)
    for source in (small, other):
        with pytest.raises(engine.EngineError):
            vec.ego_update(w, source=source)
    strided = torch.zeros(10, dtype=torch.uint8)[::2]
    with pytest.raises(engine.EngineError):
        vec.ego_update(w, mask=strided)
    assert len(lib.calls) == n0         # nothing reached the library


def test_adapter_is_off_by_default_and_reports_the_window_when_asked(monkeypatch):
    import torch
    from miniworld_amd.vector import MiniWorldVectorEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    plain = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2)
    _, info = plain.reset(seed=0)
    assert "ego_map" not in info
    _, _, _, _, info = plain.step(torch.zeros(2, dtype=torch.int32))
    assert plain.ego is None and "ego_map" not in info
    assert "mw_ego_map" not in [c[0] for c in lib.calls]
    for bad in (True, 9, dict(planes=())):
        with pytest.raises(ValueError):
            MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, ego_map=bad)
    n0 = len(lib.calls)
    envs = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, ego_map=dict(size=9, planes=("wall", "visible")))
    _, info = envs.reset(seed=0)
    assert envs.ego.size == 9 and set(info) == {"ego_map"}
    _, _, _, _, info = envs.step(torch.zeros(2, dtype=torch.int32))
    assert info["ego_map"].dtype == torch.uint8 and tuple(info["ego_map"].shape) == (2, 2, 9, 9) and info["ego_map"] is not envs.ego.planes
    assert len([c for c in lib.calls[n0:] if c[0] == "mw_ego_map"]) == 2        # one behind the reset, one behind the step
