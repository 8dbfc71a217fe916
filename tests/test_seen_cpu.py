"""Explored-area maps (mw_seen_update; MiniWorldVecEnv.seen_map / seen_update) without a GPU.

The phases the kernel runs (miniworld_amd/csrc/mw_seen.h) run on the host with (lane, stride) = (0, 1) in a program of its own
(tests/hostcheck/seen_map.cpp), built with the address and undefined-behaviour sanitizers, on worlds the host classes generate; its
maps, `new` and `count` over a short scripted walk are compared, exactly, with the restatement of tests/seen_reference.py.  The
properties of the definition are asserted on both alike.  Beside that: the ABI names, the launch arithmetic, the refusals of the
binding over a stub engine and the library call of one seen_update."""
import math
import os
import re

import numpy as np
import pytest

import nav_reference as nav
import seen_reference as ref
from helpers import stub_engine
from query_checks import (CSRC, ROOT, build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, host_world, launch_of as _policy,
                          run, walk as _walk, world_lines)

CELL = 0.25
FOV = 2.0 * math.atan(math.tan(math.radians(60.0) / 2.0) * 80.0 / 60.0)        # the default camera's horizontal field of view


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("seen_map", tmp_path_factory.mktemp("seen_map"))


def _run(program, tmp_path, w, gx, gz, max_range, cos_half, flags, steps, fill=0, count=0, new=0, cell=CELL):
    """steps: (x, z, dir, carry, clear, mask) -> per step (covered, new, count, uint8[gz, gx])"""
    lines = [f"{float(cell)!r} {gx} {gz}", f"{float(max_range)!r} {float(cos_half)!r} {flags}", f"{fill} {count} {new}"] + world_lines(w)
    lines.append(str(len(steps)))
    lines += [f"{float(x)!r} {float(z)!r} {float(d)!r} {int(carry)} {int(clear)} {int(mask)}" for x, z, d, carry, clear, mask in steps]
    rows = [line.split() for line in run(program, tmp_path / "world.txt", lines)]
    assert len(rows) == 2 * len(steps)
    return [(int(rows[2 * k][0]), int(rows[2 * k][1]), int(rows[2 * k][2]), np.array(rows[2 * k + 1], np.uint8).reshape(gz, gx)) for k in range(len(steps))]


def _reference(w, gx, gz, max_range, cos_half, entities, steps, fill=0, count=0, new=0, cell=CELL):
    m = ref.Map(gx, gz, fill, count, new)
    out = []
    for x, z, d, carry, clear, mask in steps:
        cands = ref.update(m, dict(w, carry=carry), cell, (x, z, d), max_range, cos_half, entities, clear=bool(clear), mask=bool(mask))
        out.append((cands, m.new, m.count, m.seen.copy()))
    return out


# (class, seeds, entities): MazeS3's seeds are different floor plans; PickupObjects has entities, one of them carried for part of the walk
WORLDS = [("Hallway", (0,), False), ("FourRooms", (0,), False), ("MazeS3", (0, 1), False), ("PickupObjects", (0,), True)]


@pytest.mark.parametrize("cls_name,seeds,entities", WORLDS)
def test_walk_equals_the_restatement(program, tmp_path, cls_name, seeds, entities):
    rng = np.random.default_rng(3100)
    blocked_by_entity = 0
    for seed in seeds:
        w = host_world(cls_name, seed)[2]
        gx, gz = ref.grid_shape(w["extent"], CELL)
        poses = _walk(w, rng, 12)
        # a clear in the middle, a masked-off step (with a clear that must not happen), a pose on a cell's centre (dist == 0)
        steps = [(x, z, d, (0 if entities and 4 <= k < 9 else -1), int(k == 6), 1) for k, (x, z, d) in enumerate(poses)]
        steps[8] = steps[8][:4] + (1, 0)
        steps.append((w["extent"][0] + 4.5 * CELL, w["extent"][2] + 3.5 * CELL, 0.3, -1, 0, 1))
        for max_range, fov in ((10.0, FOV), (3.0, 2 * math.pi), (30.0, 0.05)):
            got = _run(program, tmp_path, w, gx, gz, max_range, ref.cos_half_of(fov), int(entities), steps)
            want = _reference(w, gx, gz, max_range, ref.cos_half_of(fov), entities, steps)
            for k, ((covered, new, count, seen), (_, wnew, wcount, wseen)) in enumerate(zip(got, want)):
                assert covered == 1
                assert np.array_equal(seen, wseen), (seed, max_range, fov, k, "cells that differ", np.argwhere(seen != wseen)[:8].tolist())
                assert (new, count) == (wnew, wcount), (seed, max_range, fov, k)
            assert got[-1][2] > 0
            if entities:
                walls_only = _reference(w, gx, gz, max_range, ref.cos_half_of(fov), False, steps)
                blocked_by_entity += int(sum((a[3] != b[3]).sum() for a, b in zip(want, walls_only)))
    if entities:
        assert blocked_by_entity, "no entity ever stood in a line of sight"


def _both(program, tmp_path, w, gx, gz, max_range, cos_half, entities, steps, **kw):
    """the host build's and the restatement's (new, count, map) per step"""
    host = [(n, c, m) for _, n, c, m in _run(program, tmp_path, w, gx, gz, max_range, cos_half, int(entities), steps, **kw)]
    rest = [(n, c, m) for _, n, c, m in _reference(w, gx, gz, max_range, cos_half, entities, steps, **kw)]
    return {"host": host, "restatement": rest}


def test_properties_hold_on_the_restatement_and_the_host_build(program, tmp_path):
    rng = np.random.default_rng(3101)
    w = host_world("FourRooms", 0)[2]
    gx, gz = ref.grid_shape(w["extent"], CELL)
    poses = _walk(w, rng, 10)
    plain = [(x, z, d, -1, 0, 1) for x, z, d in poses]
    for who, run in _both(program, tmp_path, w, gx, gz, 4.0, ref.cos_half_of(FOV), False, plain).items():
        total = 0
        for k, (new, count, seen) in enumerate(run):
            total += new
            assert total == count == int(seen.sum()), (who, k)                  # sum(new) == count == map.sum()
            assert set(np.unique(seen)) <= {0, 1}
            if k:
                assert (seen >= run[k - 1][2]).all(), (who, k)                  # monotone: a seen cell stays seen
        assert total > 0
        # every visible cell lies within range: the first step's cells, by the cell centres
        x, z, _ = poses[0]
        cx, cz = nav.centres(w["extent"], CELL, gx, gz)
        dist = np.hypot(cx[None, :] - x, cz[:, None] - z)
        assert (dist[run[0][2] == 1] <= 4.0).all() and (run[0][2] == 1).any(), who
    # all round is a superset of any cone
    for fov in (0.05, 1.0, FOV, 6.0):
        cone = _both(program, tmp_path, w, gx, gz, 4.0, ref.cos_half_of(fov), False, plain[:3])
        full = _both(program, tmp_path, w, gx, gz, 4.0, -1.0, False, plain[:3])
        for who in cone:
            for (_, _, a), (_, _, b) in zip(cone[who], full[who]):
                assert (b >= a).all() and (b.sum() > a.sum() or fov > FOV), (who, fov)
    # clear gives count == new; the mask wins over clear: nothing of a masked-off env moves, whatever it held
    steps = [plain[0], plain[5], plain[9][:4] + (1, 1), plain[2][:4] + (1, 0)]
    for who, run in _both(program, tmp_path, w, gx, gz, 4.0, -1.0, False, steps).items():
        assert run[2][0] == run[2][1] == int(run[2][2].sum()) > 0, who
        assert run[3][0] == run[2][0] and run[3][1] == run[2][1] and np.array_equal(run[3][2], run[2][2]), who
    garbage = _both(program, tmp_path, w, gx, gz, 4.0, -1.0, False, [plain[0][:4] + (1, 0)], fill=0xAB, count=-77, new=-78)
    for who, run in garbage.items():
        assert (run[0][0], run[0][1]) == (-78, -77) and (run[0][2] == 0xAB).all(), who
    # a NaN pose marks nothing
    nan = float("nan")
    for bad in ((nan, 1.0, 0.0), (1.0, nan, 0.0), (nan, nan, nan)):
        for who, run in _both(program, tmp_path, w, gx, gz, 4.0, -1.0, False, [bad + (-1, 0, 1)]).items():
            assert run[0][0] == run[0][1] == 0 and not run[0][2].any(), (who, bad)
    # ... and a NaN heading only the agent's own cell centre, if it stands on one (dist == 0), under a cone
    for who, run in _both(program, tmp_path, w, gx, gz, 4.0, 0.5, False, [(poses[0][0], poses[0][1], nan, -1, 0, 1)]).items():
        assert run[0][0] == 0, who


def test_a_grid_that_does_not_cover_the_extent_is_refused(program, tmp_path):
    w = host_world("Hallway", 0)[2]
    gx, gz = ref.grid_shape(w["extent"], CELL)
    step = [w["agent"] + (-1, 0, 1)]
    got = _run(program, tmp_path, w, gx - 2, gz, 5.0, -1.0, 0, step, fill=1, count=9, new=9)
    want = _reference(w, gx - 2, gz, 5.0, -1.0, False, step, fill=1, count=9, new=9)
    assert got[0][0] == 0 and want[0][0] == -1
    assert (got[0][1], got[0][2]) == (want[0][1], want[0][2]) == (0, 0) and not got[0][3].any() and not want[0][3].any()


# ---------------------------------------------------------------------------------------------------------------- the interface

def test_header_declares_the_entry_point_and_the_build_has_the_units():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    text = " ".join(header.split())
    proto = ("int mw_seen_update(mw_engine *e, const mw_nav_params *grid /* cell, gx, gz are read; the rest is ignored */, const double *host_sight "
             "/* [2] on the host, read during the call: range in metres, cos(fov / 2) or -1 */, int32_t flags, const uint8_t *d_mask, const uint8_t "
             "*d_clear, uint8_t *d_seen, int32_t *d_count, int32_t *d_new /* or NULL */, void *stream);")
    assert proto in text
    assert re.search(r"#define MW_SEEN_ENTITIES 1\b", header) and engine.SEEN_ENTITIES == 1
    assert re.search(r"#define MW_ABI_VERSION 4\b", header)
    check_units_built("mw_seen.hip", "mw_engine_seen.hip")
    check_kernel("mw_seen_kernel", "mw_seen.hip")
    # the arithmetic is the shared one: the seen header defines no ray or grid formula of its own
    seen_h = open(os.path.join(CSRC, "mw_seen.h")).read()
    for shared in ("mwray::ray_of", "mwray::wall_of", "mwray::disc_of", "mwray::ray_wall", "mwray::ray_circle", "mwray::take", "mwnav::grid_of",
                   "mwnav::centre", "mwnav::beyond", "mwnav::covers", "mwnav::box_of"):
        assert shared in seen_h, shared
    check_does_not_wait("mw_engine_seen.hip")


def test_library_exports_the_entry_point_and_refuses_a_null_engine():
    from miniworld_amd import engine
    check_refuses_null_engine("mw_seen_update", engine.MwNavParams(0.25, 0.0, 0.0, 4, 4, 0, 0), None, 0, None, None, None, None, None, None)


def test_seen_launch_is_a_workgroup_per_env_and_refuses_what_lds_does_not_hold(program):
    src = open(os.path.join(CSRC, "mw_seen.h")).read()
    threads = int(re.search(r"#define MW_SEEN_THREADS (\d+)", src).group(1))
    cands = int(re.search(r"#define MW_SEEN_CANDS (\d+)", src).group(1))
    assert threads % 64 == 0 and cands % threads == 0
    tail = 2 * cands + 16
    for n, segs, ents in ((1, 1, 1), (8, 4, 1), (1024, 256, 1), (67, 64, 35), (4096, 8, 8)):
        p = _policy(program, n, segs, ents)
        assert p == {"grid": n, "threads": threads, "lds": -(-(48 * segs + 32 * ents) // 16) * 16 + tail, "fits": 1}, (n, segs, ents, p)
    # the boundary: 48 bytes per segment, 32 per slot and the tail against 64 KiB
    most = (64 * 1024 - tail - 32) // 48
    assert _policy(program, 3, most, 1)["fits"] == 1 and _policy(program, 3, most, 1)["lds"] <= 64 * 1024
    assert _policy(program, 3, most + 1, 1)["fits"] == 0 and _policy(program, 3, most + 1, 1)["lds"] > 64 * 1024


def test_vec_env_refusals_and_the_recorded_call(monkeypatch):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import MiniWorldVecEnv, NavField, SeenMap
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    t = vec.template
    gx, gz = ref.grid_shape((t.min_x, t.max_x, t.min_z, t.max_z), 0.25)
    n0 = len(lib.calls)
    m = vec.seen_map()
    assert len(lib.calls) == n0         # a map is made without the library
    assert isinstance(m, SeenMap) and (m.cell, m.gx, m.gz) == (0.25, gx, gz) and m.max_range == 10.0 and m.obstacles == "walls"
    assert m.seen.dtype == torch.uint8 and tuple(m.seen.shape) == (5, gz, gx) and not m.seen.any()
    assert m.count.dtype == m.new.dtype == torch.int32 and tuple(m.count.shape) == tuple(m.new.shape) == (5,)
    assert m.cos_half == math.cos(FOV / 2) and vec.default_fov() == FOV          # the default camera's horizontal field of view
    assert "horizontal field of view of the default camera" in " ".join(MiniWorldVecEnv.seen_map.__doc__.split())
    assert vec.seen_map(fov=2 * math.pi).cos_half == -1.0 and vec.seen_map(fov=1.0).cos_half == math.cos(0.5)
    # the one library call of a seen_update
    assert vec.seen_update(m) is m.new
    assert [c[0] for c in lib.calls[n0:]] == ["mw_seen_update"]
    args = lib.calls[-1][1]
    p = args[1]._obj
    assert (p.cell, p.gx, p.gz) == (0.25, gx, gz) and list(args[2]) == [10.0, math.cos(FOV / 2)] and args[3] == 0
    assert args[4] is None and args[5] is None
    assert args[6].value == m.seen.data_ptr() and args[7].value == m.count.data_ptr() and args[8].value == m.new.data_ptr()
    done = torch.tensor([1, 0, 0, 1, 0], dtype=torch.uint8)
    mask = torch.tensor([1, 1, 0, 1, 0], dtype=torch.uint8)
    m2 = vec.seen_map(cell=0.5, max_range=3.0, fov=2 * math.pi, obstacles="walls+entities")
    vec.seen_update(m2, clear=done, mask=mask)
    args = lib.calls[-1][1]
    assert (args[1]._obj.cell, list(args[2]), args[3]) == (0.5, [3.0, -1.0], engine.SEEN_ENTITIES)
    assert args[4].value == mask.data_ptr() and args[5].value == done.data_ptr() and args[6].value == m2.seen.data_ptr()
    vec.seen_update(m2, clear=done.bool(), mask=mask.bool())             # booleans are copied over as bytes
    args = lib.calls[-1][1]
    assert args[4].value not in (None, mask.data_ptr()) and args[5].value not in (None, done.data_ptr())
    # like=: the grid of a nav field
    field = NavField(torch.zeros((5, 7, 9), dtype=torch.uint16), engine.MwNavParams(0.4, 0.2, 0.0, 9, 7, 0, 0), 0, "walls")
    m3 = vec.seen_map(like=field)
    assert (m3.cell, m3.gx, m3.gz) == (0.4, 9, 7) and tuple(m3.seen.shape) == (5, 7, 9)
    # refusals: every argument of seen_map ...
    n0 = len(lib.calls)
    for kw in (dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")), dict(cell="a"), dict(cell=0.001),
               dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=float("inf")), dict(max_range=float("nan")), dict(max_range=True),
               dict(fov=0.0), dict(fov=-1.0), dict(fov=7.0), dict(fov=float("nan")), dict(fov="wide"), dict(obstacles="entities"),
               dict(like=m), dict(like=field.field), dict(like=field, cell=0.5)):
        with pytest.raises(ValueError):
            vec.seen_map(**kw)
    # ... and every tensor of seen_update
    for kw in (dict(clear=[1, 0, 0, 1, 0]), dict(clear=done[:4]), dict(clear=done.to(torch.int32)), dict(clear=done[None]),
               dict(mask=[1, 0, 0, 1, 0]), dict(mask=mask[:4]), dict(mask=mask.float()), dict(mask=torch.zeros((5, 1), dtype=torch.uint8))):
        with pytest.raises(ValueError):
            vec.seen_update(m, **kw)
    for bad in (None, m.seen, field, {"seen": m.seen}):
        with pytest.raises(ValueError):
            vec.seen_update(bad)

    def broken(**kw):
        b = SeenMap(m.seen, m.count, m.new, m.params, m.max_range, m.cos_half, m.obstacles)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    wide = torch.zeros((5, gz, gx + 1), dtype=torch.uint8)
    for b in (broken(seen=m.seen.to(torch.int8)), broken(seen=m.seen[:4]), broken(seen=m.seen.reshape(5, gx, gz)), broken(seen=m.seen.reshape(5, -1)),
              broken(seen=wide[:, :, :gx]), broken(seen=None), broken(count=m.count.to(torch.int64)), broken(count=m.count[:4]), broken(count=None),
              broken(new=m.new.to(torch.int64)), broken(new=torch.zeros(6, dtype=torch.int32)), broken(new=torch.zeros(10, dtype=torch.int32)[::2])):
        with pytest.raises(engine.EngineError):
            vec.seen_update(b)
    for strided in (torch.zeros(10, dtype=torch.uint8)[::2],):
        with pytest.raises(engine.EngineError):
            vec.seen_update(m, clear=strided)
        with pytest.raises(engine.EngineError):
            vec.seen_update(m, mask=strided)
    assert len(lib.calls) == n0         # nothing reached the library


def test_adapter_is_off_by_default_and_reports_the_counters_when_asked(monkeypatch):
    import torch
    from miniworld_amd.vector import MiniWorldVectorEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    plain = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2)
    plain.reset(seed=0)
    _, _, _, _, info = plain.step(torch.zeros(2, dtype=torch.int32))
    assert plain.seen is None and "seen_new" not in info and "seen_count" not in info
    assert "mw_seen_update" not in [c[0] for c in lib.calls]
    with pytest.raises(ValueError):
        MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, seen_map=True)
    n0 = len(lib.calls)
    envs = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, seen_map=dict(max_range=4.0))
    _, info = envs.reset(seed=0)
    assert envs.seen.max_range == 4.0 and set(info) == {"seen_new", "seen_count"}
    _, _, _, _, info = envs.step(torch.zeros(2, dtype=torch.int32))
    assert info["seen_new"].dtype == info["seen_count"].dtype == torch.int32 and info["seen_new"] is not envs.seen.new
    assert "final_info" not in info         # the counters are no family info: nothing of a finished episode to report
    calls = [c for c in lib.calls[n0:] if c[0] == "mw_seen_update"]
    assert len(calls) == 2 and calls[0][1][5] is not None and calls[1][1][5] is not None      # reset clears every env, a step the finished ones
