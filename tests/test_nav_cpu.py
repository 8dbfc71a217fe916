"""Navigation fields (mw_nav_build / mw_nav_query; MiniWorldVecEnv.nav_field / nav_query) without a GPU.

The arithmetic the kernels inline (miniworld_amd/csrc/mw_nav.h) runs on the host in a program of its own
(tests/hostcheck/nav_field.cpp), built with the address and undefined-behaviour sanitizers, on worlds the host classes generate; its
field and its query answers are compared, exactly, with the restatement of tests/nav_reference.py (numpy occupancy, heapq Dijkstra).
Beside that: the ABI names, the argument errors of the two vec-env methods over a stub engine, and the follower on the oracle's
dynamics."""
import math
import os
import re

import numpy as np
import pytest

import nav_reference as ref
from helpers import stub_engine
from query_checks import ROOT, build, check_kernel, check_refuses_null_engine, check_units_built, host_world, run, world_lines


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("nav_field", tmp_path_factory.mktemp("nav_field"))


def _host_world(cls_name, seed):
    """... and the slot of the box to go to"""
    env, sc, w = host_world(cls_name, seed)
    ents = [e for e in env.entities if e is not env.agent]
    return env, sc, w, ents.index(env.box) if hasattr(env, "box") else 0


def _run(program, tmp_path, w, cell, margin, flags, target, reach, shape, positions):
    gx, gz = shape
    slot = isinstance(target, int)
    lines = [f"{cell!r} {margin!r} {float(reach or 0.0)!r} {gx} {gz} {flags} {target if slot else 0}"] + world_lines(w, carry=True)
    lines.append("1 " + " ".join(repr(float(v)) for v in target) if not slot else "0")
    lines.append(str(len(positions)))
    lines += [f"{float(x)!r} {float(z)!r}" for x, z in positions]
    out = run(program, tmp_path / "world.txt", lines)
    head = out[0].split()
    assert head[0] == "field"
    f = np.array(out[1].split(), np.int64).astype(np.uint16).reshape(gz, gx)
    answers = []
    for line in out[2:2 + len(positions)]:
        c, n, wx, wz = line.split()
        answers.append((int(c), int(n), float.fromhex(wx), float.fromhex(wz)))
    return int(head[1]), f, answers, (int(head[2]), int(head[3]))


def _positions(rng, w, f, cell, n):
    """random positions: inside the extent, outside it on every side, and the centres of blocked cells"""
    ext = w["extent"]
    span = max(ext[1] - ext[0], ext[3] - ext[2])
    pos = [(rng.uniform(ext[0], ext[1]), rng.uniform(ext[2], ext[3])) for _ in range(n - 60)]
    pos += [(rng.uniform(ext[0] - span, ext[1] + span), rng.uniform(ext[2] - span, ext[3] + span)) for _ in range(30)]
    bj, bi = np.nonzero(f == ref.BLOCKED)
    for k in rng.integers(0, len(bj), 30):
        pos.append((ext[0] + (bi[k] + rng.uniform(0.05, 0.95)) * cell, ext[2] + (bj[k] + rng.uniform(0.05, 0.95)) * cell))
    return pos


def _check_world(program, tmp_path, w, cell, target, entities, rng, reach=None):
    shape = ref.grid_shape(w["extent"], cell)
    want = ref.field(w, cell, target, reach=reach, entities=entities)
    pos = _positions(rng, w, want, cell, 200)
    ok, got, answers, passes = _run(program, tmp_path, w, cell, cell / 2, 1 if entities else 0, target, reach, shape, pos)
    assert ok == 1
    assert got.shape == want.shape and np.array_equal(got, want), ("cells that differ", int((got != want).sum()))
    tx, tz, _ = ref.target_of(w, target, reach)
    seen = set()
    for (x, z), a in zip(pos, answers):
        q = ref.query(want, w["extent"], cell, (tx, tz), x, z)
        assert a == q, ((x, z), a, q)
        seen.add("none" if q[0] < 0 else "source" if q[0] == 0 else "way")
    return want, seen, passes


@pytest.mark.parametrize("cls_name", ["MazeS2", "FourRooms", "YMaze", "Sidewalk"])
@pytest.mark.parametrize("cell", [0.25, 0.5])
def test_field_and_query_equal_the_restatement(program, tmp_path, cls_name, cell):
    rng = np.random.default_rng(2100 + int(cell * 100))
    for seed in (0, 1):
        env, sc, w, goal = _host_world(cls_name, seed)
        f, seen, passes = _check_world(program, tmp_path, w, cell, goal, False, rng)
        assert (f == 0).any() and (f == ref.BLOCKED).any() and ((f > 0) & (f < ref.UNREACHED)).any()
        assert {"way", "none"} <= seen, seen
        # the agent's own cell is reached: the box can be walked to
        c, _, _, _ = ref.query(f, w["extent"], cell, (0.0, 0.0), float(sc["agent_pos"][0]), float(sc["agent_pos"][2]))
        assert c >= 0
    if cls_name == "Sidewalk" and cell == 0.25:
        assert f.shape == (640, 36)


@pytest.mark.parametrize("entities", [False, True])
def test_three_rooms_in_both_obstacle_modes(program, tmp_path, entities):
    rng = np.random.default_rng(2150)
    for seed in (0, 1):
        env, sc, w, goal = _host_world("ThreeRooms", seed)
        assert len(w["kind"]) > 1
        f, _, _ = _check_world(program, tmp_path, w, 0.25, goal, entities, rng)
        walls = ref.field(w, 0.25, goal, entities=False)
        assert ((f == ref.BLOCKED) & (walls != ref.BLOCKED)).any() == entities      # the other objects block cells, or nothing does


def test_point_targets_and_a_target_inside_a_wall(program, tmp_path):
    rng = np.random.default_rng(2160)
    env, sc, w, goal = _host_world("FourRooms", 0)
    ap = [float(v) for v in sc["agent_pos"]]
    f, seen, _ = _check_world(program, tmp_path, w, 0.25, (ap[0], 0.0, ap[2]), False, rng, reach=0.6)
    assert "source" in seen or (f == 0).any()
    # a point on a wall: no source, every unblocked cell unreached, and that is no error
    s = w["segs"][0]
    f, seen, _ = _check_world(program, tmp_path, w, 0.25, (float(s[0] + s[2]) / 2, 0.0, float(s[1] + s[3]) / 2), False, rng, reach=0.2)
    assert not (f < ref.UNREACHED).any() and seen == {"none"}


def test_a_grid_too_small_for_the_extent_is_refused(program, tmp_path):
    env, sc, w, goal = _host_world("FourRooms", 0)
    gx, gz = ref.grid_shape(w["extent"], 0.25)
    for shape in ((gx - 1, gz), (gx, gz - 1)):
        ok, f, answers, _ = _run(program, tmp_path, w, 0.25, 0.125, 0, goal, None, shape, [(0.0, 0.0)])
        assert ok == 0 and (f == ref.BLOCKED).all() and answers[0][:2] == (-1, -1)
    # ... and a grid that reaches past it is built: the cells beyond the extent are blocked
    ok, f, _, _ = _run(program, tmp_path, w, 0.25, 0.125, 0, goal, None, (gx + 2, gz + 3), [])
    assert ok == 1 and (f[:, gx:] == ref.BLOCKED).all() and (f[gz:, :] == ref.BLOCKED).all()
    assert np.array_equal(f[:gz, :gx], ref.field(w, 0.25, goal))


def test_a_cost_that_does_not_fit_is_refused(program, tmp_path):
    """a corridor of 2 x 16000 cells with the target at one end: the far end would cost 5 * 15999 > 0xFFFE"""
    n = 16000
    w = {"segs": np.array([[0.0, 0.0, 2.0, 0.0], [2.0, 0.0, 2.0, float(n)], [2.0, float(n), 0.0, float(n)], [0.0, float(n), 0.0, 0.0]]),
         "extent": np.array([0.0, 2.0, 0.0, float(n)]), "kind": np.zeros(1, np.int32), "pos": np.zeros((1, 3)), "radius": np.zeros(1), "carry": -1,
         "agent_radius": 0.1, "max_forward_step": 0.17}
    ok, f, _, _ = _run(program, tmp_path, w, 1.0, 0.0, 0, (1.0, 0.0, 0.5), 0.8, (2, n), [])
    assert ok == 0 and (f == ref.BLOCKED).all()
    ok, f, _, _ = _run(program, tmp_path, w, 1.0, 0.0, 0, (1.0, 0.0, 0.5), 0.8, (2, 13000), [])      # (refused: the extent)
    assert ok == 0
    w["extent"][3] = 13000.0
    # (the far wall moves with the extent)
    w["segs"] = np.array([[0.0, 0.0, 2.0, 0.0], [2.0, 0.0, 2.0, 13000.0], [2.0, 13000.0, 0.0, 13000.0], [0.0, 13000.0, 0.0, 0.0]])
    ok, f, _, _ = _run(program, tmp_path, w, 1.0, 0.0, 0, (1.0, 0.0, 0.5), 0.8, (2, 13000), [])
    assert ok == 1 and int(f.max()) == 5 * 12999 and int(f.min()) == 0


# ---------------------------------------------------------------------------------------------------------------- the interface

def test_header_declares_the_entry_points():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"int mw_nav_query\(mw_engine \*e, const mw_nav_params \*params, ", header)
    text = " ".join(header.split())
    for cite in ("intersect_circle_segs (math.py:30-62)", "near(ent) (miniworld.py:965-975)"):
        assert cite in text, cite
    struct = header[header.index("typedef struct mw_nav_params {"):header.index("} mw_nav_params;")]
    assert tuple(re.findall(r"(\w+);", struct.replace(", gz", "; gz"))) == tuple(n for n, _ in engine.MwNavParams._fields_)
    assert (engine.NAV_BLOCKED, engine.NAV_UNREACHED, engine.NAV_MAX_CELLS) == (0xFFFF, 0xFFFE, 32768)
    for k, v in (("MW_NAV_ENTITIES", engine.NAV_ENTITIES), ("MW_NAV_BLOCKED", "0xFFFF"), ("MW_NAV_UNREACHED", "0xFFFE"), ("MW_NAV_MAX_CELLS", 32768)):
        assert re.search(rf"#define {k} {v}\b", header), k
    check_units_built("mw_nav.hip")
    for k in ("mw_nav_build_kernel", "mw_nav_query_kernel"):
        check_kernel(k, "mw_nav.hip")


def test_library_exports_the_entry_points_and_refuses_a_null_engine():
    from miniworld_amd import engine
    p = engine.MwNavParams(0.25, 0.125, 0.0, 4, 4, 0, 0)
    check_refuses_null_engine("mw_nav_build", p, None, None, None, None)
    check_refuses_null_engine("mw_nav_query", p, None, None, None, None, None, None, None)


def test_vec_env_argument_errors_and_calls(monkeypatch):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import MiniWorldVecEnv, NavField
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    n0 = len(lib.calls)
    fld = vec.nav_field()
    assert [c[0] for c in lib.calls[n0:]] == ["mw_nav_build"]
    assert isinstance(fld, NavField) and fld.field.dtype == torch.uint16
    t = vec.template
    gx, gz = math.ceil((t.max_x - t.min_x) / 0.25), math.ceil((t.max_z - t.min_z) / 0.25)
    assert tuple(fld.field.shape) == (5, gz, gx) and (fld.gx, fld.gz, fld.cell, fld.margin) == (gx, gz, 0.25, 0.125)
    assert fld.target == int(vec.engine.cfg.goal_ent) and fld.points is None
    args = lib.calls[-1][1]
    assert args[2] is None and args[3] is None and args[4].value == fld.field.data_ptr()
    mask = torch.tensor([1, 0, 0, 1, 0], dtype=torch.uint8)
    assert vec.nav_field(into=fld, mask=mask) is fld
    args = lib.calls[-1][1]
    assert args[2].value == mask.data_ptr() and args[4].value == fld.field.data_ptr()
    assert vec.nav_field(into=fld, mask=mask.bool()) is fld
    pts = torch.zeros((5, 3), dtype=torch.float64)
    pf = vec.nav_field(target=pts, reach=0.5, cell=0.5, obstacles="walls+entities", margin=0.0)
    assert pf.points is pts and pf.params.flags == engine.NAV_ENTITIES and pf.params.reach == 0.5 and pf.margin == 0.0
    assert lib.calls[-1][1][3].value == pts.data_ptr()
    n0 = len(lib.calls)
    for kw in (dict(cell=0), dict(cell=-1.0), dict(cell=float("nan")), dict(obstacles="entities"), dict(margin=-0.1), dict(target=99), dict(target=-1),
               dict(target=1.5), dict(target=pts), dict(target=pts, reach=0.0), dict(target=pts.float(), reach=1.0), dict(target=pts[:4], reach=1.0),
               dict(reach=1.0), dict(cell=0.01), dict(mask=torch.zeros(4, dtype=torch.uint8)), dict(mask=torch.zeros(5)), dict(mask=[1, 0, 0, 0, 0]),
               dict(into=fld.field), dict(into=fld, cell=0.5), dict(into=fld, target=0)):
        with pytest.raises(ValueError):
            vec.nav_field(**kw)
    assert len(lib.calls) == n0         # nothing reached the library
    q = vec.nav_query(fld)
    assert [c[0] for c in lib.calls[n0:]] == ["mw_nav_query"]
    assert set(q) == {"cost", "next", "waypoint", "distance"}
    assert q["cost"].dtype == torch.int32 and q["next"].dtype == torch.int32 and tuple(q["waypoint"].shape) == (5, 2) and q["waypoint"].dtype == torch.float64
    assert q["distance"].dtype == torch.float32 and tuple(q["distance"].shape) == (5,)
    args = lib.calls[-1][1]
    assert args[2] is None and args[3].value == fld.field.data_ptr() and args[4] is None
    vec.nav_query(pf, pos=pts)
    args = lib.calls[-1][1]
    assert args[2].value == pts.data_ptr() and args[4].value == pts.data_ptr()
    for bad in (dict(field=fld.field), dict(field=fld, pos=pts.float()), dict(field=fld, pos=pts[:3]), dict(field=fld, pos=[[0, 0, 0]] * 5)):
        with pytest.raises(ValueError):
            vec.nav_query(**bad)
    assert "grid's metric" in MiniWorldVecEnv.nav_query.__doc__ and "Euclidean geodesic" in MiniWorldVecEnv.nav_query.__doc__
    # distance: cost * cell / 5, inf without a path
    b = vec._nav_bufs
    b["cost"].copy_(torch.tensor([0, 5, 7, -1, 1442], dtype=torch.int32))
    d = vec.nav_query(fld)["distance"]
    assert d.tolist() == [0.0, 0.25, np.float32(7 * 0.25 / 5), float("inf"), np.float32(1442 * 0.05)]


# ---------------------------------------------------------------------------------------------------------------- the follower

def test_follower_reaches_the_box_on_the_oracles_dynamics():
    """MazeS3, reset(seed=0 .. 15): the expert of examples/expert_nav.py — turn towards the waypoint, else forward — over the
    restatement's field and query, stepped by the oracle's dynamics with the env's default step sizes, reaches the box within
    max_episode_steps and is never blocked."""
    import pyoracle
    for seed in range(16):
        env, sc, w, goal = _host_world("MazeS3", seed)
        f = ref.field(w, 0.25, goal)
        tx, tz, _ = ref.target_of(w, goal, None)
        dyn = pyoracle.Dynamics(sc, pyoracle.TASK_GOTO, int(env.max_episode_steps), goal_ent=goal, num_objs=len(w["kind"]),
                                max_forward_step=w["max_forward_step"], agent_radius=w["agent_radius"])
        fwd, turn = float(env.params.get_max("forward_step")), float(env.params.get_max("turn_step"))
        done, steps = False, 0
        while not done and steps < int(env.max_episode_steps):
            p = [dyn.ag.pos[0], dyn.ag.pos[1], dyn.ag.pos[2]]
            c, _, wx, wz = ref.query(f, w["extent"], 0.25, (tx, tz), p[0], p[2])
            assert c >= 0, (seed, steps, p)
            a = ref.follow(p, dyn.ag.dir, wx, wz, math.radians(turn))
            rew, term, trunc = dyn.step(a, fwd, 0.0, turn)
            steps += 1
            if a == ref.FORWARD:
                assert (dyn.ag.pos[0], dyn.ag.pos[2]) != (p[0], p[2]), ("blocked move", seed, steps)
            done = term or trunc
        assert done and term and rew > 0, (seed, steps)
