"""Navigation fields on the GPU (mw_nav_build / mw_nav_query; MiniWorldVecEnv.nav_field / nav_query) against the restatement of
tests/nav_reference.py — numpy occupancy and heapq Dijkstra fed by engine.get_geometry(env) and engine.get_state() — bit for bit: the
fixed point is unique, so there are no tolerances.  The restatement itself asserts that no cell centre of a case lies within 1e-9 m of
a threshold and that no cost reaches 0xFFFE."""
import math
import os
import sys

import numpy as np
import pytest

import nav_reference as ref
from query_checks import vec_env as _vec

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))

pytestmark = pytest.mark.gpu
PICKUP = 4


def _want(vec, fld, envs=None, reach=None):
    """the restatement's field of the envs listed, from the host routes"""
    st = vec.engine.get_state()
    pts = None if fld.points is None else fld.points.cpu().numpy()
    out = {}
    for i in range(vec.num_envs) if envs is None else envs:
        w = ref.world_of_engine(vec.engine, st, i)
        tgt = fld.target if pts is None else tuple(pts[i])
        out[i] = ref.field(w, fld.cell, tgt, reach=fld.params.reach if pts is not None else None, entities=fld.obstacles == "walls+entities",
                           margin=fld.margin, shape=(fld.gx, fld.gz))
    return out, st


def _bits(t):
    """a uint16 tensor as int16, the same bits: the type every torch kernel knows"""
    return t.view(__import__("torch").int16)


def _got(fld):
    return _bits(fld.field).cpu().numpy().view(np.uint16)


def _assert_field(vec, fld, envs=None):
    want, st = _want(vec, fld, envs)
    got = _got(fld)
    for i, w in want.items():
        assert np.array_equal(got[i], w), (i, "cells that differ", int((got[i] != w).sum()))
    return want, st


def _nav_actions(vec, fld, torch):
    from expert_nav import expert
    st = vec.state(("agent_pos", "agent_dir"))
    q = vec.nav_query(fld)
    return expert(st["agent_pos"], st["agent_dir"], q["waypoint"], math.radians(float(vec.engine.cfg.turn_step.default))), q


@pytest.mark.parametrize("env_id,n,cell,shape", [
    ("MiniWorld-MazeS2-v0", 67, 0.25, None),            # per-env geometry: one full group of 64 envs and a partial one
    ("MiniWorld-FourRooms-v0", 5, 0.25, None),          # shared geometry
    ("MiniWorld-YMaze-v0", 3, 0.25, None),              # walls off the axes
    ("MiniWorld-Sidewalk-v0", 2, 0.25, (36, 640)),      # the largest grid: 23 040 cells
    ("MiniWorld-Maze-v0", 3, 0.25, (103, 103)),         # an odd width
    ("MiniWorld-Hallway-v0", 1, 1.0, (12, 4)),          # fewer cells than lanes
])
def test_field_equals_the_restatement(env_id, n, cell, shape):
    import torch
    vec = _vec(env_id, n)
    fld = vec.nav_field(cell=cell)
    if shape:
        assert (fld.gx, fld.gz) == shape
    first, _ = _assert_field(vec, fld)
    assert all((f == ref.BLOCKED).any() and (cell >= 1.0 or (f == 0).any()) for f in first.values())
    # the whole-grid passes reach the same fixed point as the sweeps
    jac = vec.nav_field(cell=cell)
    jac.params.flags |= 2
    vec.nav_field(into=jac)
    assert torch.equal(_bits(jac.field), _bits(fld.field))
    # 30 random steps under the auto-reset, then the field again
    g = torch.Generator(device="cuda").manual_seed(7)
    done_any = torch.zeros(n, dtype=torch.bool, device="cuda")
    for _ in range(30):
        _, _, term, trunc = vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
        done_any |= (term | trunc) != 0
    vec.nav_field(into=fld)
    _assert_field(vec, fld)
    # ... and steps of the expert, the field kept current by masked rebuilds, until an env has finished (its new world must show)
    for _ in range(800):
        if bool(done_any.any()):
            break
        act, _ = _nav_actions(vec, fld, torch)
        _, _, term, trunc = vec.step(act)
        done = (term | trunc) != 0
        vec.nav_field(into=fld, mask=done)
        done_any |= done
    assert bool(done_any.any()), "no env finished an episode"
    vec.nav_field(into=fld, mask=done_any)
    second, _ = _assert_field(vec, fld)
    i = int(done_any.nonzero()[0])
    assert not np.array_equal(first[i], second[i])
    vec.engine.check()
    vec.close()


def test_a_masked_build_writes_the_masked_rows_only():
    import torch
    n = 9
    vec = _vec("MiniWorld-MazeS2-v0", n)
    fld = vec.nav_field()
    bits = _bits(fld.field)
    full = bits.clone()
    pattern = torch.arange(bits.numel(), dtype=torch.int32, device="cuda").remainder(32000).to(torch.int16).reshape(bits.shape)
    for mask in ([1, 0, 0, 1, 0, 0, 0, 0, 1], [0] * 9, [1] * 9):
        m = torch.tensor(mask, dtype=torch.uint8, device="cuda")
        for mm in (m, m.bool()):
            bits.copy_(pattern)
            vec.nav_field(into=fld, mask=mm)
            for i in range(n):
                assert torch.equal(bits[i], full[i] if mask[i] else pattern[i]), (mask, i)
    vec.engine.check()
    vec.close()


def _fetch(vec, slot, torch, budget=260):
    """walks every env's agent to entity `slot` around the other entities and picks it up; returns the envs where that worked (an
    object too close to a wall cannot be picked up: the reference's pickup test meets the wall first)"""
    from expert_nav import expert, FORWARD
    fld = vec.nav_field(target=slot, obstacles="walls+entities")
    turn = math.radians(float(vec.engine.cfg.turn_step.default))
    got = torch.zeros(vec.num_envs, dtype=torch.bool, device="cuda")
    for t in range(budget):
        st = vec.state(("agent_pos", "agent_dir", "carrying", "ent_kind"))
        got |= (st["carrying"] == slot) | (st["ent_kind"][:, slot] == 0)
        if bool(got.all()):
            break
        q = vec.nav_query(fld)
        act = expert(st["agent_pos"], st["agent_dir"], q["waypoint"], turn)
        act = torch.where((q["cost"] == 0) & (act == FORWARD), PICKUP, act)      # at the object and facing it
        act = torch.where(got, 1, act).to(torch.int32)                             # (done: turn on the spot)
        vec.step(act)
        vec.nav_field(into=fld)     # the agent moved nothing but itself; a carried or removed object changes the other envs' cells
    st = vec.state(("carrying", "ent_kind"))
    got |= (st["carrying"] == slot) | (st["ent_kind"][:, slot] == 0)
    assert bool(got.any()), "the scripted fetch picked the object up in no env"
    return got.cpu().numpy()


@pytest.mark.parametrize("env_id", ["MiniWorld-ThreeRooms-v0", "MiniWorld-PutNext-v0"])
def test_entities_block_cells(env_id):
    vec = _vec(env_id, 4)
    walls = vec.nav_field(target=0)
    both = vec.nav_field(target=0, obstacles="walls+entities")
    _assert_field(vec, walls)
    _assert_field(vec, both)
    w, b = _got(walls), _got(both)
    assert ((b == ref.BLOCKED) & (w != ref.BLOCKED)).any() and not ((w == ref.BLOCKED) & (b != ref.BLOCKED)).any()
    vec.engine.check()
    vec.close()


def test_a_removed_object_does_not_block():
    import torch
    vec = _vec("MiniWorld-PickupObjects-v0", 4, autoreset=False)
    got = _fetch(vec, 0, torch)
    vec.step(torch.full((4,), 1, dtype=torch.int32, device="cuda"))       # (the frame's tail has taken the slot out of the list)
    st = vec.engine.get_state()
    assert (st["ent_kind"][got, 0] == 0).all()
    fld = vec.nav_field(target=1, obstacles="walls+entities")
    want, _ = _assert_field(vec, fld)
    # ... and the comparison would have seen it: with the slot still listed the restatement's field is another
    for i in np.nonzero(got)[0]:
        w = ref.world_of_engine(vec.engine, st, int(i))
        w["kind"] = w["kind"].copy()
        w["kind"][0] = 1
        assert not np.array_equal(ref.field(w, 0.25, 1, entities=True), want[int(i)])
    vec.engine.check()
    vec.close()


def test_a_carried_object_does_not_block():
    import torch
    vec = _vec("MiniWorld-PutNext-v0", 4, autoreset=False)
    got = _fetch(vec, 0, torch)
    st = vec.engine.get_state()
    assert (st["carrying"][got] == 0).all()
    fld = vec.nav_field(target=1, obstacles="walls+entities")
    want, _ = _assert_field(vec, fld)
    for i in np.nonzero(got)[0]:        # (with the carried slot blocking, the restatement's field is another)
        w = ref.world_of_engine(vec.engine, st, int(i))
        w["carry"] = -1
        assert not np.array_equal(ref.field(w, 0.25, 1, entities=True), want[int(i)])
    free = vec.nav_field(target=1)
    assert not np.array_equal(_got(fld), _got(free))        # the others still block
    vec.engine.check()
    vec.close()


def test_point_targets():
    import torch
    n = 4
    vec = _vec("MiniWorld-FourRooms-v0", n)
    st = vec.engine.get_state()
    _, segs = vec.engine.get_geometry(0)
    seg = np.asarray(segs, np.float64).reshape(-1, 4)[0]
    pts = st["agent_pos"].copy()
    pts[1] = [(seg[0] + seg[2]) / 2, 0.0, (seg[1] + seg[3]) / 2]        # inside a wall: nothing is reached, and that is no error
    pts[2] = [st["extent"][2][0] - 5.0, 0.0, st["extent"][2][2] - 5.0]   # outside the extent
    fld = vec.nav_field(target=torch.from_numpy(pts).cuda(), reach=0.45)
    want, _ = _assert_field(vec, fld)
    got = _got(fld)
    assert (got[0] == 0).any() and (got[3] == 0).any()
    for i in (1, 2):
        assert not (got[i] < ref.UNREACHED).any() and (got[i] == ref.UNREACHED).any()
    q = vec.nav_query(fld)
    assert q["cost"].tolist()[1:3] == [-1, -1] and q["distance"][1].item() == float("inf") and q["cost"][0].item() >= 0
    if q["cost"][0].item() == 0:
        assert q["waypoint"][0].tolist() == [pts[0][0], pts[0][2]]
    vec.engine.check()          # clean
    vec.close()


@pytest.mark.parametrize("env_id,n,obstacles", [("MiniWorld-MazeS2-v0", 5, "walls"), ("MiniWorld-YMaze-v0", 2, "walls"),
                                                ("MiniWorld-ThreeRooms-v0", 2, "walls+entities")])
def test_query_equals_the_restatement(env_id, n, obstacles):
    import torch
    vec = _vec(env_id, n)
    fld = vec.nav_field(target=0, obstacles=obstacles)
    want, st = _assert_field(vec, fld)
    cell, gx, gz = fld.cell, fld.gx, fld.gz

    def check(pos, q):
        cost, nxt, wp = q["cost"].cpu().numpy(), q["next"].cpu().numpy(), q["waypoint"].cpu().numpy()
        dist = q["distance"].cpu().numpy()
        classes = set()
        for i in range(n):
            t = st["ent_pos"][i][0]
            r = ref.query(want[i], st["extent"][i], cell, (float(t[0]), float(t[2])), float(pos[i][0]), float(pos[i][2]))
            assert (int(cost[i]), int(nxt[i]), float(wp[i][0]), float(wp[i][1])) == r, (i, pos[i], r)
            assert dist[i] == (np.float32(np.inf) if r[0] < 0 else np.float32(r[0]) * np.float32(cell / 5.0))
            classes.add("none" if r[0] < 0 else "source" if r[0] == 0 else "way")
        return classes
    check(st["agent_pos"], vec.nav_query(fld))
    # 64 chosen positions per env: cells of every class, the grid's corners, positions outside the extent on every side
    rng = np.random.default_rng(2170)
    classes, rounds = set(), []
    for k in range(64):
        pos = np.zeros((n, 3))
        for i in range(n):
            ext, f = st["extent"][i], want[i]
            if k < 4:
                jj, ii = ((0, 0), (0, gx - 1), (gz - 1, 0), (gz - 1, gx - 1))[k]
            elif k < 12:
                d = ((-3, 0), (3, 0), (0, -3), (0, 3), (-50, -50), (50, 50), (-0.01, 0), (0, -0.01))[k - 4]
                pos[i] = [(ext[0] if d[0] <= 0 else ext[1]) + d[0], 0.0, (ext[2] if d[1] <= 0 else ext[3]) + d[1]]
                continue
            else:
                cls = (f == 0, f == ref.BLOCKED, f == ref.UNREACHED, (f > 0) & (f < ref.UNREACHED))[k % 4]
                js, is_ = np.nonzero(cls if cls.any() else f == f)
                pick = int(rng.integers(0, len(js)))
                jj, ii = int(js[pick]), int(is_[pick])
            pos[i] = [ext[0] + (ii + rng.uniform(0.02, 0.98)) * cell, rng.uniform(0, 1), ext[2] + (jj + rng.uniform(0.02, 0.98)) * cell]
        classes |= check(pos, vec.nav_query(fld, pos=torch.from_numpy(pos).cuda()))
    assert classes == {"none", "source", "way"}
    vec.engine.check()
    vec.close()


def test_the_expert_reaches_the_box_in_every_maze():
    """MazeS3 x 16, seed 0, no domain randomisation, no auto-reset: the expert of examples/expert_nav.py for max_episode_steps steps;
    every env terminates with a positive reward (on the oracle's dynamics: at most 145 steps, no move blocked — tests/test_nav_cpu.py)"""
    import torch
    n = 16
    vec = _vec("MiniWorld-MazeS3-v0", n, autoreset=False, domain_rand=False)
    fld = vec.nav_field()
    won = torch.zeros(n, dtype=torch.bool, device="cuda")
    over = torch.zeros(n, dtype=torch.bool, device="cuda")
    for _ in range(int(vec.engine.cfg.max_episode_steps)):
        act, _ = _nav_actions(vec, fld, torch)
        _, rew, term, trunc = vec.step(torch.where(over, 1, act).to(torch.int32))
        won |= ~over & (term != 0) & (rew > 0)
        over |= (term | trunc) != 0
        if bool(over.all()):
            break
    assert bool(won.all()), won.tolist()
    vec.engine.check()
    vec.close()


def test_refusals():
    import torch
    from miniworld_amd import engine
    vec = _vec("MiniWorld-FourRooms-v0", 3)
    e = vec.engine
    fld = vec.nav_field()
    # before any launch
    big = torch.zeros((3, 200, 200), dtype=torch.int16, device="cuda").view(torch.uint16)
    for p, f in ((engine.MwNavParams(0.1, 0.05, 0.0, 200, 200, 0, 0), big), (engine.MwNavParams(0.0, 0.05, 0.0, fld.gx, fld.gz, 0, 0), fld.field),
                 (engine.MwNavParams(0.25, -0.1, 0.0, fld.gx, fld.gz, 0, 0), fld.field), (engine.MwNavParams(0.25, 0.1, 0.0, fld.gx, fld.gz, 0, 64), fld.field),
                 (engine.MwNavParams(0.25, 0.1, 0.0, 0, fld.gz, 0, 0), fld.field)):
        with pytest.raises(engine.EngineError):
            e.nav_build(p, f)
    with pytest.raises(engine.EngineError):     # point targets without a reach
        e.nav_build(engine.MwNavParams(0.25, 0.1, 0.0, fld.gx, fld.gz, 0, 0), fld.field, target=torch.zeros((3, 3), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        vec.nav_field(cell=0.05)
    e.check()
    # a grid too small for the extent: the status bit, rows of 0xFFFF, one report
    small = engine.MwNavParams(0.25, 0.125, 0.0, fld.gx - 1, fld.gz, 0, int(e.cfg.goal_ent))
    rows = torch.zeros((3, fld.gz, fld.gx - 1), dtype=torch.int16, device="cuda").view(torch.uint16)
    e.nav_build(small, rows)
    with pytest.raises(engine.EngineError):
        e.check()
    assert bool((_bits(rows) == -1).all())
    e.check()
    vec.close()


def test_the_engine_is_left_as_it_was():
    """a twin that never calls the nav functions returns identical observations, rewards, flags and state over 20 steps"""
    import torch
    n = 6
    a, b = _vec("MiniWorld-MazeS2-v0", n), _vec("MiniWorld-MazeS2-v0", n)
    fld = a.nav_field()
    g = torch.Generator(device="cuda").manual_seed(11)
    for _ in range(20):
        act = torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32)
        a.nav_query(fld)
        ra, rb = a.step(act), b.step(act)
        for x, y in zip(ra, rb):
            assert torch.equal(x, y)
        a.nav_field(into=fld, mask=(ra[2] | ra[3]) != 0)
        a.nav_field(target=0, obstacles="walls+entities")
    sa, sb = a.engine.get_state(), b.engine.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    a.engine.check()
    a.close()
    b.close()
