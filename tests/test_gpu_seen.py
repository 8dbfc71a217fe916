"""Explored-area maps on the GPU (mw_seen_update; MiniWorldVecEnv.seen_map / seen_update) against the restatement of
tests/seen_reference.py — numpy in the documented order of operations, fed by engine.get_geometry(env), engine.get_state() and the
poses of vec.state() — bit for bit: the map, `new` and `count` at every step; and against the engine's own ray casts to the same cell
centres.  Then the launch shapes that can go wrong, mask and clear, the auto-reset boundary, a grid that does not cover the extent,
and that the calls leave a stepped batch alone."""
import math
import os
import re

import numpy as np
import pytest

import seen_reference as ref
from query_checks import dev, poses as _poses, teleport as _teleport, vec_env, worlds as _worlds

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu
N = 8
_SEEN_H = open(os.path.join(HERE, "..", "miniworld_amd", "csrc", "mw_seen.h")).read()
THREADS = int(re.search(r"#define MW_SEEN_THREADS (\d+)", _SEEN_H).group(1))
CANDS = int(re.search(r"#define MW_SEEN_CANDS (\d+)", _SEEN_H).group(1))


def _vec(env_id, n=N, **kw):
    return vec_env(env_id, n, **kw)


def _maps(m):
    """the restatement's maps holding what the device map holds now"""
    seen, count, new = m.seen.cpu().numpy(), m.count.cpu().numpy(), m.new.cpu().numpy()
    out = []
    for i in range(seen.shape[0]):
        r = ref.Map(m.gx, m.gz, 0, count[i], new[i])
        r.seen[:] = seen[i]
        out.append(r)
    return out


def _update_both(vec, m, maps, clear=None, mask=None):
    """one seen_update on the device and on the restatement's maps; asserts equality; returns the restatement's candidate counts"""
    import torch
    worlds, poses = _worlds(vec), _poses(vec)
    entities = m.obstacles == "walls+entities"
    cands = [ref.update(maps[i], worlds[i], m.cell, poses[i], m.max_range, m.cos_half, entities,
                        clear=bool(clear is not None and clear[i]), mask=bool(mask is None or mask[i])) for i in range(vec.num_envs)]
    assert vec.seen_update(m, clear=dev(clear), mask=dev(mask)) is m.new
    seen, count, new = m.seen.cpu().numpy(), m.count.cpu().numpy(), m.new.cpu().numpy()
    for i in range(vec.num_envs):
        assert np.array_equal(seen[i], maps[i].seen), (i, "cells that differ", np.argwhere(seen[i] != maps[i].seen)[:8].tolist())
        assert (int(new[i]), int(count[i])) == (maps[i].new, maps[i].count), (i, "new, count")
    return cands


# ---------------------------------------------------------------------------------------------------------------- the reference

@pytest.mark.parametrize("env_id,obstacles", [("MiniWorld-Hallway-v0", "walls"), ("MiniWorld-FourRooms-v0", "walls"), ("MiniWorld-MazeS3-v0", "walls"),
                                              ("MiniWorld-PickupObjects-v0", "walls+entities")])
def test_walk_equals_the_restatement_at_every_step(env_id, obstacles):
    import torch
    vec = _vec(env_id)
    rng = np.random.default_rng(3200)
    m = vec.seen_map(obstacles=obstacles)
    maps = _maps(m)
    _update_both(vec, m, maps)
    assert (m.count > 0).all()
    grown = 0
    for _ in range(12):
        vec.step(torch.as_tensor(rng.integers(0, vec.n_actions, N), dtype=torch.int32, device="cuda"))
        _update_both(vec, m, maps)
        grown += int(m.new.sum())
    assert grown > 0
    assert torch.equal(m.seen.sum((1, 2)).to(torch.int32), m.count)
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("env_id,obstacles", [("MiniWorld-MazeS3-v0", "walls"), ("MiniWorld-PickupObjects-v0", "walls+entities")])
def test_map_equals_the_engines_own_ray_casts(env_id, obstacles):
    """max_range 3 at 0.25 m per cell: the cells within range lie in the 27 x 27 window around the agent's cell — 729 rays per env,
    cast to every centre with direction = c - o and max_t = 1.  Tests 1 - 3 in torch on the host in float64 (one operation per call:
    nothing is contracted), the line of sight from the cast."""
    import torch
    vec = _vec(env_id)
    rng = np.random.default_rng(3201)
    for _ in range(5):
        vec.step(torch.as_tensor(rng.integers(0, vec.n_actions, N), dtype=torch.int32, device="cuda"))
    cell, rng_m, half = 0.25, 3.0, 13
    for fov in (None, 2 * math.pi):
        m = vec.seen_map(cell=cell, max_range=rng_m, fov=fov, obstacles=obstacles)
        vec.seen_update(m)
        st = vec.state(("agent_pos", "extent"))
        o, ext = st["agent_pos"][:, [0, 2]].cpu(), st["extent"].cpu()
        h = vec.raycast(offsets=torch.zeros(1, dtype=torch.float64, device="cuda"))["dir"][:, 0].cpu()
        ic = torch.floor((o[:, 0] - ext[:, 0]) / cell).long()
        jc = torch.floor((o[:, 1] - ext[:, 2]) / cell).long()
        k = torch.arange(-half, half + 1)
        i = (ic[:, None, None] + k[None, None, :]).expand(N, 27, 27)
        j = (jc[:, None, None] + k[None, :, None]).expand(N, 27, 27)
        on_grid = (i >= 0) & (i < m.gx) & (j >= 0) & (j < m.gz)
        cx = ext[:, 0, None, None] + (i.double() + 0.5) * cell
        cz = ext[:, 2, None, None] + (j.double() + 0.5) * cell
        vx, vz = cx - o[:, 0, None, None], cz - o[:, 1, None, None]
        d = torch.stack([vx, vz], dim=-1).reshape(N, 729, 2).contiguous().cuda()
        cast = vec.raycast(direction=d, max_t=1.0, obstacles=obstacles)
        free = ((cast["hit"] == -1) & (cast["t"] == 1.0)).cpu().reshape(N, 27, 27)
        inside = ~((cx > ext[:, 1, None, None]) | (cz > ext[:, 3, None, None]))
        dist = torch.sqrt(vx * vx + vz * vz)
        cone = (dist == 0.0) | (vx * h[:, 0, None, None] + vz * h[:, 1, None, None] >= m.cos_half * dist)
        if m.cos_half == -1.0:
            cone = torch.ones_like(cone)
        vis = on_grid & inside & (dist <= rng_m) & cone & free
        want = torch.zeros((N, m.gz, m.gx), dtype=torch.uint8)
        e = torch.arange(N)[:, None, None].expand(N, 27, 27)
        want[e[vis], j[vis], i[vis]] = 1
        got = m.seen.cpu()
        assert torch.equal(got, want), (fov, "cells that differ", (got != want).nonzero()[:8].tolist())
        assert torch.equal(m.count.cpu(), want.sum((1, 2)).to(torch.int32)) and torch.equal(m.new, m.count)
        assert (m.count > 0).all() and not vis.all()
        # no cell outside the window is within range: the window holds the whole map
        assert int(want.sum()) == int(vis.sum())
    vec.engine.check()
    vec.close()


# ---------------------------------------------------------------------------------------------------------------- launch shapes

def test_box_clipped_in_a_corner_and_a_cell_count_off_the_wavefront():
    vec = _vec("MiniWorld-FourRooms-v0")
    m = vec.seen_map(cell=0.3, max_range=4.0, fov=2 * math.pi)
    assert (m.gx * m.gz) % 64 != 0
    ext = vec.engine.get_state()["extent"]
    # every env's agent into a corner of its extent, a different corner in turn: the box is clipped on two sides
    x = [ext[i][0] + 0.6 if i % 2 == 0 else ext[i][1] - 0.6 for i in range(N)]
    z = [ext[i][2] + 0.6 if (i // 2) % 2 == 0 else ext[i][3] - 0.6 for i in range(N)]
    _teleport(vec, (x, z))
    maps = _maps(m)
    _update_both(vec, m, maps)
    assert (m.count > 0).all()
    vec.engine.check()
    vec.close()


def test_a_range_larger_than_the_world_takes_several_rounds():
    """MazeS3, all round, 30 m: the box is the whole grid, and the cells that pass tests 1 - 3 are more than a turn of the workgroup
    and more than one round of the candidate list holds"""
    vec = _vec("MiniWorld-MazeS3-v0")
    m = vec.seen_map(max_range=30.0, fov=2 * math.pi)
    maps = _maps(m)
    cands = _update_both(vec, m, maps)
    assert min(cands) > CANDS > THREADS and m.gx * m.gz > CANDS
    assert (m.count > 0).all() and (m.count < m.gx * m.gz).all()
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("shared", [True, False])
def test_narrow_short_and_full_sight_on_shared_and_per_env_geometry(shared):
    import torch
    vec = _vec("MiniWorld-FourRooms-v0" if shared else "MiniWorld-MazeS3-v0")
    assert bool(vec.engine.cfg.shared_geometry) == shared
    rng = np.random.default_rng(3202)
    for kw in (dict(max_range=0.1, fov=2 * math.pi),        # a range below half a cell: at most the cell the agent stands on the centre of
               dict(max_range=8.0, fov=0.05), dict(max_range=8.0, fov=2 * math.pi)):
        m = vec.seen_map(**kw)
        maps = _maps(m)
        for _ in range(2):
            _update_both(vec, m, maps)
            vec.step(torch.as_tensor(rng.integers(0, vec.n_actions, N), dtype=torch.int32, device="cuda"))
        if kw["max_range"] < 0.125:
            assert (m.count <= 2).all()         # (one cell per pose at the most)
        elif kw["fov"] == 2 * math.pi:
            assert (m.count > 0).all()
    narrow, full = vec.seen_map(max_range=8.0, fov=0.05), vec.seen_map(max_range=8.0, fov=2 * math.pi)
    vec.seen_update(narrow), vec.seen_update(full)
    assert (full.seen >= narrow.seen).all() and (full.count > narrow.count).all() and int(narrow.count.sum()) > 0
    vec.engine.check()
    vec.close()


def test_more_segments_than_the_workgroup_has_lanes():
    vec = _vec("MiniWorld-Maze-v0")
    worlds = _worlds(vec)
    assert max(len(w["segs"]) for w in worlds) == 256 > THREADS        # the family with the most segments
    m = vec.seen_map(max_range=6.0)
    maps = _maps(m)
    _update_both(vec, m, maps)
    assert (m.count > 0).all()
    vec.engine.check()
    vec.close()


# ---------------------------------------------------------------------------------------------------------------- mask and clear

def test_mask_wins_over_clear_and_clear_restarts_the_count():
    import torch
    vec = _vec("MiniWorld-FourRooms-v0")
    m = vec.seen_map(max_range=5.0, fov=2 * math.pi)
    vec.seen_update(m)
    first = m.count.clone()
    mask = np.array([1, 0, 1, 0, 0, 1, 1, 0], np.uint8)
    off = torch.as_tensor(mask == 0, device="cuda")
    # masked-off envs keep every byte, whatever they hold: rows of 0xAB, sentinel counts, and a clear that must not happen
    m.seen[off] = 0xAB
    m.count[off], m.new[off] = -77, -78
    maps = _maps(m)
    _teleport(vec, ([1.5] * N, [1.5] * N), 0.7)
    _update_both(vec, m, maps, clear=np.ones(N, np.uint8), mask=mask)
    assert (m.seen[off] == 0xAB).all() and (m.count[off] == -77).all() and (m.new[off] == -78).all()
    on = ~off
    assert torch.equal(m.count[on], m.new[on]) and torch.equal(m.count[on], m.seen[on].sum((1, 2)).to(torch.int32)) and (m.count[on] > 0).all()
    # ... and without a clear the count is carried
    m2 = vec.seen_map(max_range=5.0, fov=2 * math.pi)
    m2.seen.copy_(torch.where(m.seen == 1, 1, 0).to(torch.uint8))
    m2.count.copy_(m2.seen.sum((1, 2)).to(torch.int32))
    before = m2.count.clone()
    _teleport(vec, ([-1.5] * N, [-1.5] * N), 2.0)
    _update_both(vec, m2, _maps(m2), mask=mask.astype(bool))
    assert torch.equal(m2.count, before + torch.where(off, 0, m2.new)) and (m2.new[on] > 0).all()
    assert first.min() > 0
    vec.engine.check()
    vec.close()


def test_clear_on_done_starts_the_map_of_the_new_episode():
    """same-step auto-reset, episodes of 4 steps: behind the step that ends them every env holds its next world, and
    seen_update(m, clear=done) leaves exactly the fresh map of that world's first pose"""
    import torch
    vec = _vec("MiniWorld-MazeS3-v0", max_episode_steps=4)
    m = vec.seen_map(max_range=6.0)
    vec.seen_update(m)
    ended = 0
    for k in range(9):
        _, _, term, trunc = vec.step(torch.full((N,), 2 if k % 2 else 0, dtype=torch.int32, device="cuda"))
        done = (term | trunc) != 0
        carried = m.count.clone()
        vec.seen_update(m, clear=done)
        fresh = vec.seen_map(max_range=6.0)
        vec.seen_update(fresh)
        ended += int(done.sum())
        assert torch.equal(m.seen[done], fresh.seen[done]) and torch.equal(m.count[done], fresh.count[done]) and torch.equal(m.new[done], fresh.new[done])
        assert torch.equal(m.count[~done], (carried + m.new)[~done]) and (m.seen >= fresh.seen).all()
    assert ended >= 2 * N           # (truncation after 4 steps: every env twice)
    maps = _maps(m)
    _update_both(vec, m, maps)          # the new worlds' geometry, from the engine
    vec.engine.check()
    vec.close()


# ---------------------------------------------------------------------------------------------------------------- refusals, collateral

def test_a_grid_that_does_not_cover_the_extent_zeroes_the_row_and_check_raises_once():
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import SeenMap
    vec = _vec("MiniWorld-Hallway-v0")
    full = vec.seen_map()
    p = engine.MwNavParams(full.cell, 0.0, 0.0, full.gx - 3, full.gz, 0, 0)
    m = SeenMap(torch.full((N, full.gz, full.gx - 3), 1, dtype=torch.uint8, device="cuda"), torch.full((N,), 9, dtype=torch.int32, device="cuda"),
                torch.full((N,), 9, dtype=torch.int32, device="cuda"), p, full.max_range, full.cos_half, full.obstacles)
    vec.seen_update(m)
    assert not m.seen.any() and not m.count.any() and not m.new.any()
    with pytest.raises(engine.EngineError):
        vec.engine.check()
    vec.engine.check()          # reported once, then forgotten
    vec.seen_update(full)
    assert (full.count > 0).all()
    vec.engine.check()
    # what the library itself refuses, before anything is launched
    for rng_m, cos_half, flags in ((0.0, 0.5, 0), (float("inf"), 0.5, 0), (float("nan"), 0.5, 0), (5.0, 1.5, 0), (5.0, -1.5, 0), (5.0, float("nan"), 0), (5.0, 0.5, 2)):
        before = full.seen.clone()
        with pytest.raises(engine.EngineError):
            vec.engine.seen_update(full.params, rng_m, cos_half, flags, full.seen, full.count, full.new)
        assert torch.equal(full.seen, before)
    vec.engine.check()
    vec.close()


def test_updates_in_between_leave_a_stepped_batch_alone():
    import torch
    rng = np.random.default_rng(3203)
    acts = rng.integers(0, 3, (10, N))
    runs = []
    for with_maps in (False, True):
        vec = _vec("MiniWorld-FourRooms-v0")
        m = vec.seen_map(obstacles="walls+entities") if with_maps else None
        rows = []
        for a in acts:
            obs, rew, term, trunc = vec.step(torch.as_tensor(a, dtype=torch.int32, device="cuda"))
            rows.append((obs.clone(), rew.clone(), term.clone(), trunc.clone()))
            if with_maps:
                vec.seen_update(m, clear=(term | trunc))
        rows.append(tuple(v.clone() for v in vec.state().values()))
        vec.engine.check()
        vec.close()
        runs.append(rows)
    for k, (a, b) in enumerate(zip(*runs)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), k
