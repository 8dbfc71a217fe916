"""Depth projection on the GPU (mw_depth_project; MiniWorldVecEnv.depth_window / depth_update / depth_map / depth_map_update) against the
restatement of tests/depth_reference.py — numpy in the documented order of operations, fed by the engine's own depth maps, the poses and
cameras of vec.state() — bit for bit: planes, map, count and new at every step.  Then the frame sizes and sample counts that take another
path, mask and clear, the synthetic edges through `depth=` (the one-cell pile-up is the atomic-contention path), the adapter's key, and
the geometry: the engine's frames, unprojected, lie on the world, and the sensed window agrees with the privileged one."""
import math

import numpy as np
import pytest

import depth_reference as ref
import nav_reference as nav
from query_checks import dev as _dev, vec_env

pytestmark = pytest.mark.gpu
N = 4
SENSOR = ref.SENSOR


def _vec(env_id, n=N, **kw):
    kw.setdefault("want_depth", True)
    return vec_env(env_id, n, **kw)


def _state(vec):
    """per env: pose (x, z, dir), cam (height, fwd_disp, pitch, fov_y), extent"""
    st = vec.state(("agent_pos", "agent_dir", "cam", "extent"))
    pos, d, cam, ext = (st[k].cpu().numpy() for k in ("agent_pos", "agent_dir", "cam", "extent"))
    return [((pos[i, 0], pos[i, 2], d[i]), tuple(cam[i]), tuple(ext[i])) for i in range(vec.num_envs)]


def _sensor(o):
    return dict(min_range=o.min_range, max_range=o.max_range, floor_tol=o.floor_tol, top=o.top)


def _window_both(vec, w, depth=None, mask=None):
    """one depth_update on the device and through the restatement: equal for the envs under the mask, every byte kept for the others"""
    msaa = int(vec.engine.cfg.msaa)
    frames = (vec.depth if depth is None else depth).cpu().numpy().reshape(vec.num_envs, vec.obs.shape[1], vec.obs.shape[2])
    before = w.planes.cpu().numpy()
    assert vec.depth_update(w, depth=depth, mask=_dev(mask)) is w.planes
    got = w.planes.cpu().numpy()
    out = []
    for i, (pose, cam, _) in enumerate(_state(vec)):
        if mask is not None and not mask[i]:
            assert np.array_equal(got[i], before[i]), (i, "a masked-off env's planes moved")
            out.append(None)
            continue
        want = ref.window(frames[i], pose, cam, msaa, w.size, w.cell, w.back, w.frame == "north", **_sensor(w))
        assert np.array_equal(got[i], want), (i, w.size, w.back, w.frame, "cells that differ", np.argwhere(got[i] != want)[:8].tolist())
        out.append(want)
    return out


def _map_both(vec, m, mirror, depth=None, clear=None, mask=None):
    """one depth_map_update on the device and on `mirror` (a ref.Map per env) through the restatement"""
    msaa = int(vec.engine.cfg.msaa)
    frames = (vec.depth if depth is None else depth).cpu().numpy().reshape(vec.num_envs, vec.obs.shape[1], vec.obs.shape[2])
    assert vec.depth_map_update(m, depth=depth, clear=_dev(clear), mask=_dev(mask)) is m.new
    maps, count, new = m.map.cpu().numpy(), m.count.cpu().numpy(), m.new.cpu().numpy()
    for i, (pose, cam, ext) in enumerate(_state(vec)):
        if mask is None or mask[i]:
            ref.map_update(mirror[i], frames[i], pose, cam, msaa, ext, m.cell, m.min_points, bool(clear is not None and clear[i]), **_sensor(m))
        assert np.array_equal(maps[i], mirror[i].map), (i, "map", np.argwhere(maps[i] != mirror[i].map)[:8].tolist())
        assert np.array_equal(count[i], mirror[i].count) and np.array_equal(new[i], mirror[i].new), (i, count[i], mirror[i].count, new[i], mirror[i].new)


SHAPES = [(S, a, f) for S in (1, 2, 33, 128) for a in ("centre", "bottom") for f in ("heading", "north")]


@pytest.mark.parametrize("env_id,domain_rand", [("MiniWorld-Hallway-v0", False), ("MiniWorld-FourRooms-v0", False), ("MiniWorld-MazeS3-v0", False),
                                                ("MiniWorld-Hallway-v0", True)])
def test_walk_equals_the_restatement_at_every_step(env_id, domain_rand):
    import torch
    vec = _vec(env_id, domain_rand=domain_rand)
    rng = np.random.default_rng(3500)
    # 128 x 128 points 0.1 m apart: the largest window, 64 KiB of LDS; the others at the default cell
    windows = [vec.depth_window(size=S, cell=0.1 if S == 128 else 0.25, anchor=a, frame=f) for S, a, f in SHAPES]
    field = vec.nav_field()
    m = vec.depth_map(like=field)
    assert (m.gx, m.gz) == (field.gx, field.gz)
    mirror = [ref.Map(m.gx, m.gz) for _ in range(N)]
    seen = {"floor": 0, "obstacle": 0, "cams": set()}
    for k in range(6):
        if k:
            vec.step(torch.as_tensor(rng.integers(0, vec.n_actions, N), dtype=torch.int32, device="cuda"))
        for w in (windows if k == 0 else windows[k::5]):
            for want in _window_both(vec, w):
                seen["floor"] += int(want[0].astype(np.int64).sum())
                seen["obstacle"] += int(want[1].astype(np.int64).sum())
        _map_both(vec, m, mirror)
        seen["cams"] |= {cam for _, cam, _ in _state(vec)}
    assert seen["obstacle"] > 0 and m.count.cpu().numpy().sum() > 0
    assert seen["floor"] > 0 or "Hallway" not in env_id
    assert (len(seen["cams"]) > 1) == domain_rand          # per-env cameras exactly under domain randomisation
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("width,height,msaa", [(21, 13, 8), (21, 13, 1), (80, 60, 4), (80, 60, 1)])
def test_other_frame_sizes_and_sample_counts(width, height, msaa):
    """21 x 13 = 273 pixels: a multiple of neither the lane count nor 4 (scalar loads, a ragged last round); 4 and 1 samples: the depth is
    taken elsewhere in the pixel"""
    import torch
    vec = _vec("MiniWorld-Hallway-v0", obs_width=width, obs_height=height, msaa=msaa)
    assert tuple(vec.depth.shape) == (N, height, width, 1)
    rng = np.random.default_rng(3501)
    w, wn = vec.depth_window(size=33), vec.depth_window(size=9, cell=0.5, anchor="bottom", frame="north")
    m = vec.depth_map()
    mirror = [ref.Map(m.gx, m.gz) for _ in range(N)]
    points = 0
    for k in range(3):
        if k:
            vec.step(torch.as_tensor(rng.integers(0, vec.n_actions, N), dtype=torch.int32, device="cuda"))
        points += sum(int(p.astype(np.int64).sum()) for p in _window_both(vec, w))
        _window_both(vec, wn)
        _map_both(vec, m, mirror)
    assert points > 0
    vec.engine.check()
    vec.close()


def test_a_masked_env_keeps_every_byte():
    import torch
    vec = _vec("MiniWorld-Hallway-v0")
    mask = np.array([1, 0, 1, 0], np.uint8)
    w = vec.depth_window(size=9)
    w.planes.fill_(0xAB)
    _window_both(vec, w, mask=mask)
    assert (w.planes.cpu().numpy()[mask == 0] == 0xAB).all() and not (w.planes.cpu().numpy()[mask == 1] == 0xAB).all()
    m = vec.depth_map()
    m.map.fill_(0xAB)
    m.count.view(torch.uint8).fill_(0xAB)
    m.new.view(torch.uint8).fill_(0xAB)
    mirror = [ref.Map(m.gx, m.gz, 0xAB) for _ in range(N)]
    # clear under the mask restarts rows 0 and 2; clear outside it does nothing: the mask wins
    _map_both(vec, m, mirror, clear=np.array([1, 1, 1, 0], np.uint8), mask=mask)
    maps, count, new = m.map.cpu().numpy(), m.count.cpu().numpy(), m.new.cpu().numpy()
    assert (maps[mask == 0] == 0xAB).all() and (count[mask == 0] == -0x54545455).all() and (new[mask == 0] == -0x54545455).all()
    assert set(np.unique(maps[mask == 1]).tolist()) == {0, 1} and (count[mask == 1] == new[mask == 1]).all() and (count[mask == 1] >= 0).all()
    vec.engine.check()
    vec.close()


def test_clear_behind_same_step_auto_reset_restarts_the_finished_envs_maps():
    import torch
    vec = _vec("MiniWorld-MazeS3-v0", max_episode_steps=4)
    m = vec.depth_map(min_points=2)
    mirror = [ref.Map(m.gx, m.gz) for _ in range(N)]
    _map_both(vec, m, mirror)
    rng = np.random.default_rng(3502)
    finished = 0
    for k in range(9):
        actions = rng.integers(0, 2, N)           # turns: nobody reaches the box, every episode ends at its step limit
        _, _, term, trunc = vec.step(torch.as_tensor(actions, dtype=torch.int32, device="cuda"))[:4]
        done = (term | trunc).bool()
        finished += int(done.sum())
        before = m.count.cpu().numpy().copy()
        _map_both(vec, m, mirror, clear=done.cpu().numpy().astype(np.uint8))
        after, new = m.count.cpu().numpy(), m.new.cpu().numpy()
        d = done.cpu().numpy()
        assert (after[d] == new[d]).all() and (after[~d] == before[~d] + new[~d]).all()
    assert finished >= 2 * N
    vec.engine.check()
    vec.close()


def test_synthetic_depth_through_the_depth_argument():
    import torch
    vec = _vec("MiniWorld-Hallway-v0")
    nan, inf = float("nan"), float("inf")
    w, wn = vec.depth_window(size=33), vec.depth_window(size=9, cell=0.5, frame="north")
    m = vec.depth_map()
    # nothing of these is a point
    for bad in (nan, inf, -inf, 0.0, -3.0, 100.0, 0.049, 8.000001):
        depth = torch.full((N, 60, 80, 1), bad, dtype=torch.float32, device="cuda")
        for win in (w, wn):
            win.planes.fill_(0x5A)
            _window_both(vec, win, depth=depth)
            assert not win.planes.any(), bad
        _map_both(vec, m, [ref.Map(m.gx, m.gz) for _ in range(N)], depth=depth)
        assert not m.map.any() and not m.new.any(), bad
    # exactly at the bounds a pixel counts; a [N, H, W] tensor is taken as well
    edges = vec.depth_window(size=33, min_range=0.5, max_range=2.0, top=3.0)
    for edge in (0.5, 2.0):
        got = _window_both(vec, edges, depth=torch.full((N, 60, 80), edge, dtype=torch.float32, device="cuda"))
        assert all(g.any() for g in got), edge
    # every agent against a wall at half a metre: 4800 points in a handful of cells, each lane's atomics on the same few addresses
    pile = vec.depth_window(size=9, cell=0.5)
    got = _window_both(vec, pile, depth=torch.full((N, 60, 80, 1), 0.5, dtype=torch.float32, device="cuda"))
    assert all(g.max() == 255 for g in got)
    one = vec.depth_window(size=1, cell=20.0)
    got = _window_both(vec, one, depth=torch.full((N, 60, 80, 1), 0.5, dtype=torch.float32, device="cuda"))
    assert all(g[1, 0, 0] == 255 for g in got)        # thousands of obstacle points in the one cell, none carried into the floor's half
    assert all(g[0, 0, 0] < 255 for g in got)
    # ... and a frame with each of them somewhere, per env another
    rng = np.random.default_rng(3503)
    mixed = rng.choice(np.array([nan, inf, -1.0, 0.0, 100.0, 0.05, 8.0, 0.7, 1.3, 2.9, 4.4], np.float32), (N, 60, 80, 1))
    _window_both(vec, w, depth=_dev(mixed))
    _map_both(vec, m, [ref.Map(m.gx, m.gz) for _ in range(N)], depth=_dev(mixed), clear=np.ones(N, np.uint8))
    vec.engine.check()
    vec.close()


def test_an_uncovered_extent_is_reported_once():
    from miniworld_amd import engine
    from miniworld_amd.vec_env import DepthMap
    vec = _vec("MiniWorld-Hallway-v0")
    m = vec.depth_map()
    short = DepthMap(m.map[:, :, :3, :3].contiguous().fill_(7), m.count.fill_(5), m.new.fill_(5), engine.MwNavParams(0.25, 0.0, 0.0, 3, 3, 0, 0), 1, 0.05, 8.0, 0.1,
                     1.6)
    vec.depth_map_update(short)
    assert not short.map.any() and not short.count.any() and not short.new.any()
    with pytest.raises(engine.EngineError, match="mw_depth_project refused an env"):
        vec.engine.check()
    vec.engine.check()          # once
    vec.close()


def test_the_library_refuses_what_the_header_says():
    import torch
    from miniworld_amd import engine
    vec = _vec("MiniWorld-Hallway-v0")
    e = vec.engine
    planes = torch.full((N, 2, 9, 9), 0xAB, dtype=torch.uint8, device="cuda")
    good = dict(min_range=0.05, max_range=8.0, floor_tol=0.1, top=1.6, size=9, cell=0.25, back=0.0, flags=0, planes=planes)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(min_range=0.0), dict(min_range=nan), dict(max_range=inf), dict(max_range=-1.0), dict(min_range=3.0, max_range=2.0), dict(floor_tol=-0.1),
               dict(floor_tol=nan), dict(top=0.05), dict(top=inf), dict(cell=0.0), dict(cell=inf), dict(back=nan), dict(flags=1), dict(flags=4)):
        with pytest.raises(engine.EngineError, match="mw_depth_project"):
            e.depth_project(vec.depth, **dict(good, **kw))
    big = torch.zeros((N, 2, 129, 129), dtype=torch.uint8, device="cuda")
    with pytest.raises(engine.EngineError, match="size 129"):
        e.depth_project(vec.depth, **dict(good, size=129, planes=big))
    m = vec.depth_map()
    grid = dict(min_range=0.05, max_range=8.0, floor_tol=0.1, top=1.6, params=m.params, map=m.map, count=m.count, new=m.new)
    for kw in (dict(min_points=0), dict(min_points=256), dict(flags=2)):
        with pytest.raises(engine.EngineError, match="mw_depth_project"):
            e.depth_project(vec.depth, **dict(grid, **kw))
    wide = engine.MwNavParams(0.25, 0.0, 0.0, 129, 128, 0, 0)
    with pytest.raises(engine.EngineError, match="use a larger cell"):
        e.depth_project(vec.depth, **dict(grid, params=wide, map=torch.zeros((N, 2, 128, 129), dtype=torch.uint8, device="cuda")))
    assert (planes == 0xAB).all() and not m.map.any()          # nothing was written
    vec.engine.check()
    vec.close()


def test_the_adapters_key_is_a_direct_update_at_the_same_state():
    import torch
    from miniworld_amd.vector import MiniWorldVectorEnv
    envs = MiniWorldVectorEnv("MiniWorld-Hallway-v0", N, depth_map=dict(size=17, max_range=5.0), seed=0)
    _, info = envs.reset(seed=3)
    rng = np.random.default_rng(3504)
    for k in range(4):
        if k:
            _, _, _, _, info = envs.step(torch.as_tensor(rng.integers(0, 3, N), dtype=torch.int32, device="cuda"))
        mine = envs.vec.depth_window(size=17, max_range=5.0)
        want = _window_both(envs.vec, mine)
        assert info["depth_map"].dtype == torch.uint8 and tuple(info["depth_map"].shape) == (N, 2, 17, 17)
        assert torch.equal(info["depth_map"], mine.planes) and info["depth_map"] is not envs.depth_win.planes
        assert sum(int(x.astype(np.int64).sum()) for x in want) > 0
    envs.close()


# ---------------------------------------------------------------------------------------------------------------- the geometry

def _solids(vec, i, st):
    w = nav.world_of_engine(vec.engine, st, i)
    boxes = [(float(w["pos"][k][0]), float(w["pos"][k][2]), float(w["radius"][k]), float(st["ent_geom"][i][k][8])) for k in range(len(w["kind"])) if int(w["kind"][k])]
    return {"segs": w["segs"], "wall_h": float(vec.engine.cfg.room_wall_height) or 2.74, "boxes": boxes}


# The floor statement compares a cell's POINTS with the privileged plane at the cell's CENTRE, and at wall_radius = 0 that plane is 1 exactly
# outside the env's extent: it can hold only where no sensed cell straddles the extent's border.  A point of eye depth <= 5 m lies within
# 5 * sqrt(1 + tx * tx) = 6.56 m of the camera (tx = tan(32.5 deg) * 4 / 3, the widest randomised field of view), the camera within 0.1 m of
# the agent, the centre within half a cell's diagonal of the point: the statement is asserted for the envs whose agent is 7 m or more
# inside the extent — none in the small worlds, several in the 25.75 m Maze, which is there for it.
FLOOR_MARGIN = 7.0


@pytest.mark.parametrize("env_id,n", [("MiniWorld-Hallway-v0", N), ("MiniWorld-OneRoom-v0", N), ("MiniWorld-MazeS3-v0", N), ("MiniWorld-Maze-v0", 16)])
def test_the_engines_frames_lie_on_the_world_and_agree_with_the_privileged_window(env_id, n):
    import torch
    vec = _vec(env_id, n=n, domain_rand=True)
    N = n
    rng = np.random.default_rng(3505)
    cell = 0.25
    sensed = vec.depth_window(size=41, cell=cell, max_range=5.0)
    near_wall = vec.ego_window(size=41, cell=cell, planes=("wall", "entity"), wall_radius=cell * math.sqrt(2) / 2 + 0.05, entity_pad=cell * math.sqrt(2) / 2 + 0.05)
    on_wall = vec.ego_window(size=41, cell=cell, planes=("wall",), wall_radius=0.0)
    obstacle_cells = floor_cells = floor_checked = 0
    for k in range(3):
        if k:
            vec.step(torch.as_tensor(rng.integers(0, 3, N), dtype=torch.int32, device="cuda"))
        st = vec.engine.get_state()
        frames = vec.depth.cpu().numpy().reshape(N, 60, 80)
        for i, (pose, cam, _) in enumerate(_state(vec)):
            bad, inside = ref.unclassified(frames[i], ref.z16_of(frames[i]), pose, cam, 8, _solids(vec, i, st))
            print(f"{env_id} step {k} env {i}: {bad} of {inside} pixels within 5 m unclassified")
            assert bad <= 0.02 * 80 * 60, (env_id, k, i, bad)
        vec.depth_update(sensed)
        vec.ego_update(near_wall)
        vec.ego_update(on_wall)
        obstacle = sensed.obstacle.cpu().numpy() > 0
        floor = sensed.floor.cpu().numpy() > 0
        # a cell with obstacle points holds a wall or an entity within half its diagonal plus four depth steps at 5 m; a cell with floor
        # points does not have its centre on a wall
        solid = (near_wall.wall.cpu().numpy() != 0) | (near_wall.entity.cpu().numpy() != 0)
        assert not (obstacle & ~solid).any(), (env_id, k, np.argwhere(obstacle & ~solid)[:8].tolist())
        deep = np.array([min(pose[0] - ext[0], ext[1] - pose[0], pose[1] - ext[2], ext[3] - pose[1]) >= FLOOR_MARGIN for pose, _, ext in _state(vec)])
        beyond = floor & (on_wall.wall.cpu().numpy() != 0) & deep[:, None, None]
        assert not beyond.any(), (env_id, k, np.argwhere(beyond)[:8].tolist())
        obstacle_cells += int(obstacle.sum())
        floor_cells += int(floor.sum())
        floor_checked += int(floor[deep].sum())
    assert obstacle_cells > 0 and (floor_cells > 0 or "MazeS3" in env_id)
    assert floor_checked > 0 or env_id != "MiniWorld-Maze-v0"
    vec.engine.check()
    vec.close()
