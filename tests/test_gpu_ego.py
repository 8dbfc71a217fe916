"""Egocentric map windows on the GPU (mw_ego_map; MiniWorldVecEnv.ego_window / ego_update) against the restatement of
tests/ego_reference.py — numpy in the documented order of operations, fed by engine.get_geometry(env), engine.get_state() and the poses
of vec.state() — bit for bit: every plane and the sample at every step; and against the engine's own ray casts to the same points.
Then the launch shapes that can go wrong, mask and origin, the crop identities of a north window on the grid, the auto-reset boundary,
the library's refusals, and that the calls leave a stepped batch alone."""
import math

import numpy as np
import pytest

import ego_reference as ref
import nav_reference as nav
from query_checks import dev as _dev, host as _host, poses as _poses, teleport as _teleport, vec_env, worlds as _worlds

pytestmark = pytest.mark.gpu
N = 8
CELL = 0.25


def _vec(env_id, n=N, **kw):
    return vec_env(env_id, n, **kw)


def _random_field(vec, rng):
    """a NavField of the template's grid with a different cost in (nearly) every cell: a wrong index shows"""
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import NavField
    t = vec.template
    gx, gz = nav.grid_shape((t.min_x, t.max_x, t.min_z, t.max_z), CELL)
    cells = rng.integers(0, 0xFFFE, (vec.num_envs, gz, gx)).astype(np.uint16)
    return NavField(torch.from_numpy(cells.view(np.int16)).cuda().view(torch.uint16), engine.MwNavParams(CELL, 0.0, 0.0, gx, gz, 0, 0), 0, "walls")


def _update_both(vec, w, source=None, fill=None, mask=None, pos=None):
    """one ego_update on the device and through the restatement; asserts equality of every plane and the sample for the envs under the
    mask, and that the others keep every byte; returns (planes, sample) of the restatement per env (None for a masked-off env)"""
    worlds, poses = _worlds(vec), _poses(vec)
    src = None if source is None else _host(source.seen if hasattr(source, "seen") else source.field)
    used_fill = fill if fill is not None else (0 if source is None or hasattr(source, "seen") else 0xFFFF)
    before = None if w.planes is None else w.planes.clone()
    before_sample = None
    if source is not None and mask is not None:         # (the sample is the env's own tensor: garbage into it before the call)
        import torch
        own = vec.ego_update(w, source=source, fill=fill)[1]
        (own.view(torch.int16) if own.dtype == torch.uint16 else own).fill_(0x3B)
        before_sample = own.clone()
        if before is not None:
            w.planes.copy_(before)
    got = vec.ego_update(w, source=source, fill=fill, mask=_dev(mask), pos=_dev(pos))
    planes, sample = (got, None) if source is None else got
    assert planes is w.planes
    planes = None if planes is None else planes.cpu().numpy()
    sample = None if sample is None else _host(sample)
    out = []
    for i in range(vec.num_envs):
        if mask is not None and not mask[i]:
            assert planes is None or np.array_equal(planes[i], before[i].cpu().numpy()), (i, "a masked-off env's planes moved")
            assert sample is None or np.array_equal(sample[i], _host(before_sample)[i]), (i, "a masked-off env's sample moved")
            out.append(None)
            continue
        origin = None if pos is None else (pos[i][0], pos[i][2])
        wp, ws = ref.window(worlds[i], poses[i], w.size, w.cell, w.back, w.frame == "north", w.names, w.wall_radius, w.entity_pad, w.max_range, w.cos_half,
                            w.obstacles == "walls+entities", origin=origin, src=None if src is None else src[i], src_cell=None if source is None else source.cell,
                            fill=used_fill)
        for p, name in enumerate(w.names):
            assert np.array_equal(planes[i][p], wp[p]), (i, name, "cells that differ", np.argwhere(planes[i][p] != wp[p])[:8].tolist())
        if source is not None:
            assert np.array_equal(sample[i], ws), (i, "sample", np.argwhere(sample[i] != ws)[:8].tolist())
        out.append((wp, ws))
    return out


# ---------------------------------------------------------------------------------------------------------------- the reference

@pytest.mark.parametrize("env_id,obstacles", [("MiniWorld-Hallway-v0", "walls"), ("MiniWorld-FourRooms-v0", "walls"), ("MiniWorld-MazeS3-v0", "walls"),
                                              ("MiniWorld-PickupObjects-v0", "walls+entities")])
def test_walk_equals_the_restatement_at_every_step(env_id, obstacles):
    import torch
    vec = _vec(env_id)
    assert env_id != "MiniWorld-MazeS3-v0" or not vec.engine.cfg.shared_geometry          # per-env geometry
    rng = np.random.default_rng(3400)
    seen = vec.seen_map(obstacles=obstacles)
    field = _random_field(vec, rng)
    big = vec.ego_window(size=33, obstacles=obstacles)                                                      # 1089 cells: four rounds of 256 lanes and a ragged tail
    small = vec.ego_window(size=9, anchor="bottom", frame="north", wall_radius=0.0, obstacles=obstacles)    # 81 cells: fewer than one workgroup
    values = {"wall": set(), "entity": 0, "visible": set()}
    for k in range(13):
        if k:
            vec.step(torch.as_tensor(rng.integers(0, vec.n_actions, N), dtype=torch.int32, device="cuda"))
        vec.seen_update(seen)
        for w, source in ((big, seen), (small, field)):
            for wp, _ in _update_both(vec, w, source=source):
                values["wall"] |= set(np.unique(wp[0]).tolist())
                values["entity"] += int((wp[1] != 0).sum())
                values["visible"] |= set(np.unique(wp[2]).tolist())
    assert values["wall"] == {0, 1} and values["visible"] == {0, 1}
    assert values["entity"] > 0 or env_id != "MiniWorld-PickupObjects-v0"
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("env_id,obstacles", [("MiniWorld-MazeS3-v0", "walls"), ("MiniWorld-PickupObjects-v0", "walls+entities")])
def test_visible_equals_the_engines_own_ray_casts(env_id, obstacles):
    """a ray to every point of the window, direction = p - o and max_t = 1; the points, range and cone in torch on the host in float64
    (one operation per call: nothing is contracted), the line of sight from the cast"""
    import torch
    vec = _vec(env_id)
    rng = np.random.default_rng(3401)
    for _ in range(5):
        vec.step(torch.as_tensor(rng.integers(0, vec.n_actions, N), dtype=torch.int32, device="cuda"))
    S, cell = 21, 0.5
    for fov, frame, back in ((None, "heading", 0.0), (2 * math.pi, "north", S / 2), (None, "north", 0.0)):
        w = vec.ego_window(size=S, cell=cell, anchor="bottom" if back else "centre", frame=frame, planes=("visible",), max_range=4.0, fov=fov, obstacles=obstacles)
        vec.ego_update(w)
        o = vec.state(("agent_pos",))["agent_pos"][:, [0, 2]].cpu()
        h = vec.raycast(offsets=torch.zeros(1, dtype=torch.float64, device="cuda"))["dir"][:, 0].cpu()
        idx = torch.arange(S, dtype=torch.float64) + 0.5
        lat = (idx - S * 0.5) * cell
        fwd = ((S * 0.5 - idx) + back) * cell
        F, L = fwd[None, :, None].expand(N, S, S), lat[None, None, :].expand(N, S, S)
        if frame == "north":
            fx, fz, rx, rz = torch.zeros(N), -torch.ones(N), torch.ones(N), torch.zeros(N)
        else:
            fx, fz, rx, rz = h[:, 0], h[:, 1], -h[:, 1], h[:, 0]
        e = lambda v: v.double()[:, None, None]
        px = e(o[:, 0]) + (F * e(fx) + L * e(rx))
        pz = e(o[:, 1]) + (F * e(fz) + L * e(rz))
        vx, vz = px - e(o[:, 0]), pz - e(o[:, 1])
        d = torch.stack([vx, vz], dim=-1).reshape(N, S * S, 2).contiguous().cuda()
        cast = vec.raycast(direction=d, max_t=1.0, obstacles=obstacles)
        free = ((cast["hit"] == -1) & (cast["t"] == 1.0)).cpu().reshape(N, S, S)
        dist = torch.sqrt(vx * vx + vz * vz)
        cone = (dist == 0.0) | (vx * e(h[:, 0]) + vz * e(h[:, 1]) >= w.cos_half * dist)
        if w.cos_half == -1.0:
            cone = torch.ones_like(cone)
        want = ((dist <= 4.0) & cone & free).to(torch.uint8)
        got = w.visible.cpu()
        assert torch.equal(got, want), (fov, frame, "cells that differ", (got != want).nonzero()[:8].tolist())
        assert want.any() and not want.all()
    vec.engine.check()
    vec.close()


# ---------------------------------------------------------------------------------------------------------------- shapes, mask, origin

@pytest.mark.parametrize("size", [1, 2, 9, 33])
def test_sizes_plane_sets_mask_origin_and_a_corner(size):
    import torch
    vec = _vec("MiniWorld-FourRooms-v0")
    rng = np.random.default_rng(3402)
    seen = vec.seen_map(max_range=6.0, fov=2 * math.pi)
    vec.seen_update(seen)
    field = _random_field(vec, rng)
    ext = vec.engine.get_state()["extent"]
    mask = np.array([0, 1, 1, 0, 1, 1, 1, 0], np.uint8)          # zero bytes first and last
    pos = np.zeros((N, 3), np.float64)
    pos[:, 0], pos[:, 2] = rng.uniform(-6.0, 6.0, N), rng.uniform(-6.0, 6.0, N)
    windows = [vec.ego_window(size=size), vec.ego_window(size=size, planes=("visible",), anchor="bottom"),
               vec.ego_window(size=size, planes=("wall",), frame="north"), vec.ego_window(size=size, planes=("entity", "wall"), obstacles="walls+entities"),
               vec.ego_window(size=size, planes=())]
    for corner in (False, True):
        if corner:          # every env into a corner of its extent, a different one in turn: most of the window is outside
            _teleport(vec, ([ext[i][0] + 0.3 if i % 2 == 0 else ext[i][1] - 0.3 for i in range(N)],
                            [ext[i][2] + 0.3 if (i // 2) % 2 == 0 else ext[i][3] - 0.3 for i in range(N)]), 0.9)
        outside = 0
        for w in windows:
            for source, fill in ((seen, None), (field, None), (field, 0x1234)) + (() if not w.names else ((None, None),)):
                res = _update_both(vec, w, source=source, fill=fill)
                if w.names and w.names[0] == "wall":
                    outside += sum(int(wp[0].sum()) for wp, _ in res)
            # garbage under a mask with zero bytes first and last, then an origin that is not the agent's
            if w.planes is not None:
                w.planes.fill_(0xAB)
            _update_both(vec, w, source=seen, mask=mask)
            _update_both(vec, w, source=field, mask=mask.astype(bool), pos=pos)
            _update_both(vec, w, source=seen, pos=pos)
        assert outside > 0 or not corner or size == 1
    vec.engine.check()
    vec.close()


def test_more_segments_than_the_workgroup_has_lanes_at_the_largest_window():
    vec = _vec("MiniWorld-Maze-v0", n=2)
    assert max(len(w["segs"]) for w in _worlds(vec)) == 256          # the family with the most segments: several rounds of staging
    from miniworld_amd import engine
    w = vec.ego_window(size=engine.EGO_MAX_SIZE, cell=0.125)
    _update_both(vec, w)
    assert w.wall.any() and w.visible.any() and not w.visible.all()
    vec.engine.check()
    vec.close()


# ---------------------------------------------------------------------------------------------------------------- identities

@pytest.mark.parametrize("size", [9, 8])
def test_a_north_window_on_the_grid_is_the_plain_crop_and_the_crop_of_a_fresh_seen_map(size):
    """cell == the map's cell, the agent on a cell's centre (odd size) or corner (even size): the window's points are cell centres"""
    import torch
    import torch.nn.functional as F
    vec = _vec("MiniWorld-FourRooms-v0")
    rng = np.random.default_rng(3403)
    ext = vec.engine.get_state()["extent"]
    seen = vec.seen_map(max_range=3.0, fov=2 * math.pi)
    gx, gz = seen.gx, seen.gz
    i0 = np.array([2, gx - 2, gx // 2 + 3, 5, gx - 3, 7, 1, gx // 2])
    j0 = np.array([3, gz - 3, gz // 2 - 5, gz - 2, 2, gz // 2, 1, 6])
    off = 0.5 if size % 2 else 0.0
    _teleport(vec, ([ext[i][0] + (i0[i] + off) * CELL for i in range(N)], [ext[i][2] + (j0[i] + off) * CELL for i in range(N)]), 1.3)
    vec.seen_update(seen)
    assert (seen.count > 0).all()
    field = _random_field(vec, rng)
    w = vec.ego_window(size=size, frame="north", planes=("visible",), max_range=3.0, fov=2 * math.pi)
    for source, fill in ((seen, 0), (field, 0xFFFF), (field, 0x0102)):
        res = _update_both(vec, w, source=source, fill=fill)
        src = source.seen if source is seen else source.field.view(torch.int16)
        padded = F.pad(src.to(torch.int32) & 0xFFFF, (size, size, size, size), value=fill)
        _, sample = vec.ego_update(w, source=source, fill=fill)
        sample = (sample if source is seen else sample.view(torch.int16)).to(torch.int32) & 0xFFFF
        padding = 0
        for i in range(N):
            fi, fj = int(i0[i]) - size // 2 + size, int(j0[i]) - size // 2 + size
            crop = padded[i, fj:fj + size, fi:fi + size]
            assert torch.equal(sample[i], crop), (i, fill)
            padding += int((np.asarray(res[i][1]) == fill).sum())
            if source is seen:
                assert torch.equal(w.visible[i].to(torch.int32), crop), (i, "visible now against the fresh map", (w.visible[i] != crop).nonzero()[:8].tolist())
        assert padding > 0
    vec.engine.check()
    vec.close()


def test_an_update_behind_a_same_step_reset_shows_the_new_world():
    """same-step auto-reset, episodes of 4 steps: behind the step that ends them every env holds its next world"""
    import torch
    vec = _vec("MiniWorld-MazeS3-v0", max_episode_steps=4)
    w = vec.ego_window(size=33)
    ended, moved = 0, 0
    for k in range(9):
        before = _worlds(vec)
        _, _, term, trunc = vec.step(torch.full((N,), 2 if k % 2 else 0, dtype=torch.int32, device="cuda"))
        done = ((term | trunc) != 0).cpu().numpy()
        _update_both(vec, w)                # the restatement reads the geometry the engine holds now
        after = _worlds(vec)
        ended += int(done.sum())
        moved += sum(int(done[i] and not (len(before[i]["segs"]) == len(after[i]["segs"]) and np.array_equal(before[i]["segs"], after[i]["segs"])))
                     for i in range(N))
    assert ended >= 2 * N and moved > 0          # (truncation after 4 steps: every env twice; new floor plans among them)
    vec.engine.check()
    vec.close()


# ---------------------------------------------------------------------------------------------------------------- refusals, collateral

def test_the_library_refuses_before_anything_is_launched():
    import torch
    from miniworld_amd import engine
    vec = _vec("MiniWorld-Hallway-v0")
    e = vec.engine
    w = vec.ego_window(size=9)
    seen = vec.seen_map()
    vec.ego_update(w, source=seen)
    w.planes.fill_(0x5C)
    sample = torch.full((N, 9, 9), 0x5C, dtype=torch.uint8, device="cuda")
    nan, inf = float("nan"), float("inf")
    good = dict(size=9, cell=0.25, back=0.0, wall_radius=0.125, entity_pad=0.125, max_range=10.0, cos_half=0.5, planes=7, flags=0)
    bad_grid = engine.MwNavParams(0.0, 0.0, 0.0, seen.gx, seen.gz, 0, 0)
    for change in (dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(cell=inf), dict(back=nan), dict(back=inf), dict(wall_radius=-0.1), dict(wall_radius=nan),
                   dict(wall_radius=inf), dict(entity_pad=-0.1), dict(entity_pad=inf), dict(max_range=0.0), dict(max_range=inf), dict(max_range=nan),
                   dict(cos_half=1.5), dict(cos_half=-1.5), dict(cos_half=nan), dict(flags=4), dict(planes=15), dict(src_params=bad_grid)):
        kw = dict(good, out=w.planes, src_params=seen.params, src=seen.seen, sample=sample)
        kw.update(change)
        with pytest.raises(engine.EngineError):
            e.ego_map(**kw)
        assert (w.planes == 0x5C).all() and (sample == 0x5C).all(), change
    # without VISIBLE the sight's numbers are not read
    e.ego_map(**dict(good, planes=3, max_range=nan, cos_half=nan, out=torch.zeros((N, 2, 9, 9), dtype=torch.uint8, device="cuda")))
    e.check()
    vec.close()


def test_updates_in_between_leave_a_stepped_batch_alone():
    import torch
    rng = np.random.default_rng(3404)
    acts = rng.integers(0, 3, (10, N))
    runs = []
    for with_windows in (False, True):
        vec = _vec("MiniWorld-FourRooms-v0")
        w = vec.ego_window(obstacles="walls+entities") if with_windows else None
        seen = vec.seen_map() if with_windows else None
        rows = []
        for a in acts:
            obs, rew, term, trunc = vec.step(torch.as_tensor(a, dtype=torch.int32, device="cuda"))
            rows.append((obs.clone(), rew.clone(), term.clone(), trunc.clone()))
            if with_windows:
                vec.ego_update(w, source=seen)
        rows.append(tuple(v.clone() for v in vec.state().values()))
        vec.engine.check()
        vec.close()
        runs.append(rows)
    for k, (a, b) in enumerate(zip(*runs)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), k
