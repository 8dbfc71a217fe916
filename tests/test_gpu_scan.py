"""Scan maps on the GPU (mw_scan_project; vec.scan_map / scan_map_update), bit for bit against tests/scan_reference.py: the synthetic cases
through `origin=`, live lidar scans over steps; a tie to the ray-cast and seen-map kernels; the grid calls and the vector env on the map."""
import math

import numpy as np
import pytest

import scan_reference as ref
from query_checks import dev, host, poses, worlds
from query_checks import vec_env as _vec

pytestmark, N = pytest.mark.gpu, 8
_extents = lambda vec: [[float(v) for v in w["extent"]] for w in worlds(vec)]      # noqa: E731


def _check(m, planes, count, new, mask=None):
    got_map, got_count, got_new = host(m.map), host(m.count), host(m.new)
    for i in range(N):
        for k in range(2):
            assert np.array_equal(got_map[i, k], planes[i][k]), (i, k, int((got_map[i, k] != planes[i][k]).sum()))
        assert got_count[i].tolist() == count[i].tolist() and (mask is not None and not mask[i] or got_new[i].tolist() == new[i].tolist()), i


@pytest.mark.parametrize("gz,gx,R", [(gz, gx, 65) for gz, gx in ref.GRIDS] + [(103, 103, 1), (103, 103, 4096)])
def test_the_kernel_equals_the_restatement(gz, gx, R):
    """an env per case (the random one twice) on a grid of its own over the Hallway's extent, from `origin=`; then random beams under
    `clear` on envs 1, 2, 5 and a zero mask byte on envs 2, 3.  103 x 103 is odd: the maps of the odd envs start off a 4-byte boundary."""
    import torch
    from miniworld_amd import engine
    from miniworld_amd.queries import ScanMap
    vec = _vec("MiniWorld-Hallway-v0", N)
    ext, cell = _extents(vec), 0.25
    while any((gx + 0.5) * cell <= e[1] - e[0] or (gz + 0.5) * cell <= e[3] - e[2] for e in ext):
        cell *= 2
    rng, names = np.random.default_rng(4500 + gz + R), ref.CASES + ("random",)
    planes, count = [np.zeros((2, gz, gx), np.uint8) for _ in range(N)], [np.zeros(2, np.int64) for _ in range(N)]
    clear, mask = np.array([0, 1, 1, 0, 0, 1, 0, 0], np.uint8), np.array([1, 1, 0, 0, 1, 1, 1, 1], np.uint8)
    for call in range(2):
        cases = [ref.case(names[i] if call == 0 else "random", rng, R, gx, gz, (ext[i][0], ext[i][2]), cell) for i in range(N)]
        max_range = 6.0 if call else 20.0       # (the first call cuts no case short of its own max_range: each t is capped first)
        t = np.stack([np.where(c[1] < c[3], c[1], max_range) if call == 0 else c[1] for c in cases])
        m = ScanMap(dev(np.stack(planes)), dev(np.stack(count), torch.int32), dev(np.zeros((N, 2), np.int32)), engine.MwNavParams(cell, 0.0, 0.0, gx, gz, 0, 0), R, 2 * math.pi, max_range, "walls")
        scan = {"t": dev(t), "dir": dev(np.stack([c[2] for c in cases]))}
        origin = dev(np.array([(c[0][0], 9.0, c[0][1]) for c in cases]))
        assert vec.scan_map_update(m, scan, origin=origin, clear=dev(clear) if call else None, mask=dev(mask) if call else None) is m.new
        new = [ref.update(planes[i], count[i], *ref.sets(cases[i][0], t[i], cases[i][2], max_range, ext[i][0], ext[i][2], cell, gx, gz), clear=call == 1 and bool(clear[i]))
               if call == 0 or mask[i] else None for i in range(N)]
        _check(m, planes, count, new, mask if call else None)
    assert sum(int(p[0].sum()) for p in planes) > N and sum(int(p[1].sum()) for p in planes) > 0
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("env_id", ["MiniWorld-Hallway-v0", "MiniWorld-FourRooms-v0", "MiniWorld-MazeS3-v0"])
@pytest.mark.parametrize("R", [1, 64, 257])
def test_live_scans_over_steps(env_id, R):
    """scan_map_update's own lidar() from the agents, three steps: clear = done and env `step`, envs 3 and 6 masked off at step 1"""
    import torch
    vec = _vec(env_id, N, seed=3)
    m = vec.scan_map(rays=R, fov=2 * math.pi if R != 64 else 2.0, max_range=5.0)
    g = torch.Generator(device="cuda").manual_seed(11)
    planes, count = [np.zeros((2, m.gz, m.gx), np.uint8) for _ in range(N)], [np.zeros(2, np.int64) for _ in range(N)]
    for step in range(3):
        _, _, term, trunc = vec.step(torch.randint(0, 3, (N,), generator=g, device="cuda", dtype=torch.int32))
        clear = (term | trunc).to(torch.uint8)
        clear[step] = 1
        mask = np.array([1, 1, 1, step != 1, 1, 1, step != 1, 1], np.uint8)
        vec.scan_map_update(m, clear=clear, mask=dev(mask))
        scan, ext, pose, cl = vec.lidar(R, m.fov, 5.0, obstacles="walls+entities"), _extents(vec), poses(vec), host(clear)
        t, d = host(scan["t"]), host(scan["dir"])
        new = [ref.update(planes[i], count[i], *ref.sets(pose[i][:2], t[i], d[i], 5.0, ext[i][0], ext[i][2], m.cell, m.gx, m.gz), clear=bool(cl[i])) if mask[i] else None
               for i in range(N)]
        _check(m, planes, count, new, mask)
    assert all(p[0].any() for p in planes) and (R == 1 or any(p[1].any() for p in planes))
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("env_id", ["MiniWorld-FourRooms-v0", "MiniWorld-MazeS3-v0"])
def test_rays_to_the_seen_cells_mark_them_free(env_id):
    """kernel to kernel: a ray from each agent to the centre of every cell of a 33 x 33 window about its own (direction = centre - origin,
    max_t = 1; NaN off the grid), traced with max_range = 1.  Every cell a fresh all-round seen_map of 4 m holds is then marked, 0 exceptions:
    free, unless it is in the call's obstacle set, which by the rule takes a cell out of the free one — a blocked ray to a farther cell ends on
    a wall in or on the edge of a cell whose own centre is in sight (measured: 56 of 3 618 seen cells in FourRooms, 120 of 3 125 in MazeS3) —;
    and the obstacle cells are exactly the cells that hold origin + t * dir of the blocked rays."""
    import torch
    vec = _vec(env_id, N, seed=5)
    seen = vec.seen_map(max_range=4.0, fov=2 * math.pi)
    vec.seen_update(seen)
    m = vec.scan_map(like=seen, max_range=1.0)
    ext, pose = np.array(_extents(vec)), np.array(poses(vec))
    lo, pos = dev(ext[:, [0, 2]]), dev(pose[:, :2])
    k = torch.arange(-16, 17, device="cuda", dtype=torch.float64)
    own = torch.floor((pos - lo) / m.cell)                                                       # [N, 2]: the agent's cell (i, j)
    ci, cj = (own[:, 0, None, None] + k[None, None, :]).expand(N, 33, 33), (own[:, 1, None, None] + k[None, :, None]).expand(N, 33, 33)
    centre = torch.stack([lo[:, 0, None, None] + (ci + 0.5) * m.cell, lo[:, 1, None, None] + (cj + 0.5) * m.cell], -1)
    off = (ci < 0) | (ci >= m.gx) | (cj < 0) | (cj >= m.gz)
    dirs = (centre - pos[:, None, None, :]).masked_fill(off[..., None], float("nan")).reshape(N, 33 * 33, 2).contiguous()
    r = vec.raycast(direction=dirs, max_t=1.0)
    vec.scan_map_update(m, {"t": r["t"], "dir": dirs})
    held, free, obstacle = seen.seen != 0, m.free != 0, m.obstacle != 0                         # (printed: the figures of the docstring)
    print(env_id, "seen", int(held.sum()), "not free", int((held & ~free).sum()), "unmarked", int((held & ~free & ~obstacle).sum()))
    assert int(held.sum()) > N * 20 and int((held & ~free & ~obstacle).sum()) == 0
    t, d = host(r["t"]), host(dirs)
    for i in range(N):
        want = np.zeros((m.gz, m.gx), bool)
        b = (t[i] < 1.0) & ~np.isnan(d[i, :, 0])
        u = (pose[i, 0] - ext[i, 0]) / m.cell + t[i][b] * (d[i][b, 0] / m.cell)
        w = (pose[i, 1] - ext[i, 2]) / m.cell + t[i][b] * (d[i][b, 1] / m.cell)
        ok = (u >= 0) & (u < m.gx) & (w >= 0) & (w < m.gz)
        want[np.floor(w[ok]).astype(int), np.floor(u[ok]).astype(int)] = True
        assert np.array_equal(host(obstacle[i]), want), i
    assert bool(obstacle.any()) and bool((held & ~free)[~obstacle].logical_not().all())
    vec.engine.check()
    vec.close()


def test_the_grid_calls_and_the_vector_env_take_the_map():
    import torch
    from miniworld_amd.vector import MiniWorldVectorEnv
    env = MiniWorldVectorEnv("MiniWorld-FourRooms-v0", N, scan_map=dict(rays=128))
    _, info = env.reset(seed=1)
    vec, m = env.vec, env.scan
    assert torch.equal(info["scan_map"], m.map) and torch.equal(m.count, m.new) and bool(((m.free == 0) & (m.obstacle == 0)).any())
    assert m.count.tolist() == [[int(m.free[i].sum()), int(m.obstacle[i].sum())] for i in range(N)] and not bool(((m.free != 0) & (m.obstacle != 0)).any())
    f, c = vec.grid_field(m.obstacle != 0, sources=m.free != 0, like=m), vec.grid_clearance(m.obstacle != 0, like=m)
    assert (f.gx, f.gz, c.gx, c.gz) == (m.gx, m.gz) * 2 and vec.depth_map(like=m).gx == vec.scan_map(like=f).gx == m.gx and torch.equal(c.dist2 == 0, m.obstacle != 0) and bool((f.field.view(torch.int16) == 0).any())
    _, _, _, _, info = env.step(torch.full((N,), 2, dtype=torch.int32, device="cuda"))
    assert torch.equal(info["scan_map"], m.map) and bool((m.count >= m.new).all()) and int(m.new.sum()) > 0
    vec.engine.check()
    env.close()
