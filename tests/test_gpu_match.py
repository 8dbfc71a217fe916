"""Scan matching on the GPU (mw_scan_match; vec.scan_match), bit for bit against tests/match_reference.py: the synthetic cases through
`origin=` and a mask; a tie to the scan-map kernel with no Python rule in between; an env the grid does not cover."""
import math

import numpy as np
import pytest

import match_reference as ref
import scan_reference as scan
from query_checks import dev, host, poses, worlds
from query_checks import vec_env as _vec

pytestmark, N = pytest.mark.gpu, 8
_extents = lambda vec: [[float(v) for v in w["extent"]] for w in worlds(vec)]      # noqa: E731


@pytest.mark.parametrize("gz,gx,R,K,W", [(gz, gx, 65, 5, 5) for gz, gx in scan.GRIDS] + [(103, 103, 257, 5, 1), (103, 103, 1, 1, 0), (4, 12, 65, 5, 32), (128, 256, 300, 1, 32), (128, 256, 4096, 3, 1)])
def test_the_kernel_equals_the_restatement(gz, gx, R, K, W):
    """an env per case (the random one twice) on a grid of its own over the Hallway's extent, from `origin=`, with the volume; then other
    planes into the same record under a zero mask byte on envs 2, 3: their rows stay.  103 x 103 is odd: the planes of the odd envs start
    off a 4-byte boundary.  volume=False gives the same best.  Then the engine's call with the test's own pairs, one of no unit length.
    128 x 256 with 4096 beams is the launch above 64 KiB of LDS."""
    import torch
    from miniworld_amd import engine
    from miniworld_amd.queries import ScanMap
    vec = _vec("MiniWorld-Hallway-v0", N)
    ext, cell = _extents(vec), 0.25
    while any((gx + 0.5) * cell <= e[1] - e[0] or (gz + 0.5) * cell <= e[3] - e[2] for e in ext):
        cell *= 2
    rng, names = np.random.default_rng(4800 + gz + R + W), scan.CASES + ("random",)
    grid = ScanMap(None, None, None, engine.MwNavParams(cell, 0.0, 0.0, gx, gz, 0, 0), R, 1.0, 20.0, "walls")
    cases = [scan.case(names[i], rng, R, gx, gz, (ext[i][0], ext[i][2]), cell) for i in range(N)]
    t = np.stack([np.where(c[1] < c[3], c[1], 20.0) for c in cases])            # (each case's own max_range cuts its beams: one call, one max_range)
    beams, origin = {"t": dev(t), "dir": dev(np.stack([c[2] for c in cases]))}, dev(np.array([(c[0][0], 9.0, c[0][1]) for c in cases]))
    mask, want, live = np.array([1, 1, 0, 0, 1, 1, 1, 1], np.uint8), [None] * N, dev(np.array([1, 1, 0, 0, 1, 1, 1, 1])) != 0
    kw = dict(window=W, turn=0.1 if K > 1 else 0.0, turns=K, max_range=20.0, like=grid)
    r, bare = vec.scan_match(dev(np.zeros((N, gz, gx), np.uint8)), beams, origin, volume=True, **kw), vec.scan_match(dev(np.zeros((N, gz, gx), np.uint8)), beams, origin, **kw)
    rot = [(math.cos(a), math.sin(a)) for a in r.angles.tolist()]
    for call in range(2):
        planes = np.stack([ref.plane_of(rng, gz, gx) for _ in range(N)])
        assert vec.scan_match(dev(planes), beams, origin, mask=dev(mask) if call else None, into=r) is r
        for i in range(N):
            if call == 0 or mask[i]:
                want[i] = ref.match(cases[i][0], t[i], cases[i][2], rot, W, 20.0, ext[i][0], ext[i][2], cell, planes[i])
        best, score, volume = host(r.best), host(r.score), host(r.volume)
        for i in range(N):
            assert np.array_equal(volume[i], want[i][2]), (call, i, int((volume[i] != want[i][2]).sum()))
            assert (best[i, 0], best[i, 1], best[i, 2]) == want[i][0] and score[i] == want[i][1], (call, i)
    vec.scan_match(dev(planes), beams, origin, into=bare)
    assert bare.volume is None and torch.equal(bare.best[live], r.best[live]) and torch.equal(bare.score[live], r.score[live])
    assert R == 1 or sum(w[1] > 0 for w in want) >= N - 1
    vec.engine.scan_match(grid.params, 20.0, ref.ROT5[:K], W, dev(planes), beams["t"], beams["dir"], r.best, r.score, r.volume, origin)
    for i, v in enumerate(host(r.volume)):
        assert np.array_equal(v, ref.match(cases[i][0], t[i], cases[i][2], ref.ROT5[:K], W, 20.0, ext[i][0], ext[i][2], cell, planes[i])[2]), i
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("env_id", ["MiniWorld-FourRooms-v0", "MiniWorld-MazeS3-v0"])
def test_the_scan_fits_the_map_it_drew(env_id):
    """kernel to kernel: a scan matched on the obstacle plane its own scan_map_update drew scores the number of its beams with t < max_range
    that end in the grid (every such end byte is 1, none exceeds 1), at (0, 0, 0).  Then the plane shifted by (+2 rows, -3 columns) with zero fill:
    that pushes 12 to 127 of an env's end cells on the outer walls off the grid, so the scan is cut, by NaN, to the beams whose shifted end cell stays."""
    import torch
    vec = _vec(env_id, N, seed=7)
    scan_ = vec.lidar(256)
    m = vec.scan_map()
    vec.scan_map_update(m, scan_)
    ext, pose = dev(np.array(_extents(vec))), dev(np.array(poses(vec)))
    u1 = (pose[:, 0] - ext[:, 0]).div(m.cell)[:, None] + scan_["t"] * (scan_["dir"][..., 0] / m.cell)
    w1 = (pose[:, 1] - ext[:, 2]).div(m.cell)[:, None] + scan_["t"] * (scan_["dir"][..., 1] / m.cell)
    row, col, ends = torch.floor(w1), torch.floor(u1), scan_["t"] < 10.0
    inside = lambda row, col: (row >= 0) & (row < m.gz) & (col >= 0) & (col < m.gx)
    number = (ends & inside(row, col)).sum(1).int()
    r = vec.scan_match(m.obstacle.contiguous(), scan_, window=4, like=m, volume=True)
    assert bool((number > 0).all()) and torch.equal(r.score, number) and not bool(r.best.any()) and torch.equal(r.volume[:, 0, 4, 4], number) and int(m.obstacle.max()) == 1
    shifted = torch.zeros_like(m.obstacle.contiguous())
    shifted[:, 2:, :-3] = m.obstacle[:, :-2, 3:]
    stays = ends & inside(row, col) & inside(row + 2, col - 3)
    cut = dict(scan_, t=scan_["t"].masked_fill(~stays, float("nan")))
    number = stays.sum(1).int()
    r = vec.scan_match(shifted, cut, window=4, like=m, volume=True)
    assert bool((number > 0).all()) and torch.equal(r.volume[:, 0, 4 + 2, 4 - 3], number) and torch.equal(r.score, number)
    vec.engine.check()
    vec.close()


def test_an_env_the_grid_does_not_cover_gets_zeros():
    import torch
    from miniworld_amd import engine
    vec = _vec("MiniWorld-Hallway-v0", N)
    scan_ = vec.lidar(64)
    full = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device="cuda")
    best, score, volume = full(N, 3), full(N), full(N, 3, 5, 5)
    vec.engine.scan_match(engine.MwNavParams(0.25, 0.0, 0.0, 3, 3, 0, 0), 10.0, ref.ROT5[:3], 2, torch.ones((N, 3, 3), dtype=torch.uint8, device="cuda"),
                          scan_["t"], scan_["dir"], best, score, volume)
    assert not best.any() and not score.any() and not volume.any()
    with pytest.raises(engine.EngineError, match="refused an env"):
        vec.engine.check()
    vec.engine.check()
    vec.close()
