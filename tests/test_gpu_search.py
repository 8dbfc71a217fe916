"""Scan search on the GPU (vec.scan_search) against tests/match_reference.py and against scan_match; an env the grid does not cover."""
import numpy as np
import pytest

import match_reference as ref
import scan_reference as scan
from query_checks import dev, host, worlds
from query_checks import vec_env as _vec

pytestmark, N = pytest.mark.gpu, 8
_extents = lambda vec: [[float(v) for v in w["extent"]] for w in worlds(vec)]      # noqa: E731


# (1 x 40 at W = 128: 33 x 33 blocks, a batch of one; 128 x 256 with 4096 beams: the launch's largest planes and lists)
@pytest.mark.parametrize("gz,gx,R,K,W", [(103, 103, 65, 5, 40), (103, 103, 257, 5, 4), (4, 12, 65, 5, 33), (40, 1, 1, 1, 0), (1, 40, 65, 1, 128), (128, 256, 4096, 3, 3)])
def test_the_kernel_equals_the_restatement(gz, gx, R, K, W):
    """test_gpu_match.py's envs and cases, from `origin=`; then other planes under a zero mask byte on envs 2, 3: their rows stay; pruning on and off"""
    import math
    from miniworld_amd import engine
    from miniworld_amd.queries import ScanMap
    vec = _vec("MiniWorld-Hallway-v0", N)
    ext, cell = _extents(vec), 0.25
    while any((gx + 0.5) * cell <= e[1] - e[0] or (gz + 0.5) * cell <= e[3] - e[2] for e in ext):
        cell *= 2
    rng, names = np.random.default_rng(4950 + gz + R + W), scan.CASES + ("random",)
    grid = ScanMap(None, None, None, engine.MwNavParams(cell, 0.0, 0.0, gx, gz, 0, 0), R, 1.0, 20.0, "walls")
    cases = [scan.case(names[i], rng, R, gx, gz, (ext[i][0], ext[i][2]), cell) for i in range(N)]
    t = np.stack([np.where(c[1] < c[3], c[1], 20.0) for c in cases])            # (each case's own max_range cuts its beams: one call, one max_range)
    beams, origin = {"t": dev(t), "dir": dev(np.stack([c[2] for c in cases]))}, dev(np.array([(c[0][0], 9.0, c[0][1]) for c in cases]))
    mask, want = np.array([1, 1, 0, 0, 1, 1, 1, 1], np.uint8), [None] * N
    r = vec.scan_search(dev(np.zeros((N, gz, gx), np.uint8)), beams, origin, window=W, turn=0.1 if K > 1 else 0.0, turns=K, max_range=20.0, like=grid, stats=True)
    rot, total = [(math.cos(a), math.sin(a)) for a in r.angles.tolist()], K * ((2 * W + 8) // 8) ** 2
    for call in range(2):
        planes = np.stack([ref.plane_of(rng, gz, gx) for _ in range(N)])
        for i in range(N):
            if call == 0 or mask[i]:
                want[i] = ref.match(cases[i][0], t[i], cases[i][2], rot, W, 20.0, ext[i][0], ext[i][2], cell, planes[i])[:2]
        for prune in (True, False):
            vec.engine.debug_set_search_prune(prune)
            r.best.fill_(-7), r.score.fill_(-7)
            assert vec.scan_search(dev(planes), beams, origin, mask=dev(mask) if call else None, into=r) is r
            best, score, stats = host(r.best), host(r.score), host(r.stats)
            for i in range(N):
                if call == 0 or mask[i]:
                    assert ((best[i, 0], best[i, 1], best[i, 2]), score[i]) == want[i], (call, prune, i)
                    assert 1 <= stats[i, 0] <= stats[i, 1] == total and (prune or stats[i, 0] == total), (call, prune, i, stats[i])
                else:
                    assert (best[i] == -7).all() and score[i] == -7, (call, prune, i)
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("env_id", ["MiniWorld-FourRooms-v0", "MiniWorld-MazeS3-v0"])
def test_search_equals_match_on_the_map_the_engine_drew(env_id):
    """kernel to kernel at W = 4 and 32, on the obstacle plane scan_map_update drew and on it shifted by (+2 rows, -3 columns) with the scan
    cut to the beams whose shifted end cell stays in the grid (as test_gpu_match.py ties it): that gives (a, b) = (-3, 2)"""
    import torch
    from miniworld_amd import engine
    vec = _vec(env_id, N, seed=7)
    scan_ = vec.lidar(256)
    m = vec.scan_map()
    vec.scan_map_update(m, scan_)
    ext, st = dev(np.array(_extents(vec))), vec.state(("agent_pos",))["agent_pos"]
    col = torch.floor((st[:, 0] - ext[:, 0]).div(m.cell)[:, None] + scan_["t"] * (scan_["dir"][..., 0] / m.cell))
    row = torch.floor((st[:, 2] - ext[:, 2]).div(m.cell)[:, None] + scan_["t"] * (scan_["dir"][..., 1] / m.cell))
    inside = lambda row, col: (row >= 0) & (row < m.gz) & (col >= 0) & (col < m.gx)     # noqa: E731
    stays = (scan_["t"] < 10.0) & inside(row, col) & inside(row + 2, col - 3)
    shifted = torch.zeros_like(m.obstacle.contiguous())
    shifted[:, 2:, :-3] = m.obstacle[:, :-2, 3:]
    cut = dict(scan_, t=scan_["t"].masked_fill(~stays, float("nan")))
    for W in (4, 32):
        for plane, beams in ((m.obstacle.contiguous(), scan_), (shifted, cut)):
            a, b = vec.scan_match(plane, beams, window=W, turn=0.1, turns=3, like=m), vec.scan_search(plane, beams, window=W, turn=0.1, turns=3, like=m)
            assert torch.equal(a.best, b.best) and torch.equal(a.score, b.score) and bool((b.score > 0).all()), W
        assert torch.equal(b.best[:, 1:], torch.tensor([[-3, 2]] * N, dtype=torch.int32, device="cuda")) and torch.equal(b.score, stays.sum(1).int()), W
    vec.engine.check()
    # a grid of 3 x 3 cells covers no env's extent: zeros, the stats too, and check() raises once
    best, score, stats = (torch.full(shape, 7, dtype=torch.int32, device="cuda") for shape in ((N, 3), (N,), (N, 2)))
    vec.engine.scan_search(engine.MwNavParams(0.25, 0.0, 0.0, 3, 3, 0, 0), 10.0, ref.ROT5[:3], 40, torch.ones((N, 3, 3), dtype=torch.uint8, device="cuda"),
                           scan_["t"], scan_["dir"], best, score, stats)
    assert not best.any() and not score.any() and not stats.any()
    with pytest.raises(engine.EngineError, match="refused an env"):
        vec.engine.check()
    vec.engine.check()
    vec.close()
