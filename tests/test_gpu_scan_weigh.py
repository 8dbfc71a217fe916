"""Scan weighing and resampling on the GPU (mw_scan_weigh, mw_resample), bit for bit against tests/scan_weigh_reference.py: every launch
form, a mask, the capacity limit, the tie to the scan-match kernel, an env the grid does not cover, the resampling cases."""
import numpy as np
import pytest

import scan_reference as scan
import scan_weigh_reference as ref
from match_reference import plane_of
from query_checks import dev, host, worlds
from query_checks import vec_env as _vec

pytestmark, N = pytest.mark.gpu, 8
MASK = np.array([1, 1, 0, 0, 1, 1, 1, 1], np.uint8)


@pytest.fixture(scope="module")
def vec():
    v = _vec("MiniWorld-Hallway-v0", N)
    yield v
    v.close()


def _grid(vec, gz, gx):
    """(extents, cell, params): the smallest doubling of 0.25 m at which gz x gx cells cover every env's extent"""
    from miniworld_amd import engine
    ext, cell = [[float(v) for v in w["extent"]] for w in worlds(vec)], 0.25
    while any((gx + 0.5) * cell <= e[1] - e[0] or (gz + 0.5) * cell <= e[3] - e[2] for e in ext):
        cell *= 2
    return ext, cell, engine.MwNavParams(cell, 0.0, 0.0, gx, gz, 0, 0)


def _planes(rng, n, gz, gx):
    """an empty plane, a full one, then two thirds of the cells set"""
    return np.stack([np.zeros((gz, gx), np.uint8), np.full((gz, gx), 255, np.uint8)] + [plane_of(rng, gz, gx) for _ in range(n - 2)])


@pytest.mark.parametrize("R", [1, 65, 300])
@pytest.mark.parametrize("gz,gx", scan.GRIDS)
def test_the_weigh_kernel_equals_the_restatement(vec, gz, gx, R):
    """an env per scan case and plane density; the particles through the engine's call (a NaN or no unit (c, s) cannot come from an angle)
    under the policy's form and each form forced; then other planes under a zero mask byte on envs 2, 3: their rows stay.  103 x 103 is
    odd: the planes of the odd envs start off a 4-byte boundary.  Last the binding's call, against the rows it reports."""
    import torch
    ext, cell, params = _grid(vec, gz, gx)
    rng, names = np.random.default_rng(5000 + gz + R), scan.CASES + ("random",)
    cases = [scan.case(names[i], rng, R, gx, gz, (ext[i][0], ext[i][2]), cell) for i in range(N)]
    t = np.stack([np.where(c[1] < c[3], c[1], 20.0) for c in cases])            # (each case's own max_range cuts its beams: one call, one max_range)
    d_t, d_dir, counted = dev(t), dev(np.stack([c[2] for c in cases])), 0
    weigh = lambda i, pose, plane: ref.weigh(pose[i], t[i], cases[i][2], 20.0, ext[i][0], ext[i][2], cell, plane[i])       # noqa: E731
    for P in (1, 63, 65, 257, 1000):
        pose = np.stack([ref.poses_of(rng, P, cases[i][0], gx, gz, (ext[i][0], ext[i][2]), cell) for i in range(N)])
        planes, full = _planes(rng, N, gz, gx), lambda k: torch.full((N, k), -7, dtype=torch.int32, device="cuda")      # noqa: E731
        want = [weigh(i, pose, planes) for i in range(N)]
        counted += sum(int(w[1].sum() > 0) for w in want)
        for form in (0, 1, 2):
            out, inside, best = full(P), full(P), full(2)
            vec.engine.debug_set_weigh_form(form)
            vec.engine.scan_weigh(params, 20.0, dev(planes), d_t, d_dir, dev(pose), out, inside, best)
            if form == 2:       # (a second call under the mask, other planes: the masked rows keep the first call's)
                other = _planes(rng, N, gz, gx)[::-1].copy()
                vec.engine.scan_weigh(params, 20.0, dev(other), d_t, d_dir, dev(pose), out, inside, best, mask=dev(MASK))
                want = [weigh(i, pose, other) if MASK[i] else want[i] for i in range(N)]
            got = host(out), host(inside), host(best)
            for i in range(N):
                assert np.array_equal(got[0][i], want[i][0]) and np.array_equal(got[1][i], want[i][1]), (P, form, i, int((got[0][i] != want[i][0]).sum()))
                assert tuple(got[2][i]) == want[i][2], (P, form, i)
        vec.engine.debug_set_weigh_form(0)
    assert R == 1 or counted >= 5 * (N - 2)         # (on the restatement alone: beams count and end inside)
    from miniworld_amd.queries import ScanMap
    turns = dev(np.concatenate([pose[..., :2], rng.uniform(-4, 4, (N, P, 1))], 2))
    r = vec.scan_weigh(dev(planes), {"t": d_t, "dir": d_dir}, turns, max_range=20.0, like=ScanMap(None, None, None, params, R, 1.0, 20.0, "walls"))
    rows = host(r.pose)
    assert np.array_equal(rows[..., :2], pose[..., :2], equal_nan=True) and torch.equal(r.pose[..., 2], torch.cos(turns[..., 2])) and torch.equal(r.pose[..., 3], torch.sin(turns[..., 2]))
    for i in range(N):
        score, inside, best = weigh(i, rows, planes)
        assert np.array_equal(host(r.score)[i], score) and np.array_equal(host(r.inside)[i], inside) and tuple(host(r.best)[i]) == best, i
    vec.engine.check()


def test_the_capacity_limit():
    """128 x 256 cells, 4096 beams, 4096 particles: 128 KiB of LDS, and on the full plane of env 0 the int32 bound 4096 * 255"""
    import torch
    vec, (gz, gx, R, P) = _vec("MiniWorld-Hallway-v0", 2), (128, 256, 4096, 4096)
    ext, cell, params = _grid(vec, gz, gx)
    rng = np.random.default_rng(5100)
    ang, planes = rng.uniform(0, 2 * np.pi, (2, R)), np.stack([np.full((gz, gx), 255, np.uint8), plane_of(rng, gz, gx)])
    t, d = rng.uniform(0, 8 * cell, (2, R)), np.stack([np.cos(ang), -np.sin(ang)], 2)
    pose = np.stack([ref.poses_of(rng, P, (ext[i][0] + 0.5 * gx * cell, ext[i][2] + 0.5 * gz * cell), gx, gz, (ext[i][0], ext[i][2]), cell) for i in range(2)])
    for form in (1, 2):
        out, inside, best = (torch.full(s, -7, dtype=torch.int32, device="cuda") for s in ((2, P), (2, P), (2, 2)))
        vec.engine.debug_set_weigh_form(form)
        vec.engine.scan_weigh(params, 20.0, dev(planes), dev(t), dev(d), dev(pose), out, inside, best)
        for i in range(2):
            parts = [ref.weigh(pose[i, k:k + 512], t[i], d[i], 20.0, ext[i][0], ext[i][2], cell, planes[i]) for k in range(0, P, 512)]
            score = np.concatenate([p[0] for p in parts])
            assert np.array_equal(host(out)[i], score) and np.array_equal(host(inside)[i], np.concatenate([p[1] for p in parts])), (form, i)
            assert tuple(host(best)[i]) == (int(np.argmax(score)), int(score.max())), (form, i)
        assert int(out[0].max()) == 4096 * 255
    vec.engine.check()
    vec.close()


def test_particles_at_the_matchers_rotations_score_its_volume(vec):
    """kernel to kernel: particles at (origin, ScanMatch.rot[r]) score volume[:, r, W, W] exactly, on the map the scan itself drew"""
    import torch
    scan_, W = vec.lidar(256), 2
    m = vec.scan_map()
    vec.scan_map_update(m, scan_)
    origin, plane = vec.state(("agent_pos",))["agent_pos"].contiguous(), m.obstacle.contiguous()
    r = vec.scan_match(plane, scan_, origin, window=W, turn=0.3, turns=7, like=m, volume=True)
    pose = torch.cat([origin[:, None, [0, 2]].expand(N, 7, 2), r.rot[None].expand(N, 7, 2)], 2).contiguous()
    out = torch.full((N, 7), -7, dtype=torch.int32, device="cuda")
    vec.engine.scan_weigh(m.params, 10.0, plane, scan_["t"], scan_["dir"], pose, out)
    assert torch.equal(out, r.volume[:, :, W, W]) and bool((out[:, 0] > 0).all())
    vec.engine.check()


def test_an_env_the_grid_does_not_cover_gets_zeros(vec):
    import torch
    from miniworld_amd import engine
    scan_ = vec.lidar(64)
    out, inside, best = (torch.full(s, 7, dtype=torch.int32, device="cuda") for s in ((N, 5), (N, 5), (N, 2)))
    vec.engine.scan_weigh(engine.MwNavParams(0.25, 0.0, 0.0, 3, 3, 0, 0), 10.0, torch.ones((N, 3, 3), dtype=torch.uint8, device="cuda"), scan_["t"], scan_["dir"],
                          torch.zeros((N, 5, 4), dtype=torch.float64, device="cuda"), out, inside, best)
    assert not out.any() and not inside.any() and not best.any()
    with pytest.raises(engine.EngineError, match="refused an env"):
        vec.engine.check()
    vec.engine.check()


@pytest.mark.parametrize("P", [1, 64, 65, 1000, 4096])
def test_the_resample_kernel_equals_the_restatement(vec, P):
    """an env per kind of weights (all 2^32 - 1 at P = 4096: the 2^56 bound) under the offsets 0, S - 1 and 2^63 - 1; the poses are the gather
    by the ancestors; then other weights under a zero mask byte on envs 2, 3: their rows stay"""
    import torch
    rng = np.random.default_rng(5200 + P)
    half = lambda: rng.integers(0, 2 ** 32, P) * (rng.random(P) < 0.5)         # noqa: E731
    w = np.stack([np.zeros(P, np.int64), np.where(np.arange(P) == P // 3, 5, 0), np.full(P, 3), np.full(P, 2 ** 32 - 1)] + [half() for _ in range(N - 4)]).astype(np.int64)
    S, poses = w.sum(1), dev(rng.normal(size=(N, P, 4)))
    for offset in (np.zeros(N, np.int64), np.maximum(S - 1, 0), np.full(N, 2 ** 63 - 1, np.int64)):
        out = vec.resample(dev(w), dev(offset), poses)
        want = np.stack([ref.resample(w[i], offset[i]) for i in range(N)])
        assert np.array_equal(host(out["ancestor"]), want), int((host(out["ancestor"]) != want).sum())
        assert torch.equal(out["pose"], torch.gather(poses, 1, dev(want)[..., None].expand(N, P, 4)))
        assert np.array_equal(want[0], np.arange(P)) and np.array_equal(want[2], np.arange(P)) and (want[1] == P // 3).all()
    other = w[::-1].copy()
    vec.resample(dev(other), dev(offset), poses, mask=dev(MASK), into=out)
    want = np.stack([ref.resample(other[i], offset[i]) if MASK[i] else want[i] for i in range(N)])
    assert np.array_equal(host(out["ancestor"]), want) and torch.equal(out["pose"], torch.gather(poses, 1, dev(want)[..., None].expand(N, P, 4)))
    small = w % 1000         # (int32 weights are the same words)
    assert torch.equal(vec.resample(dev(small.astype(np.int32)), dev(offset))["ancestor"], vec.resample(dev(small), dev(offset))["ancestor"])
    vec.engine.check()
