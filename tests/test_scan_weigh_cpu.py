"""Scan weighing and resampling without a GPU: the kernels' phases (csrc/mw_weigh.h) on the host under sanitizers
(hostcheck/scan_weigh.cpp), bit for bit against scan_weigh_reference.py under both forms' host paths; the launches and the interface."""
import numpy as np
import pytest

import scan_reference as scan
import scan_weigh_reference as ref
from helpers import stub_engine
from match_reference import plane_of
from query_checks import build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, launch_of, run, LAUNCH

RAY_MAX = PARTICLE_MAX = 4096


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("scan_weigh", tmp_path_factory.mktemp("scan_weigh"))


@pytest.mark.parametrize("gz,gx,shift,R,P", [g + c for g in ((103, 103, 1), (4, 12, 2), (1, 40, 3), (40, 1, 0)) for c in ((1, 1), (65, 63), (300, 65))])
def test_weigh_one_equals_the_restatement(program, tmp_path, gz, gx, shift, R, P):
    """every case of scan_reference at these counts, an env per run, under both forms' host paths"""
    rng, scored = np.random.default_rng(4900 + gz + R + P), 0
    extent = (scan.MIN[0], scan.MIN[0] + gx * scan.CELL - 0.1, scan.MIN[1], scan.MIN[1] + gz * scan.CELL - 0.1)
    for name in scan.CASES:
        origin, t, d, max_range = scan.case(name, rng, R, gx, gz)
        plane, pose = plane_of(rng, gz, gx), ref.poses_of(rng, P, origin, gx, gz, scan.MIN, scan.CELL)
        score, inside, best = ref.weigh(pose, t, d, max_range, scan.MIN[0], scan.MIN[1], scan.CELL, plane)
        for waves in (0, 1):
            lines = ["0", "0.0 0.0 0.0", " ".join(repr(v) for v in extent), f"{scan.CELL!r} {gx} {gz} {shift} {max_range!r} {R} {P} {waves}"]
            lines += [f"{float(a)!r} {float(x)!r} {float(z)!r}" for a, (x, z) in zip(t, d)] + [" ".join(repr(float(v)) for v in row) for row in pose]
            rows = run(program, tmp_path / "weigh.txt", lines + [" ".join(str(int(v)) for v in plane.ravel())])
            got = np.array([row.split() for row in rows[:-1]], np.int64)
            assert np.array_equal(got[:, 0], score) and np.array_equal(got[:, 1], inside), (name, waves, int((got[:, 0] != score).sum()))
            assert tuple(map(int, rows[-1].split())) == best + (1,), (name, waves)
        scored += int(score.max() > 0)
    assert R == 1 or scored >= len(scan.CASES) - 1       # (on the restatement alone: the cases score)


WEIGHTS = {"zero": lambda rng, P: np.zeros(P, np.uint64), "one": lambda rng, P: np.where(np.arange(P) == P // 3, 5, 0).astype(np.uint64),
           "equal": lambda rng, P: np.full(P, 3, np.uint64), "full": lambda rng, P: np.full(P, 2 ** 32 - 1, np.uint64),
           "random": lambda rng, P: rng.integers(0, 2 ** 32, P, dtype=np.uint64) * (rng.random(P) < 0.5).astype(np.uint64)}


@pytest.mark.parametrize("P,stride", [(1, 256), (64, 1), (65, 256), (1000, 256), (4096, 256)])
def test_resample_one_equals_the_restatement(program, tmp_path, P, stride):
    rng = np.random.default_rng(4950 + P)
    for name, make in WEIGHTS.items():
        w = make(rng, P)
        S = int(w.sum())
        for offset in (0, max(S - 1, 0), 2 ** 63 - 1):
            rows = run(program, tmp_path / "resample.txt", ["1", f"{P} {stride} {offset}", " ".join(str(int(v)) for v in w)])
            got, want = np.array([row.split() for row in rows], np.int64), ref.resample(w, offset)
            assert np.array_equal(got[:, 0], want) and np.array_equal(got[:, 1], 4 * want), (name, offset)
            draws = np.bincount(want, minlength=P)          # (on the restatement alone: the header's properties)
            assert (np.diff(want) >= 0).all() and (S == 0 or all(P * int(v) // S <= k <= -(-P * int(v) // S) for k, v in zip(draws.tolist(), w)))
            assert name not in ("zero", "equal") or np.array_equal(want, np.arange(P)), (name, offset)


def test_launches_and_interface(program):
    from miniworld_amd import engine
    names = LAUNCH + ("waves",)          # (the plane rounded up to 16, 24 bytes a beam, the tail's 16; a wavefront per particle below 128)
    for gz, gx, rays, P, forced, lds, waves in ((1, 1, 1, 1, 0, 16 + 24 + 16, 1), (103, 103, 256, 127, 0, 10624 + 6144 + 16, 1), (103, 103, 256, 128, 0, 10624 + 6144 + 16, 0),
                                                (103, 103, 256, 256, 2, 10624 + 6144 + 16, 1), (128, 256, RAY_MAX, PARTICLE_MAX, 1, 32768 + 98304 + 16, 0)):
        assert launch_of(program, 7, gz, gx, rays, P, forced, names=names) == {"grid": 7, "threads": 256, "lds": lds, "fits": 1, "waves": waves}, (gz, gx, rays, P)
        assert lds < 160 * 1024
    bad = ((0, 1, 1, 1), (128, 257, 1, 1), (4, 4, 0, 1), (4, 4, RAY_MAX + 1, 1), (4, 4, 1, 0), (4, 4, 1, PARTICLE_MAX + 1))
    assert all(launch_of(program, 7, *b, 0, names=names)["fits"] == 0 for b in bad)
    assert launch_of(program, 7, 1000) == {"grid": 7, "threads": 256, "lds": 8000 + 32, "fits": 1} and launch_of(program, 7, PARTICLE_MAX)["lds"] == 32768 + 32
    assert launch_of(program, 7, 0)["fits"] == launch_of(program, 7, PARTICLE_MAX + 1)["fits"] == 0
    assert (engine.WEIGH_MAX_PARTICLES, engine.RAY_MAX) == (PARTICLE_MAX, RAY_MAX)
    check_units_built("mw_weigh.hip", "mw_engine_weigh.hip")
    check_kernel("mw_weigh_kernel", "mw_weigh.hip")
    check_kernel("mw_resample_kernel", "mw_weigh.hip")
    check_does_not_wait("mw_engine_weigh.hip")
    check_refuses_null_engine("mw_scan_weigh", engine.MwNavParams(0.25, 0.0, 0.0, 4, 4, 0, 0), None, 1, 1, None, None, None, None, None, None, None, None, None)
    check_refuses_null_engine("mw_resample", 1, None, None, None, None, None, None, None)
    check_refuses_null_engine("mw_debug_set_weigh_form", 0)


def test_the_methods_call_and_refuse(monkeypatch):
    import torch
    from miniworld_amd.queries import ScanWeights
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    m = vec.scan_map()
    score, scan_ = torch.zeros((5, m.gz, m.gx), dtype=torch.uint8), {"t": torch.zeros((5, 9), dtype=torch.float64), "dir": torch.zeros((5, 9, 2), dtype=torch.float64)}
    poses = torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64).expand(5, 7, 3).contiguous()
    n0, r = len(lib.calls), vec.scan_weigh(score, scan_, poses, max_range=4.0, like=m)
    args = lib.calls[-1][1]
    assert [k[0] for k in lib.calls[n0:]] == ["mw_scan_weigh"] and isinstance(r, ScanWeights) and tuple(r.pose.shape) == (5, 7, 4)
    assert r.pose[2, 3].tolist() == [1.0, 2.0, float(torch.cos(poses[0, 0, 2])), float(torch.sin(poses[0, 0, 2]))] and list(args[2]) == [4.0] and list(args[3:5]) == [9, 7]
    assert [a.value for a in args[5:9]] == [score.data_ptr(), scan_["t"].data_ptr(), scan_["dir"].data_ptr(), r.pose.data_ptr()] and args[9] is None
    assert [a.value for a in args[10:13]] == [r.score.data_ptr(), r.inside.data_ptr(), r.best.data_ptr()]
    assert vec.scan_weigh(score, scan_, torch.zeros((5, 7, 4), dtype=torch.float64), into=r) is r
    weights = torch.tensor([[0, 1, 2 ** 32 - 1, 2 ** 40, -3, 7, 7]] * 5)
    out = vec.resample(weights, offset=torch.zeros(5, dtype=torch.int64), poses=r.pose)
    name, args = lib.calls[-1]
    assert name == "mw_resample" and args[1] == 7 and args[4] is None and [a.value for a in args[5:8]] == [out["ancestor"].data_ptr(), r.pose.data_ptr(), out["pose"].data_ptr()]
    assert vec.resample(weights.int(), into={"ancestor": out["ancestor"], "pose": None})["pose"] is None and lib.calls[-1][1][6] is None
    n0 = len(lib.calls)
    for kw in (dict(max_range=0.0), dict(max_range=float("inf")), dict(cell=0.5, like=m), dict(like=out), dict(score=score.bool()), dict(score=score[:4]),
               dict(scan=scan_["t"]), dict(scan={"t": scan_["t"].float(), "dir": scan_["dir"]}), dict(scan={"t": scan_["t"], "dir": scan_["dir"][:, :8]}),
               dict(poses=poses[:, :, :2]), dict(poses=poses.float()), dict(poses=poses[:, :0]), dict(poses=torch.zeros((5, 4097, 3), dtype=torch.float64)),
               dict(mask=[1] * 5), dict(into=m), dict(into=r, max_range=3.0), dict(into=r, poses=poses[:, :6].contiguous())):
        with pytest.raises(ValueError):
            vec.scan_weigh(**{"score": score, "scan": scan_, "poses": poses, **kw})
    for kw in (dict(weights=weights.double()), dict(weights=weights[:4]), dict(weights=weights[:, :0]), dict(offset=torch.zeros(5, dtype=torch.int32)), dict(offset=0),
               dict(poses=poses), dict(poses=r.pose[:, :6].contiguous()), dict(mask=[1] * 5), dict(into=r), dict(poses=r.pose, into={"ancestor": out["ancestor"], "pose": r.pose}),
               dict(poses=r.pose, into={"ancestor": out["ancestor"], "pose": None})):
        with pytest.raises(ValueError):
            vec.resample(**{"weights": weights, **kw})
    assert len(lib.calls) == n0         # nothing reached the library
