"""Scan matching without a GPU: the kernel's phases (csrc/mw_match.h) on the host under sanitizers (hostcheck/grid_match.cpp), bit for
bit against match_reference.py; the tie rule; the launch and the interface."""
import numpy as np
import pytest

import match_reference as ref
import scan_reference as scan
from helpers import stub_engine
from query_checks import build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, launch_of, run, LAUNCH

RAY_MAX = 4096


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("grid_match", tmp_path_factory.mktemp("grid_match"))


def _run(program, path, gz, gx, shift, origin, t, d, max_range, rot, W, plane, agent=False, quad=0):
    """the program on one env: (best, score, volume) as match_reference.match returns them"""
    extent = (scan.MIN[0], scan.MIN[0] + gx * scan.CELL - 0.1, scan.MIN[1], scan.MIN[1] + gz * scan.CELL - 0.1)
    lines = [f"{origin[0]!r} {origin[1]!r} 0.0", " ".join(repr(v) for v in extent),
             f"{scan.CELL!r} {gx} {gz} {shift} {max_range!r} {len(t)} {len(rot)} {W} {0 if agent else 1} {quad} {origin[0]!r} {origin[1]!r}"]
    lines += [f"{float(c)!r} {float(s)!r}" for c, s in rot] + [f"{float(a)!r} {float(x)!r} {float(z)!r}" for a, (x, z) in zip(t, d)]
    rows = run(program, path, lines + [" ".join(str(int(v)) for v in plane.ravel())])
    r, a, b, score, covered = map(int, rows[0].split())
    assert covered == 1
    return (r, a, b), score, np.array([row.split() for row in rows[1:]], np.int64).reshape(len(rot), 2 * W + 1, 2 * W + 1)


# (shift: the plane's distance from a 4-byte boundary)
@pytest.mark.parametrize("gz,gx,shift,R,K,W", [g + c for g in ((103, 103, 1), (4, 12, 2), (1, 40, 3), (40, 1, 0)) for c in ((1, 1, 0), (65, 5, 1), (257, 5, 5), (65, 1, 5))] + [(4, 12, 2, 65, 5, 32)])
def test_match_one_equals_the_restatement(program, tmp_path, gz, gx, shift, R, K, W):
    """every case of scan_reference at these counts, an env per run, from the agent or an origin in turn; W = 32 once, on 4 x 12"""
    rng, rot = np.random.default_rng(4600 + gz + R + W), ref.ROT5[:K]
    for run_no, name in enumerate(scan.CASES):
        origin, t, d, max_range = scan.case(name, rng, R, gx, gz)
        plane = ref.plane_of(rng, gz, gx)
        want = ref.match(origin, t, d, rot, W, max_range, scan.MIN[0], scan.MIN[1], scan.CELL, plane)
        for quad in (0, 1):         # (both forms of the correlation)
            got = _run(program, tmp_path / "match.txt", gz, gx, shift, origin, t, d, max_range, rot, W, plane, agent=run_no % 2 == 0, quad=quad)
            assert np.array_equal(got[2], want[2]), (name, quad, int((got[2] != want[2]).sum()))
            assert got[:2] == want[:2], (name, quad, got[:2], want[:2])
        assert R == 1 or want[1] > 0, name         # (on the restatement alone: the case scores; one beam without a window may miss)


def _centre_fan(rng, R):
    """beams that stay well inside 103 x 103 under every rotation and a window of 5: from the centre, up to 3 m = 12 cells"""
    ang = rng.uniform(0, 2 * np.pi, R)
    return (scan.MIN[0] + 51.5 * scan.CELL, scan.MIN[1] + 51.5 * scan.CELL), rng.uniform(0.5, 3.0, R), np.stack([np.cos(ang), -np.sin(ang)], 1), 6.0


def test_a_constant_plane_gives_the_guess(program, tmp_path):
    (origin, t, d, max_range), plane = _centre_fan(np.random.default_rng(4700), 65), np.full((103, 103), 7, np.uint8)
    got = _run(program, tmp_path / "flat.txt", 103, 103, 1, origin, t, d, max_range, ref.ROT5, 5, plane, quad=1)
    assert got[:2] == ((0, 0, 0), 7 * 65) == ref.match(origin, t, d, ref.ROT5, 5, max_range, scan.MIN[0], scan.MIN[1], scan.CELL, plane)[:2] and (got[2] == 7 * 65).all()


@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("peaks,best", [(((2, 1), (-2, -1)), (0, -1, -2)), (((1, 2), (1, -2)), (0, -2, 1))])
def test_equal_peaks_go_to_the_lower_b_then_a(program, tmp_path, peaks, best, quad):
    """one beam, two equal isolated peaks at offsets (b, a) of one a^2 + b^2 from its end cell: the lower b wins, then the lower a"""
    origin, t, d, max_range = _centre_fan(np.random.default_rng(4701), 1)
    row, col = int(np.floor(51.5 + t[0] * d[0, 1] / scan.CELL)), int(np.floor(51.5 + t[0] * d[0, 0] / scan.CELL))
    plane = np.zeros((103, 103), np.uint8)
    for b, a in peaks:
        plane[row + b, col + a] = 200
    got = _run(program, tmp_path / "peaks.txt", 103, 103, 3, origin, t, d, max_range, ref.ROT5[:1], 3, plane, quad=quad)
    assert got[:2] == (best, 200) == ref.match(origin, t, d, ref.ROT5[:1], 3, max_range, scan.MIN[0], scan.MIN[1], scan.CELL, plane)[:2] and int((got[2] == 200).sum()) == 2


def test_launch_and_interface(program):
    from miniworld_amd import engine
    names = LAUNCH + ("quad", "batch")       # (the quad form above 256 candidates; the pads' 144 bytes; the batch: lanes / tasks, <= 8, <= RAY_MAX / rays)
    for gz, gx, rays, W, lds, quad, batch in ((1, 1, 1, 0, 16 + 64 + 272, 0, 8), (103, 103, 256, 1, 10624 + 16384 + 272, 0, 8), (103, 103, 256, 10, 10768 + 4096 + 272, 1, 2),
                                              (128, 256, RAY_MAX, 32, 32912 + 32768 + 272, 1, 1)):
        assert launch_of(program, 7, gz, gx, rays, W, names=names) == {"grid": 7, "threads": 256, "lds": lds, "fits": 1, "quad": quad, "batch": batch}, (gz, gx, rays, W)
    bad = ((0, 1, 1, 0), (1, 0, 1, 0), (128, 257, 1, 0), (4, 4, 0, 0), (4, 4, RAY_MAX + 1, 0), (4, 4, 1, -1), (4, 4, 1, 33))
    assert all(launch_of(program, 7, *b)["fits"] == 0 for b in bad)
    assert (engine.MATCH_MAX_ROT, engine.MATCH_MAX_WINDOW, engine.RAY_MAX) == (64, 32, RAY_MAX)
    check_units_built("mw_match.hip", "mw_engine_match.hip")
    check_kernel("mw_match_kernel", "mw_match.hip")
    check_does_not_wait("mw_engine_match.hip")
    check_refuses_null_engine("mw_scan_match", engine.MwNavParams(0.25, 0.0, 0.0, 4, 4, 0, 0), None, None, 1, 0, 1, None, None, None, None, None, None, None, None, None)


def test_scan_match_calls_and_argument_errors(monkeypatch):
    import torch
    from miniworld_amd.queries import ScanMatch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    m = vec.scan_map()
    score, scan_ = torch.zeros((5, m.gz, m.gx), dtype=torch.uint8), {"t": torch.zeros((5, 9), dtype=torch.float64), "dir": torch.zeros((5, 9, 2), dtype=torch.float64)}
    origin = torch.zeros((5, 3), dtype=torch.float64)
    n0, r = len(lib.calls), vec.scan_match(score, scan_, origin, window=2, turn=0.2, turns=5, max_range=4.0, like=m, volume=True)
    args = lib.calls[-1][1]
    assert [k[0] for k in lib.calls[n0:]] == ["mw_scan_match"] and isinstance(r, ScanMatch) and tuple(r.volume.shape) == (5, 5, 5, 5)
    assert r.angles.tolist() == pytest.approx([0.0, 0.1, -0.1, 0.2, -0.2]) and list(args[3])[:4] == [1.0, 0.0, np.cos(0.1), np.sin(0.1)] and list(args[2]) == [4.0]
    assert list(args[4:7]) == [5, 2, 9] and [a.value for a in args[7:11]] == [score.data_ptr(), scan_["t"].data_ptr(), scan_["dir"].data_ptr(), origin.data_ptr()]
    assert args[11] is None and [a.value for a in args[12:15]] == [r.best.data_ptr(), r.score.data_ptr(), r.volume.data_ptr()]
    assert vec.scan_match(score, scan_, into=r) is r and lib.calls[-1][1][10] is None and not bool(r.offset().any())
    turned, moved = r.apply(scan_, origin)
    assert turned["t"] is scan_["t"] and turned["dir"].shape == scan_["dir"].shape and torch.equal(moved, origin)
    n0 = len(lib.calls)
    for kw in (dict(window=33), dict(window=-1), dict(window=1.5), dict(turns=2, turn=0.1), dict(turns=3), dict(turns=65, turn=0.1), dict(turn=0.1),
               dict(turn=float("nan"), turns=3), dict(max_range=0.0), dict(max_range=float("inf")), dict(cell=0.5, like=m), dict(like=r), dict(volume=1),
               dict(score=score.bool()), dict(score=score[:4]), dict(score=score[:, :, :-1]), dict(scan=scan_["t"]), dict(scan={"t": scan_["t"]}),
               dict(scan={"t": scan_["t"].float(), "dir": scan_["dir"]}), dict(scan={"t": scan_["t"], "dir": scan_["dir"][:, :8]}), dict(origin=origin[:, :2]),
               dict(origin=origin.float()), dict(mask=[1] * 5), dict(into=m), dict(into=r, window=3)):
        with pytest.raises(ValueError):
            vec.scan_match(**{"score": score, "scan": scan_, **kw})
    assert len(lib.calls) == n0         # nothing reached the library
