"""Scan search without a GPU: csrc/mw_search.h's phases on the host under sanitizers (hostcheck/grid_search.cpp) against match_reference.py; the interface."""
import numpy as np
import pytest

import match_reference as ref
import scan_reference as scan
from helpers import stub_engine
from query_checks import build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, launch_of, run, LAUNCH

RAY_MAX = 4096


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("grid_search", tmp_path_factory.mktemp("grid_search"))


def _run(program, path, gz, gx, shift, origin, t, d, max_range, rot, W, plane, agent=False):
    """the program on one env: ((best, score) with pruning on, stats of it, bounds int64[K, side, side] of the blocks); pruning off gives the same"""
    extent = (scan.MIN[0], scan.MIN[0] + gx * scan.CELL - 0.1, scan.MIN[1], scan.MIN[1] + gz * scan.CELL - 0.1)
    lines = [f"{origin[0]!r} {origin[1]!r} 0.0", " ".join(repr(v) for v in extent),
             f"{scan.CELL!r} {gx} {gz} {shift} {max_range!r} {len(t)} {len(rot)} {W} {0 if agent else 1} {origin[0]!r} {origin[1]!r}"]
    lines += [f"{float(c)!r} {float(s)!r}" for c, s in rot] + [f"{float(a)!r} {float(x)!r} {float(z)!r}" for a, (x, z) in zip(t, d)]
    rows = run(program, path, lines + [" ".join(str(int(v)) for v in plane.ravel())])
    on, off = (tuple(map(int, row.split())) for row in rows[:2])
    total, ns = len(rot) * ((2 * W + 8) // 8) ** 2, (2 * W + 8) // 8
    assert on[:5] == off[:5] and on[4] == 1 and 1 <= on[5] <= on[6] == total == off[5] == off[6], (on, off)
    return (on[:3], on[3]), on[5:], np.array([row.split() for row in rows[2:]], np.int64).reshape(len(rot), ns, ns)


def _block_max(volume, W):
    """the reference's volume [K, side, side] as the greatest score of each block of 8 x 8, partial ones too"""
    ns, side = (2 * W + 1 + 7) // 8, 2 * W + 1
    pad = np.zeros((volume.shape[0], 8 * ns, 8 * ns), np.int64)
    pad[:, :side, :side] = volume
    return pad.reshape(-1, ns, 8, ns, 8).max((2, 4))


# (shift: the plane's distance from a 4-byte boundary)
@pytest.mark.parametrize("gz,gx,shift,R,K,Ws", [g + c + ((0, 3, 4, 33, 40),) for g in ((103, 103, 1), (4, 12, 2), (1, 40, 3), (40, 1, 0)) for c in ((1, 1), (65, 5), (257, 5))]
                         + [(4, 12, 2, 65, 1, (128,))])
def test_search_one_equals_the_restatement(program, tmp_path, gz, gx, shift, R, K, Ws):
    """every case of scan_reference, from the agent or an origin in turn, at W = 0 (one candidate), 3 (one partial block), 4 (two blocks, the second a column
    wide), 33 (past brute force), 40 (81 = 10 x 8 + 1), and 128 once; every block's bound is at least the restatement's greatest score inside it"""
    rng, rot = np.random.default_rng(4900 + gz + R), ref.ROT5[:K]
    for W in Ws:
        for run_no, name in enumerate(scan.CASES):
            origin, t, d, max_range = scan.case(name, rng, R, gx, gz)
            plane = ref.plane_of(rng, gz, gx)
            want = ref.match(origin, t, d, rot, W, max_range, scan.MIN[0], scan.MIN[1], scan.CELL, plane)
            got, _, bounds = _run(program, tmp_path / "search.txt", gz, gx, shift, origin, t, d, max_range, rot, W, plane, agent=run_no % 2 == 0)
            assert got == want[:2], (W, name, got, want[:2])
            assert (bounds >= _block_max(want[2], W)).all(), (W, name)


def _centre_fan(rng, R):
    """beams that stay well inside 103 x 103 under every rotation and a window of 12: from the centre, up to 3 m = 12 cells"""
    ang = rng.uniform(0, 2 * np.pi, R)
    return (scan.MIN[0] + 51.5 * scan.CELL, scan.MIN[1] + 51.5 * scan.CELL), rng.uniform(0.5, 3.0, R), np.stack([np.cos(ang), -np.sin(ang)], 1), 6.0


# col: the origin's column; peaks: (rotation, b, a) from that rotation's end cell — from column 51: (51, 59) under (1, 0), (49, 58) under
# (0.9, 0.3) — in different blocks of W = 12 (anchors -12, -4, 4, 12); the other rotation sees each peak farther off than 10 cells or not
# at all.  From column 100 the end cell's column 108 is off the 103 columns: only a shift brings it in, to the peak at (52, 102).
@pytest.mark.parametrize("col,W,K,peaks,best", [(51, 12, 1, ((0, 10, 0), (0, -10, 0)), (0, 0, -10)), (51, 12, 1, ((0, 6, -8), (0, 6, 8)), (0, -8, 6)),
                                                (51, 12, 2, ((1, -10, 0), (0, 0, 10)), (0, 10, 0)), (51, 12, 2, ((0, 11, 0), (1, -10, 0)), (1, 0, -10)),
                                                (51, 4, 1, ((0, 4, 4),), (0, 4, 4)), (100, 8, 1, ((0, 1, -6),), (0, -6, 1)), (51, 12, 2, 0, (0, 0, 0)), (51, 12, 2, 200, (0, 0, 0))])
def test_equal_peaks_a_corner_peak_an_end_cell_off_the_grid_and_flat_planes(program, tmp_path, col, W, K, peaks, best):
    """one beam of 8 cells along +x, equal isolated peaks: the least a^2 + b^2 wins, then the lowest rotation, then b, then a, across blocks
    and rotations; a single peak at (+W, +W) lies in the partial corner block; an all-zero and a constant plane (peaks: the byte) give the guess"""
    origin, t, d = (scan.MIN[0] + (col + 0.5) * scan.CELL, scan.MIN[1] + 51.5 * scan.CELL), np.array([2.0]), np.array([[1.0, 0.0]])
    plane, peaks = (np.zeros((103, 103), np.uint8), peaks) if isinstance(peaks, tuple) else (np.full((103, 103), peaks, np.uint8), ())
    rot, ends = [ref.ROT5[0], ref.ROT5[3]][:K], ((51, col + 8), (49, col + 7))
    for r, b, a in peaks:
        plane[ends[r][0] + b, ends[r][1] + a] = 200
    got, _, _ = _run(program, tmp_path / "peaks.txt", 103, 103, 3, origin, t, d, 6.0, rot, W, plane)
    assert got == (best, int(plane.max())) == ref.match(origin, t, d, rot, W, 6.0, scan.MIN[0], scan.MIN[1], scan.CELL, plane)[:2]


def test_a_single_peak_prunes(program, tmp_path):
    """a plane with one nonzero cell: an end cell meets it under at most one translation of a whole block, so a block's bound IS the sum of its 64 scores, which the
    restatement gives at W + 7.  The host refines the block of the greatest bound first; every block whose sum lies below that block's best score must then be skipped."""
    (origin, t, d, max_range), plane, W = _centre_fan(np.random.default_rng(4904), 257), np.zeros((103, 103), np.uint8), 12
    plane[50, 55] = 9
    args = (max_range, scan.MIN[0], scan.MIN[1], scan.CELL, plane)
    wide = ref.match(origin, t, d, ref.ROT5[:1], W + 7, *args)[2][:, 7:7 + 32, 7:7 + 32]
    sums = wide.reshape(1, 4, 8, 4, 8).sum((2, 4))
    got, stats, bounds = _run(program, tmp_path / "peak.txt", 103, 103, 1, origin, t, d, max_range, ref.ROT5[:1], W, plane)
    assert np.array_equal(bounds, sums) and got == ref.match(origin, t, d, ref.ROT5[:1], W, *args)[:2]
    j, i = np.unravel_index(np.argmax(sums[0]), (4, 4))
    first_best = ref.match(origin, t, d, ref.ROT5[:1], W, *args)[2][0, 8 * j:8 * j + 8, 8 * i:8 * i + 8].max()
    below = int((sums[0] < first_best).sum())
    assert below >= 1 and stats[0] <= stats[1] - below < stats[1]


def test_launch_and_interface(program):
    from miniworld_amd import engine
    names = LAUNCH + ("batch",)     # (plane + bound plane + lists + bound words + 288; the batch: <= 8, <= RAY_MAX / rays, <= 2048 / blocks)
    for gz, gx, rays, W, lds, batch in ((1, 1, 1, 0, 16 + 64 + 32 + 32 + 288, 8), (103, 103, 256, 64, 10624 + 12112 + 7168 + 8096 + 288, 7),
                                        (103, 103, 256, 10, 10624 + 12112 + 8192 + 288 + 288, 8), (128, 256, RAY_MAX, 128, 32768 + 35520 + 16384 + 4368 + 288, 1)):
        assert launch_of(program, 7, gz, gx, rays, W, names=names) == {"grid": 7, "threads": 256, "lds": lds, "fits": 1, "batch": batch}, (gz, gx, rays, W)
    assert 32768 + 35520 + 16384 + 4368 + 288 <= 160 * 1024
    bad = ((0, 1, 1, 0), (1, 0, 1, 0), (128, 257, 1, 0), (4, 4, 0, 0), (4, 4, RAY_MAX + 1, 0), (4, 4, 1, -1), (4, 4, 1, 129), (1, 32768, 1, 0), (2, 16384, 1, 0))
    assert all(launch_of(program, 7, *b, names=names)["fits"] == 0 for b in bad)
    assert (engine.MATCH_MAX_ROT, engine.MATCH_MAX_WINDOW, engine.SEARCH_MAX_WINDOW) == (64, 32, 128)
    check_units_built("mw_search.hip", "mw_engine_search.hip")
    check_kernel("mw_search_kernel", "mw_search.hip")
    check_does_not_wait("mw_engine_search.hip")
    check_refuses_null_engine("mw_scan_search", engine.MwNavParams(0.25, 0.0, 0.0, 4, 4, 0, 0), None, None, 1, 0, 1, None, None, None, None, None, None, None, None, None)
    check_refuses_null_engine("mw_debug_set_search_prune", 0)


def test_scan_search_calls_and_argument_errors(monkeypatch):
    import torch
    from miniworld_amd.queries import ScanMatch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    m = vec.scan_map()
    score, scan_ = torch.zeros((5, m.gz, m.gx), dtype=torch.uint8), {"t": torch.zeros((5, 9), dtype=torch.float64), "dir": torch.zeros((5, 9, 2), dtype=torch.float64)}
    origin = torch.zeros((5, 3), dtype=torch.float64)
    n0, r = len(lib.calls), vec.scan_search(score, scan_, origin, window=100, turn=0.2, turns=5, max_range=4.0, like=m, stats=True)
    args = lib.calls[-1][1]
    assert [k[0] for k in lib.calls[n0:]] == ["mw_scan_search"] and isinstance(r, ScanMatch) and r.volume is None and tuple(r.stats.shape) == (5, 2)
    assert r.angles.tolist() == pytest.approx([0.0, 0.1, -0.1, 0.2, -0.2]) and list(args[3])[:4] == [1.0, 0.0, np.cos(0.1), np.sin(0.1)] and list(args[2]) == [4.0]
    assert list(args[4:7]) == [5, 100, 9] and [a.value for a in args[7:11]] == [score.data_ptr(), scan_["t"].data_ptr(), scan_["dir"].data_ptr(), origin.data_ptr()]
    assert args[11] is None and [a.value for a in args[12:15]] == [r.best.data_ptr(), r.score.data_ptr(), r.stats.data_ptr()]
    assert vec.scan_search(score, scan_, into=r) is r and lib.calls[-1][1][10] is None and not bool(r.offset().any())
    assert vec.scan_search(score, scan_, like=m).stats is None and lib.calls[-1][1][14] is None and lib.calls[-1][1][5] == 64
    assert torch.equal(r.apply(scan_, origin)[1], origin)
    vec.engine.debug_set_search_prune(False)
    assert lib.calls[-1][0] == "mw_debug_set_search_prune" and lib.calls[-1][1][1] == 0
    matched, n0 = vec.scan_match(score, scan_, like=m), len(lib.calls)
    for kw in (dict(window=129), dict(window=-1), dict(turns=2, turn=0.1), dict(turns=65, turn=0.1), dict(max_range=0.0), dict(stats=1), dict(score=score[:4]),
               dict(scan=scan_["t"]), dict(origin=origin.float()), dict(into=m), dict(into=matched), dict(into=r, window=3)):
        with pytest.raises(ValueError):
            vec.scan_search(**{"score": score, "scan": scan_, **kw})
    with pytest.raises(ValueError):
        vec.scan_match(score, scan_, into=r)
    assert len(lib.calls) == n0         # nothing reached the library
