"""Scan maps without a GPU: the kernel's phases (csrc/mw_scan.h) on the host under sanitizers (hostcheck/grid_scan.cpp), bit for bit
against scan_reference.py; the rule against the beams' geometry; the launch and the interface."""
import math

import numpy as np
import pytest

import scan_reference as ref
from query_checks import build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, launch_of, run

RAY_MAX = 4096


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("grid_scan", tmp_path_factory.mktemp("grid_scan"))


@pytest.mark.parametrize("gz,gx", ref.GRIDS)
def test_scan_one_equals_the_restatement(program, tmp_path, gz, gx):
    """every case at 65 beams, the random one at 1 and MW_RAY_MAX too, an env per run, each map at another distance from a 4-byte boundary;
    two calls in a row: the case from the agent or an origin, then random beams under `clear` (every other run) or a zero mask byte (every third)"""
    rng, _beams = np.random.default_rng(4300 + gz), lambda t, d: [f"{float(a)!r} {float(x)!r} {float(z)!r}" for a, (x, z) in zip(t, d)]
    extent = (ref.MIN[0], ref.MIN[0] + gx * ref.CELL - 0.1, ref.MIN[1], ref.MIN[1] + gz * ref.CELL - 0.1)
    for run_no, (name, R) in enumerate([(c, 65) for c in ref.CASES] + [("random", 1), ("random", RAY_MAX)]):
        first, second = ref.case(name, rng, R, gx, gz), ref.case("random", rng, R, gx, gz)
        agent, masked, clear = run_no % 2 == 0, run_no % 3 != 2, run_no % 2 == 1
        lines = [f"{first[0][0]!r} {first[0][1]!r} 0.0", " ".join(repr(v) for v in extent),
                 f"{ref.CELL!r} {gx} {gz} {(run_no + gz) % 4} {first[3]!r} {R} 2",
                 f"1 0 {0 if agent else 1} {first[0][0]!r} {first[0][1]!r}"] + _beams(first[1], first[2])
        lines += [f"{int(masked)} {int(clear)} 1 {second[0][0]!r} {second[0][1]!r}"] + _beams(second[1], second[2])
        rows = iter(run(program, tmp_path / "scan.txt", lines))
        planes, count = np.zeros((2, gz, gx), np.uint8), np.zeros(2, np.int64)
        for call, (origin, t, d, _) in enumerate((first, second)):
            if call == 0 or masked:
                last = ref.update(planes, count, *ref.sets(origin, t, d, first[3], ref.MIN[0], ref.MIN[1], ref.CELL, gx, gz), clear=call == 1 and clear)
            for k in range(2):
                got = np.array(next(rows).split(), np.uint8).reshape(gz, gx)
                assert np.array_equal(got, planes[k]), (name, R, call, k, int((got != planes[k]).sum()))
            assert next(rows).split() == [str(int(v)) for v in (*count, *last, 1)], (name, R, call)
        assert next(rows, None) is None
        assert R == 1 or planes.any(), (name, R)         # (the case is no empty one)


def _meets(p0, p1, lo_u, hi_u, lo_w, hi_w):
    """whether the segment p0 -> p1 meets each box [lo_u, hi_u] x [lo_w, hi_w] (arrays of one shape): slab clipping, no walk"""
    s0, s1 = np.zeros_like(lo_u), np.ones_like(lo_u)
    for a, b, lo, hi in ((p0[0], p1[0], lo_u, hi_u), (p0[1], p1[1], lo_w, hi_w)):
        if a == b:
            s0 = np.where((a >= lo) & (a <= hi), s0, np.inf)
        else:
            x, y = (lo - a) / (b - a), (hi - a) / (b - a)
            s0, s1 = np.maximum(s0, np.minimum(x, y)), np.minimum(s1, np.maximum(x, y))
    return s0 <= s1


@pytest.mark.parametrize("gz,gx", ref.GRIDS)
def test_the_rule_marks_the_cells_the_segment_meets(gz, gx):
    """apart from the rule: beam by beam over all cells, every marked cell's closed square grown by 1e-9 cells meets the beam's
    segment, and every cell whose square shrunk by 1e-9 cells meets it is marked; no exceptions"""
    rng = np.random.default_rng(4400 + gz)
    origin, t, d, max_range = ref.case("random", rng, 65, gx, gz)
    j, i = (a.astype(np.float64) for a in np.mgrid[0:gz, 0:gx])
    eps, kept = 1e-9, 0
    for b in range(65):
        free, obstacle = ref.sets(origin, t[b:b + 1], d[b:b + 1], max_range, ref.MIN[0], ref.MIN[1], ref.CELL, gx, gz)
        e = min(t[b], max_range)
        p0 = ((origin[0] - ref.MIN[0]) / ref.CELL, (origin[1] - ref.MIN[1]) / ref.CELL)
        p1 = (p0[0] + e * (d[b, 0] / ref.CELL), p0[1] + e * (d[b, 1] / ref.CELL))
        marked, kept = free | obstacle, kept + int((free | obstacle).any())
        assert not (marked & ~_meets(p0, p1, i - eps, i + 1 + eps, j - eps, j + 1 + eps)).any(), (b, "a marked cell off the segment")
        assert not (_meets(p0, p1, i + eps, i + 1 - eps, j + eps, j + 1 - eps) & ~marked).any(), (b, "a crossed cell not marked")
        assert obstacle.sum() == int(t[b] < max_range and 0 <= math.floor(p1[0]) < gx and 0 <= math.floor(p1[1]) < gz), b
    assert kept == 65


def test_launch_and_interface(program, tmp_path):
    from miniworld_amd import engine
    lines = ["0.0 3.0 0.0", "-1.5 1.5 2.25 9.0", "0.25 12 4 1 6.0 1 2", "1 0 0 0.0 0.0", "1.0 1.0 0.0", "1 0 0 0.0 0.0", "1.0 1.0 0.0"]
    rows = run(program, tmp_path / "bad.txt", lines)         # an env the grid does not cover: zeroed planes and counts, not covered
    assert all(not np.array(r.split(), int)[:-1].any() and r.split()[-1] == "0" for r in rows) and len(rows) == 6
    for cells, rays, lds in ((1, 1, 16 + 16 + 32), (103 * 103, 256, 2 * 1328 + 1056), (32768, RAY_MAX, 4096 + 4096 + 16416), (32768, 1, 8192 + 32)):
        assert launch_of(program, 7, cells, rays) == {"grid": 7, "threads": 256, "lds": lds, "fits": 1}, (cells, rays)
    assert all(launch_of(program, 7, cells, rays)["fits"] == 0 for cells, rays in ((0, 1), (32769, 1), (16, 0), (16, RAY_MAX + 1)))
    assert engine.RAY_MAX == RAY_MAX
    check_units_built("mw_scan.hip", "mw_engine_scan.hip")
    check_kernel("mw_scan_kernel", "mw_scan.hip")
    check_does_not_wait("mw_engine_scan.hip")
    check_refuses_null_engine("mw_scan_project", engine.MwNavParams(0.25, 0.0, 0.0, 4, 4, 0, 0), None, 1, None, None, None, None, None, None, None, None, None)
