"""Grid ray casts without a GPU: both forms' walks (csrc/mw_gridray.h) on the host under sanitizers (hostcheck/grid_ray.cpp), bit for
bit against grid_ray_reference.py; the launch and the interface."""
import numpy as np
import pytest

import grid_ray_reference as ref
import scan_reference as scan
from helpers import stub_engine
from query_checks import build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, launch_of, run, LAUNCH

RAY_MAX = 4096


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("grid_ray", tmp_path_factory.mktemp("grid_ray"))


def _run(program, path, gz, gx, shift, origin, d, max_t, opaque):
    """the program on one env: [(t bits, hit)] per form"""
    extent = (scan.MIN[0], scan.MIN[0] + gx * scan.CELL - 0.1, scan.MIN[1], scan.MIN[1] + gz * scan.CELL - 0.1)
    lines = [" ".join(repr(v) for v in extent), f"{scan.CELL!r} {gx} {gz} {shift} {max_t!r} {len(d)}"]
    lines += [" ".join(repr(float(v)) for v in (*o, *k)) for o, k in zip(origin, d)]
    rows, R = run(program, path, lines + [" ".join(str(int(v)) for v in opaque.ravel())]), len(d)
    assert len(rows) == 2 * R
    return [[(int(a, 16), int(b)) for a, b in (r.split() for r in rows[f * R:(f + 1) * R])] for f in range(2)]


@pytest.mark.parametrize("gz,gx,shift,R", [g + (r,) for g in ((103, 103, 1), (128, 256, 0), (4, 12, 2), (1, 40, 3), (40, 1, 0)) for r in (3, 65)] + [(103, 103, 3, RAY_MAX)])
def test_both_walks_equal_the_restatement(program, tmp_path, gz, gx, shift, R):
    """every case, an env per run, on a map of another density each (3 %, 30 %, empty, full, turning with the case): t and hit of either
    form's walk are the restatement's bits"""
    rng, hits = np.random.default_rng(4900 + gz + R), 0
    for no, name in enumerate(ref.CASES if R < RAY_MAX else ("random",)):
        origin, d = ref.case(name, rng, R, gx, gz, scan.MIN, scan.CELL)
        opaque = ref.opaque_of(rng, gz, gx, ref.DENSITIES[(no + R + gz) % 4])
        t, hit = ref.cast(origin, d, ref.MAX_T, scan.MIN[0], scan.MIN[1], scan.CELL, opaque)
        for form, got in enumerate(_run(program, tmp_path / "ray.txt", gz, gx, shift, origin, d, ref.MAX_T, opaque)):
            assert got == list(zip(t.view(np.uint64).tolist(), hit.tolist())), (name, form)
        hits += int((hit >= 0).sum())
    assert hits > 0


def test_launch_and_interface(program):
    from miniworld_amd import engine
    names = LAUNCH + ("staged",)        # (the staged form from 8 rays on: a key per pair, 1 KiB, and the bits; below it two rays per workgroup, each inside an env)
    for cells, rays, forced, grid, lds, staged in ((1, 1, 0, 7, 0, 0), (103 * 103, 7, 0, 7 * 4, 0, 0), (103 * 103, 8, 0, 7, 1024 + 1328, 1), (32768, RAY_MAX, 0, 7, 1024 + 4096, 1),
                                                   (32768, 3, 1, 7, 1024 + 4096, 1), (16, RAY_MAX, 2, 7 * 2048, 0, 0)):
        assert launch_of(program, 7, cells, rays, forced, names=names) == {"grid": grid, "threads": 256, "lds": lds, "fits": 1, "staged": staged}, (cells, rays, forced)
    assert all(launch_of(program, 7, cells, rays, 0, names=names)["fits"] == 0 for cells, rays in ((0, 1), (32769, 1), (16, 0), (16, RAY_MAX + 1)))
    check_units_built("mw_gridray.hip", "mw_engine_gridray.hip")
    check_kernel("mw_gridray_bits_kernel", "mw_gridray.hip")
    check_kernel("mw_gridray_waves_kernel", "mw_gridray.hip")
    check_does_not_wait("mw_engine_gridray.hip")
    check_refuses_null_engine("mw_grid_ray_cast", engine.MwNavParams(0.25, 0.0, 0.0, 4, 4, 0, 0), None, 1, None, None, None, None, None, None, None, None, None, None)


def test_grid_raycast_calls_and_argument_errors(monkeypatch):
    """(the checks of the map and of the opaque plane are _map_grid's and _cell_grid's, held by grid_sight's tests)"""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    m = vec.scan_map()
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64)        # noqa: E731
    ptr = lambda args: [a and a.value for a in args[4:13]]              # noqa: E731  (mask .. dir_out; the stream is behind them)
    opaque, d, origin, off, heading = torch.zeros((5, m.gz, m.gx), dtype=torch.uint8), f64(5, 9, 2), f64(5, 9, 3), f64(9), f64(5)
    n0, r = len(lib.calls), vec.grid_raycast(opaque, d, origin, max_t=2.5, like=m)
    out, args = [r[k].data_ptr() for k in ("t", "hit", "dir")], lib.calls[-1][1]
    assert [k[0] for k in lib.calls[n0:]] == ["mw_grid_ray_cast"] and tuple(r["dir"].shape) == (5, 9, 2) and list(args[2]) == [2.5] and args[3] == 9
    assert ptr(args) == [None, opaque.data_ptr(), origin.data_ptr(), d.data_ptr(), None, None] + out
    assert vec.grid_raycast(opaque, offsets=off, heading=heading, like=m, into=r) is r
    assert ptr(lib.calls[-1][1]) == [None, opaque.data_ptr(), None, None, off.data_ptr(), heading.data_ptr()] + out
    scan_ = vec.grid_lidar(opaque, rays=16, max_range=4.0, origin=f64(5, 3), like=m)
    assert list(lib.calls[-1][1][2]) == [4.0] and lib.calls[-1][1][3] == 16 and vec.grid_lidar(opaque, rays=16, max_range=4.0, like=m) is scan_
    vec.scan_map_update(m, scan=scan_)          # a grid scan is a scan
    assert lib.calls[-1][0] == "mw_scan_project"
    n0 = len(lib.calls)
    for kw in (dict(), dict(direction=d, offsets=off), dict(direction=d, heading=heading), dict(direction=d.float()), dict(direction=d[:4]), dict(direction=f64(5, 0, 2)),
               dict(offsets=f64(RAY_MAX + 1)), dict(offsets=off, heading=f64(4)), dict(direction=d, origin=f64(5, 3)), dict(direction=d, max_t=0.0),
               dict(direction=d, max_t=float("inf")), dict(direction=d, max_t=float("nan")), dict(direction=d, into={"t": r["t"]}), dict(direction=f64(5, 8, 2), into=r)):
        with pytest.raises(ValueError):
            vec.grid_raycast(opaque, like=m, **kw)
    for kw in (dict(rays=0), dict(rays=RAY_MAX + 1), dict(fov=7.0), dict(origin=f64(5, 9, 3)), dict(max_range=-1.0)):
        with pytest.raises(ValueError):
            vec.grid_lidar(opaque, like=m, **kw)
    assert len(lib.calls) == n0         # nothing reached the library
