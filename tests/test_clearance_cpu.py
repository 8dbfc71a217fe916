"""Grid clearance without a GPU: the kernel's phases (csrc/mw_clear.h) on the host under sanitizers (hostcheck/grid_clearance.cpp), bit for
bit against clearance_reference.py; threshold() against grid_field's inflation test; the launch; grid_clearance's argument errors."""
import math
import subprocess

import numpy as np
import pytest

import clearance_reference as ref
from helpers import stub_engine
from query_checks import build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, launch_of, run

BANDS = ((2, 200), (9, 90), (40, 7))
CALLS = [(0, 1, BANDS), (3, 0, ()), (3, 1, BANDS), (0, 0, ())]        # (limit, want_nearest, bands)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("grid_clearance", tmp_path_factory.mktemp("grid_clearance"))


@pytest.mark.parametrize("gz,gx", [(103, 103), (128, 256), (4, 12), (1, 40), (40, 1)])
def test_every_output_equals_the_restatement(program, tmp_path, gz, gx):
    """test_gpu_clearance.py's grids, an env per run of the program, each row at another distance from a 4-byte boundary"""
    rng = np.random.default_rng(7100 + gz)
    dens = np.array([0.05, 0.01, 0.002] if gz * gx == 32768 else [0.5, 0.05, 0.002])[:, None, None]
    marked = (rng.random((3, gz, gx)) < dens).astype(np.uint8) * rng.integers(1, 256, (3, gz, gx)).astype(np.uint8)
    for env in range(3):
        lines = [f"{gx} {gz} {(env + gz) % 4} {len(CALLS)}", " ".join(map(str, marked[env].ravel()))]
        lines += [f"{limit} {near} {len(bands)} " + " ".join(f"{t} {c}" for t, c in bands) for limit, near, bands in CALLS]
        rows = iter(run(program, tmp_path / "clear.txt", lines))
        exact = ref.transform(marked[env])
        for limit, near, bands in CALLS:
            want = ref.clearance(marked[env], limit, bands, exact)
            for k, asked in enumerate((True, near, bands)):
                if asked:
                    got = np.array(next(rows).split(), np.int64).reshape(gz, gx)
                    assert np.array_equal(got, want[k]), (env, limit, k, int((got != want[k]).sum()))
        assert next(rows, None) is None


@pytest.mark.parametrize("bands", ["9 " + " ".join(f"{t} 1" for t in range(9)), "1 -1 5", "2 4 5 4 6", "2 5 1 4 1", "1 3 256", "1 3 -1"])
def test_the_entry_points_band_check_refuses(program, tmp_path, bands):    # (mwclear::bands_error: count, negative, equal, lower, costs off 0 .. 255)
    (tmp_path / "bad.txt").write_text(f"2 2 0 1\n0 1 0 0\n0 0 {bands}\n")
    assert subprocess.run([program, str(tmp_path / "bad.txt")], capture_output=True).returncode == 2


@pytest.mark.parametrize("cell", [0.25, 0.1])
def test_threshold_is_the_inflation_test(cell):        # (radii at, just below and just above sqrt(a^2 + b^2) * cell, and between)
    from miniworld_amd.queries import GridClearance
    exact = [math.sqrt(float(t)) * cell for t in (1, 2, 4, 5, 8, 9, 10, 13, 16, 18, 25, 50, 289)]
    for r in [0.0, 1e-9, 0.3, 0.5, 0.6, 1.0, 4 * cell, 17.3 * cell] + exact + [math.nextafter(r, way) for r in exact for way in (0.0, math.inf)]:
        inside = [t for t in range(400) if math.sqrt(float(t)) * cell < r]       # mw_nav_grid.h: sqrt((double)(di*di + dj*dj)) * cell < margin
        assert GridClearance.threshold(r, cell) == (inside[-1] if inside else -1), (r, cell)
    assert GridClearance.threshold(1e9, cell) == GridClearance.threshold(1e300, cell) == 2 ** 30


def test_launch_and_interface(program):
    from miniworld_amd import engine
    for cells, lds in ((1, 16), (48, 96), (103 * 103, 21232), (32768, 65536)):
        assert launch_of(program, 7, cells) == {"grid": 7, "threads": 256, "lds": lds, "fits": 1}, cells
    assert 7 * launch_of(program, 7, 103 * 103)["lds"] <= 160 * 1024         # the Maze's grid: seven workgroups share a CU
    assert all(launch_of(program, 7, cells)["fits"] == 0 for cells in (0, -3, 32769))
    assert (engine.CLEAR_NONE, engine.CLEAR_FAR, engine.CLEAR_MAX_BANDS) == (0x7FFFFFFF, 0x7FFFFFFE, 8)
    check_units_built("mw_clear.hip", "mw_engine_clear.hip")
    check_kernel("mw_clear_kernel", "mw_clear.hip")
    check_does_not_wait("mw_engine_clear.hip")
    check_refuses_null_engine("mw_grid_clearance", engine.MwNavParams(0.25, 0.0, 0.0, 4, 4, 0, 0), 0, None, 0, None, None, None, None, None, None)


BAD = [dict(marked=None), dict(marked="float"), dict(marked="short"), dict(marked="list"), dict(radii=(0.3,)), dict(costs=(3,)),
       dict(radii=(0.3, 0.5), costs=(3,)), dict(radii=(), costs=()), dict(radii=[0.1 * k for k in range(1, 10)], costs=[1] * 9),
       dict(radii=(0.5, 0.3), costs=(1, 2)), dict(radii=(0.3, 0.3), costs=(1, 2)), dict(radii=(-0.3,), costs=(1,)), dict(radii=(0.3,), costs=(256,)),
       dict(radii=(0.3,), costs=(-1,)), dict(radii=(0.3,), costs=(1.5,)), dict(radii=0.3, costs=1), dict(limit=0), dict(limit=-1.0),
       dict(limit=float("nan")), dict(nearest=1), dict(cell=0), dict(cell=0.5, like="field"), dict(like="tensor"), dict(mask=[1, 0, 0, 1, 0]),
       dict(into="field"), dict(into="record", limit=0.7), dict(into="record", nearest=True), dict(into="record", like="field"),
       dict(into="record", radii=(0.3,), costs=(1,))]


def test_grid_clearance_calls_and_argument_errors(monkeypatch):
    import torch
    from miniworld_amd.queries import GridClearance
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    priv = vec.nav_field()
    marked = torch.zeros((5, priv.gz, priv.gx), dtype=torch.uint8)
    n0, c = len(lib.calls), vec.grid_clearance(marked)
    args = lib.calls[-1][1]
    assert [k[0] for k in lib.calls[n0:]] == ["mw_grid_clearance"] and isinstance(c, GridClearance) and bool(c.metres().isinf().all())
    assert (c.nearest, c.cost, c.bands, c.limit) == (None, None, (), 0)
    assert (args[1]._obj.cell, args[1]._obj.gx, args[1]._obj.gz) == (0.25, priv.gx, priv.gz) and args[2] == 0 and args[3] is None and args[4] == 0
    assert args[5] is None and [a.value for a in args[6:8]] == [marked.data_ptr(), c.dist2.data_ptr()] and args[8] is None and args[9] is None
    mask = torch.tensor([1, 0, 0, 1, 0], dtype=torch.uint8)   # (0.7 m: 3 cells; 0 m holds no distance, its band goes; 0.3 m: 1; 0.6 m: 5)
    c = vec.grid_clearance(marked.bool(), radii=(0.0, 0.3, 0.6), costs=[250, 100, 10], limit=0.7, nearest=True, like=priv, mask=mask)
    args = lib.calls[-1][1]
    assert c.bands == ((1, 100), (5, 10)) and c.limit == 3 and args[2] == 3 and list(args[3]) == [1, 100, 5, 10] and args[4] == 2
    assert args[5].value == mask.data_ptr() and [a.value for a in args[8:10]] == [c.nearest.data_ptr(), c.cost.data_ptr()]
    assert vec.grid_clearance(marked, into=c) is c and list(lib.calls[-1][1][3]) == [1, 100, 5, 10] and lib.calls[-1][1][7].value == c.dist2.data_ptr()
    none = vec.grid_clearance(marked, radii=(0.0,), costs=(9,), limit=1e18)      # (every band dropped: zeros, not passed on; no limit, at once)
    assert none.bands == () and not bool(none.cost.any()) and none.limit == 32768 and lib.calls[-1][1][9] is None and lib.calls[-1][1][4] == 0
    for like in (vec.seen_map(), vec.depth_map(), vec.object_map(), vec.grid_regions(marked), priv):
        vec.grid_clearance(marked, like=like)
    named, n0 = {"float": marked.float(), "short": marked[:4], "list": marked.tolist(), "field": priv, "tensor": priv.field, "record": c}, len(lib.calls)
    for kw in BAD:
        kw = {"marked": marked, **{k: named.get(v, v) if isinstance(v, str) else v for k, v in kw.items()}}
        with pytest.raises(ValueError):
            vec.grid_clearance(**kw)
    assert len(lib.calls) == n0         # nothing reached the library
