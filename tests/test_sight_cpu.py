"""Grid sight (mw_grid_sight; MiniWorldVecEnv.grid_sight) without a GPU.

The phases the kernel inlines (miniworld_amd/csrc/mw_sight.h: the staging into bits, the walk that probes at most three cells per step,
the range box) run on the host in a program of its own (tests/hostcheck/grid_sight.cpp), built with the address and undefined-behaviour
sanitizers, on random grids; its gains and its seen plane are compared, exactly, with the restatement of tests/sight_reference.py,
which has no walk: it evaluates the occlusion predicate for every opaque cell against every target.  Beside that: the symmetry of
sight, the corner seal, the ABI names, the launch arithmetic, and the argument errors of grid_sight over a stub engine."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import sight_reference as ref
from helpers import stub_engine
from query_checks import ROOT, build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, launch_of, run

# (gz, gx, cell): the Maze's grid (odd rows), the Sidewalk's, a coarse one, one of fewer cells than the kernel has lanes
GRIDS = [(103, 103, 0.25), (640, 36, 0.25), (52, 52, 0.5), (4, 12, 1.0)]
COS_HALVES = (-1.0, math.cos(math.radians(30.0)), 0.0, 1.0)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("grid_sight", tmp_path_factory.mktemp("grid_sight"))


def _lines(opaque, cell, max_range, cos_half, cells=None, dirs=None, weight=None, seen=None, shift=0, agent=None):
    gz, gx = opaque.shape
    views = 1 if cells is None else len(cells)
    lines = [f"{cell!r} {float(max_range)!r} {float(cos_half)!r} {gx} {gz} {shift} {views} {int(weight is not None)} {int(dirs is not None)} {int(agent is not None)}"]
    if agent is not None:
        extent, pose = agent
        lines += [" ".join(repr(float(v)) for v in extent), " ".join(repr(float(v)) for v in pose)]
    for g in (opaque, weight, seen if seen is not None else np.zeros_like(opaque)):
        if g is not None:
            lines.append(" ".join(str(int(v)) for v in np.asarray(g).astype(np.int64).ravel()))
    if cells is not None:
        lines.append(" ".join(str(int(c)) for c in cells))
    if dirs is not None:
        lines.append(" ".join(repr(float(d)) for d in dirs))
    return lines


def _run(program, tmp_path, opaque, *args, **kw):
    gz, gx = opaque.shape
    out = run(program, tmp_path / "sight.txt", _lines(opaque, *args, **kw))
    head = out[0].split()
    assert head[0] == "sight"
    return int(head[1]), np.array(out[1].split(), np.int64).astype(np.int32), np.array(out[2].split(), np.int64).astype(np.uint8).reshape(gz, gx)


def _grid(rng, gz, gx, density):
    """random bytes 1 .. 255 on `density` of the cells (any byte != 0 is opaque)"""
    return (rng.random((gz, gx)) < density).astype(np.uint8) * rng.integers(1, 256, (gz, gx)).astype(np.uint8)


def _viewpoints(rng, opaque, n):
    """n flat cells: the corners and two edge cells first, then opaque cells, -1 and values >= gx * gz, then random ones"""
    gz, gx = opaque.shape
    special = [0, gx - 1, (gz - 1) * gx, gz * gx - 1, (gz // 2) * gx, gx // 2]
    oj, oi = np.nonzero(opaque)
    special += [int(oj[k]) * gx + int(oi[k]) for k in rng.integers(0, len(oj), 3)] if len(oj) else []
    special += [-1, gx * gz, gx * gz + 7, 2 ** 31 - 1, -(2 ** 31)]
    cells = [int(c) for c in rng.integers(0, gx * gz, n)]
    pick = rng.permutation(len(special))[:max(1, n - 1) if n < len(special) else len(special)]
    for slot, k in zip(rng.permutation(n)[:len(pick)], pick):
        cells[int(slot)] = special[int(k)]
    return cells


def _ranges(gz, gx, cell):
    return (cell, 3.0, math.hypot(gz, gx) * cell + 1.0)     # one cell, 3 m, the whole grid


def _check(program, tmp_path, rng, opaque, cell, max_range, cos_half, cells, dirs, weight, shift):
    gz, gx = opaque.shape
    pattern = (rng.random((gz, gx)) < 0.1).astype(np.uint8) * 7         # seen as it stands: kept where nothing is seen, 1 where something is
    covered, gain, seen = _run(program, tmp_path, opaque, cell, max_range, cos_half, cells, dirs, weight, pattern, shift)
    want_gain, want_seen = ref.sight(opaque, cell, cells, dirs, max_range, cos_half, weight, pattern)
    assert covered == 1
    assert np.array_equal(gain, want_gain), ("gains that differ", int((gain != want_gain).sum()), gain[:8], want_gain[:8])
    assert np.array_equal(seen, want_seen), ("cells that differ", int((seen != want_seen).sum()))
    return gain, seen, pattern


@pytest.mark.parametrize("density", [0.03, 0.15])
@pytest.mark.parametrize("gz,gx,cell", GRIDS)
def test_gain_and_seen_equal_the_restatement(program, tmp_path, gz, gx, cell, density):
    """Per grid and density: 1, 3 and 65 viewpoints (corners, edges, opaque cells, -1 and cells past the grid among them), the three
    ranges, the four cones, with and without weights, a NaN heading among the dirs, the rows at every distance from a 4-byte boundary
    in turn.  The whole-grid range goes with 1 and 3 viewpoints on the large grids (the restatement is quadratic there)."""
    rng = np.random.default_rng(5100 + gz + int(density * 100))
    opaque = _grid(rng, gz, gx, density)
    big = gz * gx > 5000
    k = 0
    some_seen = some_kept = some_cone = False
    for views in (1, 3, 65):
        for r_index, max_range in enumerate(_ranges(gz, gx, cell)):
            if big and r_index == 2 and views == 65:
                continue
            for cos_half in COS_HALVES if not (big and r_index == 2) else COS_HALVES[k % 4:k % 4 + 1]:
                k += 1
                cells = _viewpoints(rng, opaque, views)
                weight = rng.integers(0, 256, (gz, gx)).astype(np.uint8) if k % 2 else None
                dirs = None
                if cos_half != -1.0 or k % 3 == 0:
                    dirs = [float(d) for d in rng.uniform(-7.0, 7.0, views)]
                    if views > 1:
                        dirs[int(rng.integers(0, views))] = math.nan
                gain, seen, pattern = _check(program, tmp_path, rng, opaque, cell, max_range, cos_half, cells, dirs, weight, k % 4)
                some_seen |= bool((seen == 1).any())
                some_kept |= bool((seen == 7).any())
                some_cone |= cos_half not in (-1.0, 1.0) and bool(gain.any())
    assert some_seen and some_kept and some_cone


def test_a_viewpoint_sees_itself_and_opaque_faces_and_nothing_behind(program, tmp_path):
    """by hand, 1 x 9: A = 2, walls at 4 and 7: A sees 0 .. 4 (itself, the free cells, the first wall's face), not 5 .. 8"""
    opaque = np.zeros((1, 9), np.uint8)
    opaque[0, 4] = opaque[0, 7] = 200
    weight = np.arange(1, 10, dtype=np.uint8).reshape(1, 9)
    _, gain, seen = _run(program, tmp_path, opaque, 0.25, 100.0, -1.0, [2, 4, -1, 9], None, weight)
    assert seen.tolist() == [[1, 1, 1, 1, 1, 1, 1, 1, 0]]        # (from the wall cell 4 itself: 0 .. 7)
    assert gain.tolist() == [1 + 2 + 3 + 4 + 5, sum(range(1, 9)), 0, 0]
    _, gain, seen = _run(program, tmp_path, opaque, 0.25, 0.5, -1.0, [2])
    assert gain.tolist() == [5] and seen.tolist() == [[1, 1, 1, 1, 1, 0, 0, 0, 0]]       # the range is closed: 2 cells of 0.25 m
    # a NaN heading under a cone: the viewpoint itself only (dist == 0.0 passes)
    _, gain, _ = _run(program, tmp_path, opaque, 0.25, 100.0, 0.0, [2, 2], [math.nan, 0.0])
    assert gain.tolist() == [1, 3]     # heading 0 looks along +x: cells 2, 3, 4


def _matrix(program, tmp_path, opaque, cell, max_range):
    path = tmp_path / "matrix.txt"
    path.write_text("\n".join(_lines(opaque, cell, max_range, -1.0, [0])) + "\n")
    r = subprocess.run([program, "--matrix", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    n = opaque.size
    rows = r.stdout.split()
    assert len(rows) == n
    return np.array([[ch == "1" for ch in row] for row in rows], bool)


def test_sight_is_symmetric(program, tmp_path):
    """20 x 20, 15 % opaque, all round, no range limit: A sees B iff B sees A — and every pair equals the restatement"""
    rng = np.random.default_rng(5200)
    opaque = _grid(rng, 20, 20, 0.15)
    m = _matrix(program, tmp_path, opaque, 0.25, 100.0)
    assert np.array_equal(m, m.T)
    assert m.diagonal().all() and 0.05 < m.mean() < 0.95
    want = np.stack([ref.visible(opaque, 0.25, a // 20, a % 20, 100.0).ravel() for a in range(400)])
    assert np.array_equal(m, want), int((m != want).sum())


def test_a_corner_is_sealed(program, tmp_path):
    """an anti-diagonal wall of single cells on 8 x 8: (0, 0) does not see (7, 7) — with the open form of the test it would"""
    opaque = np.zeros((8, 8), np.uint8)
    for j in range(8):
        opaque[j, 7 - j] = 1
    _, gain, seen = _run(program, tmp_path, opaque, 0.25, 100.0, -1.0, [0])
    assert seen[7, 7] == 0 and seen[0, 0] == 1
    assert not ref.visible(opaque, 0.25, 0, 0, 100.0)[7, 7] and ref.visible(opaque, 0.25, 0, 0, 100.0, closed=False)[7, 7]
    # nothing beyond the wall is seen at all: the seal holds for every target
    beyond = np.add.outer(np.arange(8), np.arange(8)) > 7
    assert not seen[beyond].any() and gain[0] == int((~beyond).sum())
    m = _matrix(program, tmp_path, opaque, 0.25, 100.0)
    side = (np.add.outer(np.arange(8), np.arange(8)).ravel() < 7)
    assert not m[np.ix_(side, ~side & (opaque.ravel() == 0))].any()


def test_the_agents_cell_and_heading(program, tmp_path):
    """agent mode: the viewpoint is the cell of the pose on the env's grid, clamped; a NaN pose sees nothing; a grid that does not cover
    the extent is refused"""
    rng = np.random.default_rng(5300)
    gz, gx, cell = 38, 30, 0.25
    opaque = _grid(rng, gz, gx, 0.05)
    extent = (-1.5, -1.5 + gx * cell - 0.1, 2.25, 2.25 + gz * cell - 0.1)
    cos_half = math.cos(math.radians(40.0))
    for pose in ((0.3, 5.1, 0.7), (-1.5 + 1e-9, 2.25 + gz * cell - 0.11, -2.0), (-9.0, 40.0, 3.0), (1.0, 4.0, math.nan), (math.nan, 4.0, 0.0)):
        covered, gain, seen = _run(program, tmp_path, opaque, cell, 3.0, cos_half, agent=(extent, pose))
        c = ref.agent_cell(pose, extent, cell, gx, gz)
        want_gain, want_seen = ref.sight(opaque, cell, [c], [pose[2]], 3.0, cos_half)
        assert covered == 1 and np.array_equal(gain, want_gain) and np.array_equal(seen, want_seen), pose
        assert (gain[0] == 0) == math.isnan(pose[0])
    covered, gain, seen = _run(program, tmp_path, opaque, cell, 3.0, cos_half, agent=((-1.5, -1.5 + gx * cell + 0.2, 2.25, 2.25 + gz * cell - 0.1), (0.3, 5.1, 0.7)))
    assert covered == 0 and gain.tolist() == [0] and not seen.any()


def test_the_program_refuses_what_the_call_refuses(program, tmp_path):
    opaque = np.zeros((4, 4), np.uint8)
    for kw in (dict(max_range=0.0), dict(max_range=math.inf), dict(max_range=math.nan), dict(cos_half=1.5), dict(cos_half=math.nan),
               dict(cos_half=0.5, dirs=None), dict(cell=0.0)):
        a = dict(cell=0.25, max_range=3.0, cos_half=-1.0, cells=[0], dirs=None)
        a.update(kw)
        path = tmp_path / "refused.txt"
        path.write_text("\n".join(_lines(opaque, a["cell"], a["max_range"], a["cos_half"], a["cells"], a["dirs"])) + "\n")
        assert subprocess.run([program, str(path)], capture_output=True, text=True).returncode == 2, kw


# ---------------------------------------------------------------------------------------------------------------- the interface

def test_launch_arithmetic(program):
    from miniworld_amd import engine
    v_max = engine.SIGHT_MAX_VIEWS
    for cells, weighted, views, lds in ((1, 0, 1, 16 + 16), (1, 1, 1, 16 + 16 + 16), (48, 1, 3, 16 + 48 + 16), (103 * 103, 0, 65, 1328 + 272),
                                        (103 * 103, 1, 65, 1328 + 10624 + 272), (32768, 0, 1, 4096 + 16), (32768, 1, v_max, 4096 + 32768 + 4 * v_max)):
        got = launch_of(program, 7, cells, weighted, views)
        assert got == {"grid": 7, "threads": 256, "lds": lds, "fits": 1}, (cells, weighted, views, got)
        assert got["lds"] <= 64 * 1024
    for cells, views in ((0, 1), (-3, 1), (32769, 1), (100, 0), (100, v_max + 1), (100, -1)):
        assert launch_of(program, 7, cells, 1, views)["fits"] == 0, (cells, views)
    # the range box: floor(range / cell) + 1 cells, at least 1 and at most the grid's longer side
    for cell, rng_, limit, r in ((0.25, 3.0, 103, 13), (0.25, 0.25, 103, 2), (0.25, 0.1, 103, 1), (0.25, 1e300, 640, 640), (1.0, 3.5, 2, 2)):
        assert int(subprocess.run([program, "--reach", repr(cell), repr(rng_), str(limit)], capture_output=True, text=True, check=True).stdout) == r


def test_header_declares_the_entry_point():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"int mw_grid_sight\(mw_engine \*e, const mw_nav_params \*grid", header)
    assert engine.SIGHT_MAX_VIEWS == 256
    for k, v in (("MW_SIGHT_MAX_VIEWS", 256), ("MW_ABI_VERSION", 4)):
        assert re.search(rf"#define {k} {v}\b", header), k
    text = " ".join(header.replace("\n * ", " ").split())
    for rule in ("2 * |dx * (j - ja) - dz * (i - ia)| <= |dx| + |dz|", "Q lies in the bounding box of A and B", "vx = (double)dx * cell",
                 "A sees itself; an opaque B is seen", "The reference has no such call", "the call never clears it"):
        assert rule in text, rule
    assert "mw_grid_sight" in engine.SIGNATURES and len(engine.SIGNATURES["mw_grid_sight"][0]) == 12
    check_units_built("mw_sight.hip", "mw_engine_sight.hip")
    check_kernel("mw_sight_kernel", "mw_sight.hip")
    check_does_not_wait("mw_engine_sight.hip")
    # the walk reuses the staging, the grid and the cone by name
    src = open(os.path.join(ROOT, "miniworld_amd", "csrc", "mw_sight.h")).read()
    for name in ("mwnav::each_byte", "mwnav::cell_of", "mwnav::grid_of", "mwnav::covers", "mwseen::in_cone", "mwseen::view_of"):
        assert name in src, name


def test_library_exports_the_entry_point_and_refuses_a_null_engine():
    import ctypes as C
    from miniworld_amd import engine
    p = engine.MwNavParams(0.25, 0.0, 0.0, 4, 4, 0, 0)
    check_refuses_null_engine("mw_grid_sight", p, (C.c_double * 2)(3.0, -1.0), 1, None, None, None, None, None, None, None, None)


def test_grid_sight_argument_errors_and_calls(monkeypatch):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    priv = vec.nav_field()
    gz, gx = priv.gz, priv.gx
    opaque = torch.zeros((5, gz, gx), dtype=torch.uint8)
    weight = torch.zeros((5, gz, gx), dtype=torch.uint8)
    seen = torch.zeros((5, gz, gx), dtype=torch.bool)
    cells = torch.zeros((5, 7), dtype=torch.int32)
    dirs = torch.zeros((5, 7), dtype=torch.float64)
    # the agent: one viewpoint, the default field of view
    n0 = len(lib.calls)
    gain = vec.grid_sight(opaque)
    assert [c[0] for c in lib.calls[n0:]] == ["mw_grid_sight"]
    assert gain.dtype == torch.int32 and tuple(gain.shape) == (5, 1)
    args = lib.calls[-1][1]
    assert (args[1]._obj.cell, args[1]._obj.gx, args[1]._obj.gz) == (0.25, gx, gz)
    assert args[2][0] == 3.0 and args[2][1] == math.cos(vec.default_fov() / 2) and args[3] == 1
    assert args[4] is None and args[5].value == opaque.data_ptr() and all(a is None for a in args[6:9]) and args[9].value == gain.data_ptr() and args[10] is None
    # candidate cells: all round without headings, a cone with them
    gain = vec.grid_sight(opaque.bool(), cells, weight=weight, max_range=4.5, like=priv, seen=seen)
    args = lib.calls[-1][1]
    assert tuple(gain.shape) == (5, 7) and args[2][0] == 4.5 and args[2][1] == -1.0 and args[3] == 7
    assert args[6].value == weight.data_ptr() and args[7].value == cells.data_ptr() and args[8] is None and args[10].value == seen.data_ptr()
    vec.grid_sight(opaque, cells, fov=2 * math.pi)
    assert lib.calls[-1][1][2][1] == -1.0
    mask = torch.tensor([1, 0, 0, 1, 0], dtype=torch.uint8)
    vec.grid_sight(opaque, cells, dirs, fov=1.0, mask=mask)
    args = lib.calls[-1][1]
    assert args[2][1] == math.cos(0.5) and args[4].value == mask.data_ptr() and args[8].value == dirs.data_ptr()
    vec.grid_sight(opaque, cells, dirs)
    assert lib.calls[-1][1][2][1] == math.cos(vec.default_fov() / 2)
    for like in (vec.seen_map(), vec.depth_map(), priv):
        vec.grid_sight(opaque, like=like)
    n0 = len(lib.calls)
    big = torch.zeros((5, engine.SIGHT_MAX_VIEWS + 1), dtype=torch.int32)
    for kw in (dict(opaque=None), dict(opaque=opaque.float()), dict(opaque=opaque[:4]), dict(opaque=opaque.transpose(1, 2)), dict(opaque=opaque.tolist()),
               dict(opaque=opaque[:, :, : gx - 1]), dict(opaque=opaque, weight=weight.to(torch.int16)), dict(opaque=opaque, weight=weight[:, :1]),
               dict(opaque=opaque, seen=seen.to(torch.int32)), dict(opaque=opaque, seen=seen[:2]), dict(opaque=opaque, cells=cells.long()),
               dict(opaque=opaque, cells=cells[:, 0]), dict(opaque=opaque, cells=cells[:4]), dict(opaque=opaque, cells=cells.t()),
               dict(opaque=opaque, cells=cells[:, :0]), dict(opaque=opaque, cells=big), dict(opaque=opaque, cells=cells.tolist()),
               dict(opaque=opaque, dirs=dirs[:, :1].contiguous()), dict(opaque=opaque, cells=cells, dirs=dirs.float()),
               dict(opaque=opaque, cells=cells, dirs=dirs[:, :6].contiguous()), dict(opaque=opaque, cells=cells, fov=1.0),
               dict(opaque=opaque, cells=cells, dirs=dirs, fov=0.0), dict(opaque=opaque, fov=7.0), dict(opaque=opaque, fov=float("nan")),
               dict(opaque=opaque, max_range=0.0), dict(opaque=opaque, max_range=float("inf")), dict(opaque=opaque, max_range=float("nan")),
               dict(opaque=opaque, max_range=None), dict(opaque=opaque, cell=0), dict(opaque=opaque, cell=0.5, like=priv), dict(opaque=opaque, like=priv.field),
               dict(opaque=opaque, mask=torch.zeros(4, dtype=torch.uint8)), dict(opaque=opaque, mask=[1, 0, 0, 1, 0])):
        with pytest.raises(ValueError):
            vec.grid_sight(**kw)
    assert len(lib.calls) == n0         # nothing reached the library
