"""Grid regions (mw_grid_regions; MiniWorldVecEnv.grid_regions) without a GPU.

The phases the kernel inlines (miniworld_amd/csrc/mw_regions.h: the staging, the hook passes, pointer jumping, the sizes
and sums gathered run by run, the ranking of the roots, the representative) run on the host in a program of its own
(tests/hostcheck/grid_regions.cpp), built with the address and undefined-behaviour sanitizers; every output is compared, exactly, with
the restatement of tests/regions_reference.py, a flood fill that shares nothing with the header.  Beside that: the shapes that take a
labelling the most rounds, the ties of the representative, the ABI names, the launch arithmetic, and the argument errors of
grid_regions over a stub engine."""
import os
import re
import subprocess

import numpy as np
import pytest

import regions_reference as ref
from helpers import stub_engine
from query_checks import ROOT, build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, launch_of, run

# (gz, gx): the Maze's grid (odd rows), the Sidewalk's, the cell limit, a coarse one, one of fewer cells than the kernel has lanes
GRIDS = [(103, 103), (640, 36), (128, 256), (52, 52), (4, 12)]
# (connectivity, min_cells, K, want_sum, want_label): both connectivities, min_cells 1 and 3, K = 256 and 1, each with and without the
# optional outputs
CALLS = [(4, 1, 256, 1, 1), (4, 3, 256, 0, 1), (4, 1, 1, 1, 0), (4, 3, 1, 0, 0), (8, 1, 256, 1, 1), (8, 3, 256, 1, 0), (8, 1, 1, 0, 1), (8, 3, 1, 1, 1)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("grid_regions", tmp_path_factory.mktemp("grid_regions"))


def _answers(program, tmp_path, member, calls, shift=0):
    """per call: (count, rounds, size[K], cell[K], sum[K, 2] or None, label[gz, gx] or None)"""
    gz, gx = member.shape
    lines = [f"0.25 {gx} {gz} {shift} {len(calls)}", " ".join(str(int(v)) for v in np.asarray(member).astype(np.int64).ravel())]
    lines += [" ".join(str(int(v)) for v in call) for call in calls]
    rows = iter(run(program, tmp_path / "regions.txt", lines))
    out = []
    for _, _, K, want_sum, want_label in calls:
        head = next(rows).split()
        assert head[0] == "regions"
        size, cell = (np.array(next(rows).split(), np.int64).astype(np.int32) for _ in range(2))
        total = np.array(next(rows).split(), np.int64).astype(np.int32).reshape(K, 2) if want_sum else None
        label = np.array(next(rows).split(), np.int64).astype(np.int16).reshape(gz, gx) if want_label else None
        out.append((int(head[1]), int(head[2]), size, cell, total, label))
    assert next(rows, None) is None
    return out


def _check(program, tmp_path, member, calls, shift=0):
    """every call's outputs against the restatement; returns the answers"""
    gz, gx = member.shape
    comps = {c: ref.components(member, c) for c in {call[0] for call in calls}}
    answers = _answers(program, tmp_path, member, calls, shift)
    for call, (count, rounds, size, cell, total, label) in zip(calls, answers):
        conn, min_cells, K = call[:3]
        want = ref.regions(member, conn, min_cells, K, comps[conn])
        assert 1 <= rounds <= gz * gx + 1, (call, rounds)
        assert count == want[0], (call, count, want[0])
        assert np.array_equal(size, want[1]), (call, size[:8], want[1][:8])
        assert np.array_equal(cell, want[2]), (call, cell[:8], want[2][:8])
        assert total is None or np.array_equal(total, want[3]), (call, total[:4], want[3][:4])
        assert label is None or np.array_equal(label, want[4]), (call, int((label != want[4]).sum()))
        # the representative is a cell of its own region
        if label is not None:
            for k in range(min(count, K)):
                assert label[cell[k] // gx, cell[k] % gx] == k + 1, (call, k)
    return answers


def _members(gz, gx, density):
    """the mask of default_rng(0) at `density`, as random bytes 1 .. 255 (any byte != 0 belongs)"""
    m = np.random.default_rng(0).random((gz, gx)) < density
    return m.astype(np.uint8) * np.random.default_rng(6100 + gz).integers(1, 256, (gz, gx)).astype(np.uint8)


@pytest.mark.parametrize("density", [0.3, 0.6])
@pytest.mark.parametrize("gz,gx", GRIDS)
def test_every_output_equals_the_restatement(program, tmp_path, gz, gx, density):
    member = _members(gz, gx, density)
    answers = _check(program, tmp_path, member, CALLS, shift=(gz + int(density * 10)) % 4)
    counts = [a[0] for a in answers]
    if gz * gx > 1000:
        assert any(c > K for c, (_, _, K, *_) in zip(counts, CALLS)), counts         # a cut list
    if (gz, gx, density) == (103, 103, 0.3):
        assert counts[0] == 1428 and counts[1] == 365       # (4-connected: all regions, those of 3 cells and more)
    if (gz, gx, density) == (128, 256, 0.6):
        assert 1 < counts[4] <= 256 and answers[4][2].max() > 19000         # an uncut list, one region of most of the mask


@pytest.mark.parametrize("shape", ["serpentine", "spiral", "staircase"])
def test_the_long_regions_settle(program, tmp_path, shape):
    """128 x 256, one region whose ends lie thousands of cells apart along it, both connectivities: in a handful of rounds, where
    the bound is 32769"""
    member = getattr(ref, shape)(128, 256)
    calls = [(c, 1, 256, 1, 1) for c in (4, 8)]
    for count, rounds, size, cell, total, label in _check(program, tmp_path, member, calls):
        print(shape, "rounds", rounds)
        assert rounds <= 64
        assert count == 1 and size[0] == int(member.sum()) and (label == member).all()


def test_checkerboard_full_and_empty(program, tmp_path):
    gz, gx = 128, 256
    calls = [(4, 1, 256, 1, 1), (8, 1, 256, 1, 1), (4, 2, 256, 1, 1)]
    board = ref.checkerboard(gz, gx)
    (c4, _, size4, cell4, _, label4), (c8, _, size8, _, _, label8), (c2, _, size2, cell2, total2, label2) = _check(program, tmp_path, board, calls)
    assert c4 == 16384 and (size4 == 1).all() and np.array_equal(cell4, np.flatnonzero(board)[:256])       # (rows 0 and 1: 128 each)
    assert (label4 > 0).sum() == 256 and (label4 == -1).sum() == 16384 - 256 and (label4[board == 0] == 0).all()
    assert c8 == 1 and size8[0] == 16384 and (label8 == board).all()
    assert c2 == 0 and not size2.any() and (cell2 == -1).all() and not total2.any() and (label2 == -board.astype(np.int16)).all()
    (cf, _, sizef, cellf, totalf, labelf), *_ = _check(program, tmp_path, np.full((gz, gx), 255, np.uint8), calls[:2])
    assert cf == 1 and sizef[0] == 32768 and (labelf == 1).all()
    assert totalf[0].tolist() == [256 * sum(range(128)), 128 * sum(range(256))] and max(totalf[0]) <= 2 ** 30
    assert cellf[0] == 63 * 256 + 127       # (the centroid (63.5, 127.5) is a corner of four cells: the lowest of them)
    for count, _, size, cell, total, label in _check(program, tmp_path, np.zeros((gz, gx), np.uint8), calls):
        assert count == 0 and not size.any() and (cell == -1).all() and not total.any() and not label.any()


def test_ties_go_to_the_lowest_cell(program, tmp_path):
    """a 2 x 2 block: its four cells are equally far from the centroid; a ring of 8 cells around a free one: its four edge cells are.
    The centroid of the ring is no member: the representative still is."""
    m = np.zeros((7, 9), np.uint8)
    m[1:3, 1:3] = 1
    m[3:6, 5:8] = 1
    m[4, 6] = 0
    for conn in (4, 8):
        (count, _, size, cell, total, label), = _check(program, tmp_path, m, [(conn, 1, 4, 1, 1)])
        assert count == 2 and size.tolist() == [4, 8, 0, 0] and cell.tolist() == [1 * 9 + 1, 3 * 9 + 6, -1, -1]
        assert total.tolist() == [[6, 6], [32, 48], [0, 0], [0, 0]] and label[4, 6] == 0
    # a diagonal pair: two regions with 4, one with 8 — whose two cells tie again
    d = np.zeros((3, 3), np.uint8)
    d[0, 1] = d[1, 2] = 1
    (c4, _, _, cell4, _, _), (c8, _, size8, cell8, _, _) = _check(program, tmp_path, d, [(4, 1, 2, 1, 1), (8, 1, 2, 1, 1)])
    assert c4 == 2 and cell4.tolist() == [1, 5] and c8 == 1 and size8.tolist() == [2, 0] and cell8.tolist() == [1, -1]


def test_the_program_refuses_what_the_call_refuses(program, tmp_path):
    for head, call in (("0.25 4 4 0 1", "5 1 4 1 1"), ("0.25 4 4 0 1", "4 0 4 1 1"), ("0.25 4 4 0 1", "4 1 0 1 1"), ("0.25 4 4 0 1", "4 1 257 1 1"),
                       ("0.0 4 4 0 1", "4 1 4 1 1"), ("0.25 0 4 0 1", "4 1 4 1 1"), ("0.25 256 129 0 1", "4 1 4 1 1")):
        path = tmp_path / "refused.txt"
        path.write_text("\n".join([head, " ".join(["0"] * 16), call]) + "\n")
        assert subprocess.run([program, str(path)], capture_output=True, text=True).returncode == 2, (head, call)


# ---------------------------------------------------------------------------------------------------------------- the interface

def test_launch_arithmetic(program):
    from miniworld_amd import engine
    k_max = engine.REGION_MAX
    # labels and sizes: 2 bytes per cell each, rounded up to 16; 24 bytes per listed region, rounded up to 16; 1 KiB of lane words
    for cells, K, lds in ((1, 1, 16 + 16 + 32 + 1024), (48, 3, 96 + 96 + 80 + 1024), (103 * 103, 32, 2 * 21232 + 768 + 1024),
                          (103 * 103, k_max, 2 * 21232 + 6144 + 1024), (32768, 1, 2 * 65536 + 32 + 1024), (32768, k_max, 2 * 65536 + 6144 + 1024)):
        got = launch_of(program, 7, cells, K)
        assert got == {"grid": 7, "threads": 256, "lds": lds, "fits": 1}, (cells, K, got)
        assert got["lds"] <= 160 * 1024
    assert 3 * launch_of(program, 7, 103 * 103, k_max)["lds"] <= 160 * 1024       # the Maze's grid: three workgroups share a CU
    for cells, K in ((0, 1), (-3, 1), (32769, 1), (100, 0), (100, k_max + 1), (100, -1)):
        assert launch_of(program, 7, cells, K)["fits"] == 0, (cells, K)


def test_header_declares_the_entry_point():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"int mw_grid_regions\(mw_engine \*e, const mw_nav_params \*grid", header)
    assert engine.REGION_MAX == engine.SIGHT_MAX_VIEWS == 256
    for k, v in (("MW_REGION_MAX", 256), ("MW_SIGHT_MAX_VIEWS", 256), ("MW_ABI_VERSION", 4)):
        assert re.search(rf"#define {k} {v}\b", header), k
    text = " ".join(header.replace("\n * ", " ").split())
    for rule in ("(size * j - sum_j)^2 + (size * i - sum_i)^2", "ties go to the lowest flat index", "its ROOT is its lowest flat index",
                 "also the four that share a corner, unconditionally", "It may exceed K", "The reference has no such call",
                 "nothing of an env under a zero mask byte is read or written"):
        assert rule in text, rule
    assert "mw_grid_regions" in engine.SIGNATURES and len(engine.SIGNATURES["mw_grid_regions"][0]) == 13
    check_units_built("mw_regions.hip", "mw_engine_regions.hip")
    check_kernel("mw_regions_kernel", "mw_regions.hip")
    check_does_not_wait("mw_engine_regions.hip")
    # the staging and the launch tail are the shared ones, by name
    assert "mwnav::each_byte" in open(os.path.join(ROOT, "miniworld_amd", "csrc", "mw_regions.h")).read()
    unit = open(os.path.join(ROOT, "miniworld_amd", "csrc", "mw_engine_regions.hip")).read()
    for name in ("grid_check(", "launch_query(", "regions_lds_set", "mwpolicy::regions_launch("):
        assert name in unit, name


def test_library_exports_the_entry_point_and_refuses_a_null_engine():
    from miniworld_amd import engine
    p = engine.MwNavParams(0.25, 0.0, 0.0, 4, 4, 0, 0)
    check_refuses_null_engine("mw_grid_regions", p, 4, 1, 4, None, None, None, None, None, None, None, None)


def test_grid_regions_argument_errors_and_calls(monkeypatch):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.queries import GridRegions
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    priv = vec.nav_field()
    gz, gx = priv.gz, priv.gx
    member = torch.zeros((5, gz, gx), dtype=torch.uint8)
    n0 = len(lib.calls)
    r = vec.grid_regions(member)
    assert [c[0] for c in lib.calls[n0:]] == ["mw_grid_regions"]
    assert isinstance(r, GridRegions) and r.label is None and (r.connectivity, r.min_cells, r.max_regions) == (4, 1, 32)
    assert (r.count.dtype, tuple(r.count.shape)) == (torch.int32, (5,)) and tuple(r.size.shape) == tuple(r.cell.shape) == (5, 32) and tuple(r.sum.shape) == (5, 32, 2)
    assert bool((r.cell == -1).all()) and tuple(r.centroid.shape) == (5, 32, 2) and bool(r.centroid.isnan().all())
    args = lib.calls[-1][1]
    assert (args[1]._obj.cell, args[1]._obj.gx, args[1]._obj.gz) == (0.25, gx, gz) and tuple(args[2:5]) == (4, 1, 32)
    assert args[5] is None and args[6].value == member.data_ptr() and [a.value for a in args[7:11]] == [t.data_ptr() for t in (r.count, r.size, r.cell, r.sum)]
    assert args[11] is None
    mask = torch.tensor([1, 0, 0, 1, 0], dtype=torch.uint8)
    r = vec.grid_regions(member.bool(), connectivity=8, min_cells=3, max_regions=engine.REGION_MAX, like=priv, mask=mask, labels=True, sums=False)
    args = lib.calls[-1][1]
    assert tuple(args[2:5]) == (8, 3, 256) and args[5].value == mask.data_ptr() and args[10] is None and args[11].value == r.label.data_ptr()
    assert r.sum is None and r.centroid is None and r.label.dtype == torch.int16 and tuple(r.label.shape) == (5, gz, gx)
    # into=: the record's own tensors and parameters again
    again = vec.grid_regions(member, into=r)
    args = lib.calls[-1][1]
    assert again is r and tuple(args[2:5]) == (8, 3, 256) and args[7].value == r.count.data_ptr() and args[11].value == r.label.data_ptr()
    for like in (vec.seen_map(), vec.depth_map(), vec.object_map(), priv):
        vec.grid_regions(member, like=like)
    n0 = len(lib.calls)
    for kw in (dict(member=None), dict(member=member.float()), dict(member=member.to(torch.int16)), dict(member=member[:4]), dict(member=member.transpose(1, 2)),
               dict(member=member[:, :, : gx - 1]), dict(member=member.tolist()), dict(member=member.to("meta")),
               dict(member=member, connectivity=6), dict(member=member, connectivity=True), dict(member=member, connectivity="8"),
               dict(member=member, max_regions=0), dict(member=member, max_regions=engine.REGION_MAX + 1), dict(member=member, max_regions=2.0),
               dict(member=member, min_cells=0), dict(member=member, min_cells=-1), dict(member=member, min_cells=1.5),
               dict(member=member, labels=1), dict(member=member, sums=None), dict(member=member, cell=0), dict(member=member, cell=0.5, like=priv),
               dict(member=member, like=priv.field), dict(member=member, mask=torch.zeros(4, dtype=torch.uint8)), dict(member=member, mask=[1, 0, 0, 1, 0]),
               dict(member=member, into=priv), dict(member=member, into=r, connectivity=8), dict(member=member, into=r, labels=True),
               dict(member=member, into=r, like=priv)):
        with pytest.raises(ValueError):
            vec.grid_regions(**kw)
    assert len(lib.calls) == n0         # nothing reached the library
