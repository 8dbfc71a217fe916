"""Grid navigation fields (mw_nav_build_grid; MiniWorldVecEnv.grid_field) without a GPU.

The phases the kernel inlines (miniworld_amd/csrc/mw_nav_grid.h) run on the host in a program of its own (tests/hostcheck/nav_grid.cpp),
built with the address and undefined-behaviour sanitizers, on random grids; its field — by whole-grid passes and by sweeps, which the
program compares — and its query answers are compared, exactly, with the restatement of tests/nav_grid_reference.py (numpy inflation,
heapq Dijkstra with extra costs).  Beside that: the ABI names, the launch arithmetic, and the argument errors of grid_field over a stub
engine."""
import os
import re

import numpy as np
import pytest

import nav_grid_reference as ref
from helpers import stub_engine
from query_checks import ROOT, build, check_kernel, check_refuses_null_engine, check_units_built, launch_of, run

AGENT_RADIUS = 0.4
# (gz, gx, cell): the Sidewalk's grid, the Maze's (odd rows), a coarse one, one of fewer cells than the kernel has lanes
GRIDS = [(640, 36, 0.25), (103, 103, 0.25), (52, 52, 0.5), (4, 12, 1.0)]
ORIGIN = (-1.5, 2.25)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("nav_grid", tmp_path_factory.mktemp("nav_grid"))


def _run(program, tmp_path, raw, cell, inflate, sources=None, extra=None, point=None, reach=None, positions=(), shift=0, flags=0, origin=ORIGIN):
    gz, gx = raw.shape
    lines = [f"{cell!r} {float(inflate)!r} {float(reach or 0.0)!r} {gx} {gz} {flags} {shift}", f"{origin[0]!r} {origin[1]!r}"]
    lines.append("1 " + " ".join(repr(float(v)) for v in point) if point is not None else "0")
    lines.append(f"{int(sources is not None)} {int(extra is not None)}")
    for g in (raw, sources, extra):
        if g is not None:
            lines.append(" ".join(str(int(v)) for v in np.asarray(g).astype(np.int64).ravel()))
    lines.append(str(len(positions)))
    lines += [f"{float(x)!r} {float(z)!r}" for x, z in positions]
    out = run(program, tmp_path / "grids.txt", lines)
    head = out[0].split()
    assert head[0] == "field"
    f = np.array(out[1].split(), np.int64).astype(np.uint16).reshape(gz, gx)
    answers = []
    for line in out[2:2 + len(positions)]:
        c, n, wx, wz = line.split()
        answers.append((int(c), int(n), float.fromhex(wx), float.fromhex(wz)))
    return int(head[1]), f, answers, (int(head[2]), int(head[3]))


def _positions(rng, f, cell, n, origin=ORIGIN):
    """random positions: over the grid, outside it on every side, inside blocked cells, inside source cells"""
    gz, gx = f.shape
    w, h = gx * cell, gz * cell
    span = max(w, h)
    pos = [(origin[0] + rng.uniform(0, w), origin[1] + rng.uniform(0, h)) for _ in range(n)]
    pos += [(origin[0] + rng.uniform(-span, w + span), origin[1] + rng.uniform(-span, h + span)) for _ in range(30)]
    for value in (ref.BLOCKED, 0):
        bj, bi = np.nonzero(f == value)
        for k in rng.integers(0, len(bj), 20) if len(bj) else ():
            pos.append((origin[0] + (bi[k] + rng.uniform(0.05, 0.95)) * cell, origin[1] + (bj[k] + rng.uniform(0.05, 0.95)) * cell))
    return pos


def _random_case(rng, gz, gx, density=0.03, n_sources=6, with_extra=True):
    raw = (rng.random((gz, gx)) < density).astype(np.uint8) * rng.integers(1, 256, (gz, gx)).astype(np.uint8)      # (any byte != 0 blocks)
    sources = np.zeros((gz, gx), np.uint8)
    sources[rng.integers(0, gz, n_sources), rng.integers(0, gx, n_sources)] = rng.integers(1, 256, n_sources)
    extra = rng.integers(0, 21, (gz, gx)).astype(np.uint8) if with_extra else None
    return raw, sources, extra


def _check(program, tmp_path, rng, raw, cell, inflate, sources=None, extra=None, point=None, reach=None, shift=0, want=None):
    want = ref.field(raw, cell, inflate, sources, extra, point, reach, ORIGIN) if want is None else want
    pos = _positions(rng, want, cell, 100)
    ok, got, answers, passes = _run(program, tmp_path, raw, cell, inflate, sources, extra, point, reach, pos, shift)
    assert ok == 1
    assert got.shape == want.shape and np.array_equal(got, want), ("cells that differ", int((got != want).sum()))
    seen = set()
    for (x, z), a in zip(pos, answers):
        q = ref.query(want, ORIGIN, cell, x, z)
        assert a == q, ((x, z), a, q)
        seen.add("none" if q[0] < 0 else "source" if q[0] == 0 else "way")
    return want, seen, passes


@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("gz,gx,cell", GRIDS)
def test_field_and_query_equal_the_restatement(program, tmp_path, gz, gx, cell, with_extra):
    """3 % raw obstacles, six random sources (a grid comes out 15 to 33 % blocked: some land on blocked cells), extra costs 0 .. 20 or
    none, the default clearance; the rows at every distance from a 4-byte boundary in turn.  The program builds by whole-grid passes and by sweeps and refuses to answer unless both agree."""
    rng = np.random.default_rng(4100 + gz + int(with_extra))
    for shift in range(4) if gz * gx < 5000 else (int(with_extra) + 1,):
        raw, sources, extra = _random_case(rng, gz, gx, with_extra=with_extra)
        f, seen, passes = _check(program, tmp_path, rng, raw, cell, AGENT_RADIUS + cell / 2, sources, extra, shift=shift)
        blocked = f == ref.BLOCKED
        assert blocked.sum() >= (raw != 0).sum() and (blocked[raw != 0]).all()
        if gz * gx > 100:
            assert (f == 0).any() and ((f > 0) & (f < ref.UNREACHED)).any() and {"way", "source"} <= seen, seen
            assert passes[0] > passes[1] >= 2       # sweeps settle in fewer rounds than whole-grid passes


def test_extra_costs_change_the_field_and_sources_stay_zero(program, tmp_path):
    rng = np.random.default_rng(4200)
    raw, sources, extra = _random_case(rng, 52, 52)
    extra[sources != 0] = 20
    plain, _, _ = _check(program, tmp_path, rng, raw, 0.5, 0.65, sources, None)
    weighted, _, _ = _check(program, tmp_path, rng, raw, 0.5, 0.65, sources, extra)
    assert np.array_equal(weighted == 0, plain == 0) and (weighted == 0).any()
    reached = plain < ref.UNREACHED
    assert (weighted[reached] >= plain[reached]).all() and (weighted[reached] > plain[reached]).any()


def test_inflate_zero_blocks_the_raw_cells_only(program, tmp_path):
    rng = np.random.default_rng(4300)
    raw, sources, extra = _random_case(rng, 103, 103, density=0.2)
    f, _, _ = _check(program, tmp_path, rng, raw, 0.25, 0.0, sources, extra, shift=3)
    assert np.array_equal(f == ref.BLOCKED, raw != 0)


def test_the_threshold_is_strict():
    """cell 0.25, inflate 0.5: offset (2, 0) is exactly 0.5 m away and stays free, (1, 1) is blocked — the stencil written out"""
    offsets, slack = ref.stencil(0.25, 0.5)
    assert slack == 0.0 and ref.radius(0.25, 0.5) == 2
    assert sorted(offsets) == sorted([(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)])


def test_exact_threshold_stencil_by_hand(program, tmp_path):
    rng = np.random.default_rng(4400)
    by_hand = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
    raw = np.zeros((21, 23), np.uint8)
    for j, i in ((10, 10), (0, 0), (20, 22), (5, 22), (15, 3), (15, 5)):
        raw[j, i] = 1
    sources = np.zeros_like(raw)
    sources[2, 12] = sources[18, 1] = 1
    blocked = ref.inflated(raw, by_hand)
    assert blocked[11, 11] and not blocked[10, 12] and not blocked[12, 10] and blocked.sum() == 9 + 4 + 4 + 6 + 15
    want, _ = ref.costs(blocked, sources)
    _check(program, tmp_path, rng, raw, 0.25, 0.5, sources, None, want=want)
    # ... and the radius the kernel walks: the smallest R with R * cell >= inflate
    import subprocess
    for cell, inflate, r in ((0.25, 0.5, 2), (0.25, 0.0, 0), (0.25, 0.525, 3), (0.25, 0.5000001, 3), (1.0, 0.9, 1), (0.25, 4.0, 16), (0.25, 4.01, -1),
                             (0.25, -0.1, -1), (0.25, float("nan"), -1)):
        assert int(subprocess.run([program, "--radius", repr(cell), repr(inflate)], capture_output=True, text=True, check=True).stdout) == r, (cell, inflate)
        if r >= 0:
            assert ref.radius(cell, inflate) == r


def test_no_source_is_no_error(program, tmp_path):
    rng = np.random.default_rng(4500)
    raw, sources, _ = _random_case(rng, 52, 52)
    # an empty mask
    f, seen, _ = _check(program, tmp_path, rng, raw, 0.5, 0.65, np.zeros_like(raw), None)
    assert not (f < ref.UNREACHED).any() and (f == ref.UNREACHED).any() and seen == {"none"}
    # sources on blocked cells only: raw ones and inflated ones
    blocked = ref.inflated(raw, ref.stencil(0.5, 0.65)[0])
    assert (blocked & (raw == 0)).any()
    f, seen, _ = _check(program, tmp_path, rng, raw, 0.5, 0.65, blocked.astype(np.uint8), None)
    assert not (f < ref.UNREACHED).any() and seen == {"none"}
    # an all-blocked grid
    f, seen, _ = _check(program, tmp_path, rng, np.ones((12, 7), np.uint8), 0.5, 0.0, np.ones((12, 7), np.uint8), None)
    assert (f == ref.BLOCKED).all() and seen == {"none"}


def test_point_sources_alone_and_with_a_mask(program, tmp_path):
    rng = np.random.default_rng(4600)
    raw, sources, extra = _random_case(rng, 103, 103)
    point = (ORIGIN[0] + 11.3, 0.0, ORIGIN[1] + 17.1)
    alone, seen, _ = _check(program, tmp_path, rng, raw, 0.25, 0.525, None, extra, point=point, reach=0.6, shift=1)
    assert 4 < (alone == 0).sum() < 30
    both, _, _ = _check(program, tmp_path, rng, raw, 0.25, 0.525, sources, extra, point=point, reach=0.6, shift=1)
    mask_only, _, _ = _check(program, tmp_path, rng, raw, 0.25, 0.525, sources, extra, shift=1)
    assert np.array_equal(both == 0, (alone == 0) | (mask_only == 0))
    assert np.array_equal(both, np.minimum(alone, mask_only))       # the cost to the nearest source


def test_a_cost_that_does_not_fit_is_refused(program, tmp_path):
    """a free 640 x 36 grid, extra 100 everywhere, one corner source: the far corner would cost 35 * 7 + 604 * 5 + 639 * 100 = 67 165"""
    raw = np.zeros((640, 36), np.uint8)
    sources = np.zeros_like(raw)
    sources[0, 0] = 1
    extra = np.full_like(raw, 100)
    out, top = ref.costs(raw != 0, sources, extra)
    assert out is None and top == 67165 >= ref.UNREACHED
    ok, f, answers, _ = _run(program, tmp_path, raw, 0.25, 0.0, sources, extra, positions=[(ORIGIN[0] + 0.1, ORIGIN[1] + 0.1)])
    assert ok == 0 and (f == ref.BLOCKED).all() and answers[0][:2] == (-1, -1)
    # ... and with extra 90 it fits
    extra[:] = 90
    out, top = ref.costs(raw != 0, sources, extra)
    assert top == 3265 + 639 * 90 < ref.UNREACHED
    ok, f, _, _ = _run(program, tmp_path, raw, 0.25, 0.0, sources, extra)
    assert ok == 1 and np.array_equal(f, out)


# ---------------------------------------------------------------------------------------------------------------- the interface

def test_launch_arithmetic(program):
    for cells, weighted, lds in ((1, 0, 16), (1, 1, 32), (48, 0, 96), (48, 1, 144), (103 * 103, 0, 21232), (103 * 103, 1, 21232 + 10624),
                                 (32768, 0, 65536), (32768, 1, 65536 + 32768)):
        got = launch_of(program, 7, cells, weighted)
        assert got == {"grid": 7, "threads": 512, "lds": lds, "fits": 1}, (cells, weighted, got)
        assert got["lds"] <= 96 * 1024
    for cells in (0, -3, 32769):
        assert launch_of(program, 7, cells, 1)["fits"] == 0


def test_header_declares_the_entry_point():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"int mw_nav_build_grid\(mw_engine \*e, const mw_nav_params \*params, const uint8_t \*d_mask,", header)
    assert (engine.NAV_GRID, engine.NAV_MAX_INFLATE) == (4, 16)
    for k, v in (("MW_NAV_GRID", 4), ("MW_NAV_MAX_INFLATE", 16), ("MW_ABI_VERSION", 4)):
        assert re.search(rf"#define {k} {v}\b", header), k
    text = " ".join(header.replace("\n * ", " ").split())
    for rule in ("sqrt((double)(di*di + dj*dj)) * cell < margin", "R the smallest integer with R * cell >= margin", "the agent's radius is NOT added",
                 "a source is 0, whatever d_extra says"):
        assert rule in text, rule
    assert "mw_nav_build_grid" in engine.SIGNATURES and len(engine.SIGNATURES["mw_nav_build_grid"][0]) == 9
    check_units_built("mw_nav_grid.hip", "mw_engine_nav.hip")
    check_kernel("mw_nav_grid_kernel", "mw_nav_grid.hip")


def test_library_exports_the_entry_point_and_refuses_a_null_engine():
    from miniworld_amd import engine
    p = engine.MwNavParams(0.25, 0.125, 0.0, 4, 4, engine.NAV_GRID, 0)
    check_refuses_null_engine("mw_nav_build_grid", p, None, None, None, None, None, None, None)


def test_grid_field_argument_errors_and_calls(monkeypatch):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import MiniWorldVecEnv, NavField
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    priv = vec.nav_field()
    gz, gx = priv.gz, priv.gx
    blocked = torch.zeros((5, gz, gx), dtype=torch.uint8)
    sources = torch.zeros((5, gz, gx), dtype=torch.bool)
    extra = torch.zeros((5, gz, gx), dtype=torch.uint8)
    n0 = len(lib.calls)
    fld = vec.grid_field(blocked, sources)
    assert [c[0] for c in lib.calls[n0:]] == ["mw_nav_build_grid"]
    assert isinstance(fld, NavField) and fld.obstacles == "grid" and fld.target is None and fld.points is None
    assert fld.field.dtype == torch.uint16 and tuple(fld.field.shape) == (5, gz, gx)
    assert (fld.cell, fld.gx, fld.gz, fld.params.flags) == (0.25, gx, gz, engine.NAV_GRID)
    assert fld.margin == float(vec.engine.cfg.agent_radius) + 0.125        # nav_field's default clearance, the agent's radius included
    args = lib.calls[-1][1]
    assert args[2] is None and args[3].value == blocked.data_ptr() and args[4].value == sources.data_ptr() and args[5] is None and args[6] is None
    assert args[7].value == fld.field.data_ptr()
    # points, extra costs, an adopted grid, no inflation
    pts = torch.zeros((5, 3), dtype=torch.float64)
    pf = vec.grid_field(blocked.bool(), target=pts, reach=0.5, extra=extra, inflate=0, like=priv)
    assert pf.points is pts and pf.params.reach == 0.5 and pf.margin == 0.0 and (pf.gx, pf.gz) == (gx, gz)
    args = lib.calls[-1][1]
    assert args[4] is None and args[5].value == pts.data_ptr() and args[6].value == extra.data_ptr()
    for like in (vec.seen_map(), vec.seen_map(like=fld), fld):
        assert vec.grid_field(blocked, sources, like=like).gx == gx
    # a rebuild in place under a mask
    mask = torch.tensor([1, 0, 0, 1, 0], dtype=torch.uint8)
    assert vec.grid_field(blocked, sources, extra=extra, mask=mask, into=fld) is fld
    args = lib.calls[-1][1]
    assert args[2].value == mask.data_ptr() and args[6].value == extra.data_ptr() and args[7].value == fld.field.data_ptr()
    assert vec.grid_field(blocked, into=pf) is pf and lib.calls[-1][1][5].value == pts.data_ptr()       # (its own points serve)
    n0 = len(lib.calls)
    for kw in (dict(blocked=None, sources=sources), dict(blocked=blocked), dict(blocked=blocked.float(), sources=sources),
               dict(blocked=blocked[:4], sources=sources), dict(blocked=blocked.transpose(1, 2), sources=sources),
               dict(blocked=blocked[:, :, : gx - 1], sources=sources[:, :, : gx - 1]), dict(blocked=blocked.tolist(), sources=sources),
               dict(blocked=blocked, sources=sources.to(torch.int32)), dict(blocked=blocked, sources=sources, extra=extra.to(torch.int16)),
               dict(blocked=blocked, sources=sources, extra=extra[:, :1]), dict(blocked=blocked, target=pts), dict(blocked=blocked, target=pts, reach=0.0),
               dict(blocked=blocked, target=pts.float(), reach=1.0), dict(blocked=blocked, target=3, reach=1.0), dict(blocked=blocked, sources=sources, reach=1.0),
               dict(blocked=blocked, sources=sources, inflate=-0.1), dict(blocked=blocked, sources=sources, inflate=float("nan")),
               dict(blocked=blocked, sources=sources, inflate=16 * 0.25 + 0.01), dict(blocked=blocked, sources=sources, cell=0),
               dict(blocked=blocked, sources=sources, cell=0.5, like=priv), dict(blocked=blocked, sources=sources, like=priv.field),
               dict(blocked=blocked, sources=sources, mask=torch.zeros(4, dtype=torch.uint8)), dict(blocked=blocked, sources=sources, into=priv),
               dict(blocked=blocked, sources=sources, into=fld.field), dict(blocked=blocked, sources=sources, into=fld, inflate=0.2),
               dict(blocked=blocked, sources=sources, into=fld, like=priv), dict(blocked=blocked, into=fld)):
        with pytest.raises(ValueError):
            vec.grid_field(**kw)
    with pytest.raises(ValueError):
        vec.nav_field(into=fld)
    assert len(lib.calls) == n0         # nothing reached the library
    # the three uses of the result
    vec.nav_query(fld)
    args = lib.calls[-1][1]
    assert lib.calls[-1][0] == "mw_nav_query" and args[2] is None and args[3].value == fld.field.data_ptr()
    w = vec.ego_window(size=9, frame="north", planes=())
    _, sample = vec.ego_update(w, source=fld)
    assert sample.dtype == torch.uint16 and lib.calls[-1][0] == "mw_ego_map"
    assert (vec.seen_map(like=fld).gx, vec.seen_map(like=fld).gz) == (gx, gz)
