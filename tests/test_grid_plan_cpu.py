"""Grid rollouts without a GPU: the plan's loop over the staged bit plane (csrc/mw_gridplan.h) on the host under sanitizers
(hostcheck/grid_plan.cpp), bit for bit against grid_plan_reference.py; the launch and the interface."""
import numpy as np
import pytest

import grid_plan_reference as ref
import scan_reference as scan
from helpers import stub_engine
from query_checks import build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, launch_of, run

MAX_PLANS, STEP = 4096, (0.15, 0.0, 15.0)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("grid_plan", tmp_path_factory.mktemp("grid_plan"))


def _run(program, path, gz, gx, shift, flags, stop_at, radius, pose, explicit, step, plans, opaque, field, extra, trace):
    """the program on one env: (pose bits [P, 3], stats [P, 5], trace bits [T, P, 3] or None)"""
    (T, P), row = plans.shape, lambda v: " ".join(str(int(x)) for x in np.ravel(v))       # noqa: E731
    extent = (scan.MIN[0], scan.MIN[0] + gx * scan.CELL - 0.1, scan.MIN[1], scan.MIN[1] + gz * scan.CELL - 0.1)
    lines = [" ".join(repr(float(v)) for v in pose), " ".join(repr(v) for v in extent), f"{scan.CELL!r} {gx} {gz} {shift} {flags} {T} {P} {stop_at} {radius!r}",
             " ".join(repr(v) for v in STEP), f"{int(explicit)} {int(step is not None)} {int(field is not None)} {int(extra is not None)} {int(trace)}"]
    lines += [" ".join(repr(float(v)) for v in step)] if step is not None else []
    lines += [row(plans), row(opaque)] + [row(v) for v in (field, extra) if v is not None]
    rows = [r.split() for r in run(program, path, lines)]
    assert len(rows) == P + (T * P if trace else 0)
    hexes = lambda rs: np.array([[int(v, 16) for v in r[:3]] for r in rs], np.uint64)      # noqa: E731
    return hexes(rows[:P]), np.array([[int(v) for v in r[3:]] for r in rows[:P]]), hexes(rows[P:]).reshape(T, P, 3) if trace else None


@pytest.mark.parametrize("gz,gx,shift", [g + (s,) for g, s in zip(scan.GRIDS, (1, 0, 2, 3, 0))])
@pytest.mark.parametrize("P", [1, 65])
@pytest.mark.parametrize("T", [1, 7, 64])
def test_the_loop_equals_the_restatement(program, tmp_path, gz, gx, shift, P, T):
    """every start pose on a map of another density, radius, `outside` mode and plan dtype each, turning with the case so that each
    grid meets them all; with and without field, extra, stop_at (0 and a mid value), a step override with a drift, an explicit pose
    and a trace: pose, stats and trace are the restatement's bits"""
    rng, bumps, stops = np.random.default_rng(5300 + gz + 7 * P + T), 0, 0
    for no, name in enumerate(ref.POSES):
        turn = no + P + T + gz
        opaque, field, extra = ref.planes_of(rng, gz, gx, ref.DENSITIES[turn % 4])
        radius, outside, byte_plans = ref.RADII[(turn // 2) % 4] * scan.CELL, (turn // 3) % 2, turn % 2
        field, extra = (field if turn % 3 else None), (extra if (turn // 2) % 2 else None)
        stop_at = (-1, 0, 25)[turn % 3] if field is not None else -1
        step, trace = ((0.2, 0.03, 22.5) if turn % 2 else None), bool(turn % 2) or T == 7
        pose, plans = ref.pose_of(name, rng, gx, gz, scan.MIN, scan.CELL), ref.plans_of(rng, T, P)
        want = ref.rollout(plans, pose, step or STEP, radius, outside, stop_at, scan.MIN, scan.CELL, opaque, field, extra)
        got = _run(program, tmp_path / "plan.txt", gz, gx, shift, outside | 2 * byte_plans, stop_at, radius, pose, no % 2, step, plans, opaque, field, extra, trace)
        assert np.array_equal(got[0], want[0].view(np.uint64)) and np.array_equal(got[1], want[1]), (name, turn)
        assert not trace or np.array_equal(got[2], want[2].view(np.uint64)), (name, turn)
        bumps, stops = bumps + int(want[1][:, 3].sum()), stops + int((want[1][:, 2] < T).sum())
    assert P * T < 400 or (bumps > 0 and (stops > 0 or T < 64 or gz * gx < 10000))        # (the larger cases do meet refusals and stops)


def test_launch_and_interface(program):
    from miniworld_amd import engine
    # (a workgroup of the plans rounded up to a wavefront, 256 lanes at most; the bit plane with its ring and a spare word, rounded up to 16)
    for gx, gz, plans, grid, threads, lds in ((1, 1, 1, 7, 64, 16), (103, 103, 64, 7, 64, 1392), (103, 103, 65, 7, 128, 1392), (256, 128, 256, 7, 256, 4208),
                                              (256, 128, MAX_PLANS, 7 * 16, 256, 4208), (1, 32768, 32, 7, 64, 12304), (32768, 1, 257, 7 * 2, 256, 12304)):
        assert launch_of(program, 7, gx, gz, plans) == {"grid": grid, "threads": threads, "lds": lds, "fits": 1}, (gx, gz, plans)
    assert all(launch_of(program, 7, gx, gz, plans)["fits"] == 0 for gx, gz, plans in ((0, 1, 1), (1, 0, 1), (256, 129, 1), (4, 4, 0), (4, 4, MAX_PLANS + 1)))
    check_units_built("mw_gridplan.hip", "mw_engine_gridplan.hip")
    check_kernel("mw_gridplan_kernel", "mw_gridplan.hip")
    check_does_not_wait("mw_engine_gridplan.hip")
    check_refuses_null_engine("mw_grid_plan", engine.MwNavParams(0.25, 0.0, 0.0, 4, 4, 0, 0), None, 0, 1, 1, -1, *[None] * 11)


def test_grid_rollout_calls_and_argument_errors(monkeypatch):
    """(the checks of the map and of the byte planes are _map_grid's and _cell_grid's, held by grid_sight's tests)"""
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    m = vec.scan_map()
    new = lambda dtype, *shape: torch.zeros(shape, dtype=dtype)                     # noqa: E731
    ptr = lambda args: [a and a.value for a in args[7:17]]                          # noqa: E731  (mask .. trace; the stream is behind them)
    blocked, plans, pose = new(torch.uint8, 5, m.gz, m.gx), new(torch.int32, 6, 5, 9), new(torch.float64, 5, 3)
    field, extra, step = new(torch.uint16, 5, m.gz, m.gx), new(torch.bool, 5, m.gz, m.gx), new(torch.float64, 5, 3)
    n0, r = len(lib.calls), vec.grid_rollout(blocked, plans, like=m)
    args = lib.calls[-1][1]
    assert [k[0] for k in lib.calls[n0:]] == ["mw_grid_plan"] and r.trace is None and tuple(r.reach.shape) == (5, 9) and r.cost.data_ptr() == r.stats.data_ptr() + 16
    assert list(args[2]) == [float(vec.engine.cfg.agent_radius)] and list(args[3:7]) == [engine.GPLAN_OUTSIDE_BLOCKS, 6, 9, -1]
    assert ptr(args) == [None, blocked.data_ptr(), plans.data_ptr(), None, None, None, None, r.pose.data_ptr(), r.stats.data_ptr(), None]
    f = engine.MwNavParams(m.cell, 0.0, 0.0, m.gx, m.gz, engine.NAV_GRID, 0)
    from miniworld_amd.queries import NavField
    t = vec.grid_rollout(blocked, plans.to(torch.uint8), field=NavField(field, f, None, "grid"), extra=extra, pose=pose, step=step, radius=0.0, outside="open", stop_at=0, trace=True)
    args = lib.calls[-1][1]
    assert list(args[2]) == [0.0] and list(args[3:7]) == [engine.GPLAN_BYTE_PLANS, 6, 9, 0] and tuple(t.trace.shape) == (6, 5, 9, 3)
    assert ptr(args)[3:7] == [pose.data_ptr(), step.data_ptr(), field.data_ptr(), extra.data_ptr()] and ptr(args)[9] == t.trace.data_ptr()
    assert vec.grid_rollout(blocked, plans, field=field, like=m, trace=True, into=t) is t
    n0 = len(lib.calls)
    for kw in (dict(plans=plans.long()), dict(plans=plans[:, :4]), dict(plans=new(torch.int32, 257, 5, 9)), dict(plans=new(torch.int32, 6, 5, MAX_PLANS + 1)),
               dict(plans=new(torch.int32, 0, 5, 9)), dict(plans=plans.transpose(0, 2)), dict(field=field.short()), dict(field=field[:, :-1]), dict(pose=pose.float()),
               dict(step=step[:4]), dict(radius=-0.1), dict(radius=float("nan")), dict(radius=8.5 * m.cell), dict(outside="closed"), dict(stop_at=0),
               dict(field=field, stop_at=-1), dict(field=field, stop_at=0x10000), dict(trace=1), dict(into=t), dict(trace=True, into=r), dict(into={"pose": r.pose}),
               dict(field=NavField(field, f, None, "grid")), dict(extra=extra[:4])):
        with pytest.raises(ValueError):
            vec.grid_rollout(blocked, **{"plans": plans, "like": m, **kw})
    assert len(lib.calls) == n0         # nothing reached the library
