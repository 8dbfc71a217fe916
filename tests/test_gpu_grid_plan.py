"""Grid rollouts on the GPU (mw_grid_plan; vec.grid_rollout), bit for bit: against tests/grid_plan_reference.py on synthetic maps, both
plan dtypes and a mask; against the engine's own rollout trace where nothing is in the way; and a wall of the map by hand."""
import math

import numpy as np
import pytest

import grid_plan_reference as ref
import scan_reference as scan
from query_checks import dev, host, poses, teleport, worlds
from query_checks import vec_env as _vec

pytestmark, N = pytest.mark.gpu, len(ref.POSES)
_extents = lambda vec: [[float(v) for v in w["extent"]] for w in worlds(vec)]      # noqa: E731
_u64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)               # noqa: E731


def _grid(gz, gx, cell=0.25):
    from miniworld_amd import engine
    from miniworld_amd.queries import ScanMap
    return ScanMap(None, None, None, engine.MwNavParams(cell, 0.0, 0.0, gx, gz, 0, 0), 1, 1.0, 20.0, "walls")


@pytest.mark.parametrize("gz,gx,P,T", [g + (p, t) for g in scan.GRIDS for p in (1, 65, 257) for t in (1, 7, 64)] + [(128, 256, 4096, 8)])
def test_the_kernel_equals_the_restatement(gz, gx, P, T):
    """an env per start pose on a grid of its own over the Hallway's extent, each on a map of another density; radius, `outside`, field,
    extra, stop_at and the step override turn with the case.  int32 plans with a trace, then uint8 plans without one: pose, stats and
    trace are the restatement's bits.  Then other maps into the same results under a zero mask byte on envs 2, 3: their rows stay.
    103 x 103 is odd: the planes of the odd envs start off a 4-byte boundary; 257 plans are one into a second workgroup of the env."""
    import torch
    vec = _vec("MiniWorld-Hallway-v0", N)
    ext, cell, turn = _extents(vec), 0.25, gz + P + T
    while any((gx + 0.5) * cell <= e[1] - e[0] or (gz + 0.5) * cell <= e[3] - e[2] for e in ext):
        cell *= 2
    rng, grid = np.random.default_rng(5400 + turn), _grid(gz, gx, cell)
    radius, outside = ref.RADII[turn % 4] * cell, ("open", "blocked")[(turn // 2) % 2]
    use_field, use_extra, step = turn % 3 != 0, (turn // 2) % 2 == 1, (np.tile((0.2 * cell / 0.25, 0.03, 22.5), (N, 1)) if turn % 2 else None)
    stop_at = (None, 0, 25)[turn % 3] if use_field else None
    default = [float(getattr(vec.engine.cfg, k).default) for k in ("forward_step", "forward_drift", "turn_step")]
    pose = np.array([ref.pose_of(name, rng, gx, gz, (ext[i][0], ext[i][2]), cell) for i, name in enumerate(ref.POSES)])
    plans = np.stack([ref.plans_of(rng, T, P) for _ in range(N)], 1)
    mask, want, a, b = np.array([1, 1, 0, 0] + [1] * (N - 4), np.uint8), [None] * N, None, None
    for call in range(2):
        planes = [ref.planes_of(rng, gz, gx, ref.DENSITIES[(i + call + turn) % 4]) for i in range(N)]
        opaque, field, extra = (np.stack([p[k] for p in planes]) for k in range(3))
        for i in range(N):
            if call == 0 or mask[i]:
                want[i] = ref.rollout(plans[:, i], pose[i], step[i] if step is not None else default, radius, outside == "blocked", -1 if stop_at is None else stop_at,
                                      (ext[i][0], ext[i][2]), cell, opaque[i], field[i] if use_field else None, extra[i] if use_extra else None)
        kw = dict(field=dev(field.view(np.int16)).view(torch.uint16) if use_field else None, extra=dev(extra) if use_extra else None, pose=dev(pose), step=dev(step),
                  radius=radius, outside=outside, stop_at=stop_at, like=grid, mask=dev(mask) if call else None)
        a = vec.grid_rollout(dev(opaque), dev(plans), trace=True, into=a, **kw)
        b = vec.grid_rollout(dev(opaque), dev(plans.astype(np.uint8)), into=b, **kw)
        for r in (a, b):
            got_pose, got_stats = host(r.pose), host(r.stats)
            for i in range(N):
                assert np.array_equal(_u64(got_pose[i]), _u64(want[i][0])) and np.array_equal(got_stats[i], want[i][1]), (call, ref.POSES[i], r is b)
        trace = host(a.trace)
        assert all(np.array_equal(_u64(trace[:, i]), _u64(want[i][2])) for i in range(N)), call
    assert P * T < 400 or sum(int(w[1][:, 3].sum()) for w in want) > 0
    vec.engine.check()
    vec.close()


def test_free_space_is_the_engines_own_step():
    """OneRoom x 8, agents at the room's centre at eight headings, the box in a corner; 12 random actions 0 .. 3 on an empty plane with
    the outside open.  No wall or entity lies within reach of the start, so the engine refuses nothing — asserted from the geometry
    first — and the grid rollout's trace is, bit for bit, the engine's own"""
    import torch
    vec, T = _vec("MiniWorld-OneRoom-v0", 8), 12
    ext = np.array(_extents(vec))
    centre = ((ext[:, 0] + ext[:, 1]) / 2, (ext[:, 2] + ext[:, 3]) / 2)
    teleport(vec, centre)
    st = vec.state(("ent_pos",))
    ent_pos = st["ent_pos"].clone()
    ent_pos[:, :, 0], ent_pos[:, :, 2] = dev(ext[:, 0] + 0.8)[:, None], dev(ext[:, 2] + 0.8)[:, None]
    ones = torch.ones(8, dtype=torch.uint8, device="cuda")
    vec.set_state_where(ones, ent_pos=ent_pos, agent_dir=dev(np.arange(8) * (math.pi / 4) + 0.1))
    cfg = vec.engine.cfg
    reach = T * float(cfg.forward_step.default) + float(cfg.agent_radius)
    assert not cfg.domain_rand and float(cfg.forward_drift.default) == 0.0
    for i, w in enumerate(worlds(vec)):
        x, z = centre[0][i], centre[1][i]
        for ax, az, bx, bz in w["segs"]:
            t = min(1.0, max(0.0, ((x - ax) * (bx - ax) + (z - az) * (bz - az)) / ((bx - ax) ** 2 + (bz - az) ** 2)))
            assert math.hypot(ax + t * (bx - ax) - x, az + t * (bz - az) - z) > reach
        for s in range(len(w["kind"])):
            assert w["kind"][s] == 0 or math.hypot(w["pos"][s][0] - x, w["pos"][s][2] - z) > reach + float(w["radius"][s])
    plans = torch.as_tensor(np.random.default_rng(5500).integers(0, 4, (T, 8)), dtype=torch.int32, device="cuda")
    m = vec.scan_map()
    r = vec.grid_rollout(torch.zeros((8, m.gz, m.gx), dtype=torch.uint8, device="cuda"), plans[:, :, None].contiguous(), trace=True, outside="open", like=m)
    vec.rollout(plans, render=False, trace=("agent_pos", "agent_dir"))
    assert torch.equal(r.trace[:, :, 0, 0], vec.trace["agent_pos"][..., 0]) and torch.equal(r.trace[:, :, 0, 1], vec.trace["agent_pos"][..., 2])
    assert torch.equal(r.trace[:, :, 0, 2], vec.trace["agent_dir"]) and int(r.bumps.sum()) == 0 and bool((r.steps == T).all())
    assert float((r.trace[-1, :, 0, :2] - r.trace[0, :, 0, :2]).abs().max()) > 0.3          # (they did move)
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("radius", [0.4, 0.0])
def test_a_wall_of_the_map_stops_what_it_should(radius):
    """a full row of opaque cells ahead of the agent, T forward moves along +z: the final pose is the last one whose disc clears the row
    by the rule, bumps is the rest; with radius 0 it ends in the last free cell; a field that is 0 beyond the row is never reached.  A
    grid that covers no env: the defined rows and the status bit"""
    import pyoracle
    import torch
    from miniworld_amd import engine
    vec, T, row = _vec("MiniWorld-Hallway-v0", 2), 24, 9
    m, ext = vec.scan_map(), _extents(vec)
    assert m.gz > row + 2
    opaque, field = np.zeros((2, m.gz, m.gx), np.uint8), np.full((2, m.gz, m.gx), 100, np.uint16)
    opaque[:, row], field[:, row + 1:] = 1, 0
    fwd, heading = float(vec.engine.cfg.forward_step.default), -math.pi / 2
    pose = np.array([(e[0] + 2.125 * m.cell, e[2] + 4.5 * m.cell, heading) for e in ext])
    r = vec.grid_rollout(dev(opaque), torch.full((T, 2, 1), 2, dtype=torch.int32, device="cuda"), field=dev(field.view(np.int16)).view(torch.uint16), pose=dev(pose),
                         radius=radius, like=m)
    s, c = pyoracle.sincos(heading)
    for i in range(2):
        x, z, moves, rc = pose[i][0], pose[i][1], 0, radius / m.cell
        for _ in range(T):
            nx, nz = x + c * fwd + s * 0.0, z + (-s) * fwd + c * 0.0
            w = (nz - ext[i][2]) / m.cell
            if math.floor(w) == row or (math.floor(w + rc) >= row and max(row - w, 0.0) ** 2 < rc * rc):
                break
            x, z, moves = nx, nz, moves + 1
        assert 0 < moves < T and host(r.pose)[i, 0].tolist() == [x, z, heading] and host(r.stats)[i, 0].tolist() == [100, 0, T, T - moves, 0]
        assert radius or math.floor((z - ext[i][2]) / m.cell) == row - 1
    vec.engine.check()
    small = vec.grid_rollout(torch.ones((2, 3, 3), dtype=torch.uint8, device="cuda"), torch.full((T, 2, 1), 2, dtype=torch.int32, device="cuda"), pose=dev(pose), trace=True,
                             like=_grid(3, 3))
    assert host(small.stats).tolist() == [[[0xFFFF, 0, 0, 0, 0]]] * 2 and np.array_equal(host(small.pose)[:, 0], pose) and np.array_equal(host(small.trace)[5, :, 0], pose)
    with pytest.raises(engine.EngineError, match="refused an env"):
        vec.engine.check()
    vec.close()
