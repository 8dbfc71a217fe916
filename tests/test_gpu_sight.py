"""Grid sight on the GPU (mw_grid_sight; MiniWorldVecEnv.grid_sight), bit for bit — gains are integer sums and the seen plane gets
same-value stores, so there are no tolerances — against the restatement of tests/sight_reference.py, which has no walk; then against the
engine's own ray casts, with no Python between the two kernels: on the blocked cells of a privileged nav field a cell the grid sight
sees is one the ray from the agent reaches, without exception.  Then the consistency of gain and seen, and the refusals."""
import math

import numpy as np
import pytest

import sight_reference as ref
from query_checks import dev, host, poses, teleport
from query_checks import vec_env as _vec

pytestmark = pytest.mark.gpu

# (env, envs, gz, gx): fewer cells than three rounds of lanes; a square grid; odd rows, so that an env's rows start off a 4-byte boundary
CASES = [("MiniWorld-Hallway-v0", 5, 16, 48), ("MiniWorld-MazeS3-v0", 4, 38, 38), ("MiniWorld-Maze-v0", 4, 103, 103)]
CELL = 0.25


def _opaque(rng, n, gz, gx):
    """random bytes 1 .. 255, on 3 % of the cells of the even envs and 15 % of the odd ones"""
    dens = np.where(np.arange(n) % 2 == 0, 0.03, 0.15)[:, None, None]
    return (rng.random((n, gz, gx)) < dens).astype(np.uint8) * rng.integers(1, 256, (n, gz, gx)).astype(np.uint8)


def _cells(rng, opaque, views):
    """int32[n, views]: random cells, and in every row that has room a corner, an opaque cell, -1 and a cell past the grid"""
    n, gz, gx = opaque.shape
    cells = rng.integers(0, gz * gx, (n, views)).astype(np.int32)
    for i in range(n):
        oj, oi = np.nonzero(opaque[i])
        k = int(rng.integers(0, len(oj)))
        special = [int(oj[k]) * gx + int(oi[k]), (0, gx - 1, (gz - 1) * gx, gz * gx - 1)[i % 4], -1, gz * gx]
        if views == 1:
            special = special[i % 4:i % 4 + 1] if i else []
        slots = rng.permutation(views)[:min(views, len(special))]
        cells[i, slots] = special[:len(slots)]
    return cells


@pytest.mark.parametrize("views", [1, 3, 65])
@pytest.mark.parametrize("env_id,n,gz,gx", CASES)
def test_the_kernel_equals_the_restatement(env_id, n, gz, gx, views):
    """65 viewpoints are more than a wavefront's worth of tasks per workgroup, a range of one cell a box of fewer targets than a
    wavefront has lanes, the whole-grid range the longest walks (with 1 and 3 viewpoints: the restatement is quadratic there).  Env 1
    is masked off: its gains and its seen row keep their bits.  The seen plane starts as a pattern of 0 and 7."""
    import torch
    vec = _vec(env_id, n)
    m = vec.seen_map(cell=CELL)
    assert (m.gz, m.gx) == (gz, gx)
    rng = np.random.default_rng(5400 + gz + views)
    opaque = _opaque(rng, n, gz, gx)
    weight = rng.integers(0, 256, (n, gz, gx)).astype(np.uint8)
    mask = np.ones(n, np.uint8)
    mask[1] = 0
    whole = math.hypot(gz, gx) * CELL + 1.0
    d_opaque, d_weight, d_mask = dev(opaque), dev(weight), dev(mask)
    combos = [(3.0, -1.0, True, False), (CELL, math.cos(math.radians(30.0)), False, True), (whole if views <= 3 else 3.0, 0.0, True, True),
              (3.0, 1.0, False, True), (3.0, -1.0, False, True)]
    for max_range, cos_half, weighted, with_dirs in combos:
        cells = _cells(rng, opaque, views)
        dirs = rng.uniform(-7.0, 7.0, (n, views)) if with_dirs else None
        if dirs is not None and views > 1:
            dirs[0, 1] = math.nan
        pattern = (rng.random((n, gz, gx)) < 0.1).astype(np.uint8) * 7
        seen, gain = dev(pattern), torch.full((n, views), -77, dtype=torch.int32, device="cuda")
        vec.engine.grid_sight(m.params, max_range, cos_half, views, d_opaque, gain, d_weight if weighted else None, dev(cells), dev(dirs), seen, d_mask)
        got_gain, got_seen = host(gain), host(seen)
        for i in range(n):
            if not mask[i]:
                assert (got_gain[i] == -77).all() and np.array_equal(got_seen[i], pattern[i]), i
                continue
            want_gain, want_seen = ref.sight(opaque[i], CELL, cells[i], None if dirs is None else dirs[i], max_range, cos_half,
                                             weight[i] if weighted else None, pattern[i])
            assert np.array_equal(got_gain[i], want_gain), (i, max_range, cos_half, got_gain[i][:6], want_gain[:6])
            assert np.array_equal(got_seen[i], want_seen), (i, max_range, cos_half, int((got_seen[i] != want_seen).sum()))
        assert (got_seen == 1).any() and (got_seen == 7).any() and (got_gain[mask != 0] > 0).any()
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("env_id,n", [("MiniWorld-FourRooms-v0", 6), ("MiniWorld-Maze-v0", 3)])
def test_the_agents_own_cell_and_cone(env_id, n):
    """cells=None after a few steps: the viewpoint is the cell of vec.state()'s pose on the env's grid and the cone the agent's"""
    import torch
    vec = _vec(env_id, n)
    rng = np.random.default_rng(5500 + n)
    for _ in range(6):
        vec.step(torch.as_tensor(rng.integers(0, 3, n), dtype=torch.int32, device="cuda"))
    m = vec.seen_map(cell=CELL)
    gz, gx = m.gz, m.gx
    opaque = _opaque(rng, n, gz, gx)
    weight = rng.integers(0, 256, (n, gz, gx)).astype(np.uint8)
    ext = vec.engine.get_state()["extent"]
    ps = poses(vec)
    for fov in (None, 2 * math.pi, 1.0):
        seen = torch.zeros((n, gz, gx), dtype=torch.uint8, device="cuda")
        gain = vec.grid_sight(dev(opaque), weight=dev(weight), max_range=3.0, fov=fov, like=m, seen=seen)
        assert tuple(gain.shape) == (n, 1) and gain.dtype == torch.int32
        cos_half = -1.0 if fov == 2 * math.pi else math.cos((vec.default_fov() if fov is None else fov) / 2)
        for i in range(n):
            c = ref.agent_cell(ps[i], ext[i], CELL, gx, gz)
            want_gain, want_seen = ref.sight(opaque[i], CELL, [c], [ps[i][2]], 3.0, cos_half, weight[i])
            assert np.array_equal(host(gain)[i], want_gain) and np.array_equal(host(seen)[i], want_seen), (i, fov)
            assert want_seen[c // gx, c % gx] == 1
    # a NaN pose is no viewpoint
    teleport(vec, ([math.nan] + [p[0] for p in ps[1:]], [p[1] for p in ps]))
    seen = torch.zeros((n, gz, gx), dtype=torch.uint8, device="cuda")
    gain = host(vec.grid_sight(dev(opaque), like=m, seen=seen))
    assert gain[0, 0] == 0 and not host(seen)[0].any() and (gain[1:, 0] > 0).all()
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("env_id", ["MiniWorld-FourRooms-v0", "MiniWorld-MazeS3-v0", "MiniWorld-Hallway-v0"])
def test_what_the_grid_sight_sees_the_ray_casts_reach(env_id):
    """opaque = the blocked cells of a privileged nav field at the default margin; each agent on the centre of an unblocked cell; all
    round at 4 m.  Every seen cell that is not opaque is reached by the engine's own ray from the agent to its centre (t == 1, hit ==
    -1): 0 exceptions.  A blocked cell's centre is within agent_radius + margin of a wall and a cell reaches only 0.18 m from its
    centre, so every cell a wall touches is opaque, and the closed test blocks every line through one.  Reported, not asserted: the
    share of the truly visible unblocked cells within 4 m that the grid sight sees."""
    import torch
    n, max_range = 12, 4.0
    vec = _vec(env_id, n, seed=1)
    st = vec.state(("agent_pos",))["agent_pos"]
    field = vec.nav_field(target=st.clone().contiguous(), reach=0.5)
    gz, gx = field.gz, field.gx
    assert gz * gx <= 4096          # (a ray per cell)
    opaque = (field.field.view(torch.int16) == -1)
    ext = vec.engine.get_state()["extent"]
    rng = np.random.default_rng(5600)
    free = ~host(opaque)
    x, z = np.zeros(n), np.zeros(n)
    for i in range(n):
        js, is_ = np.nonzero(free[i])
        k = int(rng.integers(0, len(js)))
        x[i], z[i] = ext[i][0] + (is_[k] + 0.5) * CELL, ext[i][2] + (js[k] + 0.5) * CELL
    teleport(vec, (x, z))
    seen = torch.zeros((n, gz, gx), dtype=torch.uint8, device="cuda")
    gain = vec.grid_sight(opaque, max_range=max_range, fov=2 * math.pi, like=field, seen=seen)
    # the ray from each agent to every cell's centre, on the device
    e = torch.as_tensor(np.asarray(ext), dtype=torch.float64, device="cuda")
    cx = e[:, 0:1] + (torch.arange(gx, dtype=torch.float64, device="cuda") + 0.5)[None, :] * CELL
    cz = e[:, 2:3] + (torch.arange(gz, dtype=torch.float64, device="cuda") + 0.5)[None, :] * CELL
    pos = vec.state(("agent_pos",))["agent_pos"]
    d = torch.stack([(cx[:, None, :] - pos[:, 0, None, None]).expand(n, gz, gx), (cz[:, :, None] - pos[:, 2, None, None]).expand(n, gz, gx)], dim=-1)
    cast = vec.raycast(direction=d.reshape(n, gz * gx, 2).contiguous())
    reached = ((cast["t"] == 1.0) & (cast["hit"] == -1)).reshape(n, gz, gx)
    claimed = (seen != 0) & ~opaque
    exceptions = int((claimed & ~reached).sum())
    dist = torch.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)
    truly = reached & ~opaque & (dist <= max_range)
    share = float((truly & (seen != 0)).sum()) / max(1, int(truly.sum()))
    print(f"{env_id}: {int(claimed.sum())} seen unblocked cells, {exceptions} exceptions; share of the truly visible seen {share:.3f}")
    assert int(claimed.sum()) > 40 * n and bool((gain[:, 0] > 0).all())
    assert exceptions == 0
    vec.engine.check()
    vec.close()


def test_gain_is_the_weight_of_the_seen_cells():
    """one viewpoint on a zeroed seen plane: gain == (weight * seen).sum(), and seen.sum() without weights — on the device"""
    import torch
    n = 7
    vec = _vec("MiniWorld-MazeS3-v0", n)
    m = vec.seen_map(cell=CELL)
    rng = np.random.default_rng(5700)
    opaque, weight = dev(_opaque(rng, n, m.gz, m.gx)), dev(rng.integers(0, 256, (n, m.gz, m.gx)).astype(np.uint8))
    cells = dev(rng.integers(0, m.gz * m.gx, (n, 1)).astype(np.int32))
    dirs = dev(rng.uniform(-3.0, 3.0, (n, 1)))
    for kw in (dict(), dict(dirs=dirs, fov=1.5), dict(max_range=0.6), dict(max_range=50.0)):
        for w in (weight, None):
            seen = torch.zeros((n, m.gz, m.gx), dtype=torch.uint8, device="cuda")
            gain = vec.grid_sight(opaque, cells, weight=w, like=m, seen=seen, **kw)
            assert int(seen.max()) == 1
            total = (seen.to(torch.int32) * (w.to(torch.int32) if w is not None else 1)).sum(dim=(1, 2))
            assert torch.equal(gain[:, 0], total.to(torch.int32)), kw
    # many viewpoints: the seen plane is the union, every gain at most the whole plane's weight
    cells = dev(rng.integers(0, m.gz * m.gx, (n, 16)).astype(np.int32))
    seen = torch.zeros((n, m.gz, m.gx), dtype=torch.bool, device="cuda")
    gain = vec.grid_sight(opaque, cells, weight=weight, like=m, seen=seen)
    total = (seen.to(torch.int32) * weight.to(torch.int32)).sum(dim=(1, 2))
    assert bool((gain.max(dim=1).values <= total).all()) and bool((gain.sum(dim=1) >= total).all())
    # and without a seen plane the gains are the same
    assert torch.equal(vec.grid_sight(opaque, cells, weight=weight, like=m), gain)
    vec.engine.check()
    vec.close()


def test_refusals_launch_nothing():
    import torch
    from miniworld_amd import engine
    n = 3
    vec = _vec("MiniWorld-Hallway-v0", n)
    m = vec.seen_map(cell=CELL)
    gz, gx, e, p = m.gz, m.gx, vec.engine, m.params
    opaque = torch.zeros((n, gz, gx), dtype=torch.uint8, device="cuda")
    seen = torch.full((n, gz, gx), 5, dtype=torch.uint8, device="cuda")
    cells = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    dirs = torch.zeros((n, 2), dtype=torch.float64, device="cuda")

    def fresh(v):
        return torch.full((n, v), -77, dtype=torch.int32, device="cuda")
    too_many = engine.SIGHT_MAX_VIEWS + 1
    calls = [
        lambda g: e.grid_sight(p, 0.0, -1.0, 2, opaque, g, cells=cells, seen=seen),
        lambda g: e.grid_sight(p, float("inf"), -1.0, 2, opaque, g, cells=cells, seen=seen),
        lambda g: e.grid_sight(p, float("nan"), -1.0, 2, opaque, g, cells=cells, seen=seen),
        lambda g: e.grid_sight(p, 3.0, 1.5, 2, opaque, g, cells=cells, dirs=dirs, seen=seen),
        lambda g: e.grid_sight(p, 3.0, float("nan"), 2, opaque, g, cells=cells, dirs=dirs, seen=seen),
        lambda g: e.grid_sight(p, 3.0, 0.5, 2, opaque, g, cells=cells, seen=seen),                      # a cone without headings
        lambda g: e.grid_sight(engine.MwNavParams(0.0, 0.0, 0.0, gx, gz, 0, 0), 3.0, -1.0, 2, opaque, g, cells=cells, seen=seen),
        lambda g: e.grid_sight(engine.MwNavParams(0.25, 0.0, 0.0, gx, gz + 1, 0, 0), 3.0, -1.0, 2, opaque, g, cells=cells, seen=seen),   # other tensors' shape
    ]
    for call in calls:
        g = fresh(2)
        with pytest.raises(engine.EngineError):
            call(g)
        assert bool((g == -77).all()) and bool((seen == 5).all())
    # the agent is one viewpoint and its heading its own; the viewpoints are 1 .. SIGHT_MAX_VIEWS
    g = fresh(2)
    with pytest.raises(engine.EngineError):
        e.grid_sight(p, 3.0, -1.0, 2, opaque, g, seen=seen)
    with pytest.raises(engine.EngineError):
        e.grid_sight(p, 3.0, 0.5, 1, opaque, fresh(1), dirs=torch.zeros((n, 1), dtype=torch.float64, device="cuda"), seen=seen)
    with pytest.raises(engine.EngineError):
        e.grid_sight(p, 3.0, -1.0, too_many, opaque, fresh(too_many), cells=torch.zeros((n, too_many), dtype=torch.int32, device="cuda"), seen=seen)
    with pytest.raises(engine.EngineError):
        e.grid_sight(p, 3.0, -1.0, 0, opaque, torch.zeros((n, 0), dtype=torch.int32, device="cuda"), cells=torch.zeros((n, 0), dtype=torch.int32, device="cuda"))
    assert bool((g == -77).all()) and bool((seen == 5).all())
    # ... and the largest count is served
    most = engine.SIGHT_MAX_VIEWS
    g = fresh(most)
    e.grid_sight(p, 3.0, -1.0, most, opaque, g, cells=torch.arange(n * most, dtype=torch.int32, device="cuda").reshape(n, most).remainder(gz * gx).contiguous())
    assert bool((g > 0).all())
    e.check()
    vec.close()
