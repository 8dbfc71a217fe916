"""Grid navigation fields on the GPU (mw_nav_build_grid; MiniWorldVecEnv.grid_field), bit for bit — the fixed point is unique, so there
are no tolerances — against two yardsticks: the privileged field of mw_nav_build, whose occupancy and sources, handed back as grids, must
give the same field; and the restatement of tests/nav_grid_reference.py (numpy inflation, heapq Dijkstra with extra costs), which
itself asserts that no stencil distance lies within 1e-9 m of the inflation radius and that no cost reaches 0xFFFE.  Then the refusal
of costs that do not fit, nav_query on a grid field, and the two other users of a field."""
import numpy as np
import pytest

import nav_grid_reference as ref
import nav_reference
from query_checks import dev, host, teleport
from query_checks import vec_env as _vec

pytestmark = pytest.mark.gpu

CASES = [
    ("MiniWorld-MazeS2-v0", 67, 0.25, "walls"),             # per-env geometry: one full group of 64 envs and a partial one
    ("MiniWorld-FourRooms-v0", 5, 0.25, "walls"),
    ("MiniWorld-YMaze-v0", 3, 0.25, "walls"),
    ("MiniWorld-Sidewalk-v0", 2, 0.25, "walls"),            # the largest grid: 640 x 36 = 23 040 cells
    ("MiniWorld-Maze-v0", 3, 0.25, "walls"),                # 103 x 103: an env's rows start off a 4-byte boundary
    ("MiniWorld-Hallway-v0", 1, 1.0, "walls"),              # fewer cells than lanes
    ("MiniWorld-ThreeRooms-v0", 3, 0.25, "walls+entities"),
]


def _bits(t):
    """a uint16 tensor as int16, the same bits: the type every torch kernel knows"""
    return t.view(__import__("torch").int16)


def _privileged(vec, cell, obstacles):
    return vec.nav_field(target=0 if obstacles != "walls" else None, cell=cell, obstacles=obstacles)


@pytest.mark.parametrize("env_id,n,cell,obstacles", CASES)
def test_the_privileged_fields_own_grids_give_the_privileged_field(env_id, n, cell, obstacles):
    import torch
    vec = _vec(env_id, n)
    f = _privileged(vec, cell, obstacles)
    bits = _bits(f.field)
    blocked, sources = bits == -1, bits == 0
    assert bool(blocked.any()) and (cell >= 1.0 or bool(sources.any()))
    rounds = torch.zeros(n, dtype=torch.int32, device="cuda")
    vec.engine.debug_set_nav_passes(rounds)
    g = vec.grid_field(blocked, sources, inflate=0, like=f)
    vec.engine.debug_set_nav_passes(None)
    assert bool(((rounds >= 1) & (rounds <= f.gx * f.gz)).all())       # this build's rounds are recorded too
    assert g.obstacles == "grid" and (g.gx, g.gz, g.cell) == (f.gx, f.gz, f.cell) and g.field.data_ptr() != f.field.data_ptr()
    got, want = host(g.field), host(f.field)
    assert got.dtype == np.uint16 and np.array_equal(got, want), ("cells that differ", int((got != want).sum()))
    # ... and as bytes of any value != 0, by whole-grid passes
    g.params.flags |= 2
    vec.grid_field(blocked.to(torch.uint8) * 201, sources.to(torch.uint8) * 7, into=g)
    assert np.array_equal(host(g.field), want)
    vec.engine.check()
    vec.close()


def _random_grids(rng, n, gz, gx):
    """3 % raw obstacle cells, six sources per env, extra costs 0 .. 20"""
    raw = (rng.random((n, gz, gx)) < 0.03).astype(np.uint8)
    sources = np.zeros((n, gz, gx), np.uint8)
    for i in range(n):
        sources[i, rng.integers(0, gz, 6), rng.integers(0, gx, 6)] = 1
    return raw, sources, rng.integers(0, 21, (n, gz, gx)).astype(np.uint8)


@pytest.mark.parametrize("env_id,n,cell,obstacles", CASES)
def test_random_grids_equal_the_restatement(env_id, n, cell, obstacles):
    import torch
    vec = _vec(env_id, n)
    rng = np.random.default_rng(4700 + n)
    seen = vec.seen_map(cell=cell)
    gz, gx = seen.gz, seen.gx
    raw, sources, extra = _random_grids(rng, n, gz, gx)
    inflate = float(vec.engine.cfg.agent_radius) + cell / 2
    d_raw, d_src, d_extra = dev(raw), dev(sources), dev(extra)
    # the default clearance, without and with extra costs
    plain = vec.grid_field(d_raw, d_src, like=seen)
    assert plain.margin == inflate
    weighted = vec.grid_field(d_raw, d_src, extra=d_extra, like=seen)
    want_plain = np.stack([ref.field(raw[i], cell, inflate, sources[i]) for i in range(n)])
    want_weighted = np.stack([ref.field(raw[i], cell, inflate, sources[i], extra[i]) for i in range(n)])
    for got, want in ((host(plain.field), want_plain), (host(weighted.field), want_weighted)):
        assert np.array_equal(got, want), ("cells that differ", int((got != want).sum()))
    if gz * gx > 100:
        assert (want_plain == ref.BLOCKED).sum() > 2 * raw.sum() and (want_plain == 0).any() and not np.array_equal(want_plain, want_weighted)
    # whole-grid passes reach the same fixed points
    for fld, want in ((plain, want_plain), (weighted, want_weighted)):
        jac = vec.grid_field(d_raw, d_src, extra=d_extra if fld is weighted else None, like=seen)
        jac.params.flags |= 2
        _bits(jac.field).fill_(1234)
        vec.grid_field(d_raw, d_src, extra=d_extra if fld is weighted else None, into=jac)
        assert np.array_equal(host(jac.field), want)
    # a masked rebuild over other grids leaves the other rows' bits alone
    raw2, sources2, extra2 = _random_grids(rng, n, gz, gx)
    mask = torch.zeros(n, dtype=torch.bool, device="cuda")
    mask[::2] = True
    pattern = torch.arange(gz * gx * n, dtype=torch.int32, device="cuda").remainder(32000).to(torch.int16).reshape(n, gz, gx)
    _bits(weighted.field).copy_(pattern)
    assert vec.grid_field(dev(raw2), dev(sources2), extra=dev(extra2), mask=mask, into=weighted) is weighted
    got, pat = host(weighted.field), pattern.cpu().numpy().view(np.uint16)
    for i in range(n):
        assert np.array_equal(got[i], ref.field(raw2[i], cell, inflate, sources2[i], extra2[i]) if i % 2 == 0 else pat[i]), i
    vec.engine.check()
    vec.close()


def test_costs_that_do_not_fit_refuse_that_env_alone():
    """env 0: a free 640 x 36 grid, extra 100 everywhere, one corner source — the far corner would cost 67 165; env 1: a random grid"""
    import torch
    from miniworld_amd import engine
    vec = _vec("MiniWorld-Sidewalk-v0", 2)
    seen = vec.seen_map()
    gz, gx = seen.gz, seen.gx
    assert (gz, gx) == (640, 36)
    rng = np.random.default_rng(4800)
    raw, sources, extra = _random_grids(rng, 2, gz, gx)
    raw[0], sources[0], extra[0] = 0, 0, 100
    sources[0, 0, 0] = 1
    assert ref.costs(raw[0] != 0, sources[0], extra[0]) == (None, 67165)
    vec.engine.check()
    fld = vec.grid_field(dev(raw), dev(sources), extra=dev(extra), inflate=0, like=seen)
    with pytest.raises(engine.EngineError):
        vec.engine.check()
    got = host(fld.field)
    assert (got[0] == ref.BLOCKED).all()
    assert np.array_equal(got[1], ref.field(raw[1], 0.25, 0.0, sources[1], extra[1]))
    vec.engine.check()          # reported once
    # without the extra costs the same grids fit
    fld = vec.grid_field(dev(raw), dev(sources), inflate=0, like=seen)
    assert int(host(fld.field)[0].max()) == 35 * 7 + 604 * 5
    vec.engine.check()
    # what the library refuses before a launch
    e, p = vec.engine, fld.params
    bad = [engine.MwNavParams(0.25, 0.0, 0.0, gx, gz, engine.NAV_GRID | engine.NAV_ENTITIES, 0), engine.MwNavParams(0.25, 4.01, 0.0, gx, gz, engine.NAV_GRID, 0),
           engine.MwNavParams(0.25, -0.1, 0.0, gx, gz, 0, 0), engine.MwNavParams(0.25, float("nan"), 0.0, gx, gz, 0, 0), engine.MwNavParams(0.0, 0.0, 0.0, gx, gz, 0, 0)]
    for q in bad:
        with pytest.raises(engine.EngineError):
            e.nav_build_grid(q, fld.field, dev(raw), dev(sources))
    with pytest.raises(engine.EngineError):     # no source of either kind
        e.nav_build_grid(p, fld.field, dev(raw))
    with pytest.raises(engine.EngineError):     # point sources without a reach
        e.nav_build_grid(p, fld.field, dev(raw), target=torch.zeros((2, 3), dtype=torch.float64, device="cuda"))
    with pytest.raises(engine.EngineError):     # a grid of another size
        e.nav_build_grid(p, fld.field, dev(raw[:, :-1]), dev(sources))
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("env_id,n", [("MiniWorld-MazeS2-v0", 5), ("MiniWorld-YMaze-v0", 3)])
def test_nav_query_on_a_grid_field_and_point_sources(env_id, n):
    """cost, next and waypoint equal the restatement's query, the centre of the cell itself at cost 0: for the agents and for given
    positions — over the grid, in blocked cells, in source cells, in unreached cells and outside the extent.  The field here has extra costs, a source mask
    and point sources on the env's own origin."""
    import torch
    vec = _vec(env_id, n)
    cell, rng = 0.25, np.random.default_rng(4900 + n)
    ext = vec.engine.get_state()["extent"]
    seen = vec.seen_map()
    gz, gx = seen.gz, seen.gx
    raw, sources, extra = _random_grids(rng, n, gz, gx)
    # a closed ring of obstacles in the far corner, 7 x 7 cells, nothing inside: the cells in its middle stay unreached
    assert gz >= 24 and gx >= 24
    sources[:, gz - 9:gz - 2, gx - 9:gx - 2] = 0
    raw[:, gz - 9:gz - 2, gx - 9:gx - 2] = 1
    raw[:, gz - 8:gz - 3, gx - 8:gx - 3] = 0
    pts = np.array([[ext[i][0] + rng.uniform(0.3, 0.5) * gx * cell, 0.0, ext[i][2] + rng.uniform(0.3, 0.5) * gz * cell] for i in range(n)])
    inflate = 0.3
    fld = vec.grid_field(dev(raw), dev(sources), target=dev(pts), reach=0.6, extra=dev(extra), inflate=inflate, like=seen)
    assert fld.points is not None and fld.params.flags & 4
    want = [ref.field(raw[i], cell, inflate, sources[i], extra[i], point=pts[i], reach=0.6, origin=(ext[i][0], ext[i][2])) for i in range(n)]
    got = host(fld.field)
    for i in range(n):
        assert np.array_equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))
        assert want[i][gz - 6, gx - 6] == ref.UNREACHED
    alone = vec.grid_field(dev(raw), target=dev(pts), reach=0.6, inflate=inflate, like=seen)
    for i in range(n):
        assert np.array_equal(host(alone.field)[i], ref.field(raw[i], cell, inflate, point=pts[i], reach=0.6, origin=(ext[i][0], ext[i][2]))), i

    def check(pos, q):
        classes = set()
        c, nx, wp = q["cost"].cpu().numpy(), q["next"].cpu().numpy(), q["waypoint"].cpu().numpy()
        for i in range(n):
            a = ref.query(want[i], (ext[i][0], ext[i][2]), cell, float(pos[i][0]), float(pos[i][2]))
            assert (int(c[i]), int(nx[i]), float(wp[i][0]), float(wp[i][1])) == a, (i, pos[i], a)
            classes.add("none" if a[0] < 0 else "source" if a[0] == 0 else "way")
        return classes
    agents = vec.state(("agent_pos",))["agent_pos"].cpu().numpy()
    classes = check(agents, vec.nav_query(fld))
    for k in range(25):
        pos = np.zeros((n, 3))
        for i in range(n):
            f = want[i]
            kind = (k + i) % 5
            if kind == 4:       # outside the extent, on any side
                pos[i] = [ext[i][0] + rng.uniform(-1.0, 2.0) * gx * cell, 0.3, ext[i][2] + rng.uniform(-1.0, 2.0) * gz * cell]
                continue
            cls = (f == ref.BLOCKED, f == 0, f < ref.UNREACHED, f == ref.UNREACHED)[kind]
            js, is_ = np.nonzero(cls if cls.any() else f == f)
            pick = int(rng.integers(0, len(js)))
            pos[i] = [ext[i][0] + (is_[pick] + rng.uniform(0.02, 0.98)) * cell, rng.uniform(0, 1), ext[i][2] + (js[pick] + rng.uniform(0.02, 0.98)) * cell]
        classes |= check(pos, vec.nav_query(fld, pos=torch.from_numpy(pos).cuda()))
    assert classes == {"none", "source", "way"}
    # a privileged field's answers are what nav_reference's query gives, the target's own x, z at cost 0: the flag changes nothing there
    priv = vec.nav_field(target=dev(pts), reach=0.6)
    q = vec.nav_query(priv, pos=dev(pts))
    pf = host(priv.field)
    for i in range(n):
        a = nav_reference.query(pf[i], ext[i], cell, (pts[i][0], pts[i][2]), pts[i][0], pts[i][2])
        assert (int(q["cost"][i]), int(q["next"][i]), float(q["waypoint"][i][0]), float(q["waypoint"][i][1])) == a, (i, a)
    vec.engine.check()
    vec.close()


def test_an_ego_window_and_a_seen_map_take_a_grid_field():
    import torch
    import torch.nn.functional as F
    n, size, cell = 5, 9, 0.25
    vec = _vec("MiniWorld-FourRooms-v0", n)
    rng = np.random.default_rng(5000)
    ext = vec.engine.get_state()["extent"]
    seen = vec.seen_map()
    gz, gx = seen.gz, seen.gx
    raw, sources, extra = _random_grids(rng, n, gz, gx)
    fld = vec.grid_field(dev(raw), dev(sources), extra=dev(extra), like=seen)
    # seen_map(like=) adopts its grid
    m = vec.seen_map(like=fld)
    assert (m.gx, m.gz, m.cell) == (gx, gz, cell) and tuple(m.seen.shape) == (n, gz, gx)
    vec.seen_update(m)
    # a north window with the agent on a cell's centre is the plain crop of the field, 0xFFFF beyond it
    i0, j0 = np.array([2, gx - 2, gx // 2 + 3, 5, gx - 3]), np.array([3, gz - 3, gz // 2 - 5, gz - 2, 2])
    teleport(vec, ([ext[i][0] + (i0[i] + 0.5) * cell for i in range(n)], [ext[i][2] + (j0[i] + 0.5) * cell for i in range(n)]), 1.3)
    w = vec.ego_window(size=size, cell=cell, frame="north", planes=())
    _, sample = vec.ego_update(w, source=fld)
    sample = _bits(sample).to(torch.int32) & 0xFFFF
    padded = F.pad(_bits(fld.field).to(torch.int32) & 0xFFFF, (size, size, size, size), value=0xFFFF)
    for i in range(n):
        fi, fj = int(i0[i]) - size // 2 + size, int(j0[i]) - size // 2 + size
        assert torch.equal(sample[i], padded[i, fj:fj + size, fi:fi + size]), i
    assert int((sample == 0xFFFF).sum()) > 0 and int((sample < 0xFFFE).sum()) > 0
    vec.engine.check()
    vec.close()
