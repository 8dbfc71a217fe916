"""Grid regions on the GPU (mw_grid_regions; MiniWorldVecEnv.grid_regions), bit for bit — every output is an integer the rule defines, so
there are no tolerances — against the restatement of tests/regions_reference.py, a flood fill; then against kernels already here, with
no Python arithmetic between the two: what a nav field reaches is a 4-connected region, a grid field from a region's representative
reaches exactly that region, and grid_sight takes a row of representatives as it stands.  Then `into=` and the refusals."""
import numpy as np
import pytest

import regions_reference as ref
from query_checks import dev, host
from query_checks import vec_env as _vec

pytestmark = pytest.mark.gpu

SENTINEL = -77


def _params(gz, gx):
    from miniworld_amd import engine
    return engine.MwNavParams(0.25, 0.0, 0.0, gx, gz, 0, 0)


def _outputs(n, gz, gx, K):
    """count, size, cell, sum, label, prefilled with the sentinel"""
    import torch
    new = lambda shape, dtype: torch.full(shape, SENTINEL, dtype=dtype, device="cuda")
    return new((n,), torch.int32), new((n, K), torch.int32), new((n, K), torch.int32), new((n, K, 2), torch.int32), new((n, gz, gx), torch.int16)


def _compare(got, member, mask, conn, min_cells, K, comps=None):
    """every env's rows of `got` (host arrays) against the restatement; a masked-off env keeps the sentinel everywhere"""
    count, size, cell, total, label = got
    for i in range(member.shape[0]):
        if not mask[i]:
            assert count[i] == SENTINEL and all((a[i] == SENTINEL).all() for a in (size, cell, total, label) if a is not None), i
            continue
        want = ref.regions(member[i], conn, min_cells, K, None if comps is None else comps[i])
        assert count[i] == want[0], (i, conn, min_cells, K, count[i], want[0])
        assert np.array_equal(size[i], want[1]), (i, conn, min_cells, K, size[i][:8], want[1][:8])
        assert np.array_equal(cell[i], want[2]), (i, conn, min_cells, K, cell[i][:8], want[2][:8])
        assert total is None or np.array_equal(total[i], want[3]), (i, conn, min_cells, K)
        assert label is None or np.array_equal(label[i], want[4]), (i, conn, min_cells, K, int((label[i] != want[4]).sum()))


@pytest.mark.parametrize("gz,gx", [(103, 103), (128, 256), (4, 12)])
def test_the_kernel_equals_the_restatement(gz, gx):
    """Three envs, three grids of one shape at densities 0.3, 0.5 and 0.6; env 1 is masked off and keeps the sentinel in every output.
    103 x 103 is odd: the rows of envs 1 and 2 start off a 4-byte boundary.  K = 256 and K = 1, both connectivities, min_cells 1 and 3,
    with and without the optional outputs."""
    vec = _vec("MiniWorld-Hallway-v0", 3)
    rng = np.random.default_rng(6200 + gz)
    dens = np.array([0.3, 0.5, 0.6])[:, None, None]
    member = (rng.random((3, gz, gx)) < dens).astype(np.uint8) * rng.integers(1, 256, (3, gz, gx)).astype(np.uint8)
    mask = np.array([1, 0, 1], np.uint8)
    d_member, d_mask = dev(member), dev(mask)
    comps = {c: [ref.components(member[i], c) if mask[i] else None for i in range(3)] for c in (4, 8)}
    cut = False
    for conn, min_cells, K, optional in ((4, 1, 256, True), (8, 3, 256, True), (4, 3, 1, True), (8, 1, 1, False), (4, 1, 256, False)):
        count, size, cell, total, label = _outputs(3, gz, gx, K)
        vec.engine.grid_regions(_params(gz, gx), conn, min_cells, K, d_member, count, size, cell, total if optional else None, label if optional else None, d_mask)
        got = (host(count), host(size), host(cell), host(total), host(label))
        if not optional:
            assert (got[3] == SENTINEL).all() and (got[4] == SENTINEL).all()
            got = got[:3] + (None, None)
        _compare(got, member, mask, conn, min_cells, K, comps[conn])
        cut |= bool((got[0][mask != 0] > K).any())
    assert cut
    vec.engine.check()
    vec.close()


def test_the_long_regions_settle():
    """128 x 256, the cell limit: a serpentine corridor, a square spiral, a one-cell staircase and a checkerboard, an env each — the
    inputs that take a labelling the most rounds; both connectivities (the checkerboard: 16384
    regions of one cell, 256 listed, against one region)"""
    gz, gx, K = 128, 256, 256
    vec = _vec("MiniWorld-Hallway-v0", 4)
    member = np.stack([ref.serpentine(gz, gx), ref.spiral(gz, gx), ref.staircase(gz, gx), ref.checkerboard(gz, gx)])
    d_member = dev(member)
    for conn in (4, 8):
        count, size, cell, total, label = _outputs(4, gz, gx, K)
        vec.engine.grid_regions(_params(gz, gx), conn, 1, K, d_member, count, size, cell, total, label)
        got = (host(count), host(size), host(cell), host(total), host(label))
        _compare(got, member, np.ones(4, np.uint8), conn, 1, K)
        assert got[0].tolist() == [1, 1, 1, 16384 if conn == 4 else 1]
        assert (got[4][3] == -1).sum() == (16384 - 256 if conn == 4 else 0)
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("env_id", ["MiniWorld-FourRooms-v0", "MiniWorld-MazeS3-v0", "MiniWorld-Hallway-v0"])
def test_what_a_nav_field_reaches_is_a_region(env_id):
    """the privileged nav field f of 16 envs: a field's moves never cut a corner, so the cells it reaches (f < 0xFFFE) are exactly the
    4-connected regions of the unblocked cells (f != 0xFFFF) that hold a source cell (f == 0) — two kernels, compared on the device"""
    import torch
    n, K = 16, 256
    vec = _vec(env_id, n, seed=2)
    f = vec.nav_field()
    cost = f.field.view(torch.int16).to(torch.int32) & 0xFFFF
    r = vec.grid_regions(cost != 0xFFFF, connectivity=4, max_regions=K, like=f, labels=True)
    assert bool((r.count >= 1).all()) and bool((r.count <= K).all())
    src = cost == 0
    assert bool(src.flatten(1).any(dim=1).all()) and bool((r.label[src] > 0).all())
    # has[env][k + 1]: the k-th listed region holds a source cell
    has = torch.zeros((n, K + 1), dtype=torch.bool, device="cuda")
    has.scatter_(1, (r.label.to(torch.int64) * src).flatten(1), True)
    reached = has.gather(1, r.label.clamp(min=0).to(torch.int64).flatten(1)).view_as(r.label) & (r.label > 0)
    assert torch.equal(reached, cost < 0xFFFE), int((reached != (cost < 0xFFFE)).sum())
    assert int(reached.sum()) > 20 * n
    vec.engine.check()
    vec.close()


def test_a_grid_field_from_a_representative_reaches_its_region():
    """random 64 x 64 grids, 40 % blocked, seeds 0 .. 2 as three envs: grid_field(blocked, sources = one-hot of regions.cell[:, k],
    inflate=0) reaches exactly the cells with label == k + 1, for the first, the second and the largest listed region of every env"""
    import torch
    from miniworld_amd.queries import NavField
    gz = gx = 64
    vec = _vec("MiniWorld-Hallway-v0", 3)
    like = NavField(None, _params(gz, gx), None, "grid")
    blocked = dev(np.stack([np.random.default_rng(s).random((gz, gx)) < 0.4 for s in range(3)]))
    r = vec.grid_regions(~blocked, connectivity=4, max_regions=256, like=like, labels=True)
    assert bool((r.count >= 3).all())
    for k in (torch.zeros(3, dtype=torch.int64, device="cuda"), torch.ones(3, dtype=torch.int64, device="cuda"), r.size.argmax(dim=1)):
        cell = r.cell.gather(1, k[:, None]).to(torch.int64)
        assert bool((cell >= 0).all())
        sources = torch.zeros((3, gz * gx), dtype=torch.uint8, device="cuda").scatter_(1, cell, 1).view(3, gz, gx)
        fld = vec.grid_field(blocked, sources, inflate=0, like=like)
        cost = fld.field.view(torch.int16).to(torch.int32) & 0xFFFF
        want = r.label == (k + 1).to(torch.int16)[:, None, None]
        assert torch.equal(cost < 0xFFFE, want), int(((cost < 0xFFFE) != want).sum())
    vec.engine.check()
    vec.close()


def test_grid_sight_takes_a_row_of_representatives():
    """regions.cell goes to grid_sight as its `cells`, unchanged: a listed region's representative sees at least itself, a -1 nothing"""
    import torch
    vec = _vec("MiniWorld-MazeS3-v0", 5)
    m = vec.seen_map(cell=0.25)
    rng = np.random.default_rng(6300)
    opaque = dev((rng.random((5, m.gz, m.gx)) < 0.1).astype(np.uint8))
    frontier = dev((rng.random((5, m.gz, m.gx)) < np.array([0.002, 0.01, 0.02, 0.05, 0.3])[:, None, None]).astype(np.uint8))
    r = vec.grid_regions(frontier, connectivity=8, max_regions=32, like=m)
    gain = vec.grid_sight(opaque, r.cell, like=m)
    assert tuple(gain.shape) == (5, 32)
    assert torch.equal(gain == 0, r.cell == -1)
    assert bool((r.cell == -1).any()) and bool((r.cell >= 0).any()) and bool((r.count > 32).any())
    # the centroid: sum / size on the device, NaN for none
    c = r.centroid
    assert torch.equal(c.isnan().any(dim=2), r.cell == -1)
    k = r.cell >= 0
    assert torch.equal((c[k] * r.size[k][:, None].double()).round().to(torch.int32), r.sum[k])
    vec.engine.check()
    vec.close()


def test_into_reuses_storage():
    import torch
    vec = _vec("MiniWorld-Hallway-v0", 4)
    m = vec.seen_map(cell=0.25)
    rng = np.random.default_rng(6400)
    a, b = (dev((rng.random((4, m.gz, m.gx)) < 0.4).astype(np.uint8)) for _ in range(2))
    r = vec.grid_regions(a, connectivity=8, min_cells=2, max_regions=16, like=m, labels=True)
    ptrs = [t.data_ptr() for t in (r.count, r.size, r.cell, r.sum, r.label)]
    first = [t.clone() for t in (r.count, r.size, r.cell, r.sum, r.label)]
    fresh = vec.grid_regions(b, connectivity=8, min_cells=2, max_regions=16, like=m, labels=True)
    mask = torch.tensor([1, 1, 0, 1], dtype=torch.uint8, device="cuda")
    assert vec.grid_regions(b, mask=mask, into=r) is r
    assert [t.data_ptr() for t in (r.count, r.size, r.cell, r.sum, r.label)] == ptrs
    for t, old, new in zip((r.count, r.size, r.cell, r.sum, r.label), first, (fresh.count, fresh.size, fresh.cell, fresh.sum, fresh.label)):
        assert torch.equal(t[2], old[2]) and torch.equal(t[mask.bool()], new[mask.bool()])
    assert not torch.equal(r.label[0], first[4][0])
    vec.engine.check()
    vec.close()


def test_refusals_launch_nothing():
    import torch
    from miniworld_amd import engine
    n, gz, gx, K = 3, 16, 48, 4
    vec = _vec("MiniWorld-Hallway-v0", n)
    e, p = vec.engine, _params(gz, gx)
    member = torch.ones((n, gz, gx), dtype=torch.uint8, device="cuda")
    outs = _outputs(n, gz, gx, K)
    count, size, cell, total, label = outs
    big = engine.REGION_MAX + 1
    calls = [
        lambda: e.grid_regions(p, 5, 1, K, member, count, size, cell, total, label),
        lambda: e.grid_regions(p, 0, 1, K, member, count, size, cell, total, label),
        lambda: e.grid_regions(p, 4, 0, K, member, count, size, cell, total, label),
        lambda: e.grid_regions(p, 4, 1, 0, member, count, torch.zeros((n, 0), dtype=torch.int32, device="cuda"), torch.zeros((n, 0), dtype=torch.int32, device="cuda")),
        lambda: e.grid_regions(p, 4, 1, big, member, count, torch.zeros((n, big), dtype=torch.int32, device="cuda"), torch.zeros((n, big), dtype=torch.int32, device="cuda")),
        lambda: e.grid_regions(engine.MwNavParams(0.0, 0.0, 0.0, gx, gz, 0, 0), 4, 1, K, member, count, size, cell, total, label),
        lambda: e.grid_regions(engine.MwNavParams(0.25, 0.0, 0.0, gx, gz + 1, 0, 0), 4, 1, K, member, count, size, cell, total, label),   # other tensors' shape
        lambda: e.grid_regions(p, 4, 1, K, member, count, size, cell, total, label.to(torch.int32)),
        lambda: e.grid_regions(p, 4, 1, K, member, None, size, cell),
    ]
    for call in calls:
        with pytest.raises(engine.EngineError):
            call()
        assert all(bool((t == SENTINEL).all()) for t in outs)
    e.check()           # a refused call leaves the status word clean
    # ... and the largest list is served
    most = engine.REGION_MAX
    r = vec.grid_regions(member, max_regions=most, like=vec.seen_map(cell=0.25))
    assert r.count.tolist() == [1] * n and r.size[:, 0].tolist() == [gz * gx] * n and bool((r.size[:, 1:] == 0).all())
    e.check()
    vec.close()
