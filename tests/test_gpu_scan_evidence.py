"""Scan evidence on the GPU (mw_scan_evidence; vec.scan_evidence / scan_evidence_update), bit for bit against tests/evidence_reference.py: the
synthetic cases through `origin=`; a tie to the scan-map kernel; and what the evidence is for — a later scan takes back a wrong one."""
import math

import numpy as np
import pytest

import evidence_reference as ev_ref
import scan_reference as ref
from query_checks import dev, host, worlds
from query_checks import vec_env as _vec

pytestmark, N = pytest.mark.gpu, 8
_extents = lambda vec: [[float(v) for v in w["extent"]] for w in worlds(vec)]      # noqa: E731
SHAPES = [(gz, gx, 65, 1 + 4095 * (k % 2)) for k, (gz, gx) in enumerate(ref.GRIDS)] + [(103, 103, 1, 4096), (103, 103, 4096, 1), (103, 103, 4096, 4096)]


@pytest.mark.parametrize("gz,gx,R,cap", SHAPES)
def test_the_kernel_equals_the_restatement(gz, gx, R, cap):
    """an env per case (the random one twice) on a grid of its own over the Hallway's extent, from `origin=`, every output asked for; then
    random beams with hit = 100 under `clear` on envs 1, 2, 5 and a zero mask byte on envs 2, 3, the optional outputs left out.  103 x 103
    is odd: the rows of the odd envs start off a 4-byte boundary, each plane at another distance."""
    import torch
    from miniworld_amd import engine
    from miniworld_amd.queries import ScanEvidence
    vec = _vec("MiniWorld-Hallway-v0", N)
    ext, cell = _extents(vec), 0.25
    while any((gx + 0.5) * cell <= e[1] - e[0] or (gz + 0.5) * cell <= e[3] - e[2] for e in ext):
        cell *= 2
    rng, names = np.random.default_rng(4900 + gz + R), ref.CASES + ("random",)
    ev = [np.zeros((gz, gx), np.int8) for _ in range(N)]
    clear, mask = np.array([0, 1, 1, 0, 0, 1, 0, 0], np.uint8), np.array([1, 1, 0, 0, 1, 1, 1, 1], np.uint8)
    params, first = engine.MwNavParams(cell, 0.0, 0.0, gx, gz, 0, 0), None
    for call in range(2):
        cases = [ref.case(names[i] if call == 0 else "random", rng, R, gx, gz, (ext[i][0], ext[i][2]), cell) for i in range(N)]
        max_range = 6.0 if call else 20.0       # (the first call cuts no case short of its own max_range: each t is capped first)
        t = np.stack([np.where(c[1] < c[3], c[1], max_range) if call == 0 else c[1] for c in cases])
        rule = (100 if call else 3, 1, cap, -20, 20, -2, 3)
        zeros = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda")       # noqa: E731
        m = ScanEvidence(dev(np.stack(ev)), None if call else zeros(N, 2, gz, gx), None if call else zeros(N, gz, gx), zeros(N, 2, dtype=torch.int32),
                         None if call else zeros(N, 2, dtype=torch.int32), params, R, 2 * math.pi, max_range, "walls", rule)
        scan = {"t": dev(t), "dir": dev(np.stack([c[2] for c in cases]))}
        origin = dev(np.array([(c[0][0], 9.0, c[0][1]) for c in cases]))
        assert vec.scan_evidence_update(m, scan, origin=origin, clear=dev(clear) if call else None, mask=dev(mask) if call else None) is m.changed
        got_ev, got_count = host(m.ev), host(m.count)
        for i in range(N):
            if call and not mask[i]:
                assert np.array_equal(got_ev[i], ev[i]) and not got_count[i].any(), i       # (untouched: the fresh count tensor's zeros)
                continue
            hits, passes = ev_ref.counts(cases[i][0], t[i], cases[i][2], max_range, ext[i][0], ext[i][2], cell, gx, gz)
            planes, score, count, changed = ev_ref.update(ev[i], hits, passes, rule, clear=call == 1 and bool(clear[i]))
            assert np.array_equal(got_ev[i], ev[i]), (i, call, int((got_ev[i] != ev[i]).sum()))
            assert got_count[i].tolist() == count.tolist(), (i, call)
            if call == 0:
                assert np.array_equal(host(m.map[i]), planes) and np.array_equal(host(m.score[i]), score) and host(m.changed[i]).tolist() == changed.tolist(), i
        first = first or m
    assert R == 1 or int(first.count.sum()) > N and max(int(e.max()) for e in ev) == 20 and min(int(e.min()) for e in ev) < 0
    vec.engine.check()
    vec.close()


def test_one_vote_from_zero_is_the_scan_map():
    """kernel to kernel: from zero with hit = miss = cap = 1 and a clamp of -1 .. 1, one update leaves ev > 0 exactly on the obstacle plane and
    ev < 0 exactly on the free plane of a fresh ScanMap updated with the same scan, and the likelihood plane is the obstacle plane"""
    import torch
    vec = _vec("MiniWorld-FourRooms-v0", N, seed=3)
    m = vec.scan_evidence(rays=257, max_range=5.0, hit=1, miss=1, cap=1, lo=-1, hi=1)
    binary = vec.scan_map(like=m, rays=257, max_range=5.0)
    scan = vec.lidar(257, m.fov, 5.0)
    vec.scan_map_update(binary, scan)
    assert vec.scan_evidence_update(m, scan) is m.changed
    assert torch.equal(m.ev > 0, binary.obstacle != 0) and torch.equal(m.ev < 0, binary.free != 0) and torch.equal(m.map, binary.map)
    assert torch.equal(m.score, binary.obstacle) and torch.equal(m.count, binary.count) and torch.equal(m.changed, binary.new) and int(m.count.min()) > 0
    vec.engine.check()
    vec.close()


def test_later_scans_take_back_a_wrong_one():
    """a scan traced from an origin half a metre off, then the same scan three times from the true one: with hit = 3, miss = 1 every
    obstacle cell of the evidence map is one of the true-pose ScanMap; the binary ScanMap fed the same four updates keeps cells that
    are not.  The Hallway's walls alone, 1024 beams: every cell inside is passed by a true beam, and nothing hides one."""
    import torch
    vec = _vec("MiniWorld-Hallway-v0", N, seed=2)
    m = vec.scan_evidence(rays=1024, max_range=20.0, obstacles="walls")         # (20 m: past the room's diagonal, so no beam is cut short)
    truth, binary = (vec.scan_map(like=m, rays=1024, max_range=20.0, obstacles="walls") for _ in range(2))
    scan = vec.lidar(1024, m.fov, m.max_range, obstacles="walls")
    pos = vec.state(("agent_pos",))["agent_pos"].clone()
    off = pos + torch.tensor([0.5, 0.0, 0.5], dtype=torch.float64, device="cuda")
    vec.scan_map_update(truth, scan, origin=pos)
    for origin in (off, pos, pos, pos):
        vec.scan_evidence_update(m, scan, origin=origin)
        vec.scan_map_update(binary, scan, origin=origin)
    assert int(m.count[:, 1].min()) > 0 and not bool(((m.obstacle != 0) & (truth.obstacle == 0)).any())
    assert bool(((binary.obstacle != 0) & (truth.obstacle == 0)).flatten(1).any(1).all())
    assert not bool(((m.free != 0) & (m.obstacle != 0)).any()) and torch.equal(m.score, m.ev.clamp(min=0).to(torch.uint8))
    vec.engine.check()
    vec.close()
