"""Scan evidence without a GPU: the kernel's phases (csrc/mw_evidence.h) on the host under sanitizers (hostcheck/scan_evidence.cpp), bit for
bit against evidence_reference.py; the new restatement anchored on scan_reference.py; the launch and the interface."""
import numpy as np
import pytest

import evidence_reference as ev_ref
import scan_reference as ref
from query_checks import build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, launch_of, run

RAY_MAX = 4096
RULES = [(3, 1, 1, -20, 20, -1, 1), (3, 2, 3, -8, 9, -2, 4), (5, 2, RAY_MAX, -127, 127, -127, 127)]        # cap 1, 3, MW_RAY_MAX


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("scan_evidence", tmp_path_factory.mktemp("scan_evidence"))


@pytest.mark.parametrize("gz,gx", ref.GRIDS)
def test_evidence_one_equals_the_restatement(program, tmp_path, gz, gx):
    """every case at 65 beams, the random one at 1 and 300 too, an env per run, the rows at every distance from a 4-byte boundary, the caps
    in turn, both forms of the start cell; three calls in a row: the case from the agent or an origin; random beams with hit = 100 on the
    result; random beams under `clear` (every other run) or a zero mask byte (every third).  Each call asks for another set of outputs."""
    rng, _beams = np.random.default_rng(4800 + gz), lambda t, d: [f"{float(a)!r} {float(x)!r} {float(z)!r}" for a, (x, z) in zip(t, d)]
    extent = (ref.MIN[0], ref.MIN[0] + gx * ref.CELL - 0.1, ref.MIN[1], ref.MIN[1] + gz * ref.CELL - 0.1)
    bound = set()
    for run_no, (name, R) in enumerate([(c, 65) for c in ref.CASES] + [("random", 1), ("random", 300)]):
        rule = RULES[run_no % 3]
        calls = [ref.case(name, rng, R, gx, gz), ref.case("random", rng, R, gx, gz), ref.case("random", rng, R, gx, gz)]
        rules = [rule, (100,) + rule[1:], rule]
        agent, masked, clear = run_no % 2 == 0, run_no % 3 != 2, run_no % 2 == 1
        flags = [(1, 0, 0 if agent else 1), (1, 0, 1), (int(masked), int(clear), 1)]
        outputs = [(run_no + 3 * call) % 8 for call in range(3)]
        lines = [f"{calls[0][0][0]!r} {calls[0][0][1]!r} 0.0", " ".join(repr(v) for v in extent),
                 f"{ref.CELL!r} {gx} {gz} {(run_no + gz) % 4} {calls[0][3]!r} {R} 3 {run_no % 2}"]
        for (origin, t, d, _), r, fl, out in zip(calls, rules, flags, outputs):
            lines += [" ".join(map(str, fl)) + f" {origin[0]!r} {origin[1]!r}", " ".join(map(str, r + (out,)))] + _beams(t, d)
        rows = iter(run(program, tmp_path / "evidence.txt", lines))
        ev = np.zeros((gz, gx), np.int8)
        held = [np.zeros((2, gz, gx), np.uint8), np.zeros((gz, gx), np.uint8), np.zeros(2, np.int64), np.full(2, -7, np.int64)]
        for call, ((origin, t, d, _), r, fl, out) in enumerate(zip(calls, rules, flags, outputs)):
            if fl[0]:
                hits, passes = ev_ref.counts(origin, t, d, calls[0][3], ref.MIN[0], ref.MIN[1], ref.CELL, gx, gz)
                if call == 0:       # the anchor: from zero, what gains is scan_reference's obstacle set, what loses its free set
                    free, obstacle = ref.sets(origin, t, d, calls[0][3], ref.MIN[0], ref.MIN[1], ref.CELL, gx, gz)
                    assert np.array_equal((hits > 0).reshape(gz, gx), obstacle) and np.array_equal(((hits == 0) & (passes > 0)).reshape(gz, gx), free), name
                planes, score, held[2], changed = ev_ref.update(ev, hits, passes, r, clear=bool(fl[1]))
                held = [planes if out & 1 else held[0], score if out & 2 else held[1], held[2], changed if out & 4 else held[3]]
                bound |= {k for k, v in (("lo", ev.min() == r[3]), ("hi", ev.max() == r[4])) if v and call == 1}
            for k, want in enumerate((ev, held[0][0], held[0][1], held[1])):
                got = np.array(next(rows).split(), np.int64).reshape(gz, gx)
                assert np.array_equal(got, want), (name, R, call, k, int((got != want).sum()))
            assert next(rows).split() == [str(int(v)) for v in (*held[2], *held[3], 1)], (name, R, call)
        assert next(rows, None) is None
        assert R == 1 or (ev != 0).any(), (name, R)
    assert bound == {"lo", "hi"}        # (both clamps bound in a second call)


def test_launch_and_interface(program, tmp_path):
    from miniworld_amd import engine
    call = ["1 0 0 0.0 0.0", "3 1 1 -20 20 -1 1 7", "1.0 1.0 0.0"]
    rows = run(program, tmp_path / "bad.txt", ["0.0 3.0 0.0", "-1.5 1.5 2.25 9.0", "0.25 12 4 1 6.0 1 2 1"] + call * 2)
    assert all(not np.array(r.split(), int)[:-1].any() and r.split()[-1] == "0" for r in rows) and len(rows) == 10       # not covered: all zero
    for cells, rays, lds in ((1, 1, 16 + 64), (103 * 103, 256, 42448 + 1088), (32768, RAY_MAX, 131072 + 16448), (32768, 1, 131072 + 64)):
        assert launch_of(program, 7, cells, rays) == {"grid": 7, "threads": 512, "lds": lds, "fits": 1}, (cells, rays)
    assert all(launch_of(program, 7, cells, rays)["fits"] == 0 for cells, rays in ((0, 1), (32769, 1), (16, 0), (16, RAY_MAX + 1)))
    check_units_built("mw_evidence.hip", "mw_engine_evidence.hip")
    check_kernel("mw_evidence_kernel", "mw_evidence.hip")
    check_does_not_wait("mw_engine_evidence.hip")
    check_refuses_null_engine("mw_scan_evidence", engine.MwNavParams(0.25, 0.0, 0.0, 4, 4, 0, 0), None, 1, None, None, None, None, None, 3, 1, 1, -20, 20, -1, 1,
                              None, None, None, None, None, None)
    good = (3, 1, 1, -20, 20, -1, 1)
    assert engine.evidence_rule(list(good)) == good and engine.evidence_rule((0, 0, RAY_MAX, -127, 127, -127, 127))
    for k, values in enumerate(((-1, 128), (-1, 128), (0, RAY_MAX + 1), (-128, 0), (0, 128), (-21, 0), (0, 21))):     # each below and above its range
        for v in values + (1.0, True):
            with pytest.raises(engine.EngineError, match=engine.EVIDENCE_RANGES[k][0] if isinstance(v, int) and not isinstance(v, bool) else "rule"):
                engine.evidence_rule(good[:k] + (v,) + good[k + 1:])
