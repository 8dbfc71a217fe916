"""The dealing rule of the small-scene geometry kernel (miniworld_amd/csrc/mw_geom_deal.h: mw_deal_select, mw_geom_deal) and the
helper that switches it on (mw_policy.h: geom_deals), without a GPU: tests/hostcheck/geom_deal.cpp is compiled as a stand-alone
program with the address and undefined-behaviour sanitizers and its answers are checked here.

The rule: a group is 64 consecutive envs and the wavefronts that serve them — L of them with 64 / L slots each, fewer for a ragged
last group —; slot j of wavefront i builds the env whose set bit of the group's mask has rank i + j * waves.  Three properties, for
L in {8, 16, 32}: every set bit is dealt exactly once, no clear bit is dealt, and the wavefronts' slot counts differ by at most one."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "geom_deal.cpp")
LANES = (8, 16, 32)
FULL = (1 << 64) - 1


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("geom_deal") / "geom_deal")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    return exe


def _ask(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return [[int(x) for x in o.split()] for o in out]


def _masks():
    """(envs of the group, mask): empty, full, single bits, every popcount 0..64 at seeded positions, ragged last groups"""
    rng = np.random.default_rng(26)
    cases = [(64, 0), (64, FULL)] + [(64, 1 << b) for b in range(64)]
    for pop in range(65):
        for _ in range(3):
            bits = rng.choice(64, pop, replace=False)
            cases.append((64, sum(1 << int(b) for b in bits)))
    for n in (1, 2, 3, 5, 7, 8, 9, 31, 33, 49, 63):         # a ragged last group: envs 0 .. n - 1 only
        inside = (1 << n) - 1
        cases += [(n, 0), (n, inside), (n, 1 << (n - 1))]
        cases += [(n, int(rng.integers(0, 1 << 62)) * 4 + int(rng.integers(0, 4)) & inside) for _ in range(6)]
    return cases


def test_every_set_bit_is_dealt_once_no_clear_bit_and_the_counts_differ_by_at_most_one(program):
    queries = [(L, n, m) for L in LANES for n, m in _masks()]
    got = _ask(program, [f"D {L} {n} {m:x}" for L, n, m in queries])
    assert len(queries) > 3 * 300
    for (L, n, m), g in zip(queries, got):
        epw = 64 // L
        waves = min(L, -(-n // epw))
        assert g[0] == waves and len(g) == 1 + waves * epw, (L, n, hex(m))
        slots = np.asarray(g[1:]).reshape(waves, epw)
        dealt = slots[slots >= 0]
        want = [b for b in range(64) if (m >> b) & 1]
        assert sorted(dealt.tolist()) == want, (L, n, hex(m), "every set bit exactly once, no clear bit")
        counts = (slots >= 0).sum(1)
        assert counts.max() - counts.min() <= 1, (L, n, hex(m), counts.tolist())
        # the rule itself: rank i + j * waves, so a wavefront's filled slots come first and its envs ascend
        for i in range(waves):
            for j in range(epw):
                r = i + j * waves
                assert slots[i, j] == (want[r] if r < len(want) else -1), (L, n, hex(m), i, j)
        if m:
            assert slots[0, 0] == want[0]               # wavefront 0 is never empty while any env is built
        assert counts.max() == -(-len(want) // waves)   # the fullest wavefront holds no more than an even share


def test_a_group_reaches_four_envs_per_wavefront_only_beyond_48_built_envs(program):
    """The benchmark's shape, 16 lanes per env: two or three envs per wavefront at the usual drawn share, never four up to 48."""
    rng = np.random.default_rng(4)
    pops = list(range(65))
    masks = [sum(1 << int(b) for b in rng.choice(64, p, replace=False)) for p in pops]
    for p, g in zip(pops, _ask(program, [f"D 16 64 {m:x}" for m in masks])):
        counts = (np.asarray(g[1:]).reshape(16, 4) >= 0).sum(1)
        assert counts.max() == -(-p // 16) and (counts.max() == 4) == (p > 48), p


def test_select_names_the_bit_of_a_rank_and_refuses_what_is_not_there(program):
    rng = np.random.default_rng(5)
    masks = [0, 1, 1 << 63, FULL, 0x8000000000000001, 0xAAAAAAAAAAAAAAAA] + [int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)) for _ in range(20)]
    queries = [(m, r) for m in masks for r in (-1, 0, 1, 31, 32, 33, 62, 63, 64, 1000, -2**31, 2**31 - 1)]
    for (m, r), g in zip(queries, _ask(program, [f"S {m:x} {r}" for m, r in queries])):
        bits = [b for b in range(64) if (m >> b) & 1]
        assert g == [bits[r] if 0 <= r < len(bits) else -1], (hex(m), r)


def test_the_kernel_deals_exactly_where_a_plan_follows_and_the_switch_is_on(program):
    queries = [(p, e, l) for p in (0, 1) for e in (0, 1) for l in (8, 16, 32, 64)]
    for (p, e, l), g in zip(queries, _ask(program, [f"P {p} {e} {l}" for p, e, l in queries])):
        assert g == [int(bool(p and e and l < 64))], (p, e, l)


def test_the_accessor_is_declared_exported_and_refuses_a_null_engine():
    import re
    from miniworld_amd import engine
    header = open(os.path.join(os.path.dirname(HERE), "include", "mwengine.h")).read()
    assert re.search(r"int mw_get_geom_built\(mw_engine \*e, uint8_t \*host_out, void \*stream\);", header)
    engine.build_library()
    lib = engine.load_library()
    assert lib.mw_get_geom_built(None, None, None) == -1          # no engine: MW_E_INVALID
