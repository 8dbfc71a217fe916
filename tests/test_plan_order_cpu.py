"""The ordered frame plan's shared functions (miniworld_amd/csrc/mw_frame_plan.h: mw_plan_cost_class, mw_plan_class_count,
mw_plan_slot) and the helper that bounds it (mw_policy.h: frame_plan_ordered), without a GPU: tests/hostcheck/plan_order.cpp is
compiled as a stand-alone program with the address and undefined-behaviour sanitizers and its answers are compared with models
written here.

The rule: an env's cost class is min(7, length // 4) of its display-list length (0 for a length below 1); the quad kernel's
workgroups 0 .. n_draw - 1 take the draw entries from class 7 down to class 0, each class's entries by rank, the next n_copy take
the copy entries in order, the rest leave."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "plan_order.cpp")
CLASSES, HEAD, MAX_N = 8, 96, 0xFFFF


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_order") / "plan_order")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    return exe


def _ask(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return [[int(x) for x in o.split()] for o in out]


def test_the_cost_class_is_monotone_and_clamped_at_both_ends(program):
    lengths = list(range(-3, 70)) + [255, 256, 4096, 2**31 - 1, -2**31]
    got = _ask(program, [f"C {len(lengths)} " + " ".join(map(str, lengths))])[0]
    assert got == [min(CLASSES - 1, max(v, 0) // 4) for v in lengths]
    order = np.argsort(lengths, kind="stable")
    assert (np.diff(np.asarray(got)[order]) >= 0).all()
    assert min(got) == 0 and max(got) == CLASSES - 1 and set(got) == set(range(CLASSES))


def test_a_plan_is_ordered_up_to_the_batch_its_counts_hold(program):
    ns = [1, 64, 4096, MAX_N, MAX_N + 1, 0xFFFFFF]
    for n, got in zip(ns, _ask(program, [f"O {n}" for n in ns])):
        ordered = n <= MAX_N
        assert got[0] == int(ordered), n
        assert got[1] == HEAD + n * (1 + CLASSES if ordered else 2), n
        assert got[2] == HEAD and got[3:] == [HEAD + n * (1 + c) for c in range(CLASSES)], n
        assert got[3 + CLASSES - 1] + n <= got[1] or not ordered        # the last segment ends inside an ordered block


def _model(n, n_copy, counts):
    """per workgroup b: (kind, class, rank, the address of the word it loads)"""
    out, b = [], 0
    for c in reversed(range(CLASSES)):
        for rank in range(counts[c]):
            out.append((1, c, rank, HEAD + n * (1 + c) + rank))
    n_draw = len(out)
    out = out[:n]
    for b in range(len(out), n):
        i = b - n_draw
        out.append((2, 0, i, HEAD + i) if i < n_copy else (3, 0, i, 0))
    return out


def _count_vectors():
    rng = np.random.default_rng(22)
    cases = [(1, 0, [0] * 8), (1, 1, [0] * 8), (1, 0, [0, 0, 0, 1, 0, 0, 0, 0]),
             (130, 0, [0] * 8),                                     # zero draws, zero copies: every workgroup leaves
             (130, 130, [0] * 8),                                   # zero draws: every workgroup copies
             (130, 0, [0, 0, 0, 0, 0, 130, 0, 0]),                  # everything in one class, zero copies
             (130, 0, [130, 0, 0, 0, 0, 0, 0, 0]), (130, 0, [0, 0, 0, 0, 0, 0, 0, 130]),
             (130, 40, [7, 0, 0, 33, 0, 0, 20, 0]),                 # empty classes between full ones; 30 workgroups leave
             (130, 30, [10, 20, 5, 15, 10, 20, 10, 10]),            # every class, and the launch exactly full
             (65, 1, [0, 64, 0, 0, 0, 0, 0, 0]),
             (MAX_N, 0, [0, 0, 0, MAX_N, 0, 0, 0, 0]),              # the capacity of the policy helper: one class holds every env,
             (MAX_N, 0, [0, 0, 0, 0, MAX_N, 0, 0, 0]),              # in either word of the head,
             (MAX_N, 0, [MAX_N, 0, 0, 0, 0, 0, 0, 0]), (MAX_N, 0, [0, 0, 0, 0, 0, 0, 0, MAX_N]),
             (MAX_N, MAX_N, [0] * 8),
             (MAX_N, 5, [8191, 8191, 8191, 8191, 8191, 8191, 8191, 8193])]
    for _ in range(40):
        n = int(rng.integers(1, 400))
        cuts = np.sort(rng.integers(0, n + 1, CLASSES + 1))
        parts = np.diff(np.concatenate([[0], cuts]))               # 8 classes, the copies, and what leaves
        counts = [int(x) for x in parts[:CLASSES]]
        for c in rng.choice(CLASSES, int(rng.integers(0, 6)), replace=False):
            counts[c] = 0
        cases.append((n, int(parts[CLASSES]), counts))
    return cases


def test_the_lookup_visits_every_entry_once_in_non_increasing_class_order(program):
    cases = _count_vectors()
    got = _ask(program, [f"L {n} {n_copy} " + " ".join(map(str, counts)) for n, n_copy, counts in cases])
    for (n, n_copy, counts), g in zip(cases, got):
        rows = [tuple(g[4 * b:4 * b + 4]) for b in range(n)]
        assert len(g) == 4 * n and rows == _model(n, n_copy, counts), (n, n_copy, counts)
        n_draw = sum(counts)
        draws = [r for r in rows if r[0] == 1]
        assert len(draws) == min(n_draw, n) and rows[:len(draws)] == draws                  # dense: the drawing workgroups come first
        assert all(a[1] >= b[1] for a, b in zip(draws, draws[1:]))                           # non-increasing class
        assert len({r[3] for r in draws}) == len(draws)                                      # no entry twice
        if n_draw <= n:
            assert sorted((r[1], r[2]) for r in draws) == sorted((c, k) for c in range(CLASSES) for k in range(counts[c]))      # every entry
        copies = [r for r in rows if r[0] == 2]
        assert [r[2] for r in copies] == list(range(min(n_copy, max(n - n_draw, 0))))
        assert all(HEAD <= r[3] < HEAD + n for r in copies)


def test_the_accessor_is_declared_exported_and_refuses_a_null_engine():
    import re
    from miniworld_amd import engine
    header = open(os.path.join(os.path.dirname(HERE), "include", "mwengine.h")).read()
    engine.build_library()
    lib = engine.load_library()
    assert lib.mw_get_frame_plan(None, None, 0, None, None) == -1          # no engine: MW_E_INVALID


def test_one_env_beyond_the_capacity_is_an_unordered_plan(program):
    """A batch of 65536 envs could put 65536 entries into one 16-bit count: the helper must say no, and the block is the unordered one."""
    got = _ask(program, [f"O {MAX_N + 1}"])[0]
    assert got[0] == 0 and got[1] == HEAD + 2 * (MAX_N + 1)
