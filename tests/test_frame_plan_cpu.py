"""The frame plan's decision (miniworld_amd/csrc/mw_frame_plan.h) and the helper that says when a plan is made (mw_policy.h:
frame_plans), without a GPU: tests/hostcheck/frame_plan.cpp is compiled as a stand-alone program with the address and
undefined-behaviour sanitizers and its answers are compared with models written here.

The rule (mw_get_frame_source): a clean env is left alone where frame reuse applies (1); else the lowest-numbered slot whose 80 bytes
equal the key is copied (2 + j); else the frame is drawn (0) into slot min(header, slots - 1)."""
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "frame_plan.cpp")
KEY_WORDS, PATH_QUAD = 10, 1


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_plan") / "frame_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    return exe


def _ask(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return [[int(x) for x in o.split()] for o in out]


def _model(clean, reuse, key, slots_keys, header):
    """(source byte, slot): the rule, over Python lists"""
    if reuse and clean:
        return 1, 0
    for j, k in enumerate(slots_keys):
        if k == key:
            return 2 + j, j
    return 0, (min(header, len(slots_keys) - 1) if slots_keys else 0)


def _random_key(rng):
    # (words that differ in one bit of one word only must still part two keys: a small alphabet per word makes near-duplicates common)
    return [int(x) for x in rng.integers(0, 3, KEY_WORDS, dtype=np.uint64) << rng.integers(0, 64, KEY_WORDS, dtype=np.uint64)]


def test_the_verdict_agrees_with_the_rule(program):
    rng = np.random.default_rng(2001)
    lines, want, seen = [], [], set()
    for case in range(4000):
        slots = int(rng.integers(0, 9))                      # 0: no cache at all
        key = _random_key(rng)
        table = [_random_key(rng) for _ in range(slots)]
        mode = case % 5
        hits = []
        if slots and mode in (1, 2):                         # the key sits in one slot, or duplicated in several
            hits = sorted(set(int(x) for x in rng.integers(0, slots, 1 if mode == 1 else 3)))
            for j in hits:
                table[j] = list(key)
        if slots and mode == 3:                              # all but one bit of the key in a slot: no match
            j = int(rng.integers(0, slots))
            table[j] = list(key)
            table[j][int(rng.integers(0, KEY_WORDS))] ^= 1 << int(rng.integers(0, 64))
        if slots and mode == 4:                              # nothing cached yet: the all-zero rows of a cleared table
            table = [[0] * KEY_WORDS for _ in range(slots)]
        # the header: a slot, the last slot, or a value beyond slots - 1 (a table cleared for fewer slots cannot happen, a clamp must hold anyway)
        header = int(rng.choice([0, max(slots - 1, 0), slots, slots + 5, 0xFFFFFFFF, int(rng.integers(0, 9))]))
        clean, reuse = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        words = key + ([header, 0] + [w for k in table for w in k] if slots else [])
        lines.append(f"V {clean} {reuse} {slots} {len(words)} " + " ".join(f"{w:x}" for w in words))
        src, slot = _model(clean, reuse, key, table, header)
        want.append([src, slot, src, slot])
        seen.add(("dup" if len(hits) > 1 else "one" if hits else "none", src if src < 2 else 2, header > slots - 1 and slots > 0))
    got = _ask(program, lines)
    bad = [i for i in range(len(lines)) if got[i] != want[i]]
    assert not bad, [(lines[i], got[i], want[i]) for i in bad[:4]]
    for need in [("dup", 2, False), ("one", 2, False), ("none", 0, True), ("none", 0, False), ("one", 1, False), ("none", 1, False)]:
        assert need in seen, ("the random tables never produced", need)


def test_every_slot_count_hits_its_lowest_duplicate_and_clamps_its_header(program):
    lines, want = [], []
    key = list(range(1, KEY_WORDS)) + [1]
    other = [7] * (KEY_WORDS - 1) + [1]
    for slots in range(1, 9):
        for lo in range(slots):
            for hi in range(lo, slots):
                table = [list(key) if j in (lo, hi) else list(other) for j in range(slots)]
                words = key + [3, 0] + [w for k in table for w in k]
                lines.append(f"V 0 1 {slots} {len(words)} " + " ".join(f"{w:x}" for w in words))
                want.append([2 + lo, lo] * 2)
        for header in range(0, 12):
            words = key + [header, 0] + other * slots
            lines.append(f"V 1 0 {slots} {len(words)} " + " ".join(f"{w:x}" for w in words))
            want.append([0, min(header, slots - 1)] * 2)
    assert _ask(program, lines) == want


def test_a_plan_is_made_exactly_for_plain_quad_frames_that_may_skip_an_env(program):
    lines, want = [], []
    for reuse, source, cache, hold in itertools.product((0, 1), repeat=4):
        for path in range(4):
            for listed in (0, 1):
                for n in (1, 4096, 0xFFFFFF, 0x1000000):
                    lines.append(f"P {reuse} {source} {cache} {hold} {path} {listed} {n}")
                    want.append([int(not listed and path == PATH_QUAD and (reuse or cache) and n <= 0xFFFFFF)])
    got = _ask(program, lines)
    assert got == want, [(l, g, w) for l, g, w in zip(lines, got, want) if g != w][:4]
    assert any(w == [1] for w in want) and any(w == [0] for w in want)
