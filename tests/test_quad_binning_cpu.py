"""The quad kernel's binning arithmetic (miniworld_amd/csrc/mw_quad_bin.h), without a GPU: tests/hostcheck/quad_binning.cpp is
compiled as a stand-alone program with the address and undefined-behaviour sanitizers; it walks a frame's tiles and quads the way
phases A and B of mw_rasterq.hip do — an edge triple evaluated at the first rectangle of a run, one add per edge for each one after
it — and its values and verdicts are compared with the flat formula written here, at every tile and every quad.

The flat formula: E_k = mul24(A_k, px) + mul24(B_k, gy) + C_k modulo 2^32 at the rectangle's first pixel (px, gy), gy counted
upwards (gy = H - h - row * h); mul24 multiplies the sign-extended low 24 bits; touched iff E_k > T_k for every k as signed 32-bit
values, covered iff E_k > F_k.  Equality throughout: a stepped value is the flat value bit for bit."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "quad_binning.cpp")
SIZES = [(16, 4), (16, 60), (80, 4), (80, 60), (64, 64), (128, 64)]
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
EMPTY_BOX = 0x00FF00FF


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("quad_binning") / "quad_binning")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    return exe


def _ask(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return [np.array(o.split(), dtype=np.int64) for o in out]


def _sext24(v):
    v = np.asarray(v, np.int64) & 0xFFFFFF
    return v - ((v & 0x800000) << 1)


def _wrap32(v):
    v = np.asarray(v, np.int64) & 0xFFFFFFFF
    return v - ((v & 0x80000000) << 1)


def flat(W, H, rw, rh, tri):
    """(E int64 [ny][nx][3] as signed 32-bit values, verdict [ny][nx]) by the flat formula"""
    A, B, C, T, F = (np.array(tri[3 * i:3 * i + 3], np.int64) for i in range(5))
    px = (np.arange(W // rw) * rw)[None, :, None]
    gy = (H - rh - np.arange(H // rh) * rh)[:, None, None]
    E = _wrap32(_wrap32(_sext24(A) * px) + _wrap32(_sext24(B) * gy) + _wrap32(C))
    touch, full = (E > T).all(axis=2), (E > F).all(axis=2)
    return E, touch.astype(np.int64) | (full.astype(np.int64) << 1)


def triangles():
    """[A[3] B[3] C[3] T[3] F[3]]: A, B random 24-bit values, the +-2^23 extremes and zeros; C over the whole 32-bit range, values
    that make the sums wrap among them; thresholds random, at INT_MIN and at INT_MAX"""
    rng = np.random.default_rng(34)
    lo24, hi24 = -2 ** 23, 2 ** 23 - 1
    tris = []
    extremes = [lo24, hi24, 0]
    for a in extremes:
        for b in extremes:
            for c in (0, INT_MAX, INT_MIN, -1, INT_MAX - 5 * 2 ** 23, INT_MIN + 5 * 2 ** 23):
                tris.append([a, b, -a, b, a, 0, c, -c - 1 if c != INT_MIN else INT_MAX, c ^ 0x55555555,
                             INT_MIN, INT_MAX, 0, INT_MIN, INT_MAX, c])
    for _ in range(30):
        ab = rng.integers(lo24, hi24 + 1, 6)
        ab[rng.random(6) < 0.15] = 0
        c = rng.integers(INT_MIN, INT_MAX + 1, 3)
        t = rng.integers(INT_MIN, INT_MAX + 1, 6)
        t[rng.random(6) < 0.2] = INT_MIN
        t[rng.random(6) < 0.1] = INT_MAX
        tris.append([int(x) for x in (*ab, *c, *t)])
    for _ in range(20):         # small coefficients, as a frame's own triangles have: verdicts that change inside the frame
        ab = rng.integers(-3000, 3001, 6) * 256
        c = rng.integers(-2 ** 24, 2 ** 24, 3)
        t = rng.integers(-2 ** 16, 2 ** 16, 3)
        f = t + rng.integers(0, 2 ** 18, 3)
        tris.append([int(x) for x in (*ab, *c, *t, *f)])
    return tris


def _walks(W, H):
    """(direction, rectangle width, height, run): phase A's tile rows, phase B's runs of 4 and 8 quads, and both stepped down columns"""
    return [("H", 16, 4, W // 16), ("H", 2, 2, 4), ("H", 2, 2, 8), ("V", 16, 4, H // 4), ("V", 2, 2, 2), ("H", 16, 4, 1)]


@pytest.mark.parametrize("W,H", SIZES)
def test_stepped_values_and_verdicts_equal_the_flat_formula(program, W, H):
    tris = triangles()
    queries, keys = [], []
    for d, rw, rh, run in _walks(W, H):
        for i, tri in enumerate(tris):
            queries.append(f"W {d} {W} {H} {rw} {rh} {run} " + " ".join(map(str, tri)))
            keys.append((rw, rh, i, d, run))
    wanted = {}
    seen = set()
    for (rw, rh, i, d, run), got in zip(keys, _ask(program, queries)):
        if (rw, rh, i) not in wanted:
            wanted[rw, rh, i] = flat(W, H, rw, rh, tris[i])
        E, verdict = wanted[rw, rh, i]
        got = got.reshape(H // rh, W // rw, 4)
        assert np.array_equal(got[..., :3], E), (W, H, rw, rh, d, run, tris[i])
        assert np.array_equal(got[..., 3], verdict), (W, H, rw, rh, d, run, tris[i])
        seen |= set(np.unique(verdict).tolist())
    assert seen == {0, 1, 2, 3}          # (2: covered and not touched — thresholds that only a wrapped sum can give — is compared like the rest)


def test_the_sums_wrap_in_the_cases(program):
    """the cases hold values whose exact sum leaves the 32-bit range: the compare is of the wrapped value, in both programs"""
    W, H = 128, 64
    wrapped = 0
    for tri in triangles():
        A, B, C = (np.array(tri[3 * i:3 * i + 3], np.int64) for i in range(3))
        exact = _sext24(A) * (W - 16) + _sext24(B) * (H - 4) + C
        wrapped += int(((exact > INT_MAX) | (exact < INT_MIN)).any())
    assert wrapped >= 20


def _box(x0, x1, y0, y1):
    return x0 | x1 << 8 | y0 << 16 | y1 << 24


@pytest.mark.parametrize("W,H", SIZES)
def test_the_box_walk_visits_exactly_the_boxs_tiles(program, W, H):
    tx, ty = W // 16, H // 4
    rng = np.random.default_rng(W * 1000 + H)
    boxes = [(0, tx - 1, 0, ty - 1), (0, 0, 0, 0), (tx - 1, tx - 1, ty - 1, ty - 1), (0, tx - 1, ty - 1, ty - 1), (tx - 1, tx - 1, 0, ty - 1)]
    for _ in range(40):
        x = np.sort(rng.integers(0, tx, 2))
        y = np.sort(rng.integers(0, ty, 2))
        boxes.append((int(x[0]), int(x[1]), int(y[0]), int(y[1])))
    got = _ask(program, [f"B {_box(*b)} {tx} {ty}" for b in boxes])
    for b, g in zip(boxes, got):
        want = [(y, x) for y in range(b[2], b[3] + 1) for x in range(b[0], b[1] + 1)]
        assert [tuple(r) for r in g.reshape(-1, 2).tolist()] == want, (W, H, b)
    # the empty box, and boxes with one empty side: no tile at all
    for g in _ask(program, [f"B {EMPTY_BOX} {tx} {ty}", f"B {_box(1, 0, 0, 0)} {tx} {ty}", f"B {_box(0, 0, 1, 0)} {tx} {ty}"]):
        assert len(g) == 0
    # a box that reaches past the frame is held inside it
    g = _ask(program, [f"B {_box(0, 254, 0, 254)} {tx} {ty}"])[0]
    assert [tuple(r) for r in g.reshape(-1, 2).tolist()] == [(y, x) for y in range(ty) for x in range(tx)]
