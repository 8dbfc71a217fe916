"""The raster records' 24-bit edge arithmetic at the limits the code states, without a GPU: tests/hostcheck/edge_limits.cpp runs the
text the record writer and the tile and quad kernels call (miniworld_amd/csrc/mw_edge_rec.h, with the device's multiply modelled:
mw_qb_mul24) against the exact definition — 64-bit edge functions at every sample of every pixel of the raster grid, and the touch /
full classification of every tile and quad as tests/hostcheck/mwhost.cpp's mwhost_rect_counts defines it — on a family of triangles
that holds every extreme coefficient a frame can: all triples of {0, 1/256, 1/2, W/2, W - 1/256, W} x {the same for H}, both windings,
and 2 000 seeded random triangles.

(a) every size the launch policy (tests/hostcheck/policy.cpp: asked, not restated) sends to the tile, ragged-tile or quad kernels has
    no differing verdict at all;
(b) the model is not vacuous: at 128 x 48 (96 x 128) the triangles with B = +2^23 (A = +2^23) differ from the definition, in samples
    and in the quad kernel's classifications — the frames the engine drew wrongly while the policy admitted W = 128 and H = 128;
(c) for the sizes the policy refuses the test prints which bound the family violates there: the 24-bit operand, the 32-bit sum, or
    neither (found: the operand everywhere; the exact edge value never leaves 32 bits on these grids, up to 144 x 132).

A size a -> b is a frame of a pixels on a raster grid of b (ragged: padding pixels right of column a - 1 or below row a - 1); the
program rounds a frame up to its grid itself.  The program runs as a plain -O2 build for the whole sweep and once more under the address
and undefined-behaviour sanitizers on a few sizes; it is never loaded into Python."""
import itertools
import os
import subprocess

import pytest

import query_checks as qc
from test_launch_policy_cpu import RASTER_PATH, ask, policy_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "edge_limits.cpp")
WIDTHS = [16, 96, 112, 127, 128, 144]           # 127 -> 128
HEIGHTS = [4, 48, 64, 96, 126, 128, 132]        # 126 -> 128
SAMPLES = [8, 4]
SIZES = list(itertools.product(WIDTHS, HEIGHTS))
PATH_GENERIC = 3
VERDICTS = ("samples", "outside_box", "thr", "qtile_touch", "qtile_full", "qquad_touch", "qquad_full", "ttile_touch", "ttile_full")
SANITIZED = [(128, 48, 8), (96, 128, 4), (127, 96, 8), (16, 4, 4)]


def _run(exe, queries, *args):
    r = subprocess.run([exe, *args], input="".join(f"{w} {h} {s}\n" for w, h, s in queries), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    rows = r.stdout.split("\n")[:-1]
    assert len(rows) == len(queries)
    out = {}
    for q, row in zip(queries, rows):
        f = row.split()
        out[q] = {k: int(v) for k, v in zip(f[::2], f[1::2])}
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("edge_limits") / "edge_limits")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def threads():
    return str(max(1, min(16, len(os.sched_getaffinity(0)))))


@pytest.fixture(scope="module")
def counts(program, threads):
    """the program's answer for every size and sample count, computed once"""
    return _run(program, [(w, h, s) for (w, h), s in itertools.product(SIZES, SAMPLES)], "--threads", threads)


def reaches_the_24_bit_kernels(w, h, msaa):
    """does ANY engine of this frame size and sample count draw through the tile, ragged-tile, quad or quad-mesh kernels: with or
    without mesh entities and a visiting order, MW_K2Q on or off, a quad-kernel LDS plan that fits (0 bytes: the most the policy admits)"""
    lib = policy_lib()
    paths = {ask(lib, RASTER_PATH, [msaa, w, h, meshes, order, k2q, 0, 0, 0, depth, 0])[0]
             for meshes, order, k2q, depth in itertools.product((0, 1), (0, 1), (0, 1), (0, 1))}
    return paths != {PATH_GENERIC}


def test_the_policy_admits_and_refuses_sizes_of_the_sweep():
    admitted = [(w, h) for w, h in SIZES if reaches_the_24_bit_kernels(w, h, 8)]
    assert (127, 96) in admitted and (96, 126) in admitted and (112, 96) in admitted and (16, 4) in admitted       # ragged ones among them
    for size in ((128, 48), (48, 128), (128, 96), (96, 128), (128, 64), (128, 128), (144, 64), (127, 126)):
        assert not reaches_the_24_bit_kernels(*size, 8) and not reaches_the_24_bit_kernels(*size, 4), size


@pytest.mark.parametrize("msaa", SAMPLES)
@pytest.mark.parametrize("size", SIZES)
def test_admitted_sizes_have_no_differing_verdict(counts, size, msaa):
    """(a): samples, thresholds, tile bounds and the tile and quad classifications of both kernels, on the whole grid"""
    n = counts[(*size, msaa)]
    print(size, msaa, n)
    assert n["tris"] > 7000 and n["covered"] > 0
    if reaches_the_24_bit_kernels(*size, msaa):
        assert {k: n[k] for k in VERDICTS} == dict.fromkeys(VERDICTS, 0), (size, msaa)
        assert n["op24"] == 0 and n["sum32"] == 0


@pytest.mark.parametrize("msaa", SAMPLES)
def test_the_model_sees_the_coefficient_one_past_24_bits(counts, msaa):
    """(b): the records' formula at W = 128 and at H = 128, sizes the policy admitted before it asked for the coefficients' range"""
    wide, high = counts[(128, 48, msaa)], counts[(96, 128, msaa)]
    print(wide, high)
    assert wide["b23"] > 0 and wide["a23"] == 0 and wide["samples_b23"] > 0 and wide["samples"] == wide["samples_b23"]
    assert high["a23"] > 0 and high["b23"] == 0 and high["samples_a23"] > 0 and high["samples"] == high["samples_a23"]
    for n in (wide, high):
        assert n["qtile_touch"] > 0 and n["qtile_full"] > 0 and n["qquad_touch"] > 0 and n["qquad_full"] > 0
        assert n["op24"] == n["a23"] + n["b23"] and n["sum32"] == 0
        # the tile kernels' classification multiplies in full 32 bits: only their per-pixel edge values misread the coefficient
        assert n["ttile_touch"] == 0 and n["ttile_full"] == 0 and n["thr"] == 0 and n["outside_box"] == 0


def test_which_bound_the_refused_sizes_violate(counts):
    """(c): printed per size; the 32-bit sum is never the one — the exact edge value stays inside 32 bits on every grid of the sweep,
    128 x 128 and 144 x 132 included (|E| <= W H 2^16 inside the frame) —, and a size that holds no coefficient past 24 bits has no
    differing verdict either (127 x 126 on the 128 x 128 grid: refused by the stated sum bound, exact all the same)"""
    found = set()
    for (w, h), msaa in itertools.product(SIZES, SAMPLES):
        if reaches_the_24_bit_kernels(w, h, msaa):
            continue
        n = counts[(w, h, msaa)]
        which = "24-bit operand" if n["op24"] else "32-bit sum" if n["sum32"] else "neither"
        print(f"{w} x {h} at {msaa} samples: {which}; operand {n['op24']} triangles, sum {n['sum32']}, |E| <= {n['maxabs']}, differing samples {n['samples']}")
        found.add(which)
        assert n["sum32"] == 0 and n["maxabs"] < 2 ** 31
        assert (n["op24"] > 0) == (w >= 128 or h >= 128)
        if not n["op24"]:
            assert {k: n[k] for k in VERDICTS} == dict.fromkeys(VERDICTS, 0), (w, h, msaa)
        else:
            assert n["samples"] > 0
    assert found == {"24-bit operand", "neither"}


def test_the_halved_form_is_exact_where_the_records_form_is_not(program, threads):
    """DESIGN.md section 9's lever — A / 2 and B / 2 against 2 px and 2 gy: the same value, operands inside 24 bits up to 255 pixels a side"""
    for n in _run(program, [(128, 48, 8), (96, 128, 4), (128, 128, 8), (144, 132, 8)], "--formula", "halved", "--threads", threads).values():
        assert n["op24"] > 0 and {k: n[k] for k in VERDICTS} == dict.fromkeys(VERDICTS, 0)


def test_the_program_is_clean_under_the_sanitizers(counts, tmp_path_factory):
    """the same answers from the address / undefined-behaviour build, on a few sizes of the sweep"""
    exe = qc.build("edge_limits", tmp_path_factory.mktemp("edge_limits_asan"))
    got = _run(exe, SANITIZED, "--threads", "4")
    for q in SANITIZED:
        assert got[q] == counts[q], q
    assert got[(96, 128, 4)]["samples_a23"] > 0 and got[(127, 96, 8)]["samples"] == 0
