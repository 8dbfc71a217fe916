"""The engine's own vertex / fragment arithmetic (miniworld_amd/csrc/mw_glmath.h, mw_frag.h — the functions the HIP kernels
call), compiled for the host and wrapped in a plain frame loop (tests/hostcheck/mwhost.cpp, test infrastructure), against the
reference's frames on real OpenGL (tests/golden/gl_*.npz) and against the oracle.  No GPU: this is the part of the kernels
that can go wrong in the last bit; what only a GPU can show (lanes, LDS, launches) is in the -m gpu tests."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import pyoracle
from test_oracle_vs_reference_gl import gl_cases, load_gl

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "mwhost.cpp")
LIB = os.path.join(HERE, "hostcheck", "libmwhost.so")
ROOT = os.path.dirname(HERE)


def build_host():
    """tests/hostcheck/libmwhost.so, (re)built when a source is newer; also used by the -m gpu selftests."""
    deps = [SRC, os.path.join(ROOT, "oracle", "mwo_math.c")] + [
        os.path.join(ROOT, "miniworld_amd", "csrc", h)
        for h in ("mw_glmath.h", "mw_frag.h", "mw_cover.h", "mw_quad_bin.h", "mw_math.h", "mw_selftest.h", "mw_hd.h", "mw_assets.h", "mw_asset_types.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        fma = ["-mfma"] if " fma " in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", *fma, "-pthread", "-shared", SRC,
                               os.path.join(ROOT, "oracle", "mwo_math.c"), "-o", LIB])
    lib = C.CDLL(LIB)
    lib.mwhost_render.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mwhost_sincosf.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.mwhost_lod_bits_mismatches.argtypes = [C.c_void_p, C.c_long]
    lib.mwhost_lod_bits_mismatches.restype = C.c_long
    lib.mwhost_cover_mismatches.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.POINTER(C.c_long)]
    lib.mwhost_cover_mismatches.restype = C.c_long
    lib.mwhost_sincosf_mismatches.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.mwhost_sincosf_mismatches.restype = C.c_long
    lib.mwhost_sincosf_sums.argtypes = [C.c_int, C.c_void_p]
    lib.mwhost_sincos_det_sums.argtypes = [C.c_uint64, C.c_int, C.c_void_p]
    lib.mwhost_sincos_det_check.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    lib.mwhost_build_pyramid.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.mwhost_build_pyramid.restype = C.c_long
    lib.mwhost_prepare_mesh.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 9
    return lib


@pytest.fixture(scope="module")
def host():
    return build_host()


@pytest.mark.parametrize("size", [(80, 60), (128, 96), (16, 4)])
def test_coverage_by_sample_columns_equals_the_per_sample_definition(host, size):
    """mw_cover.h (the mesh entity kernel's triangle setup in 32 bits and its coverage loop over the sample columns that cross
    a small triangle's bounding box) against setup_triangle_pos + the inside test at every sample of every pixel: the same
    culling, edges, bounds and depth plane, the same samples — each once — with the same 16-bit depths.  Sub-pixel triangles
    (a ball's), triangles of a few pixels, vertices ON sample positions and pixel corners (the fill rule's ties), triangles
    across the frame's border and larger than the frame."""
    W, H = size
    rng = np.random.default_rng(5)
    tris = []

    def add(centre, radius, n, snap=None):
        c = centre[:, None, :] + rng.uniform(-1, 1, (n, 3, 2)) * radius[:, None, None]
        if snap:
            c = np.round(c * snap) / snap
        z = rng.uniform(0.05, 0.999, (n, 3, 1))
        oow = rng.uniform(0.1, 10.0, (n, 3, 1))
        tris.append(np.concatenate([c, z, oow], axis=2).astype(np.float32))

    frame = np.array([W, H], np.float64)
    for radius, n in ((0.15, 30000), (0.5, 30000), (1.5, 20000), (6.0, 4000), (60.0, 400)):
        add(rng.uniform(-0.5, 1.0, (n, 2)) * frame * [1, 1] + rng.uniform(0, 1, (n, 2)) * 0, np.full(n, radius), n)
        add(rng.uniform(0, 1, (n // 2, 2)) * frame, np.full(n // 2, radius), n // 2, snap=16)        # vertices on the sample lattice
        add(rng.uniform(0, 1, (n // 4, 2)) * frame, np.full(n // 4, radius), n // 4, snap=1)         # ... on pixel corners
    win = np.ascontiguousarray(np.concatenate(tris))
    win[:, :, 0] = np.clip(win[:, :, 0], 0, W)       # unclipped vertices lie inside the viewport
    win[:, :, 1] = np.clip(win[:, :, 1], 0, H)
    covered = C.c_long(0)
    bad = host.mwhost_cover_mismatches(win.ctypes.data, len(win), W, H, C.byref(covered))
    assert bad == 0, f"{bad} of {len(win)} triangles differ"
    assert covered.value > 100_000


def test_lod_from_the_bits_of_rho2_equals_the_float_arithmetic(host):
    """mwgl::lod_from_rho2_bits (mw_rasterq.hip's lod: the conversion of exponent.mantissa to float IS the rounding of
    (float)e + (m - 1)) against mwgl::lod_from_rho2 (llvmpipe's arithmetic as the oracle states it): every exponent with
    its extreme and tie mantissas, 4 M random bit patterns, zeros, infinities, NaNs.  (The GPU test runs all 2^32.)"""
    rng = np.random.default_rng(0)
    mant = np.array([0, 1, 2, 3, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFE, 0x7FFFFF, 0x0FFFF, 0x10000, 0x7F8000, 0x7FFF80, 0x7FFFC0], np.uint32)
    edges = (np.arange(256, dtype=np.uint32)[:, None] << np.uint32(23)) | mant[None, :]
    edges = np.concatenate([edges.ravel(), edges.ravel() | np.uint32(0x80000000)])
    rand = rng.integers(0, 2 ** 32, 4_000_000, dtype=np.uint64).astype(np.uint32)
    # the range where the weight's low bits depend on the rounding: rho2 in [1, 2^24)
    near = (rng.integers(127, 151, 1_000_000, dtype=np.uint64).astype(np.uint32) << np.uint32(23)) | rng.integers(0, 2 ** 23, 1_000_000, dtype=np.uint64).astype(np.uint32)
    bits = np.ascontiguousarray(np.concatenate([edges, rand, near]))
    assert host.mwhost_lod_bits_mismatches(bits.ctypes.data, len(bits)) == 0


def host_render(lib, scene, nsamples, meshes, view="agent", render_agent=False, width=80, height=60):
    sc, keep = pyoracle.pack_scene(scene, width, height, nsamples, meshes, None, view, render_agent)
    rgb = np.zeros((height, width, 3), np.uint8)
    z16 = np.zeros((height, width), np.uint16)
    assert lib.mwhost_render(C.byref(sc), rgb.ctypes.data, z16.ctypes.data) == 0
    return rgb, z16


@pytest.mark.parametrize("case", gl_cases())
def test_engine_math_equals_the_reference_on_opengl(host, case):
    for k, (sc, fr) in load_gl(case).items():
        meshes = helpers.golden_meshes(sc)
        rgb, z16 = host_render(host, sc, 4, meshes)
        assert np.array_equal(z16, fr["z16"]), f"{case} frame {k}: depth"
        assert np.array_equal(rgb, fr["rgb"]), f"{case} frame {k}: {np.count_nonzero(rgb != fr['rgb'])} RGB values differ"
        top, _ = host_render(host, sc, 4, meshes, view="top", render_agent=True)
        assert np.array_equal(top, fr["top"]), f"{case} frame {k}: top view"


@pytest.mark.parametrize("case", ["hallway_s0", "pickup_dr_s1", "maze_s0", "sign_s0", "sidewalk_s0"])
def test_engine_math_equals_the_oracle_at_8_and_1_samples(host, case):
    """the sample counts llvmpipe cannot show: the engine's default (8, what the reference asks for) and 1"""
    for k, (sc, fr) in load_gl(case).items():
        meshes = helpers.golden_meshes(sc)
        for ns in (8, 1):
            want = pyoracle.render(sc, nsamples=ns, meshes=meshes)
            rgb, z16 = host_render(host, sc, ns, meshes)
            assert np.array_equal(z16, want["z16"]) and np.array_equal(rgb, want["rgb"]), f"{case} frame {k} at {ns} samples"


THREADS = min(16, len(os.sched_getaffinity(0)))


def restated_libm_missing():
    """Why this machine's libm is not the sinf / cosf that mw_glmath.h restates (glibc >= 2.28, the FMA variant), or None."""
    name, version = os.confstr("CS_GNU_LIBC_VERSION").split() if hasattr(os, "confstr") else ("", "0")
    if name != "glibc" or tuple(int(v) for v in version.split(".")[:2]) < (2, 28):
        return f"libm is {name} {version}: mw_glmath.h restates the sinf / cosf of glibc >= 2.28"
    if " fma " not in open("/proc/cpuinfo").read():
        return "the CPU lacks FMA: libm's sinf / cosf is not the FMA variant mw_glmath.h restates"
    return None


def sincosf_mismatches(host, sin_fn=None, cos_fn=None):
    bad = (C.c_uint64 * 512)()
    first = (C.c_uint32 * 512)()
    n = host.mwhost_sincosf_mismatches(sin_fn, cos_fn, THREADS, bad, first)
    binades = [(k, int(bad[k]), float(np.uint32(first[k]).view(np.float32))) for k in range(512) if bad[k]]
    return n, binades


def test_device_sinf_cosf_restate_glibc(host):
    """Mesa's glRotatef calls glibc's sinf / cosf; the device evaluates the same algorithm (mw_glmath.h sincosf_glibc):
    the host build of it equals libm's sinf and cosf, bit for bit, for ALL 2^32 floats (NaN as NaN) — the fast reduction
    below 120, the 4 / pi table above (an entity's dir grows with every turn of the agent that carries it), +-inf, NaN."""
    why = restated_libm_missing()
    if why:
        pytest.skip(why)
    n, binades = sincosf_mismatches(host)
    assert n == 0, (f"{n} floats differ; binades (sign|exponent, count, first input): {binades[:12]}")


def test_oracle_sinf_cosf_equal_libm_for_every_float(host):
    """The oracle's own restatement (oracle/mwo_geom.c mwo_sinf / mwo_cosf, written separately from the engine's and no
    longer calling libm above 120): libm's bits for all 2^32 floats."""
    why = restated_libm_missing()
    if why:
        pytest.skip(why)
    mwo = pyoracle.lib()
    n, binades = sincosf_mismatches(host, C.cast(mwo.mwo_sinf, C.c_void_p), C.cast(mwo.mwo_cosf, C.c_void_p))
    assert n == 0, (f"{n} floats differ; binades (sign|exponent, count, first input): {binades[:12]}")


def four_over_pi_bits(bits):
    """floor(4 / pi * 2^bits) from Machin's formula in Python integers (pi / 4 = 4 acot 5 - acot 239), 64 guard bits."""
    unity = 1 << (bits + 64)

    def acot(x):
        total = term = unity // x
        n, sign = 3, -1
        while term:
            term //= x * x
            total += sign * (term // n)
            sign, n = -sign, n + 2
        return total

    pi_unity = 4 * (4 * acot(5) - acot(239))
    return ((4 << bits) * unity) // pi_unity


def test_four_over_pi_tables_hold_the_bits_of_four_over_pi():
    """The large-argument reduction's 4 / pi (mw_glmath.h kInvPio4: entry i = floor(4 / pi * 2^(7 + 8 i)) mod 2^32; the
    oracle's FOUR_OVER_PI: floor(4 / pi * 2^191) in three words) against 4 / pi computed here, independently of both."""
    import re
    v = four_over_pi_bits(191)
    assert v.bit_length() == 192 and v >> 188 == 0xA                # 4 / pi = 1.27... = 0b1.0100010...
    src = open(os.path.join(ROOT, "miniworld_amd", "csrc", "mw_glmath.h")).read()
    table = re.search(r"kInvPio4\[24\] = \{([^}]*)\}", src).group(1)
    engine = [int(w.rstrip("uU"), 16) for w in re.findall(r"0x[0-9a-fA-F]+u?", table)]
    assert engine == [(v >> (184 - 8 * i)) & 0xFFFFFFFF for i in range(24)]
    src = open(os.path.join(ROOT, "oracle", "mwo_geom.c")).read()
    words = re.search(r"FOUR_OVER_PI\[3\] = \{([^}]*)\}", src).group(1)
    oracle = [int(w.rstrip("ulUL"), 16) for w in re.findall(r"0x[0-9a-fA-F]+(?:ull)?", words)]
    assert oracle == [(v >> 128) & (2 ** 64 - 1), (v >> 64) & (2 ** 64 - 1), v & (2 ** 64 - 1)]


def test_f64_headings_engine_equals_oracle_and_libm_within_one_ulp(host):
    """mw::sincos_det (mw_math.h, the engine's headings) against the oracle's mwo_sincos (oracle/mwo_math.c, written
    separately) bit for bit, and both within 1 ulp of libm's sin / cos, over the headings' domain |x| < 1e6: 2^26 inputs
    spread by exponent (2^-40 .. 2^19, both signs), the doubles nearest k pi / 4 (+-2 ulps) for every k there, zeros,
    subnormals, tiny values and 1e6 +- 1 ulp."""
    k = np.arange(-1273239, 1273240, dtype=np.float64)
    near = k * (np.pi / 4)                                           # within an ulp or so of the nearest double
    pts = [near]
    for side in (np.inf, -np.inf):
        x = near
        for _ in range(2):
            x = np.nextafter(x, side)
            pts.append(x)
    big = np.float64(1e6)
    tiny = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-300, 1e-20, 2.0 ** -27,
            -2.0 ** -27, 1e-8, 0.7853981633974483, 1.5707963267948966, 3.141592653589793]
    ends = [np.nextafter(big, 0.0), np.nextafter(big, np.inf), -np.nextafter(big, 0.0), -np.nextafter(big, np.inf)]
    extra = np.concatenate(pts + [np.array(tiny + ends)])
    extra = np.ascontiguousarray(extra[np.abs(extra) <= np.nextafter(big, np.inf)])
    assert len(extra) > 12_000_000
    out = (C.c_uint64 * 4)()
    ex = (C.c_double * 2)()
    host.mwhost_sincos_det_check(1 << 26, extra.ctypes.data, len(extra), THREADS, out, ex)
    assert out[0] == 0, f"{out[0]} inputs where the engine and the oracle differ, first {ex[0]!r}"
    if os.confstr("CS_GNU_LIBC_VERSION").split()[0] != "glibc":
        pytest.skip("libm is not glibc's: the 1-ulp bound is stated against glibc's sin / cos")
    assert out[1] <= 1 and out[2] <= 1 and out[3] == 0, (f"{out[3]} inputs more than 1 ulp from libm (engine up to {out[1]}, "
                                                         f"oracle up to {out[2]} ulps), first {ex[1]!r}")


def test_compact_clip_vertices_clip_like_full_ones(host):
    """The geometry kernel's work lists hold mwgl::ClipVert (clip, window, texture coordinates: a flat primitive's colour
    stays in registers); the clipper instantiated on them yields the same polygon as on full vertices, bit for bit."""
    rng = np.random.default_rng(5)
    host.mwhost_clip_variants_agree.restype = C.c_int
    clipped = 0
    for _ in range(4000):
        clip = rng.normal(0, 1.5, (3, 4)).astype(np.float32)
        clip[:, 3] = rng.uniform(-0.5, 2.5, 3).astype(np.float32)
        st = rng.uniform(-2, 2, (3, 2)).astype(np.float32)
        r = host.mwhost_clip_variants_agree(clip.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p), 80, 60)
        assert r >= 1, (clip, st)
        clipped += r > 1
    assert clipped > 500        # plenty of them really went through the planes


def test_edge_parallel_clipper_gives_the_serial_clippers_polygon(host):
    """The geometry kernel clips with eight lanes to a triangle, an edge of the polygon per lane, one step per frustum
    plane (mw_geom.hip); that algorithm, with the lanes as a loop over the same per-vertex functions, yields
    clip_triangle's polygon bit for bit — vertex count, order, clip / window / texture coordinates."""
    rng = np.random.default_rng(9)
    host.mwhost_edge_parallel_clip_agrees.restype = C.c_int
    clipped = many = 0
    for _ in range(6000):
        clip = rng.normal(0, 1.5, (3, 4)).astype(np.float32)
        clip[:, 3] = rng.uniform(-0.5, 2.5, 3).astype(np.float32)
        if rng.random() < 0.2:      # big triangles around the whole frustum: many planes, many vertices
            clip[:, :3] *= 6.0
        st = rng.uniform(-2, 2, (3, 2)).astype(np.float32)
        r = host.mwhost_edge_parallel_clip_agrees(clip.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p), 80, 60)
        assert r >= 1, (clip, st)
        clipped += r > 1
        many += r > 6
    assert clipped > 1000 and many > 20


def test_clearly_back_facing_triangles_never_leave_setup(host):
    """Big scenes drop polygons seen from behind while sifting (mw_geom.hip): `clearly_back` must only say yes where the
    setup's own test on the snapped vertices drops the triangle — also for slivers, sub-pixel triangles and vertices a hair
    apart, where snapping to 1/256 px can turn the area's sign."""
    rng = np.random.default_rng(10)
    host.mwhost_clearly_back_is_wrong.restype = C.c_int
    host.mwhost_clearly_back.restype = C.c_int
    said_yes = 0
    for k in range(30000):
        kind = k % 4
        if kind == 0:       # anything on the 80 x 60 frame
            w = rng.uniform(-5, 85, (3, 2))
        elif kind == 1:     # slivers: the third vertex a hair off the line through the first two
            a, b = rng.uniform(0, 80, 2), rng.uniform(0, 80, 2)
            t = rng.uniform(0, 1)
            n = np.array([-(b - a)[1], (b - a)[0]]) / max(np.linalg.norm(b - a), 1e-6)
            w = np.stack([a, b, a + t * (b - a) + n * rng.normal(0, 3e-3)])
        elif kind == 2:     # sub-pixel triangles
            w = rng.uniform(0, 80, 2) + rng.normal(0, 5e-3, (3, 2))
        else:               # on the snapping grid's half steps
            w = (np.round(rng.uniform(0, 80, (3, 2)) * 256) + rng.choice([0.0, 0.5, 0.4999, 0.5001], (3, 2))) / 256
        win = np.zeros((3, 4), np.float32)
        win[:, :2] = w
        win[:, 2] = 0.5; win[:, 3] = 1.0
        for ms in (0, 1):
            assert host.mwhost_clearly_back_is_wrong(win.ctypes.data_as(C.c_void_p), ms) == 0, (win, ms)
        said_yes += host.mwhost_clearly_back(win.ctypes.data_as(C.c_void_p))
    assert said_yes > 3000      # and it does say yes for ordinary back faces


def test_a_box_outside_the_frustum_holds_only_vertices_outside_it(host):
    """Big scenes sift boxes of eight polygons before the polygons (mw_geom.hip, mwgl::box_view): a plane the box is
    outside of (with box_view's margin) has every point of the box outside in transform_vertex's arithmetic — the box may
    stand for its polygons —, and a box in front of the eye bounds its points' window x and depth (the occlusion test)."""
    rng = np.random.default_rng(11)
    host.mwhost_box_cull_contradictions.restype = C.c_int
    culled = 0
    for k in range(3000):
        eye = np.array([rng.uniform(-30, 30), rng.uniform(0.5, 2.5), rng.uniform(-30, 30)])
        yaw, pitch = rng.uniform(0, 2 * np.pi), rng.uniform(-0.5, 0.5) * (k % 3 == 0)
        d = np.array([np.cos(yaw) * np.cos(pitch), np.sin(pitch), -np.sin(yaw) * np.cos(pitch)])
        at = eye + d
        c = eye + rng.normal(0, 12, 3) if k % 2 else eye + d * rng.uniform(-3, 30) + rng.normal(0, 4, 3)
        half = rng.uniform(0.05, 4, 3)
        # boxes that graze a frustum plane are the interesting ones: shift some so that a face lies almost in a plane
        mn, mx = (c - half).astype(np.float32), (c + half).astype(np.float32)
        n = 64
        pts = rng.uniform(mn, mx, (n, 3)).astype(np.float32)
        pts[:8] = [[(mx if (j >> a) & 1 else mn)[a] for a in range(3)] for j in range(8)]       # the corners themselves
        planes = C.c_int(0)
        bad = host.mwhost_box_cull_contradictions(eye.ctypes.data_as(C.c_void_p), at.ctypes.data_as(C.c_void_p), C.c_double(60.0), 80, 60,
                                                  mn.ctypes.data_as(C.c_void_p), mx.ctypes.data_as(C.c_void_p),
                                                  pts.ctypes.data_as(C.c_void_p), n, C.byref(planes))
        assert bad == 0, (eye, at, mn, mx, planes.value)
        culled += planes.value != 0
    assert 500 < culled < 2900      # both outcomes occur



# ------------------------------------------------------------------ asset preparation (mw_assets.h)

GL_META = np.load(os.path.join(HERE, "golden", "gl_meta.npz"))
MIP_NAMES = [str(n) for n in GL_META["mip_names"]]


@pytest.mark.parametrize("name", MIP_NAMES)
def test_engine_mip_pyramid_equals_glGenerateMipmap_in_footprint_records(host, name):
    """mwasset::build_pyramid — what mw_upload_texture uploads — for a shipped texture: every level's texels, decoded from the
    footprint records (channel = A >> 8 of a record's first row), are the oracle's level byte for byte and carry the checksum
    of the driver's own level (gl_meta.npz); every record holds what its layout promises — A = a * 256 + 128 and
    D = (right neighbour - a) mod 2^16 for the texel's row and for the row above, GL_REPEAT applied, packed
    (A_r | A_b << 16, D_r | D_b << 16, A_g, D_g); the descriptor's level table agrees with the level sizes."""
    import zlib
    rgb = np.ascontiguousarray(pyoracle.texture_rgb_bottom_up(name), np.uint8)
    h, w, _ = rgb.shape
    desc = np.zeros(4 + 16 * 8, np.uint32)
    n = host.mwhost_build_pyramid(rgb.ctypes.data, w, h, None, desc.ctypes.data)
    recs = np.zeros(n, np.uint32)
    assert host.mwhost_build_pyramid(rgb.ctypes.data, w, h, recs.ctypes.data, desc.ctypes.data) == n
    want_levels = pyoracle.mip_levels(rgb)
    crcs = [int(x) for x in GL_META["mip_crc"][MIP_NAMES.index(name)]]
    assert [int(x) for x in desc[:4]] == [w, h, len(want_levels), 0]
    assert all(c == 0 for c in crcs[len(want_levels):])

    def row(a, b):
        A, D = a * np.uint32(256) + np.uint32(128), (b - a) & np.uint32(0xFFFF)
        return np.stack([A[..., 0] | A[..., 2] << np.uint32(16), D[..., 0] | D[..., 2] << np.uint32(16), A[..., 1], D[..., 1]], -1)

    off, lw, lh = 0, w, h
    for l, want in enumerate(want_levels):
        lv = desc[4 + 8 * l:12 + 8 * l]
        assert [int(x) for x in lv[[0, 1, 2, 3, 6, 7]]] == [off, lw, lw - 1, lh - 1, lh, 0], f"{name} level {l}"
        assert [float(x) for x in lv[4:6].view(np.float32)] == [float(lw), float(lh)], f"{name} level {l}"
        R = recs[off * 8:(off + lw * lh) * 8].reshape(lh, lw, 2, 4)
        A = np.stack([R[:, :, 0, 0] & np.uint32(0xFFFF), R[:, :, 0, 2], R[:, :, 0, 0] >> np.uint32(16)], -1)
        assert np.all(A & np.uint32(0xFF) == 128) and np.all(A < 65536), f"{name} level {l}"
        tex = (A >> np.uint32(8)).astype(np.uint8)
        assert np.array_equal(tex, want), f"{name} level {l}: differs from the oracle's level"
        assert zlib.crc32(np.ascontiguousarray(tex).tobytes()) == crcs[l], f"{name} level {l}: differs from the driver's level"
        t = tex.astype(np.uint32)
        up = np.roll(t, -1, axis=0)
        assert np.array_equal(R[:, :, 0], row(t, np.roll(t, -1, axis=1))), f"{name} level {l}: the texel's row"
        assert np.array_equal(R[:, :, 1], row(up, np.roll(up, -1, axis=1))), f"{name} level {l}: the row above"
        off, lw, lh = off + lw * lh, max(1, lw // 2), max(1, lh // 2)
    assert off * 8 == n


MW_MESH_VCAP = 3568     # mw_asset_types.h


def shipped_meshes():
    """every mesh name ObjMesh can load from the asset pack: <base>_<colour> for the coloured ones, the rest by their own name"""
    from miniworld_amd import assets
    files = list(assets._pack_file().keys())
    coloured = [k[3:] for k in files if k.startswith("kd:")]
    bases = {n.split("_")[0] for n in coloured}
    return sorted(coloured + [k[4:] for k in files if k.startswith("obj:") and k[4:] not in bases])


def synthetic_mesh(kind):
    rng = np.random.default_rng(11)
    if kind == "over_the_cap":      # 1400 triangles of their own vertices: 4200 distinct positions
        verts = rng.uniform(-1, 1, (1400, 3, 3)).astype(np.float32)
        verts[::7, 0, 0] = 0.0
        verts[3::7, 1, 2] = -0.0
    else:                           # "signed_zeros": shared vertices that differ in the sign of a zero only, degenerate triangles
        grid = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
        grid[:20, 1] = 0.0
        grid[20:, :] = grid[:20, :]
        grid[20:, 1] = -0.0
        verts = grid[rng.integers(0, 40, (300, 3))]
    n = len(verts)
    norms = rng.uniform(-1, 1, (n, 3, 3)).astype(np.float32)
    return verts, norms, rng.uniform(0, 1, (n, 3, 2)).astype(np.float32), rng.uniform(0, 1, (n, 3, 3)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", shipped_meshes() + ["synthetic:over_the_cap", "synthetic:signed_zeros"])
def test_mesh_preparation_keeps_every_triangle_and_bounds_the_mesh(host, name):
    """mwasset::prepare_mesh — the host half of mw_upload_mesh — for every shipped mesh, a mesh with more distinct positions
    than MW_MESH_VCAP (no vertex table) and one whose vertices differ in the sign of a zero: the rasterisation order is a
    permutation; the entity kernel's stream and attribute rows are the input rows of that order's triangles bit for bit; the
    index table decodes through the vertex table to the same positions bit for bit; the table exists exactly when the
    positions fit; box, spheres and the last normal hold what the descriptor says."""
    if name.startswith("synthetic:"):
        verts, norms, texcs, colors = synthetic_mesh(name[10:])
        tex = 3
    else:
        from miniworld_amd.objmesh import ObjMesh
        m = ObjMesh.get(name)
        verts, norms, texcs, colors = m.verts, m.norms, m.texcs, m.colors
        tex = -1 if m.tex_variant is None else 5
    verts, norms, colors = (np.ascontiguousarray(x, np.float32) for x in (verts, norms, colors))
    texcs = np.ascontiguousarray(texcs, np.float32) if tex >= 0 else None
    n = len(verts)
    pos, nrm, rgb, uv = np.zeros((n, 10), np.float32), np.zeros((n, 9), np.float32), np.zeros((n, 9), np.float32), np.zeros((n, 6), np.float32)
    vtab, itab = np.full((MW_MESH_VCAP, 4), np.nan, np.float32), np.zeros((n, 2), np.uint32)
    stream, attr = np.zeros((n, 12), np.float32), np.zeros((n, 24), np.float32)
    desc = np.zeros(20, np.uint32)
    nverts = host.mwhost_prepare_mesh(verts.ctypes.data, norms.ctypes.data, texcs.ctypes.data if texcs is not None else None,
                                      colors.ctypes.data, n, tex, *(x.ctypes.data for x in (pos, nrm, rgb, uv, vtab, itab, stream, attr, desc)))
    want_uv = texcs.reshape(n, 6) if texcs is not None else np.zeros((n, 6), np.float32)
    # the pools' rows, drawing order
    order = bits(pos[:, 9]).astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(n))
    assert np.array_equal(bits(pos[:, :9]), bits(verts.reshape(n, 9)))
    assert np.array_equal(bits(nrm), bits(norms.reshape(n, 9))) and np.array_equal(bits(rgb), bits(colors.reshape(n, 9)))
    assert np.array_equal(bits(uv), bits(want_uv))
    # the entity kernel's rows, rasterisation order
    assert np.array_equal(bits(stream[:, :9]), bits(verts.reshape(n, 9)[order]))
    assert np.array_equal(bits(stream[:, 9]), order) and not bits(stream[:, 10:]).any()
    assert np.array_equal(bits(attr), bits(np.concatenate([norms.reshape(n, 9), colors.reshape(n, 9), want_uv], 1)[order]))
    # the tables
    distinct = len(np.unique(bits(verts.reshape(-1, 3)), axis=0))
    d_u, d_f = desc, desc.view(np.float32)
    assert (nverts == 0) == (distinct > MW_MESH_VCAP) and int(d_u[9]) == nverts
    if name == "synthetic:over_the_cap":
        assert nverts == 0
    if name == "synthetic:signed_zeros":
        assert distinct == 40 and len(np.unique(verts.reshape(-1, 3), axis=0)) == 20
    if nverts:
        assert nverts == distinct and len(np.unique(bits(vtab[:nverts, :3]), axis=0)) == distinct
        assert not bits(vtab[:nverts, 3]).any() and np.isnan(vtab[nverts:]).all()
        idx = np.stack([itab[:, 0] & 0xFFFF, itab[:, 0] >> 16, itab[:, 1] & 0xFFFF], 1).astype(np.int64)
        assert np.array_equal(itab[:, 1] >> 16, order) and idx.max() < nverts
        assert np.array_equal(bits(vtab[idx, :3]), bits(verts[order]))
    # the descriptor: ntris, tex, first, bound_bits, last_n[3], pad, vfirst, nverts, bmin[3], bmax[3], center[3], radius
    assert [int(d_u[0]), int(d_u[1].view(np.int32)), int(d_u[2]), int(d_u[7]), int(d_u[8])] == [n, tex, 0, 0, 0]
    assert np.array_equal(d_u[4:7], bits(norms[n - 1, 2]))
    v = verts.reshape(-1, 3)
    bmin, bmax, center, radius, bound = d_f[10:13], d_f[13:16], d_f[16:19], float(d_f[19]), float(d_f[3])
    assert np.all(v >= bmin) and np.all(v <= bmax)
    assert np.array_equal(bmin, v.min(0)) and np.array_equal(bmax, v.max(0))        # (min and max are exact)
    assert np.array_equal(center, np.float32(0.5) * (bmin + bmax))
    v64 = v.astype(np.float64)
    assert np.sqrt(((v64 - center.astype(np.float64)) ** 2).sum(1)).max() <= radius
    assert np.sqrt((v64 ** 2).sum(1)).max() <= bound
