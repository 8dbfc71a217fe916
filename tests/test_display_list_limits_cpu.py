"""Frames ON the raster kernels' capacity limits, CPU half: the synthetic scenes of tests/synthetic_scenes.py really sit where
the GPU tests (tests/test_gpu_display_list_limits.py) need them — by the oracle alone and by the definition of the kernels'
touch / full counts (tests/hostcheck's mwhost_rect_counts) —, and the engine's own arithmetic (mw_glmath.h / mw_frag.h on the
host) draws them like the oracle, bit for bit, at 8, 4 and 1 samples.  So a GPU mismatch on these frames is the kernels'
bookkeeping, not their arithmetic.

The limits (miniworld_amd/csrc/mw_rasterq.hip, mw_raster.hip, mw_shape.h):
  list length   q_cap: 48 records staged, 40 with a depth channel; the tile kernels' 16 / 32 / MW_LDS_RECS = 32 switches and
                the 64 / nvis packing (21 | 22, 32 | 33); the index arithmetic divides by every length from 1 up
  per tile      MWQ_SLOTS = 16 triangles listed: exactly 16 (a full list) and more (that tile's quads take the fallback class)
                s_tfull: 1, 2, 3 covering triangles merge their ids, more than 3 take the exact path over the tile's list
  per quad      four 6-bit ids: more than 4, 2 .. 4 with a covering triangle, 2 .. 4 without (painter classes, contested samples)
"""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers
import pyoracle
import synthetic_scenes as syn
from test_engine_math_cpu import build_host, host_render

W, H = 80, 60
SLAT_TILE = (7, 2)          # (tile row, tile column) the view axis runs through

# (station of synthetic_scenes.fence_world, agent_dir, cam_pitch, display list length): one pose per length 1 .. 70, found
# once by sweeping the heading with tests/hostcheck's mwhost_list_length; the same length at 8, 4 and 1 samples
LENGTH_POSES = [
    ("open", 1.215, 3.0, 1), ("open", -1.176, 0.0, 2), ("open", -1.21575, 0.0, 3), ("open", -1.11375, 0.0, 4),
    ("open", -1.15575, 0.0, 5), ("open", -1.04775, 0.0, 6), ("open", -1.092, 0.0, 7), ("open", -0.97725, 0.0, 8),
    ("open", -1.0245, 0.0, 9), ("open", -0.90375, 0.0, 10), ("open", -0.95325, 0.0, 11), ("open", -0.82725, 0.0, 12),
    ("open", -0.87825, 0.0, 13), ("open", -0.7485, 0.0, 14), ("open", -0.801, 0.0, 15), ("open", -0.669, 0.0, 16),
    ("open", -0.72225, 0.0, 17), ("open", -0.58875, 0.0, 18), ("open", -0.642, 0.0, 19), ("room", -2.083424, 0.0, 20),
    ("room", -2.090174, 0.0, 21), ("room", -2.048924, 0.0, 22), ("room", -2.074424, 0.0, 23), ("room", -1.973174, 0.0, 24),
    ("room", -2.039174, 0.0, 25), ("room", -1.930424, 0.0, 26), ("room", -1.961924, 0.0, 27), ("room", -1.885424, 0.0, 28),
    ("room", -1.918424, 0.0, 29), ("room", -1.835924, 0.0, 30), ("room", -1.871924, 0.0, 31), ("room", -1.784174, 0.0, 32),
    ("room", -1.822424, 0.0, 33), ("room", -1.727924, 0.0, 34), ("room", -1.769174, 0.0, 35), ("room", -1.668674, 0.0, 36),
    ("room", -1.712174, 0.0, 37), ("room", -1.606424, 0.0, 38), ("room", -1.652174, 0.0, 39), ("room", -1.540424, 0.0, 40),
    ("room", -1.550924, 0.0, 41), ("room", -1.472174, 0.0, 42), ("room", -1.521674, 0.0, 43), ("room", -1.401674, 0.0, 44),
    ("room", -1.452674, 0.0, 45), ("room", -1.328924, 0.0, 46), ("room", -1.381424, 0.0, 47), ("room", -1.256174, 0.0, 48),
    ("room", -1.309424, 0.0, 49), ("room", 0.222076, 0.0, 50), ("room", -1.235924, 0.0, 51), ("room", -1.182674, 0.0, 52),
    ("room", -1.197674, 0.0, 53), ("room", -1.109924, 0.0, 54), ("room", -1.162424, 0.0, 55), ("room", 0.129826, 0.0, 56),
    ("room", -1.097174, 0.0, 57), ("room", -0.737174, 0.0, 58), ("room", -1.038674, 0.0, 59), ("room", -1.090424, 0.0, 60),
    ("room", -0.969674, 0.0, 61), ("room", -1.019924, 0.0, 62), ("room", -0.951674, 0.0, 63), ("room", -0.950924, 0.0, 64),
    ("room", -0.878924, 0.0, 65), ("room", -0.395174, 0.0, 66), ("room", -0.347174, 0.0, 67), ("room", -0.376424, 0.0, 68),
    ("room", -0.300674, 0.0, 69), ("room", -0.319424, 0.0, 70),
    # the open fence whole and the lengths around the tile kernels' packing switches without the room behind them
    ("open", 0.0, 0.0, 32), ("open", -0.51, 0.0, 20), ("open", -0.5625, 0.0, 21),
]
LENGTHS = [p[3] for p in LENGTH_POSES]

# the display list of every pose of synthetic_scenes.crowded_world and overlap_world, 8 / 4 / 1 samples alike
SHAPE_LENGTHS = {"slats": 61, "slivers": 35, "slats16": 16, "interleaved": 14, "crossing": 4, "twins": 4,
                 "layers1": 4, "layers2": 8, "layers3": 12, "layers4": 16, "layers5": 20, "slats17": 17}


@functools.lru_cache(maxsize=None)
def hallway_frame():
    s0, tr, meta, obs = helpers.load_case("hallway_s0")
    return helpers.frame_scene(s0, obs[sorted(obs)[0]])


def wall_texture(base):
    return int(base["polys_tex"][2])


@functools.lru_cache(maxsize=None)
def shapes():
    """({"crowded" | "overlaps": world}, {name: scene}, {name: slice of its world's polygons})"""
    base = hallway_frame()
    worlds, scenes, parts = {}, {}, {}
    for which, build in (("crowded", syn.crowded_world), ("overlaps", syn.overlap_world)):
        worlds[which], poses, p = build(base, tex=wall_texture(base))
        scenes.update({name: syn.posed(worlds[which], pose) for name, pose in poses.items()})
        parts.update(p)
    return worlds, scenes, parts


def shape_batch(which):
    """(world, {name: scene}) of one of the two worlds"""
    worlds, scenes, _ = shapes()
    crowded = ("slats", "slivers", "slats16")
    names = crowded if which == "crowded" else [n for n in scenes if n not in crowded]
    return worlds[which], {n: scenes[n] for n in names}


@functools.lru_cache(maxsize=None)
def length_sweep():
    """(world, [scene of LENGTH_POSES[i]])"""
    base = hallway_frame()
    world, stations = syn.fence_world(base, tex=wall_texture(base))
    return world, [syn.posed(world, dict(stations[which], agent_dir=d, cam_pitch=pitch)) for which, d, pitch, _ in LENGTH_POSES]


MESH_FRAMES = (0, 60, 199)
MESH_LENGTHS = [37, 18, 16]         # without the meshes' own triangles, which the mesh entity kernel draws: the engine's count


@functools.lru_cache(maxsize=None)
def mesh_batch():
    """(world, scenes, slivers' polygons, fixture scene): the PickupObjects fixture with 18 slivers above the horizon of its first
    frame's camera; one scene per frame of MESH_FRAMES (only the first looks at the slivers from where they were built for)"""
    s0, tr, meta, obs = helpers.load_case("pickup_s0")
    world, pose, part = syn.mesh_world(helpers.frame_scene(s0, obs[MESH_FRAMES[0]]), tex=None)
    scenes = [syn.posed(world, pose)]
    for f in MESH_FRAMES[1:]:
        sc = dict(world)
        for k in ("agent_pos", "agent_dir", "ents_pos", "ents_dir", "ents_kind"):
            sc[k] = obs[f][k]
        scenes.append(sc)
    return world, scenes, part, s0


@functools.lru_cache(maxsize=None)
def host_library():
    lib = build_host()
    lib.mwhost_list_length.argtypes = [C.c_void_p]
    lib.mwhost_rect_counts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def host():
    return host_library()


def list_length(lib, scene, nsamples=8, width=W, height=H, meshes=None):
    sc, keep = pyoracle.pack_scene(scene, width, height, nsamples, meshes)
    return lib.mwhost_list_length(C.byref(sc))


def rect_counts(lib, scene, rw, rh, nsamples):
    """(touch, full) int32 [H / rh][W / rw]: the list's triangles that touch / cover each rectangle, by the definition"""
    sc, keep = pyoracle.pack_scene(scene, W, H, nsamples, None)
    touch, full = np.zeros((H // rh, W // rw), np.int32), np.zeros((H // rh, W // rw), np.int32)
    assert lib.mwhost_rect_counts(C.byref(sc), rw, rh, touch.ctypes.data, full.ctypes.data) >= 0
    return touch, full


def winners(prim, rw, rh):
    """distinct winning primitives per rectangle of the oracle's per-sample ids (-1: sky)"""
    out = np.zeros((H // rh, W // rw), np.int32)
    for y in range(H // rh):
        for x in range(W // rw):
            ids = np.unique(prim[y * rh:(y + 1) * rh, x * rw:(x + 1) * rw])
            out[y, x] = np.count_nonzero(ids >= 0)
    return out


@pytest.mark.parametrize("ns", [8, 4])
@pytest.mark.parametrize("name", ["slats", "slivers"])
def test_slats_overflow_one_tile_between_tiles_that_do_not(host, name, ns):
    """24 slats / 22 slivers in the room: the oracle shows at least 17 primitives winning samples of ONE tile (so more than
    MWQ_SLOTS triangles touch it) while other tiles of the frame show at most 4, and a quad with at least 5 (more than its four
    ids); by the kernels' own counts that tile is over 16 and its neighbours in the tile row are not.  The slats' list (61) is
    longer than the quad kernel stages — at 8 samples the tile code draws that env —, the slivers' (35) is not: there the quad
    kernel's own per-tile overflow runs, with and without a depth channel."""
    _, scenes, parts = shapes()
    assert (SHAPE_LENGTHS[name] <= 40) == (name == "slivers") and SHAPE_LENGTHS["slats"] > 48
    prim = pyoracle.render(scenes[name], nsamples=ns, want_prim=True)["prim"]
    per_tile, per_quad = winners(prim, 16, 4), winners(prim, 2, 2)
    assert per_tile[SLAT_TILE] >= 17 and per_tile[SLAT_TILE] == per_tile.max()
    assert per_tile.min() <= 4 and np.count_nonzero(per_tile <= 4) > W // 16 * (H // 4) // 2
    assert per_quad.max() >= 5
    touch, full = rect_counts(host, scenes[name], 16, 4, ns)
    row = touch[SLAT_TILE[0]]
    assert row[SLAT_TILE[1]] > 16 and all(row[x] <= 16 for x in range(W // 16) if x != SLAT_TILE[1])


@pytest.mark.parametrize("ns", [8, 4])
def test_eight_slats_fill_one_tiles_list_exactly(host, ns):
    """8 slats and nothing else: exactly 16 triangles in the list, all 16 touch the tile of the view axis and no tile has
    more — `slot < MWQ_SLOTS` with a full list, `s_tcnt[t] > MWQ_SLOTS` false by one.  Its quads hold up to 8: more than four ids."""
    _, scenes, parts = shapes()
    sc = scenes["slats16"]
    assert list_length(host, sc, ns) == 16
    touch, full = rect_counts(host, sc, 16, 4, ns)
    assert touch[SLAT_TILE] == 16 and touch.max() == 16 and np.count_nonzero(touch == 16) == 1
    qtouch, _ = rect_counts(host, sc, 2, 2, ns)
    assert qtouch.max() > 4
    prim = pyoracle.render(sc, nsamples=ns, want_prim=True)["prim"]
    shown = np.unique(prim[prim >= 0])
    assert shown.tolist() == list(range(parts["slats16"].start, parts["slats16"].stop))       # every slat wins samples


@pytest.mark.parametrize("ns", [8, 4])
def test_eight_slats_and_a_sliver_are_one_too_many_for_a_tile(host, ns):
    """17 triangles, all on the tile of the view axis and nowhere else as many: the smallest count that overflows the list —
    a kernel that listed 16 and forgot to fall back would lose exactly one of them, and every one of the 9 wins samples"""
    _, scenes, parts = shapes()
    sc = scenes["slats17"]
    assert list_length(host, sc, ns) == 17
    touch, _ = rect_counts(host, sc, 16, 4, ns)
    assert touch[SLAT_TILE] == 17 and np.count_nonzero(touch > 16) == 1
    prim = pyoracle.render(sc, nsamples=ns, want_prim=True)["prim"]
    assert np.unique(prim[prim >= 0]).tolist() == list(range(parts["slats17"].start, parts["slats17"].stop))


@pytest.mark.parametrize("ns", [8, 4])
def test_layers_cover_every_tile_one_to_five_times(host, ns):
    """k parallel quads over the whole frame (each clips to four triangles): every layer alone leaves no sample to the sky;
    together k triangles cover a tile in full where no diagonal crosses it (s_tfull's count: 1, 2, 3 merge ids, 4 and 5
    are past its three), 3 k touch it where the diagonals meet; the layer drawn last is the nearest and wins everywhere."""
    world, scenes, parts = shapes()
    for k in syn.LAYER_COUNTS:
        name = f"layers{k}"
        part = parts[name]
        for j in range(part.start, part.stop):
            alone = pyoracle.render(syn.only(scenes[name], slice(j, j + 1)), nsamples=ns, want_prim=True)["prim"]
            assert alone.min() == 0 and alone.max() == 0, f"layer {j - part.start} of {k} leaves sky"
        touch, full = rect_counts(host, scenes[name], 16, 4, ns)
        assert full.max() == k and np.count_nonzero(full == k) >= 20 and touch.max() == 3 * k and touch.min() == k
        prim = pyoracle.render(scenes[name], nsamples=ns, want_prim=True)["prim"]
        assert prim.min() == prim.max() == part.stop - 1


@pytest.mark.parametrize("ns", [8, 4])
def test_interleaved_crossing_and_twin_quads_contest_samples(host, ns):
    """interleaved slats: quads that 2 .. 4 triangles touch and none covers (the painter classes), some of them with two
    winners (contested: the exact list), and quads with more than 4; the crossing pair: pixels whose samples go to both quads,
    quads that both cover; the twins: the one drawn first wins every sample (GL_LESS)."""
    _, scenes, parts = shapes()
    qtouch, qfull = rect_counts(host, scenes["interleaved"], 2, 2, ns)
    painter = (qtouch >= 2) & (qtouch <= 4) & (qfull == 0)
    per_quad = winners(pyoracle.render(scenes["interleaved"], nsamples=ns, want_prim=True)["prim"], 2, 2)
    assert np.count_nonzero(painter) >= 20 and np.count_nonzero(painter & (per_quad >= 2)) >= 5 and (qtouch > 4).any()
    assert {int(qtouch[painter].min()), int(qtouch[painter].max())} == {2, 4}

    prim = pyoracle.render(scenes["crossing"], nsamples=ns, want_prim=True)["prim"]
    a, b = parts["crossing"].start, parts["crossing"].start + 1
    both = (prim == a).any(axis=2) & (prim == b).any(axis=2)
    assert np.count_nonzero(both) >= 8 and not (prim[both] < 0).any()          # pixels inside both quads, split between them
    qtouch, qfull = rect_counts(host, scenes["crossing"], 2, 2, ns)
    assert np.count_nonzero((qtouch >= 2) & (qtouch <= 4) & (qfull == 2)) > 100

    prim = pyoracle.render(scenes["twins"], nsamples=ns, want_prim=True)["prim"]
    assert np.unique(prim).tolist() == [-1, parts["twins"].start]
    _, qfull = rect_counts(host, scenes["twins"], 2, 2, ns)
    assert qfull.max() == 2


@pytest.mark.parametrize("ns", [8, 4, 1])
def test_committed_poses_hold_every_list_length_from_1_to_70(host, ns):
    _, scenes = length_sweep()
    assert [list_length(host, sc, ns) for sc in scenes] == LENGTHS
    assert set(range(1, 71)) <= set(LENGTHS) and len(scenes) <= 80
    _, shape_scenes, _ = shapes()
    assert {name: list_length(host, sc, ns) for name, sc in shape_scenes.items()} == SHAPE_LENGTHS


def test_mesh_fixture_keeps_the_slats_away_from_the_meshes(host):
    """the PickupObjects batch: the slivers' tile holds more than 16 triangles and no mesh triangle wins a sample within a tile
    row of it (the meshes lie on the floor, below the horizon; the slivers above), in a list the quad kernel stages with a
    depth channel too — the quad kernel draws the slivers"""
    world, scenes, part, s0 = mesh_batch()
    meshes = helpers.golden_meshes(s0)
    for sc, want in zip(scenes, MESH_LENGTHS):
        no_mesh = dict(sc, ents_kind=np.where(np.asarray(sc["ents_kind"]) == 2, 0, sc["ents_kind"]).astype(np.int32))
        assert list_length(host, no_mesh, 8, meshes=meshes) == want
    assert 16 < MESH_LENGTHS[0] <= 40
    prim = pyoracle.render(scenes[0], want_prim=True, meshes=meshes)["prim"]
    n_polys = len(world["polys_nv"])
    slat_rows = np.where(((prim >= part.start) & (prim < part.stop)).any(axis=(1, 2)))[0]
    mesh_rows = np.where((prim >= n_polys + 6 * np.count_nonzero(np.asarray(world["ents_kind"]) == 1)).any(axis=(1, 2)))[0]
    assert len(slat_rows) > 0 and 16 <= slat_rows.min() and slat_rows.max() <= 19 and len(mesh_rows) > 0 and mesh_rows.min() >= 24
    assert winners(prim, 16, 4)[4, 2] >= 17


def synthetic_frames():
    out = [(f"shapes/{name}", sc, None) for name, sc in shapes()[1].items()]
    out += [(f"length {n}", sc, None) for n, sc in zip(LENGTHS, length_sweep()[1])]
    world, scenes, part, s0 = mesh_batch()
    return out + [(f"meshes/{f}", sc, helpers.golden_meshes(s0)) for f, sc in zip(MESH_FRAMES, scenes)]


@pytest.mark.parametrize("ns", [8, 4, 1])
def test_engine_math_equals_the_oracle_on_the_synthetic_scenes(host, ns):
    """thin slats, interpenetrating and coplanar quads, quads far larger than the frame, textured and flat: mw_glmath.h /
    mw_frag.h on the host against the oracle, RGB and the 16-bit depth bit for bit"""
    for what, sc, meshes in synthetic_frames():
        want = pyoracle.render(sc, nsamples=ns, meshes=meshes)
        rgb, z16 = host_render(host, sc, ns, meshes)
        assert np.array_equal(z16, want["z16"]), f"{what} at {ns} samples: depth"
        assert np.array_equal(rgb, want["rgb"]), f"{what} at {ns} samples: {np.count_nonzero(rgb != want['rgb'])} RGB values differ"


def test_engine_math_equals_the_oracle_off_the_grid(host):
    """the shapes at 72 x 58, the frame the GPU test draws through the ragged tile kernels; its lists are other lists (the
    slats' env still holds more than the quad kernel's 48 records)"""
    _, scenes, _ = shapes()
    for name, sc in scenes.items():
        want = pyoracle.render(sc, width=72, height=58)
        rgb, z16 = host_render(host, sc, 8, None, width=72, height=58)
        assert np.array_equal(z16, want["z16"]) and np.array_equal(rgb, want["rgb"]), name
    assert list_length(host, scenes["slats"], 8, 72, 58) > 48


def test_every_synthetic_polygon_has_its_own_colour():
    for world in (*shapes()[0].values(), length_sweep()[0], mesh_batch()[0]):
        n = len(hallway_frame()["polys_nv"]) if world is not mesh_batch()[0] else mesh_batch()[2].start
        rgb = np.asarray(world["polys_rgb"])[n:]
        assert len(np.unique(np.round(rgb * 255).astype(int), axis=0)) == len(rgb)
