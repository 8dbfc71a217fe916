"""The quad kernel's binning (mw_rasterq.hip, phases A and B: a lane per (triangle, tile row) stepping the edge values over the tile
columns, a few lanes per partial (tile, triangle) event stepping over its quads; miniworld_amd/csrc/mw_quad_bin.h, whose arithmetic
tests/test_quad_binning_cpu.py pins without a GPU) at the smallest shapes at which its loops can go wrong, against the CPU oracle at
the same size and sample count: RGB and the depth map bit for bit, mw_check clean, the raster path as the launch policy states it.

Shapes: one tile column (W = 16), one tile row (H = 4), a single tile, 32 x 8, 80 x 60, seven tile columns (112 x 48) and the largest
frame of the quad kernel, 96 x 64 — its LDS plan (q_plan) must fit 64 KB beside W H <= 8192, and at 128 x 64 it does not (80 KB with
a depth channel).  No frame 128 pixels wide or high is the quad kernel's, or the tile kernels': an edge across the whole frame has
the coefficient 2^23 there, one past the signed 24 bits of the kernels' multiplies (miniworld_amd/csrc/mw_edge_rec.h,
tests/test_edge_limits_cpu.py; FourRooms' frame 150 at 128 x 48 holds one), so the launch policy gives 128 x 64, 128 x 48 and their like to
the generic-resolution kernels: 128 x 64 is drawn and compared here all the same, the others with scenes that sit on that limit in
tests/test_gpu_edge_limits.py.  8 and 4 samples, with and without a depth output (40 / 48 staged records).  Scenes: fixture frames (Hallway, OneRoom, FourRooms; PickupObjects: the mesh part mode) and
tests/synthetic_scenes.py — a list of one triangle, lists at capacity, slats and slivers (more than 16 triangles on a tile: the
fallback class; many partial events per tile), a quad whose edges lie exactly on a tile's borders —, the experiment flags that force
the exact, fallback and over-capacity paths, and the list form of the kernel (final observations)."""
import functools

import numpy as np
import pytest

import helpers
import synthetic_scenes as syn
import test_display_list_limits_cpu as cpu

pytestmark = pytest.mark.gpu

QUAD_SIZES = [(16, 60), (80, 4), (16, 4), (32, 8), (80, 60), (112, 48), (96, 64)]
PAST_THE_LDS_PLAN = (128, 64)
BORDER_TILE = (7, 2)            # (tile row, tile column) of the 80 x 60 frame the view axis runs through: rows 28 .. 31, columns 32 .. 47


@functools.lru_cache(maxsize=None)
def border_world():
    """A station with one quad, 16 x 4 pixels of the 80 x 60 frame at 1 m, centred on the view axis: its four edges lie on the borders
    of tile (7, 2) (vertices are snapped to 1 / 256 pixel: on them exactly)."""
    base = cpu.hallway_frame()
    px = 2.0 * np.tan(np.radians(float(base["cam_fov_y"])) / 2.0) / 60.0
    world, poses, parts = syn._world(base, cpu.wall_texture(base), [("border", syn._station(0), lambda e, f, r: [syn.quad(e + f * 1.0, r, syn.UP, 8 * px, 2 * px)])])
    return world, syn.posed(world, poses["border"])


@functools.lru_cache(maxsize=None)
def one_triangle_world():
    """A station with one triangle, 0.6 m wide and 0.4 m high at 1 m (31 x 21 pixels of the 80 x 60 frame), and nothing else in the
    world (synthetic_scenes.only): a display list of one entry"""
    base = cpu.hallway_frame()
    def tri(e, f, r):
        q = syn.quad(e + f * 1.0, r, syn.UP, 0.3, 0.2)
        return [np.stack([q[0], q[1], 0.5 * (q[2] + q[3])])]
    world, poses, parts = syn._world(base, cpu.wall_texture(base), [("only", syn._station(0), tri)])
    return syn.only(world, parts["only"]), syn.posed(syn.only(world, parts["only"]), poses["only"])


@functools.lru_cache(maxsize=None)
def batch(name):
    """(world, scenes, meshes for the oracle) — at most 8 envs.  "filling/WxH": synthetic_scenes.frame_filling_world for that frame's
    proportion, every part"""
    if name.startswith("filling/"):
        W, H = map(int, name[len("filling/"):].split("x"))
        base = cpu.hallway_frame()
        world, poses, parts = syn.frame_filling_world(base, aspect=W / H, tex=cpu.wall_texture(base))
        return world, [syn.posed(world, poses[part]) for part in syn.FILLING_PARTS], None
    if name in ("crowded", "overlaps"):
        world, scenes = cpu.shape_batch(name)
        return world, list(scenes.values())[:8], None
    if name == "only":
        world, scene = one_triangle_world()
        return world, [scene], None
    if name == "border":
        world, scene = border_world()
        return world, [scene], None
    s0, tr, meta, obs = helpers.load_case(name + "_s0")
    scenes = [helpers.frame_scene(s0, obs[f]) for f in sorted(obs)[:3]]
    return s0, scenes, helpers.golden_meshes(s0) if name == "pickup" else None


SYNTHETIC = ("crowded", "overlaps", "only", "border")


def synthetic(name):
    return name in SYNTHETIC or name.startswith("filling/")


MAX_VISIBLE = 64                # of the synthetic worlds' engines (at most 64 polygons): a small scene, no visiting order


@functools.lru_cache(maxsize=None)
def sized_batch(name, msaa, width, height):
    """the batch's scenes whose display list the engine holds at this size (a synthetic world seen through a frame of another
    shape can list more than MAX_VISIBLE triangles: by the host's own count, not by anything the kernels give)"""
    world, scenes, meshes = batch(name)
    if synthetic(name):
        scenes = [sc for sc in scenes if cpu.list_length(cpu.host_library(), sc, msaa, width, height) <= MAX_VISIBLE]
    assert scenes
    return world, scenes, meshes


@functools.lru_cache(maxsize=None)
def wanted(name, msaa, width, height):
    """the oracle's frames of a batch: rendered once, shared by the tests, never written to"""
    import pyoracle
    world, scenes, meshes = sized_batch(name, msaa, width, height)
    return [pyoracle.render(sc, width=width, height=height, nsamples=msaa, meshes=meshes) for sc in scenes]


def draw_and_compare(name, width, height, msaa, with_depth, want_path):
    import torch
    from miniworld_amd import engine as E
    world, scenes, _ = sized_batch(name, msaa, width, height)
    assert len(scenes) <= 8
    eng = helpers.make_engine_for_scene(world, len(scenes), msaa=msaa, width=width, height=height, max_visible=MAX_VISIBLE if synthetic(name) else None)
    eng.set_state(helpers.scene_state_arrays(scenes))
    rgb = torch.zeros((len(scenes), height, width, 3), dtype=torch.uint8, device="cuda")
    depth = torch.zeros((len(scenes), height, width, 1), dtype=torch.float32, device="cuda") if with_depth else None
    eng.render(rgb, depth)
    eng.check()
    path, lengths = eng.raster_path(), eng.list_lengths().tolist()
    rgb = rgb.cpu().numpy()
    depth = depth.cpu().numpy() if with_depth else None
    eng.close()
    assert path == getattr(E, want_path), (name, path)
    bad = []
    for i, want in enumerate(wanted(name, msaa, width, height)):
        n_rgb = int(np.count_nonzero(rgb[i] != want["rgb"]))
        n_z = int(np.count_nonzero(depth[i] != want["depth"])) if with_depth else 0
        if n_rgb or n_z:
            bad.append(f"{name} {i} (list of {lengths[i]}): {n_rgb} RGB values, {n_z} depths differ")
    assert not bad, "; ".join(bad)
    return lengths


@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("msaa", [8, 4])
@pytest.mark.parametrize("size", QUAD_SIZES)
def test_frames_of_every_shape_equal_the_oracle(size, msaa, with_depth):
    """fixture frames, the lists at capacity, the slats and slivers and the tile-sized quad at every shape of the quad kernel"""
    for name in ("hallway", "oneroom", "fourrooms", "crowded", "overlaps", "border"):
        draw_and_compare(name, size[0], size[1], msaa, with_depth, "PATH_QUAD")


@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("msaa", [8, 4])
def test_the_frame_past_the_lds_plan_takes_other_kernels(msaa, with_depth):
    """128 x 64 is W H = 8192, but the workgroup's plan needs 80 KB of LDS (66 KB without depth; the engine asks with), and a frame 128
    pixels wide can hold an edge coefficient past the tile kernels' 24-bit multiplies too: mw_create gives the frame to the
    generic-resolution kernels at either sample count — the same frames"""
    W, H = PAST_THE_LDS_PLAN
    for name in ("hallway", "crowded"):
        draw_and_compare(name, W, H, msaa, with_depth, "PATH_GENERIC")


@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("size", [(80, 60), (32, 8)])
def test_mesh_part_mode(size, with_depth):
    """PickupObjects: the quad kernel draws the tiles no mesh entity can touch, from the same binning"""
    draw_and_compare("pickup", size[0], size[1], 8, with_depth, "PATH_QUAD_MESH")


@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("msaa", [8, 4])
def test_a_list_of_one_triangle(msaa, with_depth):
    for W, H in ((80, 60), (16, 4)):
        lengths = draw_and_compare("only", W, H, msaa, with_depth, "PATH_QUAD")
        if (W, H) == (80, 60):
            assert lengths == [1]
    assert int((wanted("only", msaa, 80, 60)[0]["z16"] != 65535).sum()) > 0          # the sliver does cover pixels


@pytest.mark.parametrize("msaa", [8, 4])
def test_a_quad_whose_edges_lie_on_a_tiles_borders(msaa):
    """the oracle: the quad owns every sample of tile (7, 2) and none outside it; the kernel: a covered tile among untouched ones"""
    import pyoracle
    world, scene = border_world()
    prim = pyoracle.render(scene, nsamples=msaa, want_prim=True)["prim"]
    inside = np.zeros(prim.shape[:2], bool)
    ty, tx = BORDER_TILE
    inside[4 * ty:4 * ty + 4, 16 * tx:16 * tx + 16] = True
    assert (prim[inside] >= 0).all() and (prim[~inside] < 0).all()
    assert draw_and_compare("border", 80, 60, msaa, True, "PATH_QUAD") == [2]


@pytest.mark.parametrize("msaa", [8, 4])
@pytest.mark.parametrize("flags", [4, 8, 0x80])
def test_the_same_frames_under_the_experiment_flags(flags, msaa, monkeypatch):
    """MW_DEBUG_FLAGS 4: every quad through the exact path; 8: every quad in the fallback class; 0x80: records hold 8 triangles (the
    over-capacity paths) — results do not depend on the class the binning files a quad under"""
    monkeypatch.setenv("MW_DEBUG_FLAGS", str(flags))
    for name in ("hallway", "oneroom", "fourrooms", "crowded", "overlaps", "border", "only"):
        draw_and_compare(name, 80, 60, msaa, True, "PATH_QUAD")
    if msaa == 8:
        draw_and_compare("pickup", 80, 60, msaa, True, "PATH_QUAD_MESH")


@pytest.mark.parametrize("msaa", [8, 4])
def test_a_list_form_frame(msaa, monkeypatch):
    """Final observations (mw_set_final_obs): the finished envs' terminal frames are drawn by the list form of the kernel; they equal the
    oracle's frames of the state an engine without auto-reset holds after the same actions."""
    import torch
    import pyoracle
    from miniworld_amd import engine as E
    from miniworld_amd import envs
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n, steps = 8, 3

    class Short(envs.Hallway):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.max_episode_steps = steps
    Short.__name__ = Short.__qualname__ = "Hallway"
    monkeypatch.setattr(envs, "Hallway", Short)
    A = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, seed=34, msaa=msaa, want_depth=True, final_obs=True)
    C = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, seed=34, msaa=msaa, want_depth=True, autoreset=False)
    A.reset()
    C.reset()
    rng = np.random.default_rng(34)
    for t in range(steps):
        act = torch.as_tensor(rng.integers(0, 3, n), dtype=torch.int32, device="cuda")
        A.final_obs.fill_(0xA5)
        A.step(act)
        _, _, term, trunc = C.step(act)
    done = (term | trunc).cpu().numpy().astype(bool)
    assert done.all()                                   # every env's episode ends at the step limit: a list of all eight
    assert A.engine.raster_path() == E.PATH_QUAD
    final, final_depth = A.final_obs.cpu().numpy(), A.final_depth.cpu().numpy()
    st = C.engine.get_state()
    for i in range(n):
        want = pyoracle.render(helpers.scene_of_vec_env(C, st, i), nsamples=msaa)
        assert np.array_equal(final[i], want["rgb"]), f"env {i}: {np.count_nonzero(final[i] != want['rgb'])} RGB values differ"
        assert np.array_equal(final_depth[i], want["depth"]), f"env {i}: depth differs"
    for v in (A, C):
        v.engine.check()
        v.close()
