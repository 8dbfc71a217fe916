"""Frames ON the raster kernels' list, tile and quad capacity limits (tests/synthetic_scenes.py; what each scene sits on and
that it does is pinned without a GPU in tests/test_display_list_limits_cpu.py), through every raster path, against the CPU
oracle: RGB and the depth map bit for bit, mw_check clean, the path and the display list lengths as pinned.  No experiment
flags: the frames themselves take the kernels' side paths — a display list of 41 .. 48 triangles beside a depth channel
whose LDS plan holds 40, one tile over its 16 slots between tiles that are not, four and five triangles covering a tile."""
import functools

import numpy as np
import pytest

import helpers
import test_display_list_limits_cpu as cpu

pytestmark = pytest.mark.gpu


def batch(name):
    """(world, scenes, names, lengths at 80 x 60, meshes for the oracle)"""
    if name in ("crowded", "overlaps"):
        world, scenes = cpu.shape_batch(name)
        return world, list(scenes.values()), list(scenes), [cpu.SHAPE_LENGTHS[n] for n in scenes], None
    if name == "lengths":
        world, scenes = cpu.length_sweep()
        return world, scenes, [f"{which} fence, length {n}" for which, _, _, n in cpu.LENGTH_POSES], cpu.LENGTHS, None
    world, scenes, _, s0 = cpu.mesh_batch()
    return world, scenes, [f"frame {f}" for f in cpu.MESH_FRAMES], cpu.MESH_LENGTHS, helpers.golden_meshes(s0)


@functools.lru_cache(maxsize=None)
def wanted(name, ns, width, height):
    """the oracle's frames of a batch: rendered once, shared by the tests, never written to"""
    import pyoracle
    world, scenes, _, _, meshes = batch(name)
    return [pyoracle.render(sc, width=width, height=height, nsamples=ns, meshes=meshes) for sc in scenes]


def draw_and_compare(name, want_path, msaa=8, with_depth=True, max_visible=64, width=80, height=60, lengths=None, shape=None):
    """shape: keyword arguments of Engine.debug_set_launch_shape, applied to the new engine (tests/test_gpu_launch_shapes.py)"""
    import torch
    world, scenes, names, pinned, _ = batch(name)
    lengths = pinned if lengths is None else lengths
    assert len(scenes) <= 80
    eng = helpers.make_engine_for_scene(world, len(scenes), msaa=msaa, max_visible=max_visible, width=width, height=height)
    if shape is not None:
        eng.debug_set_launch_shape(**shape)
    eng.set_state(helpers.scene_state_arrays(scenes))
    rgb = torch.zeros((len(scenes), height, width, 3), dtype=torch.uint8, device="cuda")
    depth = torch.zeros((len(scenes), height, width, 1), dtype=torch.float32, device="cuda") if with_depth else None
    eng.render(rgb, depth)
    eng.check()
    path, got_lengths = eng.raster_path(), eng.list_lengths().tolist()
    rgb = rgb.cpu().numpy()
    depth = depth.cpu().numpy() if with_depth else None
    eng.close()
    assert path == want_path, path
    if lengths is not None:
        assert got_lengths == lengths
    bad = []
    for i, want in enumerate(wanted(name, msaa, width, height)):
        n_rgb = int(np.count_nonzero(rgb[i] != want["rgb"]))
        n_z = int(np.count_nonzero(depth[i] != want["depth"])) if with_depth else 0
        if n_rgb or n_z:
            bad.append(f"{names[i]} (list of {got_lengths[i]}): {n_rgb} RGB values, {n_z} depths differ")
    assert not bad, "; ".join(bad)


# name -> (msaa, environment, depth channel, max_visible, the path mw_raster_path must report)
CONFIGS = {
    "quad8-depth40": (8, {}, True, 64, "PATH_QUAD"),
    "quad8-rgb48": (8, {}, False, 64, "PATH_QUAD"),
    "quad4-depth40": (4, {}, True, 64, "PATH_QUAD"),
    "quad4-rgb48": (4, {}, False, 64, "PATH_QUAD"),
    "tile-depth": (8, {"MW_K2Q": "0"}, True, 64, "PATH_TILE"),
    "tile-rgb": (8, {"MW_K2Q": "0"}, False, 64, "PATH_TILE"),
    "generic4": (4, {"MW_GENERIC_RASTER": "1"}, True, 64, "PATH_GENERIC"),
    "generic1": (1, {}, True, 64, "PATH_GENERIC"),
    "big-depth": (8, {}, True, 65, "PATH_TILE"),
    "big-rgb": (8, {}, False, 65, "PATH_TILE"),
}


def run_config(name, config, monkeypatch, shape=None):
    from miniworld_amd import engine as E
    msaa, env, with_depth, max_visible, path = CONFIGS[config]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    draw_and_compare(name, getattr(E, path), msaa=msaa, with_depth=with_depth, max_visible=max_visible, shape=shape)


@pytest.mark.parametrize("config", CONFIGS)
def test_every_list_length_from_1_to_70(config, monkeypatch):
    """One env per display list length 1 .. 70 (a fence of small quads moved in and out of the frustum by the heading, with and
    without the room): the quad kernel's 40 / 48 staged records with 39 .. 49 on both sides of either — longer lists through
    the tile code in place at 8 samples, the scratch-staged exact path at 4 —, its division by the length; the tile kernels'
    16 / 32 switches, the 64 / nvis packing and the records in LDS or in place; the visiting order of the big-scene kernels."""
    assert set(range(39, 50)) <= set(cpu.LENGTHS)
    run_config("lengths", config, monkeypatch)


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("which", ["crowded", "overlaps"])
def test_tiles_and_quads_at_their_capacity(which, config, monkeypatch):
    """One env per scene, in two worlds of at most 64 polygons: 24 slats and 22 slivers (one tile far over its 16 slots between tiles of the room, in a list of 61 —
    longer than the quad kernel stages — and in one of 35), 8 slats (16 triangles on a
    tile, no more; quads of 8), interleaved slats (painter classes with contested samples), the crossing pair and the coplanar
    twins (the exact path; GL_LESS keeps the first drawn), 1 .. 5 layers (1 .. 5 triangles covering a tile)."""
    run_config(which, config, monkeypatch)


@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("which", ["crowded", "overlaps"])
def test_a_frame_off_the_grid(which, with_depth):
    """the same scenes at 72 x 58 (padding right of column 71 and below row 57): the ragged tile kernels"""
    from miniworld_amd import engine as E
    lengths = [cpu.list_length(cpu.host_library(), sc, 8, 72, 58) for sc in batch(which)[1]]
    draw_and_compare(which, E.PATH_TILE, with_depth=with_depth, width=72, height=58, lengths=lengths)


@pytest.mark.parametrize("with_depth", [True, False])
def test_slats_beside_mesh_entities(with_depth):
    """PickupObjects with 18 slivers above the horizon, outside every mesh's tile rectangle, in a list of 37: the quad kernel
    draws the slivers' tile (over its 16 slots) while the tiles a mesh can touch go through the tile code"""
    from miniworld_amd import engine as E
    draw_and_compare("meshes", E.PATH_QUAD_MESH, with_depth=with_depth)
