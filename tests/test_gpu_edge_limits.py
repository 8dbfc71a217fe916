"""Frames ON the limit of the raster kernels' 24-bit edge coefficients, on the device.  The tile and quad kernels evaluate an edge at a
pixel as mul24(A, px) + mul24(B, gy) + C with A = -256 dcdx and B = 256 dcdy (miniworld_amd/csrc/mw_edge_rec.h); vertices are snapped
inside [0, W] x [0, H], so a frame 128 pixels wide can hold B = +2^23 (an edge across the whole width, dcdy = +256 W) and one 128 high
A = +2^23 (dcdx = -256 H): one past the signed 24 bits.  tests/test_edge_limits_cpu.py pins the arithmetic without a GPU; here the engine
draws scenes that hold exactly those edges — synthetic_scenes.frame_filling_world: polygons that reach past the frustum, clipped onto
the frame's borders, corners and diagonals — next to fixture frames (FourRooms' frame 150 at 128 x 48 has such an edge of its own), at
the sizes around the limit:

    128 x 48, 48 x 128 (the quad kernel's before the policy asked for the coefficients' range), 128 x 64, 128 x 96, 96 x 128, 64 x 128
    (the tile kernels'), 127 x 96 and 96 x 126 (ragged frames on a 128-wide / 128-high grid: the ragged tile kernels, whose vertex range
    is the FRAME's), 112 x 96 (an interior control)

Every case is test_gpu_quad_binning.draw_and_compare: RGB and the depth map bit for bit against pyoracle.render at the same size and
sample count, mw_check clean, raster_path() as the launch policy (tests/hostcheck/policy.cpp, asked — not restated) gives it for that
size.  Before any GPU work the host's own setup (tests/hostcheck/mwhost.cpp, mwhost_edge_extremes) has to find the extreme slopes in
the new world's display lists: a scene set that misses the limit fails, and none of its scenes may fall to the list-length filter."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers
import pyoracle
import synthetic_scenes as syn
import test_display_list_limits_cpu as cpu
import test_gpu_quad_binning as qb
from test_launch_policy_cpu import RASTER_PATH, ask, policy_lib

pytestmark = pytest.mark.gpu

WIDE_OR_HIGH = [(128, 48), (48, 128), (128, 64), (128, 96), (96, 128), (64, 128)]
RAGGED = [(127, 96), (96, 126)]
CONTROL = [(112, 96)]
SIZES = WIDE_OR_HIGH + RAGGED + CONTROL
FOUR_SAMPLE_SIZES = [(128, 48), (48, 128), (128, 64)]
PATHS = {0: "PATH_TILE", 1: "PATH_QUAD", 2: "PATH_QUAD_MESH", 3: "PATH_GENERIC"}


def policy_path(width, height, msaa, meshes, with_depth, k2q=True):
    """the raster path the launch policy states for an engine of a small scene (no visiting order) at this size"""
    from miniworld_amd import engine as E
    lds = 0
    if width % 16 == 0 and height % 4 == 0:         # (the quad kernel's LDS plan exists for frames on the grid only; mw_create asks with depth)
        lib = E.load_library()
        lib.mw_rasterq_lds_bytes.argtypes = [C.c_int] * 5
        lds = lib.mw_rasterq_lds_bytes(4 if msaa == 4 else 8, width, height, (width // 16) * (height // 4), 1)
    return PATHS[ask(policy_lib(), RASTER_PATH, [msaa, width, height, int(meshes), 0, int(k2q), 0, 0, 0, int(with_depth), lds])[0]]


@functools.lru_cache(maxsize=None)
def filling(width, height, msaa):
    """the new world's batch name for this frame, after the host's checks of it: every scene kept, the extreme slopes present"""
    name = f"filling/{width}x{height}"
    _, scenes, _ = qb.batch(name)
    assert len(qb.sized_batch(name, msaa, width, height)[1]) == len(scenes) == len(syn.FILLING_PARTS)
    lib = cpu.host_library()
    lib.mwhost_edge_extremes.argtypes = [C.c_void_p, C.c_void_p]
    lo_dcdx, hi_dcdy = [], []
    for sc in scenes:
        packed, keep = pyoracle.pack_scene(sc, width, height, msaa, None)
        out = np.zeros(4, np.int32)
        assert lib.mwhost_edge_extremes(C.byref(packed), out.ctypes.data) > 0
        lo_dcdx.append(int(out[0]))
        hi_dcdy.append(int(out[3]))
    # an edge across the whole width in the direction that makes B = 256 dcdy positive, one over the whole height with A = -256 dcdx positive
    assert max(hi_dcdy) == 256 * width and min(lo_dcdx) == -256 * height, (width, height, hi_dcdy, lo_dcdx)
    if width == 128:
        assert 256 * max(hi_dcdy) == 2 ** 23
    if height == 128:
        assert -256 * min(lo_dcdx) == 2 ** 23
    return name


def draw(names, width, height, msaa, with_depth, meshes=False, k2q=True):
    want = policy_path(width, height, msaa, meshes, with_depth, k2q)
    for name in names:
        qb.draw_and_compare(name, width, height, msaa, with_depth, want)
    return want


@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("size", SIZES)
def test_frames_at_the_coefficient_limit_equal_the_oracle(size, with_depth):
    """8 samples: the frame-filling world, Hallway, FourRooms (frame 150 among its three) and the crowded world at every size"""
    W, H = size
    path = draw((filling(W, H, 8), "hallway", "fourrooms", "crowded"), W, H, 8, with_depth)
    if size in RAGGED + CONTROL:        # frames whose vertex range stays below 128 keep the (ragged) tile kernels: these cases do run them
        assert path == "PATH_TILE"


@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("size", FOUR_SAMPLE_SIZES)
def test_the_same_at_4_samples(size, with_depth):
    W, H = size
    draw((filling(W, H, 4), "hallway", "fourrooms", "crowded"), W, H, 4, with_depth)


@pytest.mark.parametrize("with_depth", [True, False])
def test_fourrooms_frame_150_at_128_x_48(with_depth):
    """the frame profiles/r34 found: 8 037 RGB values off the oracle while 128 x 48 was the quad kernel's"""
    s0, tr, meta, obs = helpers.load_case("fourrooms_s0")
    assert sorted(obs)[:3][2] == 150                    # the third scene of the "fourrooms" batch
    draw(("fourrooms",), 128, 48, 8, with_depth)


@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("size", [(128, 96), (96, 128)])
def test_mesh_entities_at_128_wide_and_128_high(size, with_depth):
    """PickupObjects: whatever chain the policy gives a frame with mesh entities at this size"""
    draw(("pickup",), size[0], size[1], 8, with_depth, meshes=True)


@pytest.mark.parametrize("size", [(128, 48), (48, 128)])
def test_without_the_quad_kernel(size, monkeypatch):
    """MW_K2Q=0: the sizes that were the quad kernel's, through whatever the policy gives them with the quad kernel switched off"""
    monkeypatch.setenv("MW_K2Q", "0")
    W, H = size
    draw((filling(W, H, 8), "hallway", "fourrooms", "crowded"), W, H, 8, True, k2q=False)
