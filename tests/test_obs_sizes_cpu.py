"""Observation and window sizes that are not multiples of the engine's 16 x 4 raster tile, host side, without a GPU.

tests/golden/sizes/*.npz hold frames of the reference itself on Mesa llvmpipe at 84 x 84 and 81 x 61 (4 samples, and one case of
its single-sampled fallback) and one render() frame at an 801 x 601 window (tools/gen_size_fixtures.py).  The oracle must
reproduce them bit for bit: that pins the fixtures the GPU tests (test_gpu_obs_sizes.py) compare the engine with.  mw_create's
size check runs before it looks for a device, so it is tested here too."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import pyoracle
from conftest import GOLDEN

SIZES = os.path.join(GOLDEN, "sizes")


def size_cases(prefix="gl_"):
    return sorted(f[len(prefix):-4] for f in os.listdir(SIZES) if f.startswith(prefix) and f.endswith(".npz"))


def load_sizes(case, prefix="gl_"):
    """(W, H, window, samples, {frame: (scene, arrays)}) of one tests/golden/sizes fixture."""
    d = np.load(os.path.join(SIZES, prefix + case + ".npz"))
    frames = {}
    for k in d["meta/frames"]:
        pre = f"gl/{int(k)}/"
        sc = {key[len(pre) + 6:]: d[key] for key in d.files if key.startswith(pre + "scene/")}
        fr = {key[len(pre):]: d[key] for key in d.files if key.startswith(pre) and not key.startswith(pre + "scene/")}
        frames[int(k)] = (sc, fr)
    W, H = (int(v) for v in d["meta/size"])
    return W, H, tuple(int(v) for v in d["meta/window"]), int(d["meta/samples"]), frames


def test_fixtures_cover_the_issue_sizes():
    cases = size_cases()
    for env in ("hallway_s0", "pickup_dr_s1", "maze_s0"):
        for size in ("84x84", "81x61"):
            assert f"{env}_{size}" in cases
    assert size_cases("gl1_")
    views = [c for c in cases if any("view_agent" in fr for _, fr in load_sizes(c)[4].values())]
    assert views, "no render() frame at an odd window size"
    for c in cases + size_cases("gl1_"):
        W, H = load_sizes(c, "gl1_" if c in size_cases("gl1_") else "gl_")[:2]
        assert W % 16 or H % 4, f"{c}: {W}x{H} is on the 16 x 4 grid"


@pytest.mark.parametrize("prefix,case", [("gl_", c) for c in size_cases()] + [("gl1_", c) for c in size_cases("gl1_")])
def test_oracle_equals_the_reference_at_odd_sizes(prefix, case):
    W, H, window, ns, frames = load_sizes(case, prefix)
    assert ns == (1 if prefix == "gl1_" else 4)
    for k, (sc, fr) in frames.items():
        meshes = helpers.golden_meshes(sc)
        r = pyoracle.render(sc, width=W, height=H, nsamples=ns, meshes=meshes)
        assert fr["rgb"].shape == (H, W, 3)
        assert np.array_equal(r["rgb"], fr["rgb"]), f"{case} frame {k}: RGB"
        assert np.array_equal(r["z16"], fr["z16"]), f"{case} frame {k}: z16"
        assert np.array_equal(r["depth"].view(np.uint32), fr["depth"].view(np.uint32)), f"{case} frame {k}: depth map"
        t = pyoracle.render(sc, width=W, height=H, nsamples=ns, meshes=meshes, view="top", render_agent=True)
        assert np.array_equal(t["rgb"], fr["top"]), f"{case} frame {k}: top view"
        v = pyoracle.visible_ents(sc, width=W, height=H, nsamples=ns)
        assert np.array_equal(v, fr["vis"]), f"{case} frame {k}: visible entities"
        if "view_agent" in fr:
            rr = pyoracle.render(sc, width=window[0], height=window[1], nsamples=ns, meshes=meshes, view="agent")
            assert fr["view_agent"].shape == (window[1], window[0], 3)
            assert np.array_equal(rr["rgb"], fr["view_agent"]), f"{case} frame {k}: render() at {window}"


def _create(width, height, msaa=8):
    """mw_create's return code and message for a small config of that size (an engine it did create is destroyed again)."""
    from miniworld_amd import engine as eng
    from miniworld_amd.scene import base_config
    lib = eng.load_library()
    cfg = base_config(4, width, height, 1, 8, 8, 16)
    cfg.msaa = msaa
    cfg.abi_version = eng.ABI_VERSION
    h = C.c_void_p()
    rc = lib.mw_create(C.byref(cfg), C.byref(h))
    msg = lib.mw_last_error(None).decode()
    if rc == 0:
        lib.mw_destroy(h)
    return rc, msg


@pytest.mark.parametrize("size", [(84, 84), (81, 61), (100, 75), (17, 5), (1, 1), (130, 97), (801, 601), (4080, 1020), (4079, 1017)])
def test_mw_create_accepts_any_size_up_to_255_tiles(size):
    rc, msg = _create(*size)
    # (no device here: the size check passed and the device check failed; on a GPU box the engine is created)
    assert rc == 0 or (rc == -5 and "no HIP device" in msg), (size, rc, msg)


@pytest.mark.parametrize("size", [(0, 60), (80, 0), (-16, 60), (80, -4), (4081, 60), (80, 1021), (4096, 1024)])
def test_mw_create_rejects_empty_and_oversized_frames(size):
    rc, msg = _create(*size)
    assert rc == -1 and "obs size" in msg, (size, rc, msg)


def test_header_documents_the_size_range():
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "mwengine.h")).read()
    assert "4080 x 1020" in header
    assert "multiples of 16 x 4)" not in header
