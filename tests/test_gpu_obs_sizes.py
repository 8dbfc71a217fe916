"""Observation and window sizes that are not multiples of the 16 x 4 raster tile (84 x 84, 81 x 61, 100 x 75, 17 x 5, 1 x 1, ...).

The engine rasterises such a frame on the grid ceil16(W) x ceil4(H), with the viewport, the projection and every output stride of
the W x H frame; the padding pixels are masked and never stored.  At 8 samples, without mesh entities and with a grid inside the
tile kernels' edge bound, the ragged tile kernels draw it (mw_raster_ragged_kernel / mw_raster_big_ragged_kernel), otherwise the
generic-resolution kernels ("Frame sizes").  Checked here, bit for bit: the reference's own frames at those sizes (tests/golden/sizes), the oracle at 8
samples in every output layout, guard bytes around odd-aligned outputs, a full batch with both auto-reset modes, and the
single-env API."""
import numpy as np
import pytest

import helpers
from test_obs_sizes_cpu import load_sizes, size_cases
from test_gpu_vs_reference_gl import _groups

pytestmark = pytest.mark.gpu



def expected_path(w, h, msaa, meshes):
    """DESIGN.md's path table for a frame off the 16 x 4 grid (MW_K2Q and MW_GENERIC_RASTER do not change it)."""
    from miniworld_amd import engine as E
    gw, gh = -(-w // 16) * 16, -(-h // 4) * 4
    # (the frame's own sides below 128: the 24-bit coefficients; the grid's area: the 32-bit sums — mw_policy.h, edge_coeffs_fit / edge_sums_fit)
    exact = w < 128 and h < 128 and gw <= 128 and gh <= 128 and gw * gh <= 128 * 96
    return E.PATH_TILE if (msaa == 8 and not meshes and exact and h % 2 == 0) else E.PATH_GENERIC


def _grey(rgb):
    r, g, b = (rgb[..., c].astype(np.float64) for c in range(3))
    return (0.30 * r + 0.59 * g) + 0.11 * b


@pytest.mark.parametrize("prefix,case", [("gl_", c) for c in size_cases()] + [("gl1_", c) for c in size_cases("gl1_")])
def test_engine_equals_the_reference_at_odd_sizes(prefix, case):
    """The reference's own 4- and 1-sample frames (llvmpipe clamps GL_MAX_SAMPLES): the generic-resolution kernels."""
    import torch
    W, H, window, ns, frames = load_sizes(case, prefix)
    for ks in _groups(frames):
        scenes = [frames[k][0] for k in ks]
        s0 = scenes[0]
        eng = helpers.make_engine_for_scene(s0, len(scenes), agent_radius=float(s0.get("agent_radius", 0.4)), msaa=ns, width=W, height=H)
        eng.set_state(helpers.scene_state_arrays(scenes))
        rgb = torch.zeros((len(scenes), H, W, 3), dtype=torch.uint8, device="cuda")
        depth = torch.zeros((len(scenes), H, W, 1), dtype=torch.float32, device="cuda")
        eng.render(rgb, depth)
        assert eng.raster_path() == expected_path(W, H, ns, len(eng._test_mesh_map) > 0), (case, eng.raster_path())
        top = torch.zeros((len(scenes), H, W, 3), dtype=torch.uint8, device="cuda")
        eng.render_top(top, None, True)
        vis = eng.visible_ents()
        eng.check()
        rgb, depth, top, vis = rgb.cpu().numpy(), depth.cpu().numpy(), top.cpu().numpy(), vis.cpu().numpy()
        for i, k in enumerate(ks):
            fr = frames[k][1]
            tag = f"{prefix}{case} frame {k}"
            assert np.array_equal(rgb[i], fr["rgb"]), f"{tag}: {np.count_nonzero(rgb[i] != fr['rgb'])} RGB values differ"
            assert np.array_equal(depth[i].view(np.uint32), fr["depth"].reshape(H, W, 1).view(np.uint32)), f"{tag}: depth map"
            assert np.array_equal(depth[i, :, :, 0], helpers.depth_from_z16(fr["z16"])), f"{tag}: depth buffer"
            assert np.array_equal(top[i], fr["top"]), f"{tag}: top view"
            n = len(fr["vis"])
            assert np.array_equal(vis[i, :n].astype(bool), np.asarray(fr["vis"]).astype(bool)), f"{tag}: visible entities"
            if "view_agent" in fr:
                out = eng.render_view(i, window[0], window[1], msaa=ns).cpu().numpy()
                assert np.array_equal(out, fr["view_agent"]), f"{tag}: render() at {window}: {np.count_nonzero(out != fr['view_agent'])} values differ"
        eng.close()


def _layout_vecs(env_id, n, w, h, kw, layouts=("hwc", "cwh", "grey")):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    return {k: MiniWorldVecEnv(env_id, n, seed=7, obs_layout=k, want_depth=(k == "hwc"), obs_width=w, obs_height=h, **kw) for k in layouts}


@pytest.mark.parametrize("k2q", ["1", "0"])
@pytest.mark.parametrize("size", [(84, 84), (81, 62), (81, 61), (100, 75), (17, 5), (1, 1), (130, 97)])
@pytest.mark.parametrize("env_id,kw", [("MiniWorld-FourRooms-v0", {}), ("MiniWorld-PickupObjects-v0", {"domain_rand": True}),
                                       ("MiniWorld-Maze-v0", {"max_episode_steps": 40})])
def test_every_layout_equals_the_oracle_at_8_samples(env_id, kw, size, k2q, monkeypatch):
    """msaa = 8 at sizes off the grid: hwc, cwh, grey and the depth map, bit for bit against pyoracle.render at that size, after a few
    steps of the same actions.  FourRooms at an even height: the ragged tile kernel; the Maze: its big-scene form (visiting order);
    PickupObjects (mesh entities), odd heights and 130 x 97 (grid beyond the tile kernels' edge bound): the generic-resolution kernels.  MW_K2Q=0 changes
    nothing for these frames."""
    import pyoracle
    import torch
    monkeypatch.setenv("MW_K2Q", k2q)
    w, h = size
    n = 6
    vecs = _layout_vecs(env_id, n, w, h, kw)
    g = torch.Generator(device="cuda").manual_seed(2)
    plan = [torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32) for _ in range(6)]
    for v in vecs.values():
        v.reset()
        for act in plan:
            v.step(act)
        v.engine.render(v.obs, v.depth)             # the state after the steps (a pickup leaves the list after its frame)
        v.engine.check()
        assert v.engine.raster_path() == expected_path(w, h, 8, bool(v.mesh_ids)), (env_id, size, v.engine.raster_path())
    hwc = vecs["hwc"]
    st = hwc.engine.get_state()
    meshes = helpers.vec_env_meshes(hwc)
    outs = {k: v.obs.cpu().numpy() for k, v in vecs.items()}
    assert outs["hwc"].shape == (n, h, w, 3) and outs["cwh"].shape == (n, 3, w, h) and outs["grey"].shape == (n, h, w, 1)
    for k, v in vecs.items():
        for key, val in v.engine.get_state().items():
            assert np.array_equal(val, st[key]), (k, key)
    for i in range(n):
        want = pyoracle.render(helpers.scene_of_vec_env(hwc, st, i), width=w, height=h, nsamples=8, meshes=meshes)
        tag = (env_id, size, i)
        assert np.array_equal(outs["hwc"][i], want["rgb"]), tag
        assert np.array_equal(hwc.depth[i].cpu().numpy().view(np.uint32), want["depth"].view(np.uint32)), tag
        assert np.array_equal(outs["cwh"][i], want["rgb"].transpose(2, 1, 0)), tag
        assert np.array_equal(outs["grey"][i, :, :, 0], _grey(want["rgb"])), tag
    for v in vecs.values():
        v.close()


@pytest.mark.parametrize("env_id,kw", [("MiniWorld-FourRooms-v0", {}), ("MiniWorld-PickupObjects-v0", {"domain_rand": True})])
def test_wrapper_layouts_on_the_generic_path(env_id, kw):
    """160 x 120 is on the grid but beyond the tile kernels: the generic-resolution kernels store cwh and grey too."""
    import torch
    from miniworld_amd import engine as E
    n = 6
    vecs = _layout_vecs(env_id, n, 160, 120, kw)
    g = torch.Generator(device="cuda").manual_seed(4)
    plan = [torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32) for _ in range(5)]
    for v in vecs.values():
        v.reset()
        for act in plan:
            v.step(act)
        assert v.engine.raster_path() == E.PATH_GENERIC
    raw = vecs["hwc"].obs.cpu().numpy()
    assert np.array_equal(vecs["cwh"].obs.cpu().numpy(), raw.transpose(0, 3, 2, 1))
    assert np.array_equal(vecs["grey"].obs.cpu().numpy()[..., 0], _grey(raw))
    for v in vecs.values():
        v.engine.check()
        v.close()


def test_no_stray_writes_around_odd_aligned_outputs():
    """64 envs at 81 x 61 (14 823 bytes per env: every row but the first starts at an odd address) into views at an odd byte
    offset of larger buffers filled with a sentinel: every row equals the oracle and every guard byte keeps its sentinel."""
    import pyoracle
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n, w, h = 64, 81, 61
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, seed=11, want_depth=True, obs_width=w, obs_height=h)
    vec.reset()
    g = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(4):
        vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
    row, guard = h * w * 3, 4099
    big = torch.full((guard + n * row + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    obs = big[guard:guard + n * row]
    assert obs.data_ptr() % 2 == 1
    dguard = 1027
    dbig = torch.full((dguard + n * h * w + dguard,), -7.25, dtype=torch.float32, device="cuda")
    dep = dbig[dguard:dguard + n * h * w]
    vec.engine.render(obs, dep)
    vec.engine.check()
    b, d = big.cpu().numpy(), dbig.cpu().numpy()
    assert np.all(b[:guard] == 0xA5) and np.all(b[guard + n * row:] == 0xA5)
    assert np.all(d[:dguard] == -7.25) and np.all(d[dguard + n * h * w:] == -7.25)
    got, gdep = b[guard:guard + n * row].reshape(n, h, w, 3), d[dguard:dguard + n * h * w].reshape(n, h, w, 1)
    st = vec.engine.get_state()
    for i in range(n):
        want = pyoracle.render(helpers.scene_of_vec_env(vec, st, i), width=w, height=h)
        assert np.array_equal(got[i], want["rgb"]), i
        assert np.array_equal(gdep[i], want["depth"]), i
    vec.close()


def _short_hallway(monkeypatch, steps):
    from miniworld_amd import envs
    base = envs.Hallway

    class Hallway(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.max_episode_steps = steps
    Hallway.__name__ = Hallway.__qualname__ = "Hallway"
    monkeypatch.setattr(envs, "Hallway", Hallway)


SAMPLE = (0, 1, 777, 2048, 4095)


@pytest.mark.parametrize("mode", ["same_step_final_obs", "next_step"])
def test_full_batch_84x84_with_auto_reset(mode, monkeypatch):
    """Hallway x 4096 at 84 x 84, 60 random steps in episodes of at most 20 steps.  For a sample of envs, each step's frame and
    depth equal the oracle render of the state mw_get_state returns; same-step: each final frame of a sampled env equals the
    oracle render of the terminal state, which engine C (no auto-reset, host reset after every end) holds after the step."""
    import pyoracle
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    _short_hallway(monkeypatch, 20)
    n, w, h = 4096, 84, 84
    kw = dict(seed=31, want_depth=True, obs_width=w, obs_height=h)
    if mode == "next_step":
        A, C_ = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, autoreset="next_step", **kw), None
    else:
        A = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, final_obs=True, **kw)
        C_ = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, autoreset=False, **kw)
        C_.reset()
    A.reset()
    g = torch.Generator(device="cuda").manual_seed(9)
    ends = finals = 0
    for t in range(60):
        act = torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32)
        o, _, term, trunc = A.step(act)
        done = (term | trunc).bool().cpu().numpy()
        st = A.engine.get_state()
        obs, dep = o.cpu().numpy(), A.depth.cpu().numpy()
        for i in SAMPLE:
            want = pyoracle.render(helpers.scene_of_vec_env(A, st, i), width=w, height=h)
            assert np.array_equal(obs[i], want["rgb"]), (mode, t, i)
            assert np.array_equal(dep[i], want["depth"]), (mode, t, i)
        if C_ is not None:
            C_.step(act)
            if done.any():
                sc = C_.engine.get_state()
                fo, fd = A.final_obs.cpu().numpy(), A.final_depth.cpu().numpy()
                for i in SAMPLE:
                    if done[i]:
                        want = pyoracle.render(helpers.scene_of_vec_env(C_, sc, i), width=w, height=h)
                        assert np.array_equal(fo[i], want["rgb"]), (mode, t, i, "final")
                        assert np.array_equal(fd[i], want["depth"]), (mode, t, i, "final")
                        finals += 1
                C_.engine.reset(done.astype(np.uint8), None)
        ends += int(done.sum())
    assert ends >= n
    if C_ is not None:
        assert finals >= len(SAMPLE)
        C_.close()
    A.engine.check()
    A.close()


def test_single_env_at_84x84_with_an_odd_window():
    """envs.Hallway(obs_width=84, obs_height=84, window 801 x 601): reset / step observations, render_depth and render() equal the
    oracle at those sizes (render() draws the 16-sample visualisation buffer, miniworld.py:518)."""
    import pyoracle
    from miniworld_amd import envs
    from miniworld_amd.scene import scene_from_env
    env = envs.Hallway(obs_width=84, obs_height=84, window_width=801, window_height=601, render_mode="rgb_array")
    assert env.observation_space.shape == (84, 84, 3)
    o, _ = env.reset(seed=3)
    assert o.shape == (84, 84, 3)
    assert np.array_equal(o, pyoracle.render(scene_from_env(env), width=84, height=84)["rgb"])
    for a in (2, 2, 0, 2, 1, 2):
        o, *_ = env.step(a)
        want = pyoracle.render(scene_from_env(env), width=84, height=84)
        assert np.array_equal(o, want["rgb"])
    assert np.array_equal(env.render_depth(), want["depth"])
    img = env.render()
    assert img.shape == (601, 801, 3)
    assert np.array_equal(img, pyoracle.render(scene_from_env(env), width=801, height=601, nsamples=16)["rgb"])
    env.close()


@pytest.mark.parametrize("size", [(0, 600), (801, 0), (-16, 600), (4081, 600), (800, 1021)])
def test_render_view_rejects_empty_and_oversized_windows(size):
    """mw_render_view refuses what mw_create refuses (a valid output pointer: the size check itself answers)."""
    import ctypes as C
    from miniworld_amd.vec_env import MiniWorldVecEnv
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 2, seed=0)
    vec.reset()
    eng = vec.engine
    rc = eng.lib.mw_render_view(eng.h, 0, 0, size[0], size[1], 8, C.c_void_p(vec.obs.data_ptr()), None, None)
    assert rc == -1 and "frame buffer size" in eng.lib.mw_last_error(eng.h).decode()
    vec.close()
