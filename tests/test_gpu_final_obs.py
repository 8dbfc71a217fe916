"""Same-step auto-reset with final observations (mw_set_final_obs, MiniWorldVecEnv(final_obs=True)): the step that ends an episode
returns the next episode's first frame as before, and writes the terminal frame of each finished env into that env's row of the
final buffers.

Three engines take the same actions: A (same-step + final_obs), B (plain same-step) and C (no auto-reset; its host calls
mw_reset(mask, NULL) + mw_render after every end — the reference's "step; if done: reset()").  Bit for bit, on every step: A's
observation, depth, reward, flags, state and final info are B's; A's observation is C's post-reset render; A's final rows of the
finished envs are C's step frame; the rows of the other envs keep a sentinel written before the step."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

SENTINEL_U8, SENTINEL_F = 0xA5, -7.25


def _short_episodes(monkeypatch, cls_name, steps):
    """Episodes of at most `steps` steps for a family whose class fixes max_episode_steps (the batched env reads it from its
    template instance)."""
    from miniworld_amd import envs
    base = getattr(envs, cls_name)

    class Short(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.max_episode_steps = steps
    Short.__name__ = Short.__qualname__ = cls_name
    monkeypatch.setattr(envs, cls_name, Short)


def _same_state(a, b, rows=None):
    rows = slice(None) if rows is None else rows
    return a.keys() == b.keys() and all(np.array_equal(a[k][rows], b[k][rows]) for k in a)


def _fill_sentinel(vec):
    vec.final_obs.fill_(SENTINEL_F if vec.final_obs.is_floating_point() else SENTINEL_U8)
    if vec.final_depth is not None:
        vec.final_depth.fill_(SENTINEL_F)


def _is_sentinel(x):
    return np.all(x == (SENTINEL_F if np.issubdtype(x.dtype, np.floating) else SENTINEL_U8))


def _final_obs_parity(env_id, n, steps, seed, n_actions, want_depth=False, p_fwd=None, **kw):
    """A, B and C as in the module docstring; returns (ends, steps without an end, steps where every env ended)."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    common = dict(seed=seed, want_depth=want_depth, **kw)
    A = MiniWorldVecEnv(env_id, n, final_obs=True, **common)
    B = MiniWorldVecEnv(env_id, n, **common)
    C = MiniWorldVecEnv(env_id, n, autoreset=False, **common)
    assert A.final_obs is not None and tuple(A.final_obs.shape) == tuple(A.obs.shape) and A.final_obs.dtype == A.obs.dtype
    assert (A.final_depth is not None) == want_depth and B.final_obs is None
    for v in (A, B, C):
        v.reset()
    rng = np.random.default_rng(seed)
    if p_fwd is None:
        queue = rng.integers(0, n_actions, (steps, n))
    else:
        queue = np.where(rng.random((steps, n)) < p_fwd, 2, rng.integers(0, n_actions, (steps, n)))
    rbuf, dbuf = torch.zeros_like(C.obs), (torch.zeros_like(C.depth) if want_depth else None)
    has_info = A._info_kind is not None
    ends = quiet = all_ended = 0
    for t in range(steps):
        act = torch.as_tensor(queue[t], dtype=torch.int32, device="cuda")
        _fill_sentinel(A)
        oa, ra, ta, tra = (x.cpu().numpy() for x in A.step(act))
        fa = A.final_obs.cpu().numpy()
        fda = A.final_depth.cpu().numpy() if want_depth else None
        da = A.depth.cpu().numpy() if want_depth else None
        sa = A.engine.get_state()
        ob, rb, tb, trb = (x.cpu().numpy() for x in B.step(act))
        tag = (env_id, t)
        # A == B: everything a plain same-step step returns
        assert np.array_equal(oa, ob), tag + ("obs A != B",)
        if want_depth:
            assert np.array_equal(da, B.depth.cpu().numpy()), tag + ("depth A != B",)
        assert np.array_equal(ra, rb) and np.array_equal(ta, tb) and np.array_equal(tra, trb), tag + ("reward / flags",)
        assert _same_state(sa, B.engine.get_state()), tag + ("state A != B",)
        if has_info:
            fia, fib = A.final_infos(), B.final_infos()
            done = (ta | tra).astype(bool)
            for k in fia:
                assert np.array_equal(fia[k].cpu().numpy()[done], fib[k].cpu().numpy()[done]), tag + ("final info", k)
        assert not A.reset_pending().any(), tag + ("reset_pending",)
        # C: the step frame (terminal frames of the finished envs), then the host resets and renders
        oc, rc_, tc, trc = (x.cpu().numpy() for x in C.step(act))
        dc = C.depth.cpu().numpy() if want_depth else None
        assert np.array_equal(ra, rc_) and np.array_equal(ta, tc) and np.array_equal(tra, trc), tag + ("reward / flags A != C",)
        done = (tc | trc).astype(bool)
        if done.any():
            C.engine.reset(done.astype(np.uint8), None)
            C.engine.render(rbuf, dbuf)
            ro, rd = rbuf.cpu().numpy(), (dbuf.cpu().numpy() if want_depth else None)
        else:
            ro, rd = oc, dc
        assert np.array_equal(oa[done], ro[done]) and np.array_equal(oa[~done], oc[~done]), tag + ("obs A != C",)
        assert _same_state(sa, C.engine.get_state()), tag + ("state A != C",)
        assert np.array_equal(fa[done], oc[done]), tag + ("final obs != C's terminal frame",)
        assert _is_sentinel(fa[~done]), tag + ("final obs row of an unfinished env written",)
        if want_depth:
            assert np.array_equal(da[done], rd[done]), tag + ("depth A != C",)
            assert np.array_equal(fda[done], dc[done]), tag + ("final depth",)
            assert _is_sentinel(fda[~done]), tag + ("final depth row of an unfinished env written",)
        ends += int(done.sum())
        quiet += int(not done.any())
        all_ended += int(done.all())
    for v in (A, B, C):
        v.engine.check()
        v.close()
    return ends, quiet, all_ended


@pytest.mark.parametrize("spare", ["0", "1"])
def test_final_obs_hallway(spare, monkeypatch):
    """Hallway: the dense K1, the quad kernel at 8 samples; RGB-D; without and with spare worlds."""
    monkeypatch.setenv("MW_SPARE", spare)
    _short_episodes(monkeypatch, "Hallway", 3)
    ends, quiet, all_ended = _final_obs_parity("MiniWorld-Hallway-v0", 40, 16, 900, 3, want_depth=True, p_fwd=0.6)
    assert ends >= 40 and quiet >= 1 and all_ended >= 1


@pytest.mark.parametrize("spare,mes", [("0", 2), ("1", 2), ("1", 1)])
def test_final_obs_oneroom_rgbd(spare, mes, monkeypatch):
    """OneRoom RGB-D with spares off and on; episodes of one step: every step ends every episode, consecutive one-step episodes
    claim spares whose refill may not have run yet."""
    monkeypatch.setenv("MW_SPARE", spare)
    _short_episodes(monkeypatch, "OneRoom", mes)
    ends, _, all_ended = _final_obs_parity("MiniWorld-OneRoom-v0", 24, 10, 901, 3, want_depth=True, p_fwd=0.6)
    assert ends >= 24 and all_ended >= 1


def test_final_obs_pickup_dr(monkeypatch):
    """PickupObjects with domain randomisation: the mesh chain (entity, slow and mesh-tile kernels) in both passes, the
    wave-per-env K1, the per-step draws (pass 1 only), the picked object drawn one last time on the step that ends the episode."""
    _short_episodes(monkeypatch, "PickupObjects", 5)
    ends, quiet, _ = _final_obs_parity("MiniWorld-PickupObjects-v0", 16, 20, 31, 5, domain_rand=True)
    assert ends >= 16 and quiet >= 1


@pytest.mark.parametrize("env_id,mes", [("MiniWorld-MazeS3Fast-v0", 2), ("MiniWorld-Maze-v0", 3)])
def test_final_obs_maze(env_id, mes):
    """The big-scene tile kernels and geometry kernel over the list; spares refilled on the side stream while pass 2 claims them."""
    ends, _, _ = _final_obs_parity(env_id, 12, 12, 77, 3, max_episode_steps=mes)
    assert ends >= 24


def test_final_obs_collecthealth(monkeypatch):
    """CollectHealth: the kit respawn belongs to pass 1 (a finished env's consumed kit does not respawn, as in plain same-step);
    the health final info."""
    _short_episodes(monkeypatch, "CollectHealth", 6)
    ends, _, _ = _final_obs_parity("MiniWorld-CollectHealth-v0", 16, 20, 13, 8, p_fwd=0.3)
    assert ends >= 32


def test_final_obs_tmaze(monkeypatch):
    """TMaze: a placement-program generator, goal_pos final info; RGB-D."""
    _short_episodes(monkeypatch, "TMaze", 3)
    ends, _, _ = _final_obs_parity("MiniWorld-TMaze-v0", 16, 12, 5, 3, want_depth=True)
    assert ends >= 48


@pytest.mark.parametrize("msaa,generic,path", [(4, "0", "quad"), (4, "1", "generic"), (1, "0", "generic")])
def test_final_obs_other_sample_counts(msaa, generic, path, monkeypatch):
    """4 samples through the quad kernel's 4-sample form and through the generic-resolution kernels, 1 sample (generic)."""
    import torch
    from miniworld_amd import engine as E
    from miniworld_amd.vec_env import MiniWorldVecEnv
    monkeypatch.setenv("MW_GENERIC_RASTER", generic)
    _short_episodes(monkeypatch, "Hallway", 3)
    probe = MiniWorldVecEnv("MiniWorld-Hallway-v0", 4, msaa=msaa, final_obs=True)
    probe.reset()
    probe.step(torch.zeros(4, dtype=torch.int32, device="cuda"))
    assert probe.engine.raster_path() == (E.PATH_QUAD if path == "quad" else E.PATH_GENERIC)
    probe.close()
    ends, _, _ = _final_obs_parity("MiniWorld-Hallway-v0", 24, 10, 902, 3, want_depth=True, p_fwd=0.6, msaa=msaa)
    assert ends >= 24


@pytest.mark.parametrize("layout", ["cwh", "grey"])
def test_final_obs_wrapper_layouts(layout, monkeypatch):
    """The wrapper layouts (the general tile kernel for the mesh scene, the quad kernel's layout stores for Hallway)."""
    _short_episodes(monkeypatch, "Hallway", 3)
    ends, _, _ = _final_obs_parity("MiniWorld-Hallway-v0", 24, 8, 903, 3, p_fwd=0.6, obs_layout=layout)
    assert ends >= 24
    _short_episodes(monkeypatch, "PickupObjects", 4)
    ends, _, _ = _final_obs_parity("MiniWorld-PickupObjects-v0", 8, 10, 904, 5, obs_layout=layout)
    assert ends >= 8


def test_final_obs_large_frame(monkeypatch):
    """A 160 x 120 observation: the generic-resolution kernels at 8 samples."""
    _short_episodes(monkeypatch, "OneRoom", 3)
    ends, _, _ = _final_obs_parity("MiniWorld-OneRoom-v0", 12, 8, 905, 3, want_depth=True, p_fwd=0.6, obs_width=160, obs_height=120)
    assert ends >= 12


@pytest.mark.parametrize("env_id,cls_name,n,mes,dr", [("MiniWorld-Hallway-v0", "Hallway", 4096, 20, False),
                                                      ("MiniWorld-PickupObjects-v0", "PickupObjects", 2048, 12, True),
                                                      ("MiniWorld-Maze-v0", None, 1024, 10, False)])
def test_final_obs_full_size(env_id, cls_name, n, mes, dr, monkeypatch):
    """BASELINE batch sizes with short episodes: A's observation equals B's on every step, and A's final rows equal C's terminal
    frames (compared on the device)."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    kw = dict(seed=55, domain_rand=dr)
    if cls_name:
        _short_episodes(monkeypatch, cls_name, mes)
    else:
        kw["max_episode_steps"] = mes
    A = MiniWorldVecEnv(env_id, n, final_obs=True, **kw)
    B = MiniWorldVecEnv(env_id, n, **kw)
    C = MiniWorldVecEnv(env_id, n, autoreset=False, **kw)
    for v in (A, B, C):
        v.reset()
    g = torch.Generator(device="cuda").manual_seed(3)
    n_act = A.n_actions if A.n_actions <= 5 else 3
    ends = 0
    for t in range(3 * mes):
        act = torch.randint(0, n_act, (n,), generator=g, device="cuda", dtype=torch.int32)
        A.final_obs.fill_(SENTINEL_U8)
        oa, ra, ta, tra = A.step(act)
        ob, rb, tb, trb = B.step(act)
        oc, _, tc, trc = C.step(act)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(ta, tb) and torch.equal(tra, trb), (env_id, t)
        done = (tc | trc).bool()
        assert torch.equal(done, (ta | tra).bool()), (env_id, t)
        assert torch.equal(A.final_obs[done], oc[done]), (env_id, t)
        assert bool((A.final_obs[~done] == SENTINEL_U8).all()), (env_id, t)
        if done.any():
            C.engine.reset(done.to(torch.uint8).cpu().numpy(), None)
            C.engine.render(C.obs, None)
            assert torch.equal(oa, C.obs), (env_id, t)
        ends += int(done.sum())
    assert ends >= n
    for v in (A, B, C):
        v.engine.check()
        v.close()


def test_final_frame_equals_the_oracle_render_of_the_terminal_state(monkeypatch):
    """8 samples: every final frame (and depth map) equals the CPU oracle's render of the terminal state — which engine C, without
    auto-reset, holds after the same step."""
    import pyoracle
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    _short_episodes(monkeypatch, "TMaze", 4)
    n = 8
    A = MiniWorldVecEnv("MiniWorld-TMaze-v0", n, seed=60, want_depth=True, final_obs=True)
    C = MiniWorldVecEnv("MiniWorld-TMaze-v0", n, seed=60, want_depth=True, autoreset=False)
    A.reset()
    C.reset()
    g = torch.Generator(device="cuda").manual_seed(1)
    checked = 0
    for t in range(10):
        act = torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32)
        _, _, term, trunc = A.step(act)
        C.step(act)
        done = (term | trunc).bool().cpu().numpy()
        if done.any():
            st = C.engine.get_state()
            for i in np.nonzero(done)[0]:
                want = pyoracle.render(helpers.scene_of_vec_env(C, st, i))
                assert np.array_equal(A.final_obs[i].cpu().numpy(), want["rgb"]), (t, i)
                assert np.array_equal(A.final_depth[i].cpu().numpy(), want["depth"]), (t, i)
                checked += 1
            C.engine.reset(done.astype(np.uint8), None)
    assert checked >= n
    A.engine.check()
    A.close()
    C.close()


def test_final_obs_mesh_stamp_wrap(monkeypatch):
    """The mesh chain's 16-bit fragment stamp reaches 0 on a pass-2 frame (mw_debug_set_mesh_frame_seq): PickupObjects' frames
    and final frames are still B's and C's."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    _short_episodes(monkeypatch, "PickupObjects", 2)
    n = 16
    A = MiniWorldVecEnv("MiniWorld-PickupObjects-v0", n, seed=41, final_obs=True)
    B = MiniWorldVecEnv("MiniWorld-PickupObjects-v0", n, seed=41)
    C = MiniWorldVecEnv("MiniWorld-PickupObjects-v0", n, seed=41, autoreset=False)
    for v in (A, B, C):
        v.reset()
    # pass 1 of step k draws frame 65529 + 2k, pass 2 frame 65530 + 2k: step 3's pass 2 has stamp 0.  (The hook keeps the
    # sequence number's parity: a render of its own, which changes nothing else, moves it when it is even.)
    if A.engine.lib.mw_debug_set_mesh_frame_seq(A.engine.h, 65529) != 0:
        A.engine.render(torch.zeros_like(A.obs))
        assert A.engine.lib.mw_debug_set_mesh_frame_seq(A.engine.h, 65529) == 0
    g = torch.Generator(device="cuda").manual_seed(9)
    for t in range(8):
        act = torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32)
        oa, _, ta, tra = A.step(act)
        ob, _, _, _ = B.step(act)
        oc, _, tc, trc = C.step(act)
        done = (tc | trc).bool()
        assert torch.equal(oa, ob), t
        assert torch.equal(A.final_obs[done], oc[done]), t
        if done.any():
            C.engine.reset(done.to(torch.uint8).cpu().numpy(), None)
    for v in (A, B, C):
        v.engine.check()
        v.close()


def test_set_final_obs_abi_edges(monkeypatch):
    """MW_E_INVALID on off / next-step / MW_GEN_NONE engines; NULL turns the feature off (the steps after it equal plain same-step
    and write no final row); mw_get_reset_pending stays zero; mw_render after a step shows the new episode."""
    import ctypes
    import torch
    from miniworld_amd import engine as E
    from miniworld_amd.scene import base_config
    from miniworld_amd.vec_env import MiniWorldVecEnv
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for mode in (False, "next_step"):
        v = MiniWorldVecEnv("MiniWorld-Hallway-v0", 2, autoreset=mode)
        assert v.engine.lib.mw_set_final_obs(v.engine.h, ctypes.c_void_p(buf.data_ptr()), None) == -1, mode
        v.close()
    lib = E.load_library()
    cfg = base_config(4, 80, 60, 1, 6, 4, 16)
    cfg.abi_version = E.ABI_VERSION
    cfg.autoreset = E.AUTORESET_SAME_STEP
    cfg.generator = E.GEN_NONE
    h = ctypes.c_void_p()
    assert lib.mw_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    assert lib.mw_set_final_obs(h, ctypes.c_void_p(buf.data_ptr()), None) == -1
    assert lib.mw_set_final_obs(h, None, None) == -1
    lib.mw_destroy(h)

    _short_episodes(monkeypatch, "Hallway", 2)
    n = 8
    A = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, seed=4, want_depth=True, final_obs=True)
    B = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, seed=4, want_depth=True)
    A.reset()
    B.reset()
    act = torch.full((n,), 2, dtype=torch.int32, device="cuda")
    out, dep = torch.zeros_like(A.obs), torch.zeros_like(A.depth)
    ended = 0
    for t in range(6):
        if t == 3:
            A.engine.set_final_obs(None)
            _fill_sentinel(A)
        oa, _, ta, tra = A.step(act)
        ob, _, _, _ = B.step(act)
        assert torch.equal(oa, ob) and torch.equal(A.depth, B.depth), t
        assert not A.reset_pending().any(), t
        A.engine.render(out, dep)
        assert torch.equal(out, oa) and torch.equal(dep, A.depth), t        # the new episode's first frame
        if t >= 3:
            assert _is_sentinel(A.final_obs.cpu().numpy()) and _is_sentinel(A.final_depth.cpu().numpy()), t
        else:
            ended += int((ta | tra).sum())
    assert ended >= n
    A.engine.check()
    A.close()
    B.close()


@pytest.mark.parametrize("to_numpy", [False, True])
def test_vector_env_adapter_final_obs(to_numpy, monkeypatch):
    """MiniWorldVectorEnv(final_obs=True): info["final_obs"] holds the terminal frames under the info["_final_obs"] mask (C's step
    frames), stays valid after the next step, and is numpy under to_numpy; without the flag there are no such keys."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    from miniworld_amd.vector import MiniWorldVectorEnv
    _short_episodes(monkeypatch, "Hallway", 3)
    n = 6
    envs = MiniWorldVectorEnv("MiniWorld-Hallway-v0", n, to_numpy=to_numpy, seed=12, final_obs=True)
    plain = MiniWorldVectorEnv("MiniWorld-Hallway-v0", n, to_numpy=True, seed=12)
    C = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, seed=12, autoreset=False)
    envs.reset(seed=12)
    plain.reset(seed=12)
    C.reset(12)
    as_np = (lambda x: x) if to_numpy else (lambda x: x.cpu().numpy())
    prev = None
    ended = 0
    for t in range(9):
        a = np.full(n, t % 3, np.int64)
        obs, rew, term, trunc, info = envs.step(a)
        _, _, _, _, pinfo = plain.step(a)
        oc, _, tc, trc = C.step(torch.as_tensor(a, dtype=torch.int32, device="cuda"))
        assert "final_obs" not in pinfo and "_final_obs" not in pinfo
        assert isinstance(info["final_obs"], np.ndarray) == to_numpy
        done = as_np(info["_final_obs"]).astype(bool)
        assert np.array_equal(done, (tc | trc).bool().cpu().numpy()) and np.array_equal(done, as_np(info["_final_info"]))
        assert np.array_equal(as_np(info["final_obs"])[done], oc.cpu().numpy()[done]), t
        if prev is not None:
            assert np.array_equal(as_np(prev[0])[prev[1]], prev[2]), t       # last step's final_obs is still intact
        prev = (info["final_obs"], done, as_np(info["final_obs"])[done].copy())
        if done.any():
            C.engine.reset(done.astype(np.uint8), None)
        ended += int(done.sum())
    assert ended >= 2 * n
    envs.close()
    plain.close()
    C.close()
