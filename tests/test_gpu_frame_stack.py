"""Frame stacking on the device (mw_set_frame_stack; MiniWorldVecEnv(frame_stack=K, stack_pad=...)): the last K returned frames of
every env, oldest first, as a view of the engine's ring.

The yardstick is never the push kernel.  It is a second MiniWorldVecEnv B WITHOUT a stack — same id, seed, actions and mode —
whose single frames, drawn by the unchanged kernels, are collected on the host; the stacking rules are applied to them in numpy
(_drive): an ordinary frame shifts the env's list, the first frame of an episode rebuilds it from the pad, a finished env's final
stack is its old list without the oldest frame plus B's final observation.  Engine A's `stack` (and `final_stack`) must equal the
host's bit for bit after reset() and after every call, and everything else A returns must equal what B returns."""
import ctypes as C_

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _short_episodes(monkeypatch, cls_name, steps):
    """Episodes of at most `steps` steps for a family whose class fixes max_episode_steps: the batched env reads it from its
    template instance (the way tests/test_gpu_action_repeat.py does it)."""
    from miniworld_amd import envs
    base = getattr(envs, cls_name)

    class Short(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.max_episode_steps = steps
    Short.__name__ = Short.__qualname__ = cls_name
    monkeypatch.setattr(envs, cls_name, Short)


def _rebuilt(frames, K, pad):
    """[n, ...] first frames of an episode -> their stacks [n, K, ...]"""
    out = np.repeat(frames[:, None], K, axis=1)
    if pad == "zero":
        out[:, :-1] = 0
    return out


def _np(t):
    return t.cpu().numpy()


def _pair(env_id, n, K, pad, seed, mode, final_obs=False, **kw):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    A = MiniWorldVecEnv(env_id, n, seed=seed, autoreset=mode, final_obs=final_obs, frame_stack=K, stack_pad=pad, **kw)
    B = MiniWorldVecEnv(env_id, n, seed=seed, autoreset=mode, final_obs=final_obs, **kw)
    assert A.frame_stack == K and B.frame_stack is None and B.stack is None
    return A, B


def _drive(env_id, n, K, pad, calls, seed, n_actions, mode="same_step", repeat=1, p_fwd=None, final_obs=False, first_steps=None, **kw):
    """A against the host lists made from B's frames; returns B's per-call done flags, clean bytes and pending bytes [calls][n].
    first_steps: step counts injected into both engines after reset() (mw_set_state: mid-episode, the stacks stay), so that the
    envs' first episodes end after different numbers of calls."""
    import torch
    A, B = _pair(env_id, n, K, pad, seed, mode, final_obs, **kw)
    rng = np.random.default_rng(seed)
    oa, ob = _np(A.reset()), _np(B.reset())
    assert np.array_equal(oa, ob)
    hist = _rebuilt(ob, K, pad)
    assert tuple(A.stack.shape) == (n, K) + ob.shape[1:] and A.stack.dtype == B.obs.dtype
    assert np.array_equal(_np(A.stack), hist), "stack after reset()"
    assert A.engine.stack_window() == (K - 1, 0)
    if first_steps is not None:
        for v in (A, B):
            v.engine.set_state({"step_count": np.asarray(first_steps, np.int32)})
        assert np.array_equal(_np(A.stack), hist), "mw_set_state touched the stacks"
    fexp = None
    if final_obs:
        A.final_stack.fill_(SENTINEL)
        fexp = np.full(tuple(A.final_stack.shape), SENTINEL, _np(A.final_stack).dtype)
    dones, cleans, pends = [], [], []
    for j in range(calls):
        pend = _np(B.reset_pending()).astype(bool)
        assert np.array_equal(_np(A.reset_pending()).astype(bool), pend)
        if p_fwd is None:
            act = rng.integers(0, n_actions, n)
        else:
            act = np.where(rng.random(n) < p_fwd, 2, rng.integers(0, n_actions, n))
        act = torch.as_tensor(act, dtype=torch.int32, device="cuda")
        ra, rb = A.step(act, repeat), B.step(act, repeat)
        for x, y, what in zip(ra, rb, ("obs", "reward", "terminated", "truncated")):
            assert torch.equal(x, y), (env_id, "call", j, what)
        assert torch.equal(A.frame_clean(), B.frame_clean()), (env_id, "call", j, "frame_clean")
        if repeat > 1:
            assert torch.equal(A.substeps, B.substeps), (env_id, "call", j, "substeps")
        if A.depth is not None:
            assert torch.equal(A.depth, B.depth), (env_id, "call", j, "depth")
        o = _np(rb[0])
        done = (_np(rb[2]) | _np(rb[3])).astype(bool)
        # the first frame of an episode: same-step, the call that ended the last one; next-step, the call an env entered pending
        first = done if mode == "same_step" else pend if mode == "next_step" else np.zeros(n, bool)
        if final_obs:
            assert torch.equal(A.final_obs, B.final_obs), (env_id, "call", j, "final_obs")
            fo = _np(B.final_obs)
            for i in np.flatnonzero(done):
                fexp[i] = np.concatenate([hist[i, 1:], fo[i][None]])
            assert np.array_equal(_np(A.final_stack), fexp), (env_id, "call", j, "final_stack", np.flatnonzero(done))
        hist = np.concatenate([hist[:, 1:], o[:, None]], axis=1)
        hist[first] = _rebuilt(o[first], K, pad)
        got = _np(A.stack)
        for i in range(n):
            assert np.array_equal(got[i], hist[i]), (env_id, "call", j, "env", i, "first" if first[i] else "ordinary", "stack")
        assert A.engine.stack_window() == (j % K, j + 1)
        assert torch.equal(A.stack[:, K - 1], A.obs)
        dones.append(done)
        cleans.append(_np(B.frame_clean()).astype(bool))
        pends.append(pend)
    assert A.frame_reuse and B.frame_reuse
    for v in (A, B):
        v.engine.check()
        v.close()
    return np.array(dones), np.array(cleans), np.array(pends)


def _gaps(dones):
    """per env: the calls between consecutive episode ends"""
    return [np.diff(np.flatnonzero(dones[:, i])) for i in range(dones.shape[1])]


def test_hallway_same_step_pad_reset(monkeypatch):
    """K = 4, pad reset, episodes of 7 steps (coprime to K: truncations land on every ring phase), forward-biased actions so that
    some envs reach the box early; 30 calls, the ring wraps seven times."""
    K, calls = 4, 30
    assert calls >= 3 * K + 7
    _short_episodes(monkeypatch, "Hallway", 7)
    dones, cleans, _ = _drive("MiniWorld-Hallway-v0", 70, K, "reset", calls, 900, 3, p_fwd=0.6)
    # the yardstick's own flags: the run is the one meant
    assert {int(j) % K for j in np.flatnonzero(dones.any(axis=1))} == set(range(K)), "episode ends on every ring phase"
    assert any((g < K).any() for g in _gaps(dones)), "an env that ended two episodes fewer than K calls apart"
    assert any((g > K).any() for g in _gaps(dones)), "an env that ran K calls without an end"
    assert cleans.any(), "a clean env-step (frame reuse left a row undrawn, the push read it)"


def test_hallway_next_step_pad_zero(monkeypatch):
    """K = 3, pad zero, next-step auto-reset: the terminal frame is stacked like any other, the rebuild happens on the call after
    it — the one the env entered with reset_pending (B's, read before the call)."""
    K = 3
    _short_episodes(monkeypatch, "Hallway", 7)
    dones, _, pends = _drive("MiniWorld-Hallway-v0", 70, K, "zero", 3 * K + 12, 901, 3, mode="next_step", p_fwd=0.6)
    assert pends.any() and np.array_equal(pends[1:], dones[:-1]) and not (dones & pends).any()
    assert {int(j) % K for j in np.flatnonzero(pends.any(axis=1))} == set(range(K))


@pytest.mark.parametrize("env_id, n, kw", [("MiniWorld-Hallway-v0", 70, {}), ("MiniWorld-Maze-v0", 8, {"max_episode_steps": 9})])
def test_action_repeat_pushes_once_per_call(env_id, n, kw, monkeypatch):
    """K = 2 with repeat = 3: one frame and one push per call, through both forms of the step kernel (Hallway: dense; Maze: a
    wavefront per env)."""
    if "Hallway" in env_id:
        _short_episodes(monkeypatch, "Hallway", 7)
    dones, _, _ = _drive(env_id, n, 2, "reset", 12, 902, 3, repeat=3, p_fwd=0.6, **kw)
    assert dones.any()


@pytest.mark.parametrize("kw, frame_bytes", [(dict(obs_layout="cwh"), 14400), (dict(obs_layout="grey"), 38400),
                                             (dict(obs_width=81, obs_height=61), 14823), (dict(obs_width=84, obs_height=84), 21168)])
def test_layouts_and_sizes(kw, frame_bytes, monkeypatch):
    """K = 2 in the other layouts and sizes: cwh, grey (float64), 81 x 61 (14 823 bytes per frame: the byte path of the kernel)
    and 84 x 84."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    _short_episodes(monkeypatch, "Hallway", 7)
    probe = MiniWorldVecEnv("MiniWorld-Hallway-v0", 3, frame_stack=2, **kw)
    assert probe.obs[0].numel() * probe.obs.element_size() == frame_bytes
    if kw.get("obs_layout") == "cwh":
        # the channel-stacked CNN input is a view of the ring too
        probe.reset()
        probe.step(torch.zeros(3, dtype=torch.int32, device="cuda"))
        W, H = probe.obs.shape[2:]
        flat = probe.stack.reshape(3, 6, W, H)
        assert flat.untyped_storage().data_ptr() == probe._ring.untyped_storage().data_ptr()
        assert torch.equal(flat[:, 3:], probe.obs)
    probe.close()
    dones, _, _ = _drive("MiniWorld-Hallway-v0", 37, 2, "zero", 10, 903, 3, p_fwd=0.6, **kw)
    assert dones.any()


@pytest.mark.parametrize("pad", ["reset", "zero"])
def test_final_stacks(pad, monkeypatch):
    """final_obs=True at K = 4: the rows of final_stack of the envs that ended, on every call; every other row keeps the bytes
    the test wrote.  Env i's first episode is i % 7 steps old at the start (injected step counts), so episodes end after 1, 2,
    ... 7 calls: ends before the pad has left the window (fewer than K - 1 calls), and on every ring phase."""
    K, n = 4, 70
    _short_episodes(monkeypatch, "Hallway", 7)
    first_steps = np.arange(n) % 7
    dones, _, _ = _drive("MiniWorld-Hallway-v0", n, K, pad, 16, 904, 3, p_fwd=0.6, final_obs=True, first_steps=first_steps)
    # env 6 ends on call 0, env 5 on call 1 (or earlier): their final stacks still show the pad
    assert dones[0, 6] and dones[:2, 5].any() and dones[:K - 1].any(axis=0).sum() >= 20
    assert {int(j) % K for j in np.flatnonzero(dones.any(axis=1))} == set(range(K))


def test_host_resets_refresh_only_their_envs(monkeypatch):
    """autoreset=False: a finished env keeps stacking its terminal state's frames until the host resets it — mw_reset(mask),
    mw_render, mw_stack_refresh; the refresh rebuilds those stacks alone and does not move the window."""
    import torch
    K, n, pad = 3, 70, "zero"
    _short_episodes(monkeypatch, "Hallway", 5)
    A, B = _pair("MiniWorld-Hallway-v0", n, K, pad, 905, False)
    rng = np.random.default_rng(905)
    hist = _rebuilt(_np(B.reset()), K, pad)
    A.reset()
    due, resets, kept_stacking = np.zeros(n, bool), 0, 0
    for j in range(17):
        act = torch.as_tensor(np.where(rng.random(n) < 0.6, 2, rng.integers(0, 3, n)), dtype=torch.int32, device="cuda")
        ra, rb = A.step(act), B.step(act)
        assert all(torch.equal(x, y) for x, y in zip(ra, rb)), j
        kept_stacking += int(due.sum())
        hist = np.concatenate([hist[:, 1:], _np(rb[0])[:, None]], axis=1)
        assert np.array_equal(_np(A.stack), hist), (j, "push")
        due |= (_np(rb[2]) | _np(rb[3])).astype(bool)
        if j % 2 == 1 and due.any():            # (every second call: the envs that ended on the call before take one more step first)
            before, window = _np(A.stack), A.engine.stack_window()
            for v in (A, B):
                v.engine.reset(due.astype(np.uint8), None)
                v.engine.render(v.obs)
            A.engine.stack_refresh(A.obs)
            assert torch.equal(A.obs, B.obs)
            got = _np(A.stack)
            assert A.engine.stack_window() == window
            assert np.array_equal(got[~due], before[~due]), (j, "a stack of an env that was not reset changed")
            hist[due] = _rebuilt(_np(B.obs)[due], K, pad)
            assert np.array_equal(got, hist), (j, "refresh")
            resets += int(due.sum())
            due[:] = False
    assert resets >= n and kept_stacking > 0 and (~due).any()
    for v in (A, B):
        v.engine.check()
        v.close()


def test_a_reset_without_refresh_is_rebuilt_by_the_next_push(monkeypatch):
    """mw_reset marks the envs it writes: without mw_stack_refresh their next push rebuilds their stacks."""
    import torch
    K, n, pad = 3, 13, "reset"
    A, B = _pair("MiniWorld-Hallway-v0", n, K, pad, 906, False)
    hist = _rebuilt(_np(B.reset()), K, pad)
    A.reset()
    act = torch.full((n,), 2, dtype=torch.int32, device="cuda")
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)
    for j in range(4):
        if j == 2:
            for v in (A, B):
                v.engine.reset(mask, None)
        o = _np(B.step(act)[0])
        assert torch.equal(A.step(act)[0], B.obs)
        hist = np.concatenate([hist[:, 1:], o[:, None]], axis=1)
        if j == 2:
            hist[mask.astype(bool)] = _rebuilt(o[mask.astype(bool)], K, pad)
        assert np.array_equal(_np(A.stack), hist), j
    for v in (A, B):
        v.close()


def test_set_state_cancels_the_pending_rebuild(monkeypatch):
    """Next-step mode: mw_set_state clears an env's pending reset, so its next call is an ordinary step — and an ordinary push."""
    import torch
    K, n, pad = 2, 9, "zero"
    _short_episodes(monkeypatch, "Hallway", 2)
    A, B = _pair("MiniWorld-Hallway-v0", n, K, pad, 907, "next_step")
    hist = _rebuilt(_np(B.reset()), K, pad)
    A.reset()
    act = torch.zeros(n, dtype=torch.int32, device="cuda")
    for j in range(2):
        hist = np.concatenate([hist[:, 1:], _np(B.step(act)[0])[:, None]], axis=1)
        A.step(act)
    assert _np(B.reset_pending()).all() and np.array_equal(_np(A.stack), hist)
    half = n // 2           # envs 0 .. half - 1 are written back as they are (step_count 0: the episode goes on), the others stay pending
    for v in (A, B):
        st = {k: a[:half] for k, a in v.engine.get_state().items()}
        st["step_count"] = np.zeros(half, np.int32)
        v.engine.set_state(st, 0, half)
    pend = _np(B.reset_pending()).astype(bool)
    assert not pend[:half].any() and pend[half:].all()
    o = _np(B.step(act)[0])
    assert torch.equal(A.step(act)[0], B.obs)
    hist = np.concatenate([hist[:, 1:], o[:, None]], axis=1)
    hist[pend] = _rebuilt(o[pend], K, pad)
    assert np.array_equal(_np(A.stack), hist)
    for v in (A, B):
        v.engine.check()
        v.close()


def test_pickup_objects_mesh_chain(monkeypatch):
    """PickupObjects x 6, K = 2: the mesh kernels and the raster kernel's two parts on two streams in front of the push."""
    _short_episodes(monkeypatch, "PickupObjects", 4)
    dones, _, _ = _drive("MiniWorld-PickupObjects-v0", 6, 2, "reset", 10, 908, 5)
    assert dones.any()


def test_the_stack_is_a_view_of_the_ring():
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    K, n = 4, 5
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, frame_stack=K)
    vec.reset()
    act = torch.zeros(n, dtype=torch.int32, device="cuda")
    ring_ptr = vec._ring.untyped_storage().data_ptr()
    for j in range(2 * K + 1):
        vec.step(act)
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        st = vec.stack
        assert torch.cuda.memory_allocated() == held, "reading vec.stack allocated device memory"
        assert st.untyped_storage().data_ptr() == ring_ptr and tuple(st.shape) == (n, K, 60, 80, 3)
        assert st.data_ptr() == vec._ring[:, j % K].data_ptr() and st.stride() == vec._ring.stride()
    vec.close()


def test_errors_leave_the_stack_alone():
    """A push under another layout than the stack's is MW_E_INVALID before anything is launched; bad arguments of
    mw_set_frame_stack change nothing; a top view, which switches the layout for its own frame, pushes nothing and stays legal."""
    import torch
    from miniworld_amd import engine as eng
    from miniworld_amd.vec_env import MiniWorldVecEnv
    K, n = 3, 7
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, frame_stack=K, obs_layout="cwh")
    vec.reset()
    act = torch.zeros(n, dtype=torch.int32, device="cuda")         # (turns: no episode ends)
    vec.step(act)
    stack0, obs0, state0, window0 = vec.stack.clone(), vec.obs.clone(), vec.engine.get_state(), vec.engine.stack_window()
    assert window0 == (0, 1)
    top = vec.render_top_view()
    assert tuple(top.shape) == (n, 60, 80, 3) and vec.engine.stack_window() == window0 and torch.equal(vec.stack, stack0)
    vec.engine.set_obs_layout(eng.OBS_HWC_U8)
    hwc = vec.engine.obs_buffer()
    for call in (lambda: vec.engine.step(act, hwc, None, vec.reward, vec.terminated, vec.truncated),
                 lambda: vec.engine.step_repeat(act, 2, hwc, None, vec.reward, vec.terminated, vec.truncated),
                 lambda: vec.engine.stack_refresh(hwc)):
        with pytest.raises(eng.EngineError, match=r"\(-1\).*layout"):
            call()
    vec.engine.set_obs_layout(eng.OBS_CWH_U8)
    lib, h = vec.engine.lib, vec.engine.h
    ptr = C_.c_void_p(vec._ring.data_ptr())
    for depth, pad in ((1, 0), (17, 0), (-3, 0), (K, 2), (K, -1)):
        assert lib.mw_set_frame_stack(h, depth, pad, ptr, None) == -1, (depth, pad)
    torch.cuda.synchronize()
    state1 = vec.engine.get_state()
    assert vec.engine.stack_window() == window0 and torch.equal(vec.stack, stack0) and torch.equal(vec.obs, obs0)
    assert all(np.array_equal(state0[k], state1[k]) for k in state0) and not hwc.any()
    # ... and the stack goes on where it was
    ref = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, obs_layout="cwh")
    ref.reset()
    ref.step(act)
    first = ref.obs.clone()
    ref.step(act)
    vec.step(act)
    assert vec.engine.stack_window() == (1, 2)
    assert torch.equal(vec.stack[:, 2], ref.obs) and torch.equal(vec.stack[:, 1], first) and torch.equal(vec.obs, ref.obs)
    # a final stack needs final observations' engine: same-step with a generator
    off = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, autoreset=False)
    ring = torch.zeros((n, 3, 60, 80, 3), dtype=torch.uint8, device="cuda")
    fin = torch.zeros((n, 2, 60, 80, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(eng.EngineError):
        off.engine.set_frame_stack(2, eng.STACK_PAD_RESET, ring, fin)
    with pytest.raises(eng.EngineError):
        off.engine.stack_window()       # no stack was set
    off.engine.set_frame_stack(2, eng.STACK_PAD_RESET, ring)
    assert off.engine.stack_window() == (1, 0)
    off.engine.set_frame_stack(0)
    with pytest.raises(eng.EngineError):
        off.engine.stack_refresh(off.obs)
    for v in (vec, ref, off):
        v.engine.check()
        v.close()


@pytest.mark.parametrize("mode", ["same_step", "next_step"])
def test_steps_without_reward_and_flag_outputs_equal_steps_with_them(mode):
    """reward, terminated and truncated are optional in mw_step, mw_step_repeat and mw_step_plan: the engine's scratch stands in.  Twin
    A passes its three tensors, twin B passes None for all of them, through every kind of call (a step, a repeat of 3, a drawn plan of 3
    and a frameless one), always moving forward so that envs reach their boxes and worlds are installed — where the stack's push
    and the frameless call's flag kernel read the flags the step kernel wrote.  obs, the stack view and the whole state must stay equal
    bit for bit after every call, and at least one episode of A must have terminated."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n, calls, forward = 8, 120, 2
    A, B = (MiniWorldVecEnv("MiniWorld-Hallway-v0", n, seed=3, autoreset=mode, frame_stack=2) for _ in range(2))
    assert torch.equal(A.reset(), B.reset()) and torch.equal(A.stack, B.stack)
    act = torch.full((n,), forward, dtype=torch.int32, device="cuda")
    plans = torch.full((3, n), forward, dtype=torch.int32, device="cuda")
    terminated = 0
    for j in range(calls):
        kind = j % 4
        for v, outs in ((A, (A.reward, A.terminated, A.truncated)), (B, (None, None, None))):
            if kind == 0:
                v.engine.step(act, v.obs, None, *outs)
            elif kind == 1:
                v.engine.step_repeat(act, 3, v.obs, None, *outs)
            else:
                v.engine.step_plan(plans, v.obs if kind == 2 else None, None, outs[0], None, outs[1], outs[2])
        terminated += int(A.terminated.sum())
        assert torch.equal(A.obs, B.obs), (j, "obs")
        assert torch.equal(A.stack, B.stack), (j, "stack")
        sa, sb = A.engine.get_state(), B.engine.get_state()
        assert sa.keys() == sb.keys()
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), (j, k)
    print(f"{mode}: {terminated} terminated flags over {calls} calls")
    A.engine.check(); B.engine.check()
    assert terminated >= 1, "no episode terminated: lengthen the run"
