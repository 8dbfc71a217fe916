"""Frame records on the device (mw_snapshot_save_frames / mw_snapshot_load_frames; save_state(frames=True), load_state, fork(src,
frames=True)): a restored or forked env shows what its source showed — observation, depth and frame stack — without a frame being
drawn, and continues like it.

Everything here is a copy, so there are no tolerances.  The yardsticks are the frames the source itself returned (kept by the test
before the load), a twin engine that reached the same state through the entry points that were there before (the construction of
tests/test_gpu_snapshot.py), and a host-side list of the last K returned frames per env."""
import ctypes as C_

import numpy as np
import pytest

from test_gpu_snapshot import ACTION_PICKUP, _actions, _ends, _make, _np, _rebuilt, _short_episodes, _step

pytestmark = pytest.mark.gpu

SNAPF_DEPTH, SNAPF_STACK = 1, 2
HALLWAY = "MiniWorld-Hallway-v0"


def _seen(v, rows=None):
    """what the agent of each env sees, as host copies: observation, depth, stack (window order)"""
    out = {"obs": _np(v.obs).copy(), "stack": _np(v.stack).copy()}
    if v.depth is not None:
        out["depth"] = _np(v.depth).copy()
    return out if rows is None else {k: a[rows] for k, a in out.items()}


def _same_seen(got, want, tag):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), tag + (k,)


def _same_call(A, B, tag, rows_a=None, rows_b=None):
    """everything a step hands out, A's rows against B's"""
    ra = slice(None) if rows_a is None else rows_a
    rb = slice(None) if rows_b is None else rows_b
    for name in ("obs", "depth", "reward", "terminated", "truncated", "stack"):
        a, b = getattr(A, name), getattr(B, name)
        if a is None and b is None:
            continue
        assert np.array_equal(_np(a)[ra], _np(b)[rb]), tag + (name,)
    assert np.array_equal(_np(A.reset_pending())[ra], _np(B.reset_pending())[rb]), tag + ("reset_pending",)


def _push(hist, v, K, pad):
    """the host-side model of a stack behind a same-step call: the last K returned frames, restarted per episode by the pad"""
    obs, done = _np(v.obs), _ends(v)
    hist = np.concatenate([hist[:, 1:], obs[:, None]], axis=1)
    hist[done] = _rebuilt(obs[done], K, pad)
    return hist


# ---------------------------------------------------------------------------------------------------------------- 1. fork

@pytest.mark.parametrize("pad", ["reset", "zero"])
def test_a_fork_carries_what_the_agent_saw(pad, monkeypatch):
    """fork(src, frames=True): env j shows what env src[j] showed and, given the same actions, goes on showing it — against a twin
    whose env j was seeded like env src[j] and fed its actions (same K: its stack is the expected one)."""
    import torch
    _short_episodes(monkeypatch, "Hallway", 7)
    n, K, T, seed = 9, 3, 7, 4100
    src = np.array([3, 3, 3, 0, 1, 7, 7, 5, 8])
    rng = np.random.default_rng(seed)
    acts = _actions(rng, 2 * T, n, 3, 0.6)
    kw = dict(frame_stack=K, stack_pad=pad, want_depth=True)
    A, Cv = _make(HALLWAY, n, seed, **kw), _make(HALLWAY, n, seed + 500, **kw)
    A.reset()
    Cv.engine.reset(None, (seed + src).astype(np.uint64))
    Cv.engine.render(Cv.obs, Cv.depth)
    Cv.engine.stack_refresh(Cv.obs)
    for t in range(T):
        _step(A, acts[t])
        _step(Cv, acts[t][src])
    before, window = _seen(A), A.engine.stack_window()
    reward, term = A.reward.clone(), A.terminated.clone()
    obs = A.fork(torch.as_tensor(src, device="cuda"), frames=True)
    assert obs is A.obs and torch.equal(A.reward, reward) and torch.equal(A.terminated, term)
    assert A.engine.stack_window() == window, "the ring position moved"
    _same_seen(_seen(A), {k: a[src] for k, a in before.items()}, ("after the fork",))
    assert not np.array_equal(before["obs"][0], before["obs"][3]), "the sources differ: the copy is visible"
    _same_seen(_seen(A), _seen(Cv), ("after the fork", "twin"))
    ends = np.zeros(n, int)
    for t in range(T, 2 * T):
        _step(A, acts[t])
        _step(Cv, acts[t])
        _same_call(A, Cv, ("call", t))
        ends += _ends(A)
    assert ends.min() >= 1
    for v in (A, Cv):
        v.engine.check()
        v.close()


# ---------------------------------------------------------------------------------------------------------------- 2. ring phase

def _round_trips(v, K, pad, acts):
    """One save with frames; then for every ring phase q: step until the push count is q mod K (1 .. K calls), load, compare with what
    the save saw, and follow 2K more calls with the host model.  The load restores the random stream too, so every round replays."""
    snap, saved, pushes_at_save = v.save_state(frames=True), _seen(v), v.engine.stack_window()[1]
    t, shifts = 0, set()
    for q in range(K):
        m = 0
        while m == 0 or v.engine.stack_window()[1] % K != q:
            _step(v, acts[t % len(acts)])
            t, m = t + 1, m + 1
        assert 1 <= m <= K
        window = v.engine.stack_window()
        shifts.add((window[1] - pushes_at_save) % K)
        assert not np.array_equal(_np(v.obs), saved["obs"])
        assert v.load_state(snap) is v.obs
        assert v.engine.stack_window() == window, "the ring position moved"
        _same_seen(_seen(v), saved, ("phase", q, "after the load"))
        hist = saved["stack"].copy()
        for i in range(2 * K):
            _step(v, acts[(20 + i) % len(acts)])
            hist = _push(hist, v, K, pad)
            assert np.array_equal(_np(v.stack), hist), ("phase", q, "call", i, "a later window (the mirror slots)")
    assert shifts == set(range(K)), "the loads met every ring phase relative to the save"


@pytest.mark.parametrize("K, pad", [(2, "reset"), (3, "zero"), (3, "reset")])
def test_the_ring_phase_does_not_matter(K, pad, monkeypatch):
    _short_episodes(monkeypatch, "Hallway", 7)
    n, seed = 5, 4200 + K
    acts = _actions(np.random.default_rng(seed), 40, n, 3, 0.6)
    A = _make(HALLWAY, n, seed, frame_stack=K, stack_pad=pad, want_depth=True)
    A.reset()
    for j in range(4):
        _step(A, acts[30 + j])
    _round_trips(A, K, pad, acts)
    A.engine.check()
    A.close()


# ---------------------------------------------------------------------------------------------------------------- 3. partial load

def test_a_partial_load_writes_its_envs_only(monkeypatch):
    _short_episodes(monkeypatch, "Hallway", 7)
    n, K, seed = 9, 3, 4300
    acts = _actions(np.random.default_rng(seed), 8, n, 3, 0.6)
    A = _make(HALLWAY, n, seed, frame_stack=K, want_depth=True)
    A.reset()
    for t in range(5):
        _step(A, acts[t])
    snap = A.save_state([7], capacity=2, frames=True)       # (one record, laid out for the two envs one call loads it into)
    assert (snap.count, snap.capacity, snap.frame_flags, snap.frame_stack) == (1, 2, SNAPF_DEPTH | SNAPF_STACK, K)
    assert snap.frames.numel() == A.engine.snapshot_frames_bytes(2, SNAPF_DEPTH | SNAPF_STACK)
    seven = _seen(A, [7])
    _step(A, acts[5])
    _step(A, acts[6])
    before, ring = _seen(A), _np(A._ring).copy()
    A.load_state(snap, envs=[2, 5], records=[0, 0])
    after, others = _seen(A), [0, 1, 3, 4, 6, 7, 8]
    for k in after:
        assert np.array_equal(after[k][others], before[k][others]), ("an env that was not loaded changed", k)
        assert np.array_equal(after[k][2], seven[k][0]) and np.array_equal(after[k][5], seven[k][0]), ("the copies show record 0", k)
    assert not np.array_equal(after["obs"][2], before["obs"][2])
    assert np.array_equal(_np(A._ring)[others], ring[others]), "a ring row of an env that was not loaded changed"
    A.engine.check()
    A.close()


# ---------------------------------------------------------------------------------------------------------------- 4. layouts

@pytest.mark.parametrize("kw, frame_bytes", [(dict(obs_width=81, obs_height=61), 14823), (dict(obs_layout="cwh"), 14400),
                                             (dict(obs_layout="grey"), 38400)])
def test_the_byte_path_and_the_other_layouts(kw, frame_bytes, monkeypatch):
    """81 x 61: 14 823 bytes per frame and 19 764 per depth map, the byte units of the kernel; cwh and grey (float64): 16-byte units"""
    _short_episodes(monkeypatch, "Hallway", 7)
    n, K, seed = 3, 2, 4400
    acts = _actions(np.random.default_rng(seed), 40, n, 3, 0.6)
    A = _make(HALLWAY, n, seed, frame_stack=K, stack_pad="zero", want_depth=True, **kw)
    assert A.obs[0].numel() * A.obs.element_size() == frame_bytes
    A.reset()
    for j in range(3):
        _step(A, acts[30 + j])
    _round_trips(A, K, "zero", acts)
    A.engine.check()
    A.close()


# ---------------------------------------------------------------------------------------------------------------- 5. pickup

def test_a_pickup_shows_the_object_one_last_time():
    """The frame a pickup step returns still shows the object; the state no longer holds it.  A load with frames gives that frame back;
    a redraw of the restored state does not show the object — the difference the frame records exist for."""
    import torch
    n, K, T, seed, env_id = 5, 2, 3, 4500, "MiniWorld-PickupObjects-v0"
    acts = _actions(np.random.default_rng(seed), T + 6, n, 3, None)        # (turns and moves; the one pickup is injected)
    A, B = (_make(env_id, n, seed, frame_stack=K, want_depth=True) for _ in range(2))
    for v in (A, B):
        v.reset()
        for t in range(T):
            if t == T - 1:
                # env 0 picks an object up: put 1.5 radii in front of it, facing it (tests/test_gpu_snapshot.py: pickup_before_save)
                st = v.engine.get_state(0, 1)
                slot = int(np.flatnonzero(st["ent_kind"][0])[0])
                pos = st["agent_pos"].copy()
                pos[0, 0], pos[0, 2] = st["ent_pos"][0, slot, 0] - 1.5 * 0.4, st["ent_pos"][0, slot, 2]
                v.engine.set_state({"agent_pos": pos, "agent_dir": np.zeros(1)}, 0, 1)
                acts[t, 0] = ACTION_PICKUP
                picked0 = int(st["num_picked_up"][0])
            _step(v, acts[t])
        assert v.engine.get_state(0, 1)["num_picked_up"][0] == picked0 + 1
    returned = _seen(A)
    _same_seen(_seen(B), returned, ("the two runs agree at the save",))
    snap = A.save_state(frames=True)
    for t in range(T, T + 3):
        _step(A, (acts[t] + 1) % 3)
    A.load_state(snap)
    _same_seen(_seen(A), returned, ("the load gives back the frames the pickup step returned",))
    fresh, fresh_depth = torch.zeros_like(A.obs), torch.zeros_like(A.depth)
    A.engine.render(fresh, fresh_depth)
    fresh = _np(fresh)
    assert not np.array_equal(fresh[0], returned["obs"][0]), "a redraw of the restored state still shows the picked-up object"
    assert np.array_equal(fresh[1:], returned["obs"][1:]), "without a pickup the redraw is the returned frame"
    for t in range(T, T + 6):
        _step(A, acts[t])
        _step(B, acts[t])
        _same_call(A, B, ("call", t))
    for v in (A, B):
        v.engine.check()
        v.close()


# ---------------------------------------------------------------------------------------------------------------- 6. across engines

def test_frame_records_travel_between_engines(monkeypatch):
    """9 envs -> the host -> 4 envs at another ring position: records are compatible whatever num_envs and the push count are"""
    _short_episodes(monkeypatch, "Hallway", 7)
    n, K, T, seed = 9, 3, 7, 4600
    recs = [8, 8, 0, 3]
    acts = _actions(np.random.default_rng(seed), 2 * T, n, 3, 0.6)
    kw = dict(frame_stack=K, want_depth=True)
    A, B = _make(HALLWAY, n, seed, **kw), _make(HALLWAY, 4, seed + 77, **kw)
    A.reset()
    B.reset()
    for t in range(T):
        _step(A, acts[t])
    for t in range(2):
        _step(B, acts[t][:4])
    assert A.engine.stack_window()[0] != B.engine.stack_window()[0], "the two rings stand at different phases"
    snap = A.save_state(frames=True)
    moved = type(snap).from_state_dict(snap.cpu().state_dict())
    assert moved.frames.device.type == "cpu" and (moved.frame_flags, moved.frame_stack) == (SNAPF_DEPTH | SNAPF_STACK, K)
    window = B.engine.stack_window()
    B.load_state(moved, envs=[0, 1, 2, 3], records=recs)
    assert B.engine.stack_window() == window
    _same_seen(_seen(B), _seen(A, recs), ("after the load",))
    for t in range(T, 2 * T):
        _step(A, acts[t])
        _step(B, acts[t][recs])
        _same_call(B, A, ("call", t), rows_b=recs)
    for v in (A, B):
        v.engine.check()
        v.close()


# ---------------------------------------------------------------------------------------------------------------- 7. pending resets

@pytest.mark.parametrize("pad", ["reset", "zero"])
def test_a_pending_next_step_reset_travels_with_the_stack(pad, monkeypatch):
    """A save on the call that ends an episode (autoreset="next_step": reset_pending set, the stack marked for a rebuild): behind the
    load the env's next call installs its world and rebuilds its stack from that first frame, as it would have in the source."""
    _short_episodes(monkeypatch, "Hallway", 7)
    n, K, seed = 9, 3, 4700
    acts = _actions(np.random.default_rng(seed), 20, n, 3, 0.3)
    kw = dict(frame_stack=K, stack_pad=pad, want_depth=True, autoreset="next_step")
    A, R = _make(HALLWAY, n, seed, **kw), _make(HALLWAY, n, seed, **kw)
    for v in (A, R):
        v.reset()
        v.engine.set_state({"step_count": (np.arange(n) % 7).astype(np.int32)})     # episodes that end on different calls
        for t in range(4):
            _step(v, acts[t])
    pend = _np(A.reset_pending()).astype(bool)
    assert pend.any() and not pend.all(), "the save is taken while some envs, not all, have a reset pending"
    snap, saved = A.save_state(frames=True), _seen(A)
    for t in range(4, 6):
        _step(A, acts[t])
    A.load_state(snap)
    _same_seen(_seen(A), saved, ("after the load",))
    _same_seen(_seen(A), _seen(R), ("after the load", "twin"))      # (rewards and flags are the last call's: a load leaves them alone)
    assert np.array_equal(_np(A.reset_pending()).astype(bool), pend)
    for t in range(6, 6 + 2 * K):
        _step(A, acts[t])
        _step(R, acts[t])
        _same_call(A, R, ("call", t))
        if t == 6:
            assert np.array_equal(_np(A.stack)[pend], _rebuilt(_np(A.obs)[pend], K, pad)), "the pending envs' stacks start over"
            assert not np.array_equal(_np(A.stack)[~pend], _rebuilt(_np(A.obs)[~pend], K, pad))
    for v in (A, R):
        v.engine.check()
        v.close()


# ---------------------------------------------------------------------------------------------------------------- 8. refusals

def test_refused_calls_launch_nothing():
    import torch
    from miniworld_amd import engine as eng
    n, K = 9, 2
    A, P = _make(HALLWAY, n, 4800, want_depth=True, frame_stack=K), _make(HALLWAY, n, 4801)       # P: no stack, no depth
    for v in (A, P):
        v.reset()
        _step(v, np.full(n, 2))
    e, lib, h = A.engine, A.engine.lib, A.engine.h
    both = SNAPF_DEPTH | SNAPF_STACK
    # the size: the header, then every section its records, padded to 16 bytes (tests/test_snapshot_frames_cpu.py pins the layout)
    fb, db = 80 * 60 * 3, 80 * 60 * 4
    for cap in (0, 1, n, 100):
        for flags in (0, SNAPF_DEPTH, SNAPF_STACK, both):
            parts = [fb] + ([db] if flags & SNAPF_DEPTH else []) + ([K * fb, 1] if flags & SNAPF_STACK else [])
            assert e.snapshot_frames_bytes(cap, flags) == 64 + sum((cap * part + 15) // 16 * 16 for part in parts), (cap, flags)
    cap = n
    buf = torch.zeros(e.snapshot_frames_bytes(cap + 1, both), dtype=torch.uint8, device="cuda")
    e.snapshot_save_frames(buf, cap, A.obs, A.depth, both)
    _step(A, np.full(n, 0))
    seen0, ring0, buf0 = _seen(A), A._ring.clone(), buf.clone()
    stream = eng._stream_ptr(e.device)
    p, o, d = (C_.c_void_p(t.data_ptr()) for t in (buf, A.obs, A.depth))
    idx = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    ip = C_.c_void_p(idx.data_ptr())
    assert lib.mw_snapshot_frames_bytes(h, -1, 0) < 0 and lib.mw_snapshot_frames_bytes(h, 4, 4) < 0
    assert lib.mw_snapshot_frames_bytes(P.engine.h, 4, SNAPF_STACK) < 0
    bad = [lib.mw_snapshot_save_frames(h, None, 1, o, d, None, cap, both, stream),                  # a null frame buffer
           lib.mw_snapshot_save_frames(h, None, 1, None, d, p, cap, both, stream),                  # a null d_obs
           lib.mw_snapshot_save_frames(h, None, 1, o, d, C_.c_void_p(buf.data_ptr() + 4), cap, both, stream),       # misaligned
           lib.mw_snapshot_save_frames(h, None, -1, o, d, p, cap, both, stream),                    # count < 0
           lib.mw_snapshot_save_frames(h, ip, cap + 1, o, d, p, cap, both, stream),                 # count > capacity
           lib.mw_snapshot_save_frames(h, None, n + 1, o, d, p, n + 1, both, stream),               # count > N on a save of envs 0 .. count - 1
           lib.mw_snapshot_save_frames(h, None, 1, o, d, p, cap, 4, stream),                        # an unknown flag bit
           lib.mw_snapshot_save_frames(h, None, 1, o, None, p, cap, both, stream),                  # MW_SNAPF_DEPTH without d_depth
           lib.mw_snapshot_save_frames(P.engine.h, None, 1, o, None, p, cap, SNAPF_STACK, stream),  # MW_SNAPF_STACK without a stack
           lib.mw_snapshot_load_frames(h, None, None, 1, None, 1, cap, both, o, d, stream),
           lib.mw_snapshot_load_frames(h, None, None, 1, p, 1, cap, both, None, d, stream),
           lib.mw_snapshot_load_frames(h, None, None, 1, C_.c_void_p(buf.data_ptr() + 4), 1, cap, both, o, d, stream),
           lib.mw_snapshot_load_frames(h, None, None, -1, p, 1, cap, both, o, d, stream),
           lib.mw_snapshot_load_frames(h, ip, ip, n + 1, p, n + 1, n + 1, both, o, d, stream),      # count > N on a load
           lib.mw_snapshot_load_frames(h, None, None, 1, p, cap + 1, cap, both, o, d, stream),      # n_recs > capacity
           lib.mw_snapshot_load_frames(h, None, None, 2, p, 2, 1, both, o, d, stream),              # count > capacity
           lib.mw_snapshot_load_frames(h, None, None, 1, p, 1, cap, 8, o, d, stream),
           lib.mw_snapshot_load_frames(h, None, None, 1, p, 1, cap, both, o, None, stream),
           lib.mw_snapshot_load_frames(P.engine.h, None, None, 1, p, 1, cap, SNAPF_STACK, o, None, stream)]
    assert bad == [-1] * len(bad), bad
    assert b"mw_snapshot_load_frames" in lib.mw_last_error(P.engine.h)
    # the stack was set under "hwc": in another layout its frames are refused
    e.set_obs_layout(eng.OBS_CWH_U8)
    assert lib.mw_snapshot_save_frames(h, None, 1, o, d, p, cap, both, stream) == -1
    assert lib.mw_snapshot_load_frames(h, None, None, 1, p, 1, cap, both, o, d, stream) == -1
    assert b"layout" in lib.mw_last_error(h)
    assert lib.mw_snapshot_frames_bytes(h, cap, both) < 0 and lib.mw_snapshot_frames_bytes(h, cap, SNAPF_DEPTH) > 0
    e.set_obs_layout(eng.OBS_HWC_U8)
    torch.cuda.synchronize()
    for v in (A, P):
        v.engine.check()
    _same_seen(_seen(A), seen0, ("a refused call changed a frame",))
    assert torch.equal(buf, buf0) and torch.equal(A._ring, ring0), "a refused call wrote to a buffer"
    for v in (A, P):
        v.close()


@pytest.mark.parametrize("case", ["env out of range", "record out of range", "other flags", "zeroed buffer"])
def test_bad_items_write_nothing_and_are_reported(case):
    """On the device: an offending item (or, with a key that does not match, every item) writes nothing and mw_check reports it; a
    valid item of the same call is loaded."""
    import torch
    from miniworld_amd import engine as eng
    n, K, both = 4, 2, SNAPF_DEPTH | SNAPF_STACK
    v = _make(HALLWAY, n, 4810, want_depth=True, frame_stack=K)
    e = v.engine
    v.reset()
    _step(v, np.full(n, 2))
    # n records in a buffer with room for one more: record n, which the engine is told does not exist, is memory of the test's either way
    room = torch.zeros(e.snapshot_frames_bytes(n + 1, both), dtype=torch.uint8, device="cuda")
    e.snapshot_save_frames(room, n, v.obs, v.depth, both)
    depth_only = torch.zeros(e.snapshot_frames_bytes(n, SNAPF_DEPTH), dtype=torch.uint8, device="cuda")
    e.snapshot_save_frames(depth_only, n, v.obs, v.depth, SNAPF_DEPTH)
    _step(v, np.full(n, 0))
    e.check()
    seen0, ring0 = _seen(v), _np(v._ring).copy()
    if case == "env out of range":
        e.snapshot_load_frames(room, n, n, v.obs, v.depth, both, envs=[1, n], records=[0, 2])
        loaded = [1]
    elif case == "record out of range":
        e.snapshot_load_frames(room, n, n, v.obs, v.depth, both, envs=[2, 1], records=[n, 1])
        loaded = [1]
    elif case == "other flags":
        e.snapshot_load_frames(depth_only, n, n, v.obs, None, 0)        # saved with MW_SNAPF_DEPTH, loaded with flags 0: another key
        loaded = []
    else:
        e.snapshot_load_frames(torch.zeros_like(room), n, n, v.obs, v.depth, both)
        loaded = []
    torch.cuda.synchronize()
    with pytest.raises(eng.EngineError, match=r"\(-1\).*mw_snapshot_load_frames.*key"):
        e.check()
    untouched = [i for i in range(n) if i not in loaded]
    _same_seen(_seen(v, untouched), {k: a[untouched] for k, a in seen0.items()}, (case, "a skipped item wrote a frame"))
    assert np.array_equal(_np(v._ring)[untouched], ring0[untouched]), (case, "a skipped item wrote a ring row")
    for i in loaded:
        assert not np.array_equal(_np(v.obs)[i], seen0["obs"][i]), "the valid item of the same call was loaded"
    v.close()


# ---------------------------------------------------------------------------------------------------------------- 9. defaults

def test_the_defaults_did_not_move(monkeypatch):
    """fork(src) and a load of a snapshot without frames still draw the frames and rebuild the stacks
    (tests/test_gpu_snapshot.py::test_frame_stacks_are_rebuilt_for_the_loaded_envs pins the rest)"""
    import torch
    _short_episodes(monkeypatch, "Hallway", 7)
    n, K, seed = 9, 3, 4900
    acts = _actions(np.random.default_rng(seed), 6, n, 3, 0.6)
    A = _make(HALLWAY, n, seed, frame_stack=K)
    A.reset()
    for t in range(5):
        _step(A, acts[t])
    snap = A.save_state()
    assert snap.frames is None and (snap.frame_flags, snap.frame_stack) == (0, 0)
    _step(A, acts[5])
    A.load_state(snap)
    assert np.array_equal(_np(A.stack), _rebuilt(_np(A.obs), K, "reset"))
    _step(A, acts[5])
    A.fork(torch.as_tensor([3, 3, 3, 0, 1, 7, 7, 5, 8], device="cuda"))
    assert np.array_equal(_np(A.stack), _rebuilt(_np(A.obs), K, "reset"))
    A.engine.check()
    A.close()
