"""Snapshot records on the device (mw_snapshot_save / mw_snapshot_load; MiniWorldVecEnv.save_state / load_state / fork): a restored or
forked env continues bit for bit as the env its record was taken from would have — observation, depth, reward, flags, sub-steps,
infos, final infos, pending resets, the device state and, for the Maze, every env's geometry.

The yardstick is never the copy kernels.  It is a second engine that reached the same state through the entry points that were
there before: the run the record was taken from itself (resume, subset, "saving changes nothing"), or an engine whose env j was
seeded like the fork's source and fed the source's actions (fork).  There are no tolerances.

Episodes are shortened (_short_episodes, the Maze's max_episode_steps) so that every env ends at least two episodes inside each
window of calls: the random stream, the spare world and the auto-reset are all exercised behind a load."""
import ctypes as C_

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _short_episodes(monkeypatch, cls_name, steps):
    """Episodes of at most `steps` steps for a family whose class fixes max_episode_steps (the way tests/test_gpu_frame_stack.py
    does it): the batched env reads it from its template instance."""
    from miniworld_amd import envs
    base = getattr(envs, cls_name)

    class Short(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.max_episode_steps = steps
    Short.__name__ = Short.__qualname__ = cls_name
    monkeypatch.setattr(envs, cls_name, Short)


def _np(t):
    return t.cpu().numpy()


def _make(env_id, n, seed, **kw):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    return MiniWorldVecEnv(env_id, n, seed=seed, **kw)


def _actions(rng, calls, n, n_actions, p_fwd):
    if p_fwd is None:
        return rng.integers(0, n_actions, (calls, n))
    return np.where(rng.random((calls, n)) < p_fwd, 2, rng.integers(0, n_actions, (calls, n)))


def _step(v, act, repeat=1):
    import torch
    return v.step(torch.as_tensor(np.ascontiguousarray(act), dtype=torch.int32, device="cuda"), repeat)


def _everything(v, stepped, geometry, rendered=False):
    """Everything an env hands out, as host arrays.  stepped: the last call was a step (reward, flags and sub-steps are that
    call's; a load leaves them alone, so they are not compared behind one).  geometry: every env's own set (the Maze).
    rendered: observation and depth are a fresh mw_render of the state into buffers of the test's, not the last step's frame —
    what a load or fork is compared with: a step's frame shows a picked-up object one last time, the state no longer holds it."""
    import torch
    obs, depth = v.obs, v.depth
    if rendered:
        obs, depth = torch.zeros_like(v.obs), (None if v.depth is None else torch.zeros_like(v.depth))
        v.engine.render(obs, depth)
    out = {"obs": _np(obs), "reset_pending": _np(v.reset_pending())}
    if depth is not None:
        out["depth"] = _np(depth)
    if stepped:
        out.update(reward=_np(v.reward), terminated=_np(v.terminated), truncated=_np(v.truncated))
        if v.substeps is not None:
            out["substeps"] = _np(v.substeps)
        if v.final_obs is not None:     # the rows of the envs whose episode ended in this call (the others keep what they held)
            done = (out["terminated"] | out["truncated"]).astype(bool)
            out["final_obs"] = _np(v.final_obs)[done]
    out.update({"info." + k: _np(t) for k, t in v.infos().items()})
    out.update({"final_info." + k: _np(t) for k, t in v.final_infos().items()})
    out.update({"state." + k: a for k, a in v.engine.get_state().items()})
    if geometry:
        for i in range(v.num_envs):
            polys, segs = v.engine.get_geometry(i)
            out[f"polys.{i}"], out[f"segs.{i}"] = polys, segs
    return out


def _assert_same(got, want, tag, rows=None):
    """rows: compare these envs' rows only (per-env arrays; the geometry of other envs is skipped)"""
    assert got.keys() == want.keys(), tag + (sorted(set(got) ^ set(want)),)
    for k in want:
        g, w = got[k], want[k]
        if rows is not None:
            if k.startswith(("polys.", "segs.")):
                if int(k.split(".")[1]) not in rows:
                    continue
            elif k != "final_obs":
                g, w = g[rows], w[rows]
            else:
                continue
        assert g.shape == w.shape and np.array_equal(g, w), tag + (k,)


def _record_rows(v, snap, comp_id, spares):
    """rows [rows][capacity] of one int32 component of a snapshot, found through the host build of the layout
    (tests/hostcheck/snapshot_layout.cpp); comp_id: the MW_SC_* number of miniworld_amd/csrc/mw_snapshot.h"""
    from test_snapshot_cpu import layout_lib, sections, snap_config
    c = v.engine.cfg
    cfg = snap_config(v.engine.E, c.max_polys, c.max_segs, c.shared_geometry, c.task, c.generator, c.rng_mode, spares)
    lib = layout_lib()
    assert lib.mwsnap_bytes(cfg.ctypes.data, snap.capacity) == snap.data.numel()
    off, size, _, ident = sections(lib, cfg, snap.capacity)
    k = list(ident).index(comp_id)
    return _np(snap.data)[off[k]:off[k] + size[k]].view(np.int32).reshape(-1, snap.capacity)


SC_PENDING_REMOVE, REMOVE_APPLIED, ACTION_PICKUP = 20, -2, 4


def _ends(v):
    return (_np(v.terminated) | _np(v.truncated)).astype(bool)


# ---------------------------------------------------------------------------------------------------------------- 1. resume

def _resume(monkeypatch, env_id, n, T, seed, n_actions, short=None, p_fwd=None, repeat=1, geometry=False, first_steps=None,
            want_pending=False, through_host=False, pickup_before_save=False, **kw):
    """A: reset(seed), 2T calls, save_state() after call T.  B: a fresh engine of the same configuration with a past of its own,
    then load_state(snap) and A's actions T + 1 .. 2T.  B equals A after the load and after every call."""
    if short:
        _short_episodes(monkeypatch, *short)
    rng = np.random.default_rng(seed)
    acts = _actions(rng, 2 * T, n, n_actions, p_fwd)
    A, B = _make(env_id, n, seed, **kw), _make(env_id, n, seed + 1000, **kw)
    A.reset()
    if first_steps is not None:     # episodes that end on different calls (mw_set_state: mid-episode injection)
        A.engine.set_state({"step_count": np.asarray(first_steps, np.int32)})
    ends1 = np.zeros(n, int)
    for t in range(T):
        if pickup_before_save and t == T - 1:
            # env 0 picks an object up on the last call before the save: the agent is put 1.5 radii in front of it, facing it
            # (mw_set_state: mid-episode injection), and its action is "pickup" (miniworld.py:708-716)
            st = A.engine.get_state(0, 1)
            slot = int(np.flatnonzero(st["ent_kind"][0])[0])
            pos = st["agent_pos"].copy()
            pos[0, 0], pos[0, 2] = st["ent_pos"][0, slot, 0] - 1.5 * 0.4, st["ent_pos"][0, slot, 2]
            A.engine.set_state({"agent_pos": pos, "agent_dir": np.zeros(1)}, 0, 1)
            acts[t, 0] = ACTION_PICKUP
            picked0 = int(st["num_picked_up"][0])
        _step(A, acts[t], repeat)
        ends1 += _ends(A)
    if want_pending:
        pend = _np(A.reset_pending()).astype(bool)
        assert pend.any() and not pend.all(), "the save is taken while some envs, not all, have a reset pending"
    snap = A.save_state()
    assert (snap.count, snap.capacity) == (n, n) and snap.data.numel() == A.engine.snapshot_bytes(n)
    if pickup_before_save:
        # The records hold both values pending_remove can have BETWEEN calls: -1 (nothing) and MW_REMOVE_APPLIED (the object the
        # last frame showed for the last time is gone from the list).  The third, a slot number, exists only inside a call —
        # written by the step kernel, replaced by the geometry kernel of the same call's frame — so no save can see it.
        pr = _record_rows(A, snap, SC_PENDING_REMOVE, spares=False)[0]
        assert pr[0] == REMOVE_APPLIED and (pr == -1).any() and set(pr) <= {-1, REMOVE_APPLIED}, pr
        assert A.engine.get_state(0, 1)["num_picked_up"][0] == picked0 + 1
    at_save = _everything(A, False, geometry, rendered=True)
    if through_host:                # a checkpoint: to the host and back (what torch.save / torch.load move)
        snap = type(snap).from_state_dict(snap.cpu().state_dict()).to("cuda")
    B.reset()
    for t in range(3):
        _step(B, (acts[t] + 1) % n_actions, repeat)
    assert not np.array_equal(B.engine.get_state()["agent_pos"], at_save["state.agent_pos"])
    obs = B.load_state(snap)
    assert obs is B.obs
    _assert_same(_everything(B, False, geometry), at_save, (env_id, "after the load"))
    _assert_same(_everything(A, False, geometry, rendered=True), at_save, (env_id, "the save changed A"))
    ends2 = np.zeros(n, int)
    for t in range(T, 2 * T):
        _step(A, acts[t], repeat)
        _step(B, acts[t], repeat)
        _assert_same(_everything(B, True, geometry), _everything(A, True, geometry), (env_id, "call", t))
        assert np.array_equal(_np(A.frame_clean()), _np(B.frame_clean())), (env_id, "call", t, "frame_clean")
        ends2 += _ends(A)
    assert ends1.min() >= 2 and ends2.min() >= 2, ("every env ends two episodes in each window", ends1.min(), ends2.min())
    for v in (A, B):
        v.engine.check()
        v.close()


def test_resume_hallway_same_step(monkeypatch):
    """dense K1, spares on; N = 70: past one wavefront of envs, no multiple of the dense K1's packing"""
    _resume(monkeypatch, "MiniWorld-Hallway-v0", 70, 16, 3100, 3, short=("Hallway", 7), p_fwd=0.6, want_depth=True)


def test_resume_hallway_without_spares(monkeypatch):
    monkeypatch.setenv("MW_SPARE", "0")
    _resume(monkeypatch, "MiniWorld-Hallway-v0", 70, 16, 3101, 3, short=("Hallway", 7), p_fwd=0.6, want_depth=True)


def test_resume_hallway_philox_through_the_host(monkeypatch):
    """the other stream; the snapshot goes to the host and back in between"""
    _resume(monkeypatch, "MiniWorld-Hallway-v0", 70, 16, 3102, 3, short=("Hallway", 7), p_fwd=0.6, rng="philox", through_host=True, want_depth=True)


def test_resume_hallway_action_repeat(monkeypatch):
    """repeat = 3: episodes of 7 sub-steps end on every third call"""
    _resume(monkeypatch, "MiniWorld-Hallway-v0", 70, 8, 3103, 3, short=("Hallway", 7), p_fwd=0.6, repeat=3, want_depth=True)


def test_resume_maze(monkeypatch):
    """per-env geometry, spares refilled on the side stream, the occlusion cache"""
    _resume(monkeypatch, "MiniWorld-MazeS2-v0", 6, 12, 3104, 3, p_fwd=0.5, geometry=True, max_episode_steps=5, want_depth=True)


def test_resume_pickup_objects_domain_rand(monkeypatch):
    """wave-per-env K1, meshes, the inline generator with per-step draws; env 0 picks an object up on the call before the save, so
    the records hold pending_remove = MW_REMOVE_APPLIED beside -1"""
    _resume(monkeypatch, "MiniWorld-PickupObjects-v0", 9, 10, 3105, 5, short=("PickupObjects", 4), domain_rand=True, want_depth=True,
            pickup_before_save=True)


def test_resume_collect_health_next_step_with_pending_resets(monkeypatch):
    """health, respawn draws, and a save taken while some envs wait for their next-step reset (episodes of 5 steps that start
    0 .. 4 steps old)"""
    _resume(monkeypatch, "MiniWorld-CollectHealth-v0", 9, 14, 3106, 8, short=("CollectHealth", 5), autoreset="next_step",
            first_steps=np.arange(9) % 5, want_pending=True, want_depth=True)


def test_resume_tmaze_final_obs(monkeypatch):
    """a placement program, the kept final info (goal_pos), the two-pass step"""
    _resume(monkeypatch, "MiniWorld-TMaze-v0", 9, 14, 3107, 3, short=("TMaze", 6), p_fwd=0.5, final_obs=True, want_depth=True)


# ---------------------------------------------------------------------------------------------------------------- 2. fork

def _fork(monkeypatch, env_id, n, T, seed, n_actions, src, short=None, p_fwd=None, geometry=False, **kw):
    """A: T calls, fork(src), T calls.  C: env j seeded seed + src[j] (per-env seeds through engine.reset and a render), fed the
    first T actions of A's env src[j], then the new actions.  A equals C after the fork and after every later call."""
    import torch
    if short:
        _short_episodes(monkeypatch, *short)
    rng = np.random.default_rng(seed)
    acts = _actions(rng, 2 * T, n, n_actions, p_fwd)
    src = np.asarray(src)
    A, Cv = _make(env_id, n, seed, **kw), _make(env_id, n, seed + 500, **kw)
    A.reset()
    Cv.engine.reset(None, (seed + src).astype(np.uint64))
    Cv.engine.render(Cv.obs, Cv.depth)
    for t in range(T):
        _step(A, acts[t])
        _step(Cv, acts[t][src])
    reward, term = A.reward.clone(), A.terminated.clone()
    obs = A.fork(torch.as_tensor(src, device="cuda"))
    assert obs is A.obs and torch.equal(A.reward, reward) and torch.equal(A.terminated, term)
    _assert_same(_everything(A, False, geometry), _everything(Cv, False, geometry, rendered=True), (env_id, "after the fork"))
    ends = np.zeros(n, int)
    for t in range(T, 2 * T):
        _step(A, acts[t])
        _step(Cv, acts[t])
        _assert_same(_everything(A, True, geometry), _everything(Cv, True, geometry), (env_id, "call", t))
        ends += _ends(A)
    assert ends.min() >= 2
    for v in (A, Cv):
        v.engine.check()
        v.close()


def test_fork_hallway_random_sources(monkeypatch):
    src = np.random.default_rng(77).integers(0, 70, 70)
    assert len(set(src)) < 70 and (np.bincount(src, minlength=70) >= 3).any()
    _fork(monkeypatch, "MiniWorld-Hallway-v0", 70, 16, 3200, 3, src, short=("Hallway", 7), p_fwd=0.6, want_depth=True)


def test_fork_maze(monkeypatch):
    """a value three times, identities, a swap (N = 6)"""
    _fork(monkeypatch, "MiniWorld-MazeS2-v0", 6, 12, 3201, 3, [0, 3, 3, 3, 5, 4], p_fwd=0.5, geometry=True, max_episode_steps=5, want_depth=True)


def test_fork_pickup_objects_domain_rand(monkeypatch):
    _fork(monkeypatch, "MiniWorld-PickupObjects-v0", 9, 10, 3202, 5, [3, 3, 3, 0, 1, 7, 7, 5, 8], short=("PickupObjects", 4), domain_rand=True,
          want_depth=True)


# ---------------------------------------------------------------------------------------------------------------- 3. subset

def test_a_subset_load_changes_its_envs_only(monkeypatch):
    """load_state(snap, envs=[2, 5], records=[0, 0]): envs 2 and 5 become the saved env; every other env's state and continuing
    trajectory equal those of an engine R that was never loaded.  And the two copies, given the saved env's actions, follow it."""
    _short_episodes(monkeypatch, "Hallway", 7)
    n, T, seed = 9, 16, 3300
    rng = np.random.default_rng(seed)
    acts = _actions(rng, 2 * T, n, 3, 0.6)
    acts[T:, 2] = acts[T:, 5] = acts[T:, 7]        # (behind the load envs 2 and 5 get env 7's actions)
    A, R = _make("MiniWorld-Hallway-v0", n, seed, want_depth=True), _make("MiniWorld-Hallway-v0", n, seed, want_depth=True)
    for v in (A, R):
        v.reset()
    for t in range(T):
        _step(A, acts[t])
        _step(R, acts[t])
    snap = A.save_state([7], capacity=2)        # (one record, laid out for the two envs one call is to load it into)
    assert (snap.count, snap.capacity) == (1, 2)
    A.load_state(snap, envs=[2, 5], records=[0, 0])
    others, a, r = [0, 1, 3, 4, 6, 7, 8], _everything(A, False, False), _everything(R, False, False)
    _assert_same(a, r, ("subset", "after the load"), rows=others)
    for k in a:
        assert np.array_equal(a[k][2], a[k][7]) and np.array_equal(a[k][5], a[k][7]), ("the copies equal the saved env", k)
    assert not np.array_equal(a["state.agent_pos"][2], r["state.agent_pos"][2])
    for t in range(T, 2 * T):
        _step(A, acts[t])
        _step(R, acts[t])
        a, r = _everything(A, True, False), _everything(R, True, False)
        _assert_same(a, r, ("subset", "call", t), rows=others)
        for k in a:
            assert np.array_equal(a[k][2], a[k][7]) and np.array_equal(a[k][5], a[k][7]), ("call", t, k)
    for v in (A, R):
        v.engine.check()
        v.close()


# ---------------------------------------------------------------------------------------------------------------- 4. a save changes nothing

def test_saving_changes_nothing_maze():
    """MazeS2: saves between the calls — behind steps whose spare refills run on the side stream — leave every later output equal
    to the same run without them."""
    n, T, seed = 6, 14, 3400
    rng = np.random.default_rng(seed)
    acts = _actions(rng, T, n, 3, 0.5)
    A, R = _make("MiniWorld-MazeS2-v0", n, seed, max_episode_steps=5), _make("MiniWorld-MazeS2-v0", n, seed, max_episode_steps=5)
    for v in (A, R):
        v.reset()
    snaps, ends = [], np.zeros(n, int)
    for t in range(T):
        if t >= 3:
            snaps.append(A.save_state() if t % 2 else A.save_state([5, 0, 0]))
        _step(A, acts[t])
        _step(R, acts[t])
        _assert_same(_everything(A, True, True), _everything(R, True, True), ("maze", "call", t))
        ends += _ends(A)
    assert ends.min() >= 2
    assert len(snaps) == T - 3
    for v in (A, R):
        v.engine.check()
        v.close()


# ---------------------------------------------------------------------------------------------------------------- 5. frame reuse

def test_a_load_drops_the_held_frame(monkeypatch):
    """An engine with frame reuse on, on its own buffers, loads a state whose next action is blocked (chosen from A's frame-clean
    history) and steps WITHOUT a render in between: the step finds those envs' state unchanged, and only because the load dropped
    the held frame does it draw them.  Without the drop the rows keep the frame from before the load."""
    import torch
    _short_episodes(monkeypatch, "Hallway", 40)
    n, T, seed = 70, 30, 3500
    rng = np.random.default_rng(seed)
    acts = _actions(rng, T, n, 3, 0.8)
    A = _make("MiniWorld-Hallway-v0", n, seed)
    A.reset()
    snaps, cleans = [], []
    for t in range(T):
        snaps.append(A.save_state())
        _step(A, acts[t])
        cleans.append(_np(A.frame_clean()).astype(bool))
    cleans = np.array(cleans)
    t = int(np.argmax(cleans.sum(axis=1)))
    blocked = np.flatnonzero(cleans[t])
    assert len(blocked) >= 1, "a call in which some env's action was blocked"
    X, Y = _make("MiniWorld-Hallway-v0", n, seed + 1, frame_reuse=True), _make("MiniWorld-Hallway-v0", n, seed + 1, frame_reuse=False)
    assert X.frame_reuse and not Y.frame_reuse
    for v in (X, Y):
        v.reset()
        for k in range(3):
            _step(v, acts[k])       # (X now holds a frame and skips clean envs)
    before = X.obs.clone()
    for v in (X, Y):
        v.engine.snapshot_load(snaps[t].data, snaps[t].count, snaps[t].capacity)
        assert not _np(v.frame_clean()).any(), "a load clears the frame-clean bytes of the envs it writes"
        _step(v, acts[t])
    assert np.array_equal(_np(X.frame_clean()).astype(bool), cleans[t])
    assert torch.equal(X.obs, Y.obs), "frame reuse kept rows from before the load"
    assert not torch.equal(X.obs[blocked], before[blocked])
    for v in (A, X, Y):
        v.engine.check()
        v.close()


# ---------------------------------------------------------------------------------------------------------------- 6. frame stack

def _rebuilt(frames, K, pad):
    """the host stacking of tests/test_gpu_frame_stack.py: first frames of an episode -> their stacks"""
    out = np.repeat(frames[:, None], K, axis=1)
    if pad == "zero":
        out[:, :-1] = 0
    return out


@pytest.mark.parametrize("pad", ["reset", "zero"])
def test_frame_stacks_are_rebuilt_for_the_loaded_envs(pad, monkeypatch):
    import torch
    _short_episodes(monkeypatch, "Hallway", 7)
    n, K, seed = 9, 3, 3600
    rng = np.random.default_rng(seed)
    acts = _actions(rng, 12, n, 3, 0.6)
    A = _make("MiniWorld-Hallway-v0", n, seed, frame_stack=K, stack_pad=pad)
    A.reset()
    for t in range(5):
        _step(A, acts[t])
    snap = A.save_state([4, 0])
    _step(A, acts[5])
    stack0, window0 = _np(A.stack).copy(), A.engine.stack_window()
    A.load_state(snap, envs=[2, 5], records=[0, 0])
    got, obs = _np(A.stack), _np(A.obs)
    assert A.engine.stack_window() == window0, "the ring position moved"
    others = [0, 1, 3, 4, 6, 7, 8]
    assert np.array_equal(got[others], stack0[others]), "a stack of an env that was not loaded changed"
    assert np.array_equal(got[[2, 5]], _rebuilt(obs[[2, 5]], K, pad)), "the loaded envs' stacks are the rebuild from their new first frame"
    # ... and the next push is an ordinary one for every env
    hist = got.copy()
    _step(A, acts[6])
    hist = np.concatenate([hist[:, 1:], _np(A.obs)[:, None]], axis=1)
    done = _ends(A)
    hist[done] = _rebuilt(_np(A.obs)[done], K, pad)
    assert np.array_equal(_np(A.stack), hist)
    # fork: every env is written, every stack is the rebuild from its new frame
    window1 = A.engine.stack_window()
    A.fork(torch.as_tensor([3, 3, 3, 0, 1, 7, 7, 5, 8], device="cuda"))
    assert A.engine.stack_window() == window1
    assert np.array_equal(_np(A.stack), _rebuilt(_np(A.obs), K, pad))
    assert np.array_equal(_np(A.obs)[0], _np(A.obs)[2]) and np.array_equal(_np(A.obs)[5], _np(A.obs)[6])
    A.engine.check()
    A.close()


# ---------------------------------------------------------------------------------------------------------------- 7. errors

def test_errors_launch_nothing_and_bad_items_are_skipped():
    import torch
    from miniworld_amd import engine as eng
    from test_snapshot_cpu import layout_lib, snap_config
    n = 9
    A = _make("MiniWorld-Hallway-v0", n, 3700, want_depth=True)
    A.reset()
    act = np.full(n, 2)
    for _ in range(3):
        _step(A, act)
    e, lib, h = A.engine, A.engine.lib, A.engine.h
    # the size is the host layout's (tests/test_snapshot_cpu.py checks that one)
    cfg = snap_config(e.E, e.cfg.max_polys, e.cfg.max_segs, e.cfg.shared_geometry, e.cfg.task, e.cfg.generator, e.cfg.rng_mode, True)
    for cap in (0, 1, n, 100):
        assert e.snapshot_bytes(cap) == layout_lib().mwsnap_bytes(cfg.ctypes.data, cap), cap
    cap = n
    buf = torch.zeros(e.snapshot_bytes(cap + 1), dtype=torch.uint8, device="cuda")      # room for one record more than the engine is told
    e.snapshot_save(buf, cap)
    _step(A, act)
    state0, buf0 = _everything(A, True, False), buf.clone()
    stream = eng._stream_ptr(e.device)
    p = C_.c_void_p(buf.data_ptr())
    idx = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    ip = C_.c_void_p(idx.data_ptr())
    assert lib.mw_snapshot_bytes(h, -1) < 0
    bad = [lib.mw_snapshot_save(h, None, 1, None, cap, stream),                 # a null buffer
           lib.mw_snapshot_save(h, None, -1, p, cap, stream),                   # count < 0
           lib.mw_snapshot_save(h, ip, cap + 1, p, cap, stream),                # count > capacity
           lib.mw_snapshot_save(h, None, n + 1, p, n + 1, stream),              # count > N on a save of envs 0 .. count - 1
           lib.mw_snapshot_save(h, None, 1, C_.c_void_p(buf.data_ptr() + 4), cap, stream),      # a misaligned buffer
           lib.mw_snapshot_load(h, None, None, 1, None, 1, cap, stream),
           lib.mw_snapshot_load(h, None, None, -1, p, 1, cap, stream),
           lib.mw_snapshot_load(h, ip, ip, n + 1, p, n + 1, n + 1, stream),     # count > N on a load
           lib.mw_snapshot_load(h, None, None, 1, p, cap + 1, cap, stream),     # n_recs > capacity
           lib.mw_snapshot_load(h, None, None, 2, p, 2, 1, stream)]             # count > capacity
    assert bad == [-1] * len(bad), bad
    assert b"mw_snapshot_load" in lib.mw_last_error(h)
    torch.cuda.synchronize()
    e.check()
    _assert_same(_everything(A, True, False), state0, ("errors", "a refused call changed the engine"))
    assert torch.equal(buf, buf0), "a refused call wrote to the buffer"
    # an out-of-range record index: record `cap` of a buffer the engine is told holds `cap` — memory the test owns either way
    e.snapshot_load(buf, cap, cap, envs=[1, 2], records=[0, cap])
    torch.cuda.synchronize()
    with pytest.raises(eng.EngineError, match=r"\(-1\).*mw_snapshot"):
        e.check()
    now = _everything(A, True, False)
    _assert_same(now, state0, ("errors", "bad record index"), rows=[0, 2, 3, 4, 5, 6, 7, 8])
    assert not np.array_equal(now["state.agent_pos"][1], state0["state.agent_pos"][1]), "the valid item of the same call was loaded"
    A.close()
    # a buffer whose header key was overwritten: nothing is loaded, mw_check reports it
    B = _make("MiniWorld-Hallway-v0", n, 3701)
    B.reset()
    snap = B.save_state()
    for _ in range(2):
        _step(B, act)
    B.engine.check()
    state1 = _everything(B, True, False)
    snap.data[8:12] += 1            # (the key's third word: max_ents)
    B.engine.snapshot_load(snap.data, snap.count, snap.capacity)
    torch.cuda.synchronize()
    with pytest.raises(eng.EngineError, match=r"\(-1\).*key"):
        B.engine.check()
    _assert_same(_everything(B, True, False), state1, ("errors", "bad key"))
    # ... and a buffer of another capacity than the call names is the same error, not a misread
    C = _make("MiniWorld-Hallway-v0", n, 3702)
    C.reset()
    good = C.save_state()
    state2 = _everything(C, False, False)
    C.engine.snapshot_load(good.data, 4, 4)
    torch.cuda.synchronize()
    with pytest.raises(eng.EngineError, match=r"\(-1\)"):
        C.engine.check()
    _assert_same(_everything(C, False, False), state2, ("errors", "capacity mismatch"))
    for v in (B, C):
        v.close()
