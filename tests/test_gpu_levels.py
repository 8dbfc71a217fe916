"""Level sets on the device (mw_snapshot_save_at / mw_snapshot_save_frames_at / mw_snapshot_load_where / mw_snapshot_load_frames_where;
MiniWorldVecEnv.make_levels, save_state(into=...), autoreset="levels"): a finished env restarts from a record the caller chose, without
the host learning that it finished.

Everything here is a copy, so there are no tolerances.  The yardsticks are the list forms of the same calls (merged and tested before:
tests/test_gpu_snapshot.py, tests/test_gpu_snapshot_frames.py), an engine reset with the level's seed, and a mirror loop that reads `done`
on the host and calls load_state for the finished envs.  Nothing here provokes a fault: a bad record index is skipped by design and
reported by mw_check."""
import numpy as np
import pytest

from test_gpu_snapshot import _actions, _ends, _make, _np, _short_episodes, _step

pytestmark = pytest.mark.gpu

HALLWAY, MAZE, PICKUP, COLLECT = "MiniWorld-Hallway-v0", "MiniWorld-MazeS2-v0", "MiniWorld-PickupObjects-v0", "MiniWorld-CollectHealth-v0"
# name: env id, num_envs, number of actions, the family whose episodes are shortened (None: max_episode_steps is a keyword), keywords
CONFIGS = {
    "hallway": (HALLWAY, 70, 3, "Hallway", {}),
    "hallway-300": (HALLWAY, 300, 3, "Hallway", {}),
    "hallway-81x61": (HALLWAY, 70, 3, "Hallway", dict(obs_width=81, obs_height=61)),
    "hallway-depth-stack3": (HALLWAY, 70, 3, "Hallway", dict(want_depth=True, frame_stack=3)),
    "maze": (MAZE, 3, 3, None, dict(want_depth=True)),
    "pickup-dr": (PICKUP, 5, 5, "PickupObjects", dict(domain_rand=True)),
    "collecthealth": (COLLECT, 4, 8, "CollectHealth", {}),
}


def _config(monkeypatch, name, steps, **more):
    env_id, n, n_actions, short, kw = CONFIGS[name]
    kw = dict(kw, **more)
    if short:
        _short_episodes(monkeypatch, short, steps)
    else:
        kw["max_episode_steps"] = steps
    return env_id, n, n_actions, kw


def _dev(a, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _handed_out(v):
    """what a consumer of the env can see of it, as host arrays: the buffers, the ring and its window, the clean bytes"""
    out = {"obs": _np(v.obs), "frame_clean": _np(v.frame_clean()), "reward": _np(v.reward), "terminated": _np(v.terminated), "truncated": _np(v.truncated)}
    if v.depth is not None:
        out["depth"] = _np(v.depth)
    if v.frame_stack:
        out.update(ring=_np(v._ring), stack=_np(v.stack), window=np.array(v.engine.stack_window()))
    return out


def _same(got, want, tag):
    assert got.keys() == want.keys(), tag
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), tag + (k,)


def _whole(v):
    """a whole-batch save with frames, as host bytes"""
    snap = v.save_state(frames=True)
    return _np(snap.data), _np(snap.frames)


# ---------------------------------------------------------------------------------------------------------------- 1. the list form

@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_a_masked_load_is_the_list_load_of_the_masked_envs(name, monkeypatch):
    """Twin engines in the same state.  A: load_state(bank, envs=idx, records=recs[idx]) with frames, the merged path.  B: the _where
    pair with the mask of idx.  Afterwards they are the same engine: whole-batch saves with frames byte for byte, and everything
    handed out.  Under zero mask bytes recs holds indices far outside the bank: they are never read as records."""
    import torch
    env_id, n, n_actions, kw = _config(monkeypatch, name, 6)
    seed = 5100
    rng = np.random.default_rng(seed + n)
    acts = _actions(rng, 9, n, n_actions, 0.5)
    A, B = _make(env_id, n, seed, **kw), _make(env_id, n, seed, **kw)
    for v in (A, B):
        v.reset()
        for t in range(4):
            _step(v, acts[t])
    bank = A.save_state(frames=True)            # the states after call 4: records 0 .. n - 1
    for v in (A, B):
        for t in range(4, 9):
            _step(v, acts[t])
    assert not np.array_equal(_whole(A)[0], _np(bank.data))
    mask = rng.random(n) < 1 / 3
    mask[0] = mask[n - 1] = True
    if n > 256:
        mask[250:262] = [True, False] * 6       # across the 256-item chunk of a component block
    recs = rng.integers(0, n, n)
    recs[n - 1] = recs[0]                       # a repeat for certain
    idx = np.flatnonzero(mask)
    A.load_state(bank, envs=idx, records=recs[idx], frames=True)
    wild = np.where(mask, recs, rng.choice([-1, -7, n, 2 ** 31 - 1, -2 ** 31], n))
    m, r = _dev(mask, torch.uint8), _dev(wild, torch.int32)
    flags = B._frame_flags()
    B.engine.snapshot_load_where(bank.data, bank.count, bank.capacity, m, r)
    B.engine.snapshot_load_frames_where(bank.frames, bank.count, bank.capacity, m, r, B.obs, B.depth, flags)
    B.engine.check()
    sa, sb = _whole(A), _whole(B)
    assert np.array_equal(sa[0], sb[0]), (name, "state records")
    assert np.array_equal(sa[1], sb[1]), (name, "frame records")
    _same(_handed_out(B), _handed_out(A), (name, "after the loads"))
    # ... and they stay the same engine: the next frame is drawn from the loaded states on both
    for v in (A, B):
        _step(v, acts[0])
    _same(_handed_out(B), _handed_out(A), (name, "a step later"))
    for v in (A, B):
        v.engine.check()
        v.close()


# ---------------------------------------------------------------------------------------------------------------- 2. save_at

def _record_bytes(v, snap, recs):
    """bool masks over snap.data and snap.frames: the bytes that belong to the records `recs`, from the host builds of the two layouts"""
    from test_snapshot_cpu import layout_lib, sections, snap_config
    from test_snapshot_frames_cpu import frames_config, layout_lib as flayout_lib, sections as fsections
    c, cap = v.engine.cfg, snap.capacity
    lib = layout_lib()
    for spares in (False, True):
        cfg = snap_config(v.engine.E, c.max_polys, c.max_segs, c.shared_geometry, c.task, c.generator, c.rng_mode, spares)
        if lib.mwsnap_bytes(cfg.ctypes.data, cap) == snap.data.numel():
            break
    else:
        raise AssertionError("no layout of the host build has the buffer's size")
    named = np.zeros(snap.data.numel(), bool)
    off, size, align, ident = sections(lib, cfg, cap)
    for o, s, a, i in zip(off, size, align, ident):
        if i < 0:       # a blob: record-major
            per = s // cap
            for r in recs:
                named[o + r * per:o + (r + 1) * per] = True
        else:           # a component: [rows][capacity] elements of `a` bytes
            rows = s // (cap * a)
            for r in recs:
                for row in range(rows):
                    at = o + (row * cap + r) * a
                    named[at:at + a] = True
    fnamed = np.zeros(snap.frames.numel(), bool)
    H, W = v.obs.shape[1:3]
    fcfg = frames_config(W, H, 0, snap.frame_flags, snap.frame_stack)
    foff, fsize, frec, _ = fsections(flayout_lib(), fcfg, cap)
    for o, per in zip(foff, frec):
        for r in recs:
            fnamed[o + r * per:o + (r + 1) * per] = True
    return named, fnamed


@pytest.mark.parametrize("name", ["hallway-depth-stack3", "maze"])
def test_a_bank_is_filled_in_chunks_through_chosen_records(name, monkeypatch):
    """A bank of 3 N records filled by three save_state(into=bank, records=perm[chunk]) calls, a few steps apart.  Record perm[k],
    loaded anywhere, is the state and the frames that were saved as item k — against a plain whole-batch save taken at the same
    moment —, and a save leaves every byte outside the records it names as it was."""
    import torch
    env_id, n, n_actions, kw = _config(monkeypatch, name, 6)
    seed = 5200
    rng = np.random.default_rng(seed)
    acts = _actions(rng, 12, n, n_actions, 0.5)
    V, W = _make(env_id, n, seed, **kw), _make(env_id, n, seed + 77, **kw)
    V.reset()
    W.reset()
    perm = rng.permutation(3 * n)
    bank = V.save_state([0], capacity=3 * n, frames=True)
    refs, t = [], 0
    for c in range(3):
        for _ in range(3):
            _step(V, acts[t])
            t += 1
        named = perm[c * n:(c + 1) * n]
        before = (_np(bank.data).copy(), _np(bank.frames).copy())
        refs.append((V.save_state(frames=True), V.engine.get_state(), _np(V.obs).copy()))
        assert V.save_state(into=bank, records=torch.as_tensor(named, dtype=torch.int32, device="cuda")) is bank
        V.engine.check()
        keep, fkeep = (~m for m in _record_bytes(V, bank, named.tolist()))
        assert np.array_equal(_np(bank.data)[keep], before[0][keep]), (name, c, "a state byte outside the named records changed")
        assert np.array_equal(_np(bank.frames)[fkeep], before[1][fkeep]), (name, c, "a frame byte outside the named records changed")
    bank.count = 3 * n
    # every record, loaded into another engine n at a time — chunk c into the envs in reverse order — equals item k of the reference save
    for c in range(3):
        ref, state, obs = refs[c]
        envs = np.arange(n)[::-1].copy()
        W.load_state(bank, envs=envs, records=perm[c * n:(c + 1) * n], frames=True)
        W.engine.check()
        got = W.engine.get_state()
        for k, a in state.items():
            assert np.array_equal(got[k][envs], a), (name, c, "state", k)
        assert np.array_equal(_np(W.obs)[envs], obs), (name, c, "obs")
        one, want = W.save_state(envs, frames=True), ref
        assert np.array_equal(_np(one.data), _np(want.data)), (name, c, "the records read back")
        assert np.array_equal(_np(one.frames), _np(want.frames)), (name, c, "the frame records read back")
    for v in (V, W):
        v.close()


@pytest.mark.parametrize("env_id, n, kw", [(HALLWAY, 70, dict(obs_width=81, obs_height=61, want_depth=True, frame_stack=2)), (MAZE, 3, dict(want_depth=True))],
                         ids=["hallway-81x61-depth-stack2", "maze"])
def test_a_save_at_without_records_is_the_plain_save(env_id, n, kw):
    """records=None names record k for item k: snapshot_save_at(buf, cap, envs, None) and snapshot_save(buf, cap, envs) into zeroed
    buffers of more records than items leave the same bytes, and so does the frames pair.  One kernel serves both calls and reads the
    rule from its arguments, so a null record list must stay what the plain save has always meant."""
    import torch
    seed = 5250
    rng = np.random.default_rng(seed)
    V = _make(env_id, n, seed, **kw)
    V.reset()
    for act in _actions(rng, 3, n, 3, 0.5):
        _step(V, act)
    e, flags, cap = V.engine, V._frame_flags(), n + 2
    envs = _dev(rng.permutation(n)[:max(2, n - 1)], torch.int32)
    at, plain = (torch.zeros(e.snapshot_bytes(cap), dtype=torch.uint8, device="cuda") for _ in range(2))
    fat, fplain = (torch.zeros(e.snapshot_frames_bytes(cap, flags), dtype=torch.uint8, device="cuda") for _ in range(2))
    assert e.snapshot_save_at(at, cap, envs, None) == e.snapshot_save(plain, cap, envs) == envs.numel()
    assert e.snapshot_save_frames_at(fat, cap, V.obs, V.depth, flags, envs, None) == e.snapshot_save_frames(fplain, cap, V.obs, V.depth, flags, envs)
    e.check()
    assert _np(plain).any() and _np(fplain).any()
    assert np.array_equal(_np(at), _np(plain)), "state records"
    assert np.array_equal(_np(fat), _np(fplain)), "frame records"
    V.close()


# ---------------------------------------------------------------------------------------------------------------- 3. a level is a reset

@pytest.mark.parametrize("name", ["hallway", "maze", "pickup-dr", "collecthealth"])
def test_a_level_is_the_reset_with_its_seed(name):
    """Record l of make_levels(seeds), loaded into env j of a level env, is env 0 of an engine reset with seed=seeds[l]: the state,
    the first observation and depth, and 12 steps of the same actions (PCG64; spares on: Hallway, Maze; off: the other two)."""
    import torch
    env_id, _, n_actions, _, kw = CONFIGS[name]
    kw = dict(kw, want_depth=True)
    n, seeds = 4, [11, 4242, 7, 2 ** 40 + 5, 99, 31337]           # six levels from four envs: two chunks
    rng = np.random.default_rng(5300)
    maker, W, R = _make(env_id, n, 1, autoreset="levels", **kw), _make(env_id, 3, 2, autoreset="levels", **kw), _make(env_id, 1, 3, autoreset=False, **kw)
    bank = maker.make_levels(seeds)
    maker.engine.check()
    assert (bank.count, bank.capacity) == (6, 6) and bank.seeds.tolist() == seeds
    W.set_levels(bank)
    for l in (0, 3, 5):
        j = l % 3
        R.reset(seed=seeds[l])
        W.next_level.fill_(l)
        W.reset()
        assert _np(W.level).tolist() == [l] * 3
        want, got = R.engine.get_state(0, 1), W.engine.get_state(j, 1)
        for k in want:
            assert np.array_equal(got[k], want[k]), (name, l, "state", k)
        assert torch.equal(W.obs[j], R.obs[0]) and torch.equal(W.depth[j], R.depth[0]), (name, l, "first frame")
        for t in range(12):
            a = int(rng.integers(0, n_actions))
            _step(R, [a])
            _step(W, [a] * 3)
            for f in ("reward", "terminated", "truncated"):
                assert torch.equal(getattr(W, f)[j], getattr(R, f)[0]), (name, l, t, f)
            if _ends(R)[0]:
                break       # (the level env has restarted; the reference stays where it ended)
            assert torch.equal(W.obs[j], R.obs[0]) and torch.equal(W.depth[j], R.depth[0]), (name, l, t, "frame")
    for v in (maker, W, R):
        v.engine.check()
        v.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the mode

MODE = {"hallway": ("hallway", 6, {}), "hallway-stack3": ("hallway", 6, dict(frame_stack=3)), "maze": ("maze", 5, {}), "pickup-dr": ("pickup-dr", 7, {})}


def _trace(v):
    out = {f: _np(getattr(v, f)).copy() for f in ("obs", "reward", "terminated", "truncated")}
    if v.depth is not None:
        out["depth"] = _np(v.depth).copy()
    if v.frame_stack:
        out["stack"] = _np(v.stack).copy()
    return out


@pytest.mark.parametrize("name", sorted(MODE))
def test_level_mode_is_the_host_driven_loop(name, monkeypatch):
    """60 steps with episodes of 5 .. 7 steps.  The mirror is an autoreset=False env whose loop reads `done` on the host and calls
    load_state(envs, records, frames=True) for the finished envs with the same next_level stream; the level env does it behind the
    step.  Every step's observation, depth, stack, reward, flags and level agree — also with the frame cache, frame reuse or both
    switched off on the level env: a loaded env never shows a frame cached or held before the load."""
    import torch
    base, steps, more = MODE[name]
    env_id, n, n_actions, kw = _config(monkeypatch, base, steps, want_depth=True, **more)
    n, T, seed = min(n, 12), 60, 5400
    L = 2 * n + n // 2
    acts = _actions(np.random.default_rng(seed), T, n, n_actions, 0.5)
    first = _make(env_id, n, seed, autoreset="levels", **kw)
    bank = first.make_levels(np.arange(L) * 13 + 1000)
    # the mirror
    M = _make(env_id, n, seed + 1, autoreset=False, **kw)
    g = torch.Generator(device="cuda").manual_seed(77)
    nxt = torch.zeros(n, dtype=torch.int32, device="cuda")
    draw = lambda: torch.randint(0, L, (n,), generator=g, out=nxt)      # noqa: E731
    draw()
    M.load_state(bank, records=nxt, frames=True)
    level = _np(nxt).copy()
    draw()
    want, ended = [dict(_trace(M), level=level.copy())], np.zeros(n, int)
    for t in range(T):
        _step(M, acts[t])
        flags = {f: _np(getattr(M, f)).copy() for f in ("reward", "terminated", "truncated")}
        idx = np.flatnonzero(_ends(M))
        ended[idx] += 1
        if len(idx):
            M.load_state(bank, envs=idx, records=_np(nxt)[idx], frames=True)
            level[idx] = _np(nxt)[idx]
        draw()
        want.append(dict(_trace(M), level=level.copy(), **flags))
    assert ended.min() >= 5, "every env restarted several times"
    M.engine.check()
    M.close()
    for variant in ({}, dict(frame_cache=0), dict(frame_reuse=False), dict(frame_cache=0, frame_reuse=False)):
        V = first if not variant else _make(env_id, n, seed + 2, autoreset="levels", **dict(kw, **variant))
        V.set_levels(bank, generator=torch.Generator(device="cuda").manual_seed(77))
        V.reset()
        _same(dict(_trace(V), level=_np(V.level)), want[0], (name, variant, "reset"))
        for t in range(T):
            _step(V, acts[t])
            _same(dict(_trace(V), level=_np(V.level)), want[t + 1], (name, variant, "step", t))
        V.engine.check()
        V.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the frame cache

@pytest.mark.parametrize("masked", [True, False])
def test_a_masked_load_leaves_the_other_envs_cached_frames(masked):
    """Left, right; a load of the odd envs (their own states of before the two turns); left, right.  Behind the masked load the even
    envs come back to frames they have cached and get them from there; the odd envs, back in the very state their cache shows, do not
    — their epoch advanced.  Behind load_state nobody does: it clears every env's cache (the behaviour of before, asserted so that the
    difference shows)."""
    import torch
    n = 8
    V = _make(HALLWAY, n, 5500, frame_cache=4)
    V.reset()
    bank = V.save_state(frames=True)
    left, right = np.zeros(n, int), np.ones(n, int)
    _step(V, left)
    _step(V, right)
    odd = np.arange(n) % 2 == 1
    if masked:
        m, r = _dev(odd, torch.uint8), _dev(np.arange(n), torch.int32)
        V.engine.snapshot_load_where(bank.data, n, n, m, r)
        V.engine.snapshot_load_frames_where(bank.frames, n, n, m, r, V.obs, V.depth, 0)
    else:
        V.load_state(bank, envs=np.flatnonzero(odd), records=np.flatnonzero(odd), frames=True)
    _step(V, left)
    went = _np(V.frame_source()).copy()
    _step(V, right)
    back = _np(V.frame_source()).copy()
    if masked:
        assert (back[~odd] >= 2).all(), (went, back)
        assert (went[odd] < 2).all(), (went, "a loaded env was served a frame cached before the load")
    else:
        assert (back < 2).all(), (went, back)
    V.engine.check()
    V.close()


# ---------------------------------------------------------------------------------------------------------------- 6. indices

def test_bad_indices_are_skipped_and_reported():
    """A bank of 8 records of which the call is told 4 are valid.  Under zero mask bytes nothing is an index.  Masked, env 1 takes
    record 3; env 2 (record n_recs) and env 5 (record -1) are left exactly as they were and mw_check reports the skipped items."""
    import torch
    from miniworld_amd import engine as eng
    n, n_recs, past = 8, 4, (2, 0, 2, 1)
    V, ref = _make(HALLWAY, n, 5600, frame_stack=2), _make(HALLWAY, n, 5600, frame_stack=2)
    for v in (V, ref):
        v.reset()
    bank = V.save_state(frames=True)
    for v in (V, ref):
        for a in past:
            _step(v, np.full(n, a))
    flags = V._frame_flags()

    def loads(mask, recs):
        m, r = _dev(mask, torch.uint8), _dev(recs, torch.int32)
        V.engine.snapshot_load_where(bank.data, n_recs, n, m, r)
        V.engine.snapshot_load_frames_where(bank.frames, n_recs, n, m, r, V.obs, V.depth, flags)
    before = _whole(V)
    recs = np.array([0, 3, n_recs, 0, 0, -1, 0, 0])
    loads(np.zeros(n, bool), recs)
    V.engine.check()
    after = _whole(V)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    # arguments: refused before anything is launched
    m, r = _dev(np.ones(n, bool), torch.uint8), _dev(recs, torch.int32)
    for call in (lambda: V.engine.snapshot_load_where(bank.data, n + 1, n, m, r),
                 lambda: V.engine.snapshot_load_where(bank.data, -1, n, m, r),
                 lambda: V.engine.snapshot_load_where(bank.data, n, n, m, None),
                 lambda: V.engine.snapshot_load_where(bank.data, n, n, None, r),
                 lambda: V.engine.snapshot_load_where(bank.data[4:], n, n, m, r),
                 lambda: V.engine.snapshot_load_frames_where(bank.frames, n + 1, n, m, r, V.obs, V.depth, flags),
                 lambda: V.engine.snapshot_load_frames_where(bank.frames, n, n, m, r, V.obs, V.depth, flags | 1),
                 lambda: V.engine.snapshot_load_frames_where(bank.frames, n, n, m, r, V.obs, V.depth, flags | 4)):
        with pytest.raises(eng.EngineError):
            call()
    V.engine.check()
    after = _whole(V)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    # the bad indices, masked (the status word keeps the report: this comes last)
    mask = np.zeros(n, bool)
    mask[[1, 2, 5]] = True
    loads(mask, recs)
    with pytest.raises(eng.EngineError, match=r"\(-1\).*skipped an item"):
        V.engine.check()
    ref.load_state(bank, envs=[1], records=[3], frames=True)       # the list form for env 1 alone
    got, exp = _whole(V), _whole(ref)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    assert not np.array_equal(got[0], before[0]), "the valid item of the same call was loaded"
    _same(_handed_out(V), _handed_out(ref), ("skipped",))
    for v in (V, ref):
        v.close()


def test_a_bank_of_another_layout_is_refused_by_its_key():
    """Two engines whose max_ents differ (five entity slots and three).  A bank from the one with the longer records — its buffer is
    large enough for the other's layout, so the call gets as far as the kernel — is offered to the other: the key differs, nothing is
    written, mw_check says so."""
    import torch
    from miniworld_amd import engine as eng
    five, three = _make(PICKUP, 4, 5700), _make(PICKUP, 4, 5700, num_objs=3)
    assert five.engine.E != three.engine.E
    five.reset()
    three.reset()
    # (which layout is the longer one is the engines' business: the one with fewer slots may keep a spare world per env)
    source, target = (five, three) if five.engine.snapshot_bytes(4) >= three.engine.snapshot_bytes(4) else (three, five)
    bank = source.save_state(frames=True)
    before, seen = _whole(target), _handed_out(target)
    m, r = torch.ones(4, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    assert bank.data.numel() >= target.engine.snapshot_bytes(4)
    target.engine.snapshot_load_where(bank.data, 4, 4, m, r)
    with pytest.raises(eng.EngineError, match=r"\(-1\).*key"):
        target.engine.check()
    after = _whole(target)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    _same(_handed_out(target), seen, ("another layout",))
    for v in (five, three):
        v.close()


# ---------------------------------------------------------------------------------------------------------------- 7. frameless

def test_a_frameless_rollout_loads_states_alone(monkeypatch):
    """rollout(render=False) in level mode: the finished envs are in their next levels' states, vec.obs is untouched, and the next
    drawn step hands those envs a fresh stack (K copies of the frame it drew)."""
    import torch
    _short_episodes(monkeypatch, "Hallway", 6)
    n, K, T = 9, 3, 4
    V = _make(HALLWAY, n, 5800, autoreset="levels", frame_stack=K)
    bank = V.make_levels(np.arange(20) + 300)
    V.set_levels(bank, generator=torch.Generator(device="cuda").manual_seed(5))
    V.reset()
    V.engine.set_state({"step_count": np.array([0, 3, 0, 4, 0, 5, 0, 3, 4], np.int32)})    # the odd envs end inside the rollout
    obs, chosen = _np(V.obs).copy(), _np(V.next_level).copy()
    plans = _dev(np.full((T, n), 0), torch.int32)                                           # (turning: nobody reaches the box)
    out = V.rollout(plans, render=False)
    assert out[0] is None
    done = _ends(V)
    assert done.tolist() == [False, True, False, True, False, True, False, True, True]
    assert np.array_equal(_np(V.obs), obs), "a frameless call wrote the observation buffer"
    assert np.array_equal(_np(V.level)[done], chosen[done]) and np.array_equal(_np(V.played_level)[~done], _np(V.level)[~done])
    # the states of the finished envs are their levels' (a record is read back through the list form into a second engine)
    W = _make(HALLWAY, n, 5801, autoreset=False, frame_stack=K)
    W.reset()
    W.load_state(bank, records=_np(V.level), frames=True)
    got, want = V.engine.get_state(), W.engine.get_state()
    for k in want:
        assert np.array_equal(got[k][done], want[k][done]), ("frameless", k)
    _step(V, np.zeros(n, int))
    stack = _np(V.stack)
    for i in np.flatnonzero(done):
        assert all(np.array_equal(stack[i, k], stack[i, K - 1]) for k in range(K)), ("a fresh stack", i)
    assert any(not np.array_equal(stack[i, 0], stack[i, K - 1]) for i in np.flatnonzero(~done))
    for v in (V, W):
        v.engine.check()
        v.close()
