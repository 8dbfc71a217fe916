"""Device-side state views on the GPU (mw_get_state_device / mw_set_state_where; MiniWorldVecEnv.state / set_state_where; the adapter's
info_state).

The yardstick is never the new kernels.  A read is compared with mw_get_state, the synchronous host route, bit for bit (floats as
their uint64 bits).  A write is compared with a twin engine of the same configuration and seed that received the same rows through
mw_set_state, env by env: observations, depth, rewards, flags and the full state must then be identical at every step.  There are no
tolerances.  N = 67 is one full group of 64 envs plus a partial one (and 16 workgroups of four envs plus one of three); N = 1 once."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 67
ENVS = ("MiniWorld-Hallway-v0", "MiniWorld-PickupObjects-v0", "MiniWorld-PutNext-v0")      # E = 1, shared geometry; E = 5, meshes, removals; carrying, drops
POSE = ("agent_pos", "agent_dir")
ENTS = ("ent_pos", "ent_dir")


def _make(env_id, n, seed, **kw):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    return MiniWorldVecEnv(env_id, n, seed=seed, **kw)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_state(got, want, tag, rows=None):
    assert got.keys() == want.keys(), tag
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if rows is not None:
            g, w = g[rows], w[rows]
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (tag, k)


def _act(v, a):
    import torch
    return v.step(torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32, device="cuda"))


def _run(v, rng, steps):
    for _ in range(steps):
        _act(v, rng.integers(0, v.n_actions, v.num_envs))


def _dev(src, fields, rows=None):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(src[k] if rows is None else src[k][rows])).cuda() for k in fields}


def _mask(bits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint8)).cuda()


def _host_write(v, src, mask, fields):
    """the twin's route: mw_set_state, one masked env at a time"""
    for i in np.flatnonzero(mask):
        v.engine.set_state({k: src[k][i:i + 1] for k in fields}, first=int(i), count=1)


def _outputs(v, stepped):
    out = {"obs": _np(v.obs), "depth": _np(v.depth), "reset_pending": _np(v.reset_pending())}
    if stepped:
        out.update(reward=_np(v.reward), terminated=_np(v.terminated), truncated=_np(v.truncated))
    out.update({"state." + k: a for k, a in v.engine.get_state().items()})
    return out


def _source(env_id, n, seed, steps=9, **kw):
    """legal values to write: the states of another seed's batch, a few steps in"""
    S = _make(env_id, n, seed, **kw)
    S.reset()
    _run(S, np.random.default_rng(seed), steps)
    src = S.engine.get_state()
    S.close()
    return src


# ---------------------------------------------------------------------------------------------------------------- 1. read == host read

@pytest.mark.parametrize("env_id,n", [(e, N) for e in ENVS] + [(ENVS[0], 1)])
def test_read_equals_the_host_read(env_id, n):
    import torch
    from miniworld_amd import engine as eng
    v = _make(env_id, n, 1801)
    e = v.engine
    v.reset()
    rng = np.random.default_rng(18)
    for phase in ("reset", "25 steps"):
        if phase != "reset":
            _run(v, rng, 24)
            # ... the last one with the read enqueued directly behind the step, nothing in between
            _act(v, rng.integers(0, v.n_actions, n))
        got = e.get_state_device()
        want = e.get_state()
        assert tuple(got) == tuple(eng.STATE_FIELDS)
        _same_state({k: _np(t) for k, t in got.items()}, want, (env_id, n, phase))
        if n > 64:
            part = e.get_state_device(first=3, count=61)
            _same_state({k: _np(t) for k, t in part.items()}, {k: a[3:64] for k, a in want.items()}, (env_id, phase, "sub-range"))
        # a view with agent_dir alone leaves the other buffers alone
        bufs = {k: torch.full_like(t, -7) for k, t in got.items()}
        e.get_state_device({"agent_dir": bufs["agent_dir"]})
        assert np.array_equal(_bits(_np(bufs["agent_dir"])), _bits(want["agent_dir"]))
        assert all(bool((t == -7).all()) for k, t in bufs.items() if k != "agent_dir")
    # the env's own view of it
    st = v.state()
    _same_state({k: _np(t) for k, t in st.items()}, {k: want[k] for k in st}, (env_id, "state()"))
    if env_id != ENVS[0]:
        assert (want["ent_kind"] != eng.ENT_NONE).any()
    # refused before anything is launched
    lib, h = e.lib, e.h
    view = eng.MwStateView()
    assert lib.mw_get_state_device(h, 0, n, eng.C.byref(view), None) == -1 and b"null" in lib.mw_last_error(h)
    view.agent_dir = got["agent_dir"].data_ptr()
    for first, count in ((-1, 1), (0, n + 1), (n, 1), (1, n), (0, -1), (2 ** 31 - 1, 2)):
        assert lib.mw_get_state_device(h, first, count, eng.C.byref(view), None) == -1, (first, count)
    assert lib.mw_get_state_device(h, 0, n, None, None) == -1
    assert lib.mw_get_state_device(h, n, 0, eng.C.byref(view), None) == 0       # count == 0: MW_OK, nothing launched
    mask = _mask(np.ones(n))
    assert lib.mw_set_state_where(h, None, eng.C.byref(view), None) == -1
    assert lib.mw_set_state_where(h, eng.C.c_void_p(mask.data_ptr()), None, None) == -1
    assert lib.mw_set_state_where(h, eng.C.c_void_p(mask.data_ptr()), eng.C.byref(eng.MwStateView()), None) == -1
    _same_state(e.get_state(), want, (env_id, "refused calls changed the engine"))
    e.check()
    v.close()


# ---------------------------------------------------------------------------------------------------------------- 2. write == host write

def _masks(n):
    alt = np.arange(n) % 2
    last = np.zeros(n, np.uint8)
    last[n - 1] = 1
    return {"zeros": np.zeros(n, np.uint8), "ones": np.ones(n, np.uint8), "alternating": alt.astype(np.uint8), "last env": last}


@pytest.mark.parametrize("env_id,n", [(e, N) for e in ENVS] + [(ENVS[0], 1)])
def test_write_equals_the_host_write(env_id, n):
    from miniworld_amd import engine as eng
    src = _source(env_id, n, 9100, want_depth=True)
    A, B = _make(env_id, n, 1802, want_depth=True), _make(env_id, n, 1802, want_depth=True)
    rng = np.random.default_rng(1802)
    for v in (A, B):
        v.reset()
    for _ in range(5):
        a = rng.integers(0, A.n_actions, n)
        _act(A, a), _act(B, a)
    for fields in (POSE, ENTS, tuple(eng.STATE_FIELDS)):
        for name, mask in _masks(n).items():
            tag = (env_id, n, fields if len(fields) < 3 else "every field", name)
            _host_write(A, src, mask, fields)
            A._redraw()
            assert B.set_state_where(_mask(mask), **_dev(src, fields)) is B.obs
            _same_state(_outputs(B, False), _outputs(A, False), tag + ("write",))
            written = np.flatnonzero(mask)
            now = B.engine.get_state()
            for k in fields:
                assert np.array_equal(_bits(now[k][written]), _bits(src[k][written])), tag + (k,)
            for t in range(12):
                a = rng.integers(0, A.n_actions, n)
                _act(A, a), _act(B, a)
                _same_state(_outputs(B, True), _outputs(A, True), tag + ("step", t))
    for v in (A, B):
        v.engine.check()
        v.close()


# ---------------------------------------------------------------------------------------------------------------- 3. zero mask rows are never read

def test_rows_under_a_zero_mask_byte_are_never_read():
    from miniworld_amd import engine as eng
    env_id = ENVS[2]
    src = _source(env_id, N, 9200)
    v = _make(env_id, N, 1803)
    v.reset()
    _run(v, np.random.default_rng(3), 4)
    before = v.engine.get_state()
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    rows = {}
    for k, a in src.items():
        a = a.copy()
        a[mask == 0] = np.nan if a.dtype == np.float64 else (9 if k == "ent_kind" else -12345)
        rows[k] = a
    assert np.isnan(rows["agent_pos"][1]).all() and rows["carrying"][1] == -12345 and (rows["ent_kind"][1] == 9).all()
    v.engine.set_state_where(_mask(mask), _dev(rows, eng.STATE_FIELDS))
    v.engine.check()
    now = v.engine.get_state()
    _same_state(now, before, "unmasked envs changed", rows=np.flatnonzero(mask == 0))
    _same_state(now, src, "masked envs were not written", rows=np.flatnonzero(mask))
    v._redraw()
    _run(v, np.random.default_rng(4), 3)
    v.engine.check()
    v.close()


# ---------------------------------------------------------------------------------------------------------------- 4. a bad env is skipped whole

def test_a_bad_env_is_skipped_whole():
    from miniworld_amd import engine as eng
    env_id = ENVS[2]
    src = _source(env_id, N, 9300)
    v = _make(env_id, N, 1804)
    v.reset()
    _run(v, np.random.default_rng(5), 4)
    before = v.engine.get_state()
    E = v.engine.E
    assert E >= 2
    written, bad = [2, 40, 66], [5, 9]
    mask = np.zeros(N, np.uint8)
    mask[written + bad] = 1
    rows = {k: a.copy() for k, a in src.items()}
    rows["carrying"][5] = E                 # one past the last slot
    rows["ent_kind"][9, E - 1] = 9          # no such kind
    v.engine.set_state_where(_mask(mask), _dev(rows, eng.STATE_FIELDS))
    with pytest.raises(eng.EngineError, match=r"\(-1\).*mw_set_state_where"):
        v.engine.check()
    v.engine.check()                        # reported once
    now = v.engine.get_state()
    _same_state(now, before, "a skipped or unmasked env changed", rows=[i for i in range(N) if i not in written])
    _same_state(now, src, "the valid envs of the same call were not written", rows=written)
    # the lower ends of the ranges: carrying = -2, a negative kind; -1 and MW_ENT_NONE / MW_ENT_FRAME are legal
    rows = {k: a.copy() for k, a in src.items()}
    rows["carrying"][5], rows["ent_kind"][9, 0] = -2, -1
    rows["carrying"][2], rows["ent_kind"][40, 0], rows["ent_kind"][66, E - 1] = -1, eng.ENT_NONE, eng.ENT_FRAME
    v.engine.set_state_where(_mask(mask), _dev(rows, ("carrying", "ent_kind")))
    with pytest.raises(eng.EngineError, match=r"\(-1\)"):
        v.engine.check()
    v.engine.check()
    now = v.engine.get_state()
    for i in bad:
        assert now["carrying"][i] == before["carrying"][i] and np.array_equal(now["ent_kind"][i], before["ent_kind"][i])
    for i in written:
        assert now["carrying"][i] == rows["carrying"][i] and np.array_equal(now["ent_kind"][i], rows["ent_kind"][i])
    # beside a sticky bit of the status word (a snapshot load with a record index out of range: skipped, nothing read or written) the
    # skipped env is still reported, first and once; every later check reports the sticky bit
    snap = v.save_state()
    v.engine.snapshot_load(snap.data, N, N, envs=[1], records=[N])
    v.engine.set_state_where(_mask(mask), _dev(rows, ("carrying", "ent_kind")))
    with pytest.raises(eng.EngineError, match=r"\(-1\).*mw_set_state_where"):
        v.engine.check()
    for _ in range(2):
        with pytest.raises(eng.EngineError, match=r"\(-1\).*mw_snapshot"):
            v.engine.check()
    v.close()


# ---------------------------------------------------------------------------------------------------------------- 5. obligations

def _short_episodes(monkeypatch, cls_name, steps):
    """episodes of at most `steps` steps (the way tests/test_gpu_snapshot.py does it)"""
    from miniworld_amd import envs
    base = getattr(envs, cls_name)

    class Short(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.max_episode_steps = steps
    Short.__name__ = Short.__qualname__ = cls_name
    monkeypatch.setattr(envs, cls_name, Short)


def test_a_written_env_loses_its_pending_reset_and_keeps_its_stack(monkeypatch):
    """Next-step engine with a frame stack (K = 3): the envs end their episodes at step 6 and are pending.  Half of them are written:
    their next step is an ordinary one and their stacks go on, the others install their next world and rebuild — as in the twin
    through mw_set_state."""
    from miniworld_amd import engine as eng
    _short_episodes(monkeypatch, "Hallway", 6)
    env_id, kw = ENVS[0], dict(autoreset="next_step", frame_stack=3, want_depth=True)
    src = _source(env_id, N, 9400, steps=3, **kw)
    A, B = _make(env_id, N, 1805, **kw), _make(env_id, N, 1805, **kw)
    rng = np.random.default_rng(1805)
    for v in (A, B):
        v.reset()
    for _ in range(6):
        a = rng.integers(0, A.n_actions, N)
        _act(A, a), _act(B, a)
    pending = _np(B.reset_pending())
    assert pending.sum() >= N - 8 and np.array_equal(pending, _np(B.truncated) | _np(B.terminated))     # (an env that met its box early is mid-episode)
    mask = (np.arange(N) % 2 == 1).astype(np.uint8)
    assert pending[mask == 1].any() and pending[mask == 0].any()
    fields = tuple(eng.STATE_FIELDS)
    _host_write(A, src, mask, fields)
    A._redraw()
    B.set_state_where(_mask(mask), **_dev(src, fields))
    assert np.array_equal(_np(B.reset_pending()), pending * (1 - mask))
    _same_state(_outputs(B, False), _outputs(A, False), "write")
    assert np.array_equal(_np(B.stack), _np(A.stack))
    for t in range(4):
        a = rng.integers(0, A.n_actions, N)
        _act(A, a), _act(B, a)
        _same_state(_outputs(B, True), _outputs(A, True), ("step", t))
        assert np.array_equal(_np(B.stack), _np(A.stack)), ("stack", t)
        if t == 0:
            steps = B.engine.get_state()["step_count"]
            # an ordinary step of the state written / the install of a new world
            assert np.array_equal(steps[mask == 1], src["step_count"][mask == 1] + 1) and (steps[(mask == 0) & (pending == 1)] == 0).all()
    for v in (A, B):
        v.engine.check()
        v.close()


def test_only_the_written_envs_cached_frames_go():
    """Hallway, four cache slots, frame reuse off: after a turn left and a turn right every env's next turn left is a cache hit —
    but for env 5, whose box was moved in between."""
    import torch
    from miniworld_amd import engine as eng
    env_id = ENVS[0]
    V = _make(env_id, N, 1806, frame_cache=4, frame_reuse=False, want_depth=True)
    W = _make(env_id, N, 1806, frame_cache=0, frame_reuse=False, want_depth=True)
    assert V.frame_cache == 4 and W.frame_cache == 0
    for v in (V, W):
        v.reset()
    for a in (0, 1):
        for v in (V, W):
            _act(v, np.full(N, a))
    assert V.engine.raster_path() == eng.PATH_QUAD
    mask = np.zeros(N, np.uint8)
    mask[5] = 1
    ent_pos = V.state(["ent_pos"])["ent_pos"].clone()
    ent_pos[5, 0, 2] += 0.25
    for v in (V, W):
        v.set_state_where(_mask(mask), ent_pos=ent_pos)
    assert torch.equal(V.obs, W.obs) and torch.equal(V.depth, W.depth)
    for v in (V, W):
        _act(v, np.full(N, 0))
    source = _np(V.frame_source())
    assert source[5] == 0, "the written env's cached frame matched again"
    assert (np.delete(source, 5) >= 2).all(), ("the other envs lost their cached frames", source)
    assert torch.equal(V.obs, W.obs) and torch.equal(V.depth, W.depth)
    for t, a in enumerate((1, 0, 2)):
        for v in (V, W):
            _act(v, np.full(N, a))
        assert torch.equal(V.obs, W.obs) and torch.equal(V.depth, W.depth), t
    _same_state(V.engine.get_state(), W.engine.get_state(), "twin")
    for v in (V, W):
        v.engine.check()
        v.close()


def test_the_step_after_a_write_draws_every_env():
    """Frame reuse on (PutNext, boxes only): a drop with empty hands changes nothing, so every env stays undrawn — until a write, after
    which the held frame is gone and the step draws every env.  The frame-clean bytes of the written envs go with the call."""
    import torch
    from miniworld_amd import engine as eng
    env_id, DROP = ENVS[2], 5
    X = _make(env_id, N, 1807, frame_cache=0, frame_reuse=True)
    Y = _make(env_id, N, 1807, frame_cache=0, frame_reuse=False)
    assert X.frame_reuse and not Y.frame_reuse
    for v in (X, Y):
        v.reset()
        _act(v, np.full(N, DROP))
        _act(v, np.full(N, DROP))
    assert X.engine.raster_path() == eng.PATH_QUAD
    assert (_np(X.frame_source()) == 1).all() and (_np(X.frame_clean()) == 1).all()
    mask = (np.arange(N) % 4 == 2).astype(np.uint8)
    dirs = X.state(["agent_dir"])["agent_dir"] + 0.5
    for v in (X, Y):
        v.engine.set_state_where(_mask(mask), {"agent_dir": dirs})
    assert np.array_equal(_np(X.frame_clean()), 1 - mask)
    for v in (X, Y):
        _act(v, np.full(N, DROP))
    assert (_np(X.frame_source()) == 0).all(), "a row from before the write was kept"
    assert torch.equal(X.obs, Y.obs)
    _act(X, np.full(N, DROP)), _act(Y, np.full(N, DROP))
    assert (_np(X.frame_source()) == 1).all() and torch.equal(X.obs, Y.obs)
    for v in (X, Y):
        v.engine.check()
        v.close()


# ---------------------------------------------------------------------------------------------------------------- 6. adapter and env

def test_the_adapter_reports_the_state_it_holds():
    import torch
    from miniworld_amd.vector import MiniWorldVectorEnv
    envs = MiniWorldVectorEnv(ENVS[0], N, info_state=("agent_pos", "agent_dir"), seed=1808)
    _, info = envs.reset(seed=1808)
    want = envs.vec.engine.get_state()
    assert set(info) == {"agent_pos", "agent_dir"}
    for k in info:
        assert np.array_equal(_bits(_np(info[k])), _bits(want[k])), k
    rng = np.random.default_rng(8)
    for _ in range(3):
        *_, info = envs.step(torch.as_tensor(rng.integers(0, 3, N), device="cuda"))
    want = envs.vec.engine.get_state()
    for k in ("agent_pos", "agent_dir"):
        assert np.array_equal(_bits(_np(info[k])), _bits(want[k])), k
    assert "_final_info" in info
    envs.close()
