"""Seeded resets on the device: mw_reset_where (MiniWorldVecEnv.reset_where) and the seeded same-step auto-reset (mw_set_reset_seeds,
MiniWorldVecEnv(autoreset="seeds")).

Every comparison is bit for bit and against a SECOND engine that uses only the host-seeded calls of before — engine.reset(mask, seeds)
from host arrays, whose worlds the other suites pin to the reference's env.reset(seed=s): states (mw_get_state), observations, depth,
rewards, flags, stacks.  The streams have no getter; they show in what the envs draw afterwards (auto-resets on the env's own stream,
per-step domain randomisation, CollectHealth's respawns), which is why every comparison goes on for several episodes.  Nothing here
provokes a fault: the refused calls are refused on the host, before anything is launched."""
import ctypes

import numpy as np
import pytest

from test_gpu_snapshot import _actions, _ends, _make, _np, _short_episodes, _step

pytestmark = pytest.mark.gpu

HALLWAY, MAZE, PICKUP, COLLECT, FOURROOMS = ("MiniWorld-Hallway-v0", "MiniWorld-Maze-v0", "MiniWorld-PickupObjects-v0", "MiniWorld-CollectHealth-v0",
                                             "MiniWorld-FourRooms-v0")
EDGE_SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63 + 5, 2 ** 64 - 1]
# name: env id, num_envs, number of actions, the family whose episodes are shortened (None: max_episode_steps is a keyword), keywords
CONFIGS = {
    "hallway-130": (HALLWAY, 130, 3, "Hallway", {}),
    "hallway-70": (HALLWAY, 70, 3, "Hallway", {}),
    "hallway-philox": (HALLWAY, 9, 3, "Hallway", dict(rng="philox")),
    "maze": (MAZE, 5, 3, None, {}),
    "pickup-dr": (PICKUP, 9, 5, "PickupObjects", dict(domain_rand=True)),
    "collecthealth": (COLLECT, 9, 8, "CollectHealth", {}),
    "fourrooms": (FOURROOMS, 9, 3, "FourRooms", {}),
}


def _config(monkeypatch, name, steps, **more):
    env_id, n, n_actions, short, kw = CONFIGS[name]
    kw = dict(kw, want_depth=True, **more)
    if short:
        _short_episodes(monkeypatch, short, steps)
    else:
        kw["max_episode_steps"] = steps
    return env_id, n, n_actions, kw


def _dev_seeds(seeds):
    """uint64 seeds as the int64 device tensor the binding takes (the bits)"""
    import torch
    return torch.from_numpy(np.asarray(seeds, np.uint64).view(np.int64).copy()).cuda()


def _dev_mask(mask):
    import torch
    return torch.from_numpy(np.asarray(mask, bool).astype(np.uint8)).cuda()


def _trace(v):
    out = {f: _np(getattr(v, f)).copy() for f in ("obs", "depth", "reward", "terminated", "truncated")}
    if v.frame_stack:
        out["stack"] = _np(v.stack).copy()
    return out


def _same(got, want, tag):
    assert got.keys() == want.keys(), tag
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), tag + (k,)


def _same_state(a, b, tag, rows=None):
    sa, sb = a.engine.get_state(), b.engine.get_state()
    for k in sb:
        x, y = (sa[k], sb[k]) if rows is None else (sa[k][rows], sb[k][rows])
        assert np.array_equal(x, y), tag + ("state", k)


def _close(*envs):
    for v in envs:
        v.engine.check()
        v.close()


# ---------------------------------------------------------------------------------------------------------------- 1. mw_reset_where

def _mask_and_seeds(name, n, rng):
    """hallway-130: the reset kernel's blocks are envs 0 .. 63, 64 .. 127 and the ragged 128 .. 129 — the first holds the edge seeds,
    the second is all zero, the third has env 129 alone.  The small batches: about half the envs, env 0 and the last one among them."""
    mask = np.zeros(n, bool)
    seeds = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    if n == 130:
        first = [1, 5, 8, 20, 33, 47, 63]
        mask[first + [0, 2, 62, 129]] = True
        seeds[first] = np.array(EDGE_SEEDS, np.uint64)
    else:
        mask[rng.random(n) < 0.5] = True
        mask[[0, n - 1]] = True
        mask[1] = False
        k = np.flatnonzero(mask)
        seeds[k[:3]] = np.array([2 ** 63 + 5, 2 ** 32 - 1, 2 ** 32], np.uint64)[:len(k[:3])]
    return mask, seeds


@pytest.mark.parametrize("name", ["hallway-130", "maze", "pickup-dr", "collecthealth", "fourrooms", "hallway-philox"])
def test_reset_where_is_the_host_reset_with_device_arrays(name, monkeypatch):
    """Twin engines with a few steps behind them.  A: reset_where(mask, seeds), both tensors on the device, garbage under the zero
    mask bytes.  B: engine.reset(mask, seeds) from host arrays, then the frame.  After the reset and after each of 20 more steps of the
    same random actions (episodes of at most 6 steps: every env auto-resets on its own stream several times) the two are the same
    engine.  The unmasked envs' states are exactly what they were before the call, and their later trajectories equal B's: their
    streams were not touched either."""
    env_id, n, n_actions, kw = _config(monkeypatch, name, 6)
    rng = np.random.default_rng(6100 + n)
    acts = _actions(rng, 23, n, n_actions, 0.5)
    A, B = _make(env_id, n, 6100, **kw), _make(env_id, n, 6100, **kw)
    for v in (A, B):
        v.reset()
        for t in range(3):
            _step(v, acts[t])
    mask, seeds = _mask_and_seeds(name, n, rng)
    before = A.engine.get_state()
    wild = np.where(mask, seeds, rng.integers(0, 2 ** 64, n, dtype=np.uint64))      # (never read under a zero mask byte)
    assert A.reset_where(_dev_mask(mask), _dev_seeds(wild)) is A.obs
    B.engine.reset(mask.astype(np.uint8), seeds)
    B._redraw()
    after = A.engine.get_state()
    for k in before:
        assert np.array_equal(after[k][~mask], before[k][~mask]), (name, "an unmasked env was written", k)
    assert any(not np.array_equal(after[k][mask], before[k][mask]) for k in before)
    _same_state(A, B, (name, "after the reset"))
    assert np.array_equal(_np(A.obs), _np(B.obs)) and np.array_equal(_np(A.depth), _np(B.depth)), (name, "first frames")
    ends = np.zeros(n, int)
    for t in range(3, 23):
        for v in (A, B):
            _step(v, acts[t])
        _same(_trace(A), _trace(B), (name, "step", t))
        ends += _ends(B)
    assert ends.min() >= 2, "every env restarted on its own stream"
    _same_state(A, B, (name, "after 20 steps"))
    _close(A, B)


def test_reset_where_keeps_the_stack_flags_and_the_other_envs_cached_frames(monkeypatch):
    """With a frame stack the masked envs' stacks are rebuilt by the refresh (K copies of the new first frame), the others keep their
    windows — as after engine.reset(mask, seeds) on the twin.  And left, right, reset_where of the odd envs, left, right: the even
    envs get their frames from the cache, the odd ones — whose epoch advanced — do not."""
    n, K = 8, 3
    A, B = (_make(HALLWAY, n, 6150, want_depth=True, frame_stack=K, frame_cache=4) for _ in range(2))
    left, right = np.zeros(n, int), np.ones(n, int)
    for v in (A, B):
        v.reset()
        _step(v, left)
        _step(v, right)
    odd = np.arange(n) % 2 == 1
    seeds = np.arange(n, dtype=np.uint64) + np.uint64(2 ** 33)
    A.reset_where(_dev_mask(odd), _dev_seeds(seeds))
    B.engine.reset(odd.astype(np.uint8), seeds)
    B._redraw()
    assert np.array_equal(_np(A.stack), _np(B.stack))
    stack = _np(A.stack)
    assert all(np.array_equal(stack[i, k], stack[i, K - 1]) for i in np.flatnonzero(odd) for k in range(K))
    _step(A, left)
    went = _np(A.frame_source()).copy()
    _step(A, right)
    back = _np(A.frame_source()).copy()
    assert (back[~odd] >= 2).all(), (went, back)
    assert (went[odd] < 2).all(), (went, "a reset env was served a frame cached before the reset")
    for act in (left, right):
        _step(B, act)
    _same(_trace(A), _trace(B), ("stack", "two steps later"))
    _close(A, B)


def test_reset_where_refuses_before_anything_is_launched():
    """MW_E_INVALID for a null mask, null seeds, and MW_GEN_PROGRAM without a program; the engine is as it was.  MW_GEN_NONE: the
    call is accepted (the masked envs are re-seeded only)."""
    import torch
    from miniworld_amd import engine as E
    from miniworld_amd.scene import base_config
    n = 6
    V = _make(HALLWAY, n, 6200)
    V.reset()
    m, s = _dev_mask(np.ones(n, bool)), _dev_seeds(np.arange(n))
    before = _np(V.save_state().data).copy()
    lib, h = V.engine.lib, V.engine.h
    assert lib.mw_reset_where(h, None, ctypes.c_void_p(s.data_ptr()), None) == -1
    assert lib.mw_reset_where(h, ctypes.c_void_p(m.data_ptr()), None, None) == -1
    for call in (lambda: V.engine.reset_where(None, s), lambda: V.engine.reset_where(m, None), lambda: V.engine.reset_where(m, s.int()),
                 lambda: V.engine.reset_where(m[:3], s), lambda: V.engine.reset_where(m.cpu(), s)):
        with pytest.raises(E.EngineError):
            call()
    torch.cuda.synchronize()
    assert np.array_equal(_np(V.save_state().data), before)
    _close(V)
    for gen, want in ((E.GEN_PROGRAM, -1), (E.GEN_NONE, 0)):
        cfg = base_config(4, 80, 60, 1, 6, 4, 16)
        cfg.abi_version = E.ABI_VERSION
        cfg.generator = gen
        hh = ctypes.c_void_p()
        assert lib.mw_create(ctypes.byref(cfg), ctypes.byref(hh)) == 0
        m4, s4 = _dev_mask(np.ones(4, bool)), _dev_seeds(np.arange(4))
        assert lib.mw_reset_where(hh, ctypes.c_void_p(m4.data_ptr()), ctypes.c_void_p(s4.data_ptr()), None) == want, gen
        torch.cuda.synchronize()
        lib.mw_destroy(hh)


# ---------------------------------------------------------------------------------------------------------------- 2. the seeded auto-reset

class _Loop:
    """The reference loop on an autoreset=False env, step by step: step; engine.reset(mask = done, seeds = next_seed) from host arrays;
    the frame (and the stack refresh).  Its own next_seed / episode_seed bookkeeping on the host."""

    def __init__(self, env_id, n, seed, **kw):
        self.v, self.n = _make(env_id, n, seed, autoreset=False, **kw), n
        self.v.reset(seed=seed)
        self.episode_seed = np.arange(n, dtype=np.int64) + seed
        self.next_seed = self.episode_seed + n
        self.terminal = None

    def step(self, act=None, repeat=1, plans=None):
        import torch
        v = self.v
        if plans is not None:
            v.rollout(torch.as_tensor(np.ascontiguousarray(plans), dtype=torch.int32, device="cuda"))
        else:
            _step(v, act, repeat)
        done = _ends(v)
        self.terminal = (_np(v.obs).copy(), _np(v.depth).copy(), None if not v.frame_stack else _np(v.stack).copy())
        v.engine.reset(done.astype(np.uint8), self.next_seed.astype(np.uint64))
        v._redraw()
        self.episode_seed[done] = self.next_seed[done]
        self.next_seed[done] += self.n
        return done


def _stagger(envs, counts):
    for v in envs:
        v.engine.set_state({"step_count": np.asarray(counts, np.int32)})


def _books(A, loop, tag):
    assert np.array_equal(_np(A.episode_seed), loop.episode_seed), tag + ("episode_seed",)
    assert np.array_equal(_np(A.next_seed), loop.next_seed), tag + ("next_seed",)


def test_seeded_autoreset_is_the_reference_loop_hallway(monkeypatch):
    """Hallway x 70, episodes of 3 steps, turning only.  step_count = i % 3 through mw_set_state staggers the ends: every step
    finishes a third of the envs.  Before step 7 a second injection (0 for the block of envs 0 .. 63; 0 or 2 for the others) brings a
    step that finishes nobody and one that finishes the whole 64-env block.  The caller writes next_seed before every step, on the
    device for A and on the host for the loop: seeds 7062 .. 7301, none of which spawns the agent within reach of the box (the host
    generator says so; such an env would end on its first step and blur the schedule), and on some steps the edge seeds for envs
    0 .. 6.  Over 12 steps every step's observation, depth, reward, flags and state equal the loop's, and so do episode_seed /
    next_seed."""
    import torch
    env_id, n, n_actions, kw = _config(monkeypatch, "hallway-70", 3)
    seed = 7062
    acts = np.random.default_rng(seed).integers(0, 2, (12, n))
    A, loop = _make(env_id, n, seed, autoreset="seeds", **kw), _Loop(env_id, n, seed, **kw)
    A.reset(seed=seed)
    B = loop.v
    _same(_trace(A), _trace(B), ("reset",))
    _books(A, loop, ("reset",))
    _stagger((A, B), np.arange(n) % 3)
    kinds, counts = set(), []
    for t in range(12):
        if t == 6:
            _stagger((A, B), np.where(np.arange(n) < 64, 0, (np.arange(n) % 2) * 2))
        if t > 0:       # (step 0 runs on the seeds reset() laid out: s + N + i)
            chosen = (7062 + (t * n + np.arange(n)) % 240).astype(np.int64)
            if t % 3 == 2:
                chosen[:7] = np.array(EDGE_SEEDS, np.uint64).view(np.int64)
            A.next_seed.copy_(torch.from_numpy(chosen))
            loop.next_seed[:] = chosen
        _step(A, acts[t])
        done = loop.step(acts[t])
        assert np.array_equal(_ends(A), done), (t, "done")
        kinds.add("none" if not done.any() else "block" if done[:64].all() else "some")
        counts.append((int(done[:64].sum()), int(done[64:].sum())))
        _same(_trace(A), _trace(B), ("step", t))
        _same_state(A, B, ("step", t))
        _books(A, loop, ("step", t))
        assert not _np(A.reset_pending()).any(), t
    assert kinds == {"none", "block", "some"}, (kinds, counts)
    _close(A, B)


@pytest.mark.parametrize("name", ["maze", "pickup-dr", "collecthealth"])
def test_seeded_autoreset_is_the_reference_loop(name, monkeypatch):
    """The same over the Maze (a wavefront per env, spare worlds, side-stream refills), PickupObjects with domain randomisation (no
    spares; the terminal step's draws come from the old stream) and CollectHealth (respawns draw from the stream), random actions,
    12 steps of 3-step episodes staggered by step_count = i % 3."""
    env_id, n, n_actions, kw = _config(monkeypatch, name, 3)
    seed = 6400
    acts = _actions(np.random.default_rng(seed), 12, n, n_actions, 0.5)
    A, loop = _make(env_id, n, seed, autoreset="seeds", **kw), _Loop(env_id, n, seed, **kw)
    A.reset(seed=seed)
    B = loop.v
    _stagger((A, B), np.arange(n) % 3)
    ends = np.zeros(n, int)
    for t in range(12):
        _step(A, acts[t])
        ends += loop.step(acts[t])
        _same(_trace(A), _trace(B), (name, "step", t))
        _same_state(A, B, (name, "step", t))
        _books(A, loop, (name, "step", t))
    assert ends.min() >= 3
    _close(A, B)


@pytest.mark.parametrize("name", ["hallway-70", "maze", "pickup-dr"])
def test_without_seeds_again_the_envs_continue_on_their_streams(name, monkeypatch):
    """Five seeded steps beside the loop, then mw_set_reset_seeds(NULL).  C is a plain same-step env that loads the loop engine's
    records (state, stream, spare worlds).  From there A and C are the same engine for 9 steps of 3-step episodes: A's streams are
    the loop's, and its finished envs restart on them like any same-step env's."""
    env_id, n, n_actions, kw = _config(monkeypatch, name, 3)
    seed = 6500
    acts = _actions(np.random.default_rng(seed), 14, n, n_actions, 0.5)
    A, loop = _make(env_id, n, seed, autoreset="seeds", **kw), _Loop(env_id, n, seed, **kw)
    A.reset(seed=seed)
    _stagger((A, loop.v), np.arange(n) % 3)
    for t in range(5):
        _step(A, acts[t])
        loop.step(acts[t])
    C = _make(env_id, n, seed + 1, **kw)
    C.reset()
    C.load_state(loop.v.save_state())
    A.engine.set_reset_seeds(None)
    ends = np.zeros(n, int)
    for t in range(5, 14):
        for v in (A, C):
            _step(v, acts[t])
        _same(_trace(A), _trace(C), (name, "step", t))
        ends += _ends(C)
    assert ends.min() >= 2
    _same_state(A, C, (name, "the end"))
    _close(A, C, loop.v)


# ---------------------------------------------------------------------------------------------------------------- 3. composition

def test_seeds_compose_with_final_observations(monkeypatch):
    """final_obs=True beside seeds: the finished envs' rows of final_obs / final_depth are the loop engine's terminal frames, the
    other rows keep their sentinel, and everything else is the loop's."""
    env_id, n, n_actions, kw = _config(monkeypatch, "hallway-70", 3)
    seed = 6600
    acts = _actions(np.random.default_rng(seed), 8, n, n_actions, 0.5)
    A, loop = _make(env_id, n, seed, autoreset="seeds", final_obs=True, **kw), _Loop(env_id, n, seed, **kw)
    A.reset(seed=seed)
    _stagger((A, loop.v), np.arange(n) % 3)
    for t in range(8):
        A.final_obs.fill_(0xA5)
        A.final_depth.fill_(-7.0)
        _step(A, acts[t])
        done = loop.step(acts[t])
        _same(_trace(A), _trace(loop.v), ("final", "step", t))
        fo, fd = _np(A.final_obs), _np(A.final_depth)
        assert np.array_equal(fo[done], loop.terminal[0][done]) and np.array_equal(fd[done], loop.terminal[1][done]), t
        assert (fo[~done] == 0xA5).all() and (fd[~done] == -7.0).all(), t
    _same_state(A, loop.v, ("final", "the end"))
    _close(A, loop.v)


@pytest.mark.parametrize("pad", ["reset", "zero"])
def test_seeds_compose_with_the_frame_stack(pad, monkeypatch):
    """frame_stack = 3: one push per step that rebuilds the finished envs' stacks; the loop pushes, resets, draws and refreshes."""
    env_id, n, n_actions, kw = _config(monkeypatch, "hallway-70", 3, frame_stack=3, stack_pad=pad)
    seed = 6700
    acts = _actions(np.random.default_rng(seed), 9, n, n_actions, 0.5)
    A, loop = _make(env_id, n, seed, autoreset="seeds", **kw), _Loop(env_id, n, seed, **kw)
    A.reset(seed=seed)
    _stagger((A, loop.v), np.arange(n) % 3)
    _same(_trace(A), _trace(loop.v), (pad, "reset"))
    for t in range(9):
        _step(A, acts[t])
        loop.step(acts[t])
        _same(_trace(A), _trace(loop.v), (pad, "step", t))
    _close(A, loop.v)


@pytest.mark.parametrize("form", ["repeat", "plan"])
def test_seeds_compose_with_repeats_and_plans(form, monkeypatch):
    """step(repeat = 4) and a drawn rollout of horizon 4, episodes of 6 steps staggered by step_count = i % 6: an env stops at the
    sub-step that ends its episode and starts the episode of its seed.  The loop engine takes the same call without auto-reset — up
    to four single steps per env that stop at done, by that call's own contract — and is reset from the host."""
    env_id, n, n_actions, kw = _config(monkeypatch, "hallway-70", 6)
    seed = 6800
    rng = np.random.default_rng(seed)
    A, loop = _make(env_id, n, seed, autoreset="seeds", **kw), _Loop(env_id, n, seed, **kw)
    A.reset(seed=seed)
    _stagger((A, loop.v), np.arange(n) % 6)
    ends = np.zeros(n, int)
    for t in range(6):
        import torch
        if form == "repeat":
            act = _actions(rng, 1, n, n_actions, 0.5)[0]
            _step(A, act, 4)
            done = loop.step(act, repeat=4)
        else:
            plans = _actions(rng, 4, n, n_actions, 0.5)
            A.rollout(torch.as_tensor(plans, dtype=torch.int32, device="cuda"))
            done = loop.step(plans=plans)
        ends += done
        _same(_trace(A), _trace(loop.v), (form, "call", t))
        assert np.array_equal(_np(A.substeps), _np(loop.v.substeps)), (form, t)
        _same_state(A, loop.v, (form, "call", t))
        _books(A, loop, (form, "call", t))
    assert ends.min() >= 2
    _close(A, loop.v)


def test_frame_reuse_and_the_frame_cache_change_nothing_and_still_serve(monkeypatch):
    """Episodes of 6 steps staggered by step_count = i % 6, every env turning left on even steps and right on odd ones, so that an
    env is back in a state it has shown before from its third step on.  The loop's trace, then four seeded envs: cache and reuse on,
    either off, both off — identical outputs.  With both on, in the steps in which some envs finished and others did not, rows of
    envs that did not finish come from the cache or stay as clean (mw_get_frame_source), and a finished env's row is a drawn one."""
    env_id, n, n_actions, kw = _config(monkeypatch, "hallway-70", 6)
    seed, T = 6900, 14
    acts = np.tile((np.arange(T) % 2)[:, None], (1, n))
    loop = _Loop(env_id, n, seed, **kw)
    _stagger((loop.v,), np.arange(n) % 6)
    want, dones = [], []
    for t in range(T):
        dones.append(loop.step(acts[t]))
        want.append(_trace(loop.v))
    _close(loop.v)
    for variant in ({}, dict(frame_cache=0), dict(frame_reuse=False), dict(frame_cache=0, frame_reuse=False)):
        A = _make(env_id, n, seed, autoreset="seeds", **dict(kw, **variant))
        A.reset(seed=seed)
        _stagger((A,), np.arange(n) % 6)
        served = 0
        for t in range(T):
            _step(A, acts[t])
            _same(_trace(A), want[t], (tuple(variant), "step", t))
            src, done = _np(A.frame_source()), dones[t]
            assert (src[done] == 0).all(), (variant, t, "a finished env's row is drawn by the list pass")
            if done.any() and not done.all():
                served += int((src[~done] >= 1).sum())
            if variant.get("frame_cache", 4) == 0:
                assert (src < 2).all(), (variant, t)
        if not variant:
            assert served > 0, "no env that did not finish was ever served a cached or clean row beside finishing ones"
        _close(A)


def test_set_reset_seeds_refuses(monkeypatch):
    """MW_E_INVALID on a next-step engine, an off engine and a MW_GEN_NONE engine.  A frameless mw_step_plan while seeds are set is
    MW_E_INVALID and leaves state and stream untouched (the records hold both); the drawn call goes through afterwards."""
    import torch
    from miniworld_amd import engine as E
    from miniworld_amd.scene import base_config
    n = 6
    seeds = _dev_seeds(np.arange(n) + 40)
    for mode in (False, "next_step"):
        v = _make(HALLWAY, n, 7000, autoreset=mode)
        assert v.engine.lib.mw_set_reset_seeds(v.engine.h, ctypes.c_void_p(seeds.data_ptr())) == -1, mode
        with pytest.raises(E.EngineError):
            v.engine.set_reset_seeds(seeds)
        v.close()
    lib = E.load_library()
    cfg = base_config(4, 80, 60, 1, 6, 4, 16)
    cfg.abi_version = E.ABI_VERSION
    cfg.autoreset = E.AUTORESET_SAME_STEP
    cfg.generator = E.GEN_NONE
    h = ctypes.c_void_p()
    assert lib.mw_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    assert lib.mw_set_reset_seeds(h, ctypes.c_void_p(seeds.data_ptr())) == -1
    assert lib.mw_set_reset_seeds(h, None) == -1
    lib.mw_destroy(h)

    _short_episodes(monkeypatch, "Hallway", 3)
    A = _make(HALLWAY, n, 7000, autoreset="seeds")
    A.reset(seed=7000)
    for call in (lambda: A.engine.set_reset_seeds(seeds.int()), lambda: A.engine.set_reset_seeds(seeds[:3]), lambda: A.engine.set_reset_seeds(seeds.cpu())):
        with pytest.raises(E.EngineError):
            call()
    _step(A, np.zeros(n, int))
    before, obs = _np(A.save_state().data).copy(), _np(A.obs).copy()
    plans = torch.zeros((4, n), dtype=torch.int32, device="cuda")
    with pytest.raises(E.EngineError, match="frameless"):
        A.engine.step_plan(plans, None, None, A.reward, None, A.terminated, A.truncated, None)
    with pytest.raises(ValueError, match="frameless"):
        A.rollout(plans, render=False)
    torch.cuda.synchronize()
    assert np.array_equal(_np(A.save_state().data), before) and np.array_equal(_np(A.obs), obs)
    A.rollout(plans)
    assert _ends(A).all() and np.array_equal(_np(A.episode_seed), np.arange(n) + 7000 + n)
    _close(A)
