"""MW_AUTORESET_NEXT_STEP: the step that ends an episode returns its terminal frame; the env's next step ignores its action,
installs the next world and returns its first frame with reward 0 and no flags (gymnasium's AutoresetMode.NEXT_STEP).

The yardstick is the reference's own loop, "obs = step(a); if done: reset()" (miniworld.py:670-730 leaves the reset to the
caller), run on a second engine without auto-reset whose host calls mw_reset(mask, seeds=NULL) + mw_render after every episode's
end: frames, depth, rewards, flags and the device state must be the same, bit for bit, step for step — the random stream
included (later episodes' worlds, domain-randomisation draws, spare worlds, CollectHealth's respawns)."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu


def _short_episodes(monkeypatch, cls_name, steps):
    """Episodes of at most `steps` steps for a family whose class fixes max_episode_steps (hallway.py:31, tmaze.py:28, ...):
    the batched env reads it from its template instance."""
    from miniworld_amd import envs
    base = getattr(envs, cls_name)

    class Short(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.max_episode_steps = steps
    Short.__name__ = Short.__qualname__ = cls_name
    monkeypatch.setattr(envs, cls_name, Short)


def _rows(st, i):
    return {k: v[i] for k, v in st.items()}


def _same_state(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def _step_then_reset_parity(env_id, n, steps, seed, n_actions, want_depth=False, domain_rand=False, p_fwd=None, **kw):
    """Engine B (next-step auto-reset) against engine C ("step; if done: reset()" from the host).  Per-env action queues: B's env
    i takes the queue's next action on every real step and a DIFFERENT random action on its reset steps (which must be ignored),
    so it lags C's env i by one step per finished episode; B's k-th step is compared with C's k-th record."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    common = dict(seed=seed, want_depth=want_depth, domain_rand=domain_rand, **kw)
    B = MiniWorldVecEnv(env_id, n, autoreset="next_step", **common)
    C = MiniWorldVecEnv(env_id, n, autoreset=False, **common)
    assert B.autoreset_mode == "next_step" and C.autoreset_mode == "off"
    B.reset()
    C.reset()
    rng = np.random.default_rng(seed)
    if p_fwd is None:
        queue = rng.integers(0, n_actions, (n, steps))
    else:
        queue = np.where(rng.random((n, steps)) < p_fwd, 2, rng.integers(0, n_actions, (n, steps)))
    rbuf, dbuf = torch.zeros_like(C.obs), (torch.zeros_like(C.depth) if want_depth else None)
    rec_c = [[] for _ in range(n)]          # C's records per env: (rgb, depth, reward, term, trunc, state)
    k_b = np.zeros(n, np.int64)             # B's records compared so far per env
    q_b = np.zeros(n, np.int64)             # B's next queue position per env
    resets = one_step = 0
    last_reset = np.full(n, -9)
    env_ix = np.arange(n)
    for t in range(steps):
        # C: the reference's loop
        o, r, te, tr = C.step(torch.as_tensor(queue[:, t], dtype=torch.int32, device="cuda"))
        o, d = o.cpu().numpy(), (C.depth.cpu().numpy() if want_depth else None)
        r, te, tr = r.cpu().numpy(), te.cpu().numpy(), tr.cpu().numpy()
        st = C.engine.get_state()
        for i in range(n):
            rec_c[i].append((o[i], None if d is None else d[i], r[i], te[i], tr[i], _rows(st, i)))
        done = (te | tr).astype(bool)
        if done.any():
            C.engine.reset(done.astype(np.uint8), None)
            C.engine.render(rbuf, dbuf)
            ro, rd, st = rbuf.cpu().numpy(), (dbuf.cpu().numpy() if want_depth else None), C.engine.get_state()
            for i in np.nonzero(done)[0]:
                rec_c[i].append((ro[i], None if rd is None else rd[i], np.float32(0), 0, 0, _rows(st, i)))
        # B: the same actions, another one on its reset steps
        pend = B.reset_pending().cpu().numpy().astype(bool)
        want = queue[env_ix, q_b]
        other = (want + 1 + rng.integers(0, n_actions - 1, n)) % n_actions
        act = np.where(pend, other, want)
        o, r, te, tr = B.step(torch.as_tensor(act, dtype=torch.int32, device="cuda"))
        o, d = o.cpu().numpy(), (B.depth.cpu().numpy() if want_depth else None)
        r, te, tr = r.cpu().numpy(), te.cpu().numpy(), tr.cpu().numpy()
        st = B.engine.get_state()
        for i in range(n):
            c = rec_c[i][k_b[i]]
            tag = (env_id, t, i, "reset step" if pend[i] else "step")
            assert np.array_equal(o[i], c[0]), tag + ("rgb",)
            if want_depth:
                assert np.array_equal(d[i], c[1]), tag + ("depth",)
            assert r[i] == c[2] and te[i] == c[3] and tr[i] == c[4], tag + ("reward / flags", r[i], te[i], tr[i], c[2:5])
            assert _same_state(_rows(st, i), c[5]), tag + ("state",)
            if pend[i]:
                assert r[i] == 0 and te[i] == 0 and tr[i] == 0, tag
                one_step += int(t - last_reset[i] == 2)        # reset, one step that ended the episode, reset
                last_reset[i] = t
                resets += 1
        k_b += 1
        q_b += ~pend
        # the flags say which envs the next step resets: those whose episode this step ended
        assert np.array_equal(B.reset_pending().cpu().numpy(), (te | tr).astype(np.uint8)), (env_id, t)
    B.engine.check()
    C.engine.check()
    B.close()
    C.close()
    return resets, one_step


@pytest.mark.parametrize("env_id,cls_name,spare,mes,depth", [
    ("MiniWorld-Hallway-v0", "Hallway", "0", 3, True), ("MiniWorld-Hallway-v0", "Hallway", "1", 3, True),
    ("MiniWorld-OneRoom-v0", "OneRoom", "0", 2, False), ("MiniWorld-OneRoom-v0", "OneRoom", "1", 1, False)])
def test_next_step_equals_step_then_reset_dense_k1(env_id, cls_name, spare, mes, depth, monkeypatch):
    """Hallway / OneRoom (the dense K1, several envs per wave, the leading lane installs), without and with spare worlds.
    OneRoom with episodes of ONE step: every other step of every env is a reset step, consecutive one-step episodes claim
    spares whose refill may not have run yet."""
    monkeypatch.setenv("MW_SPARE", spare)
    _short_episodes(monkeypatch, cls_name, mes)
    resets, one_step = _step_then_reset_parity(env_id, 40, 24, 900, 3, want_depth=depth, p_fwd=0.6)
    assert resets >= 40
    if mes == 1:
        assert one_step >= 40


def test_next_step_equals_step_then_reset_pickup_dr(monkeypatch):
    """PickupObjects with domain randomisation: meshes, the wave-per-env K1, the three per-step draws (which a reset step must
    not take, miniworld.py:677-680), the picked object drawn one last time on its step."""
    _short_episodes(monkeypatch, "PickupObjects", 5)
    resets, _ = _step_then_reset_parity("MiniWorld-PickupObjects-v0", 16, 24, 31, 5, domain_rand=True)
    assert resets >= 16


@pytest.mark.parametrize("env_id,mes", [("MiniWorld-MazeS3-v0", 2), ("MiniWorld-Maze-v0", 3)])
def test_next_step_equals_step_then_reset_maze(env_id, mes):
    """The Maze with episodes of 2 - 3 steps: its spares are refilled on the side stream, and a reset step may need one whose
    refill is still running or has not started (the wait and the inline branches of the refill_mask protocol)."""
    resets, _ = _step_then_reset_parity(env_id, 12, 14, 77, 3, max_episode_steps=mes)
    assert resets >= 24


def test_next_step_equals_step_then_reset_collecthealth(monkeypatch):
    """CollectHealth (the wave-per-env K1, no spares): kits consumed on the step that ends an episode respawn with draws from the
    env's stream before the next world is generated from it."""
    _short_episodes(monkeypatch, "CollectHealth", 6)
    resets, _ = _step_then_reset_parity("MiniWorld-CollectHealth-v0", 16, 26, 13, 8, p_fwd=0.3)
    assert resets >= 32


def test_next_step_equals_step_then_reset_placement_program(monkeypatch):
    """TMaze: a placement-program family (coin, placements, its own info key)."""
    _short_episodes(monkeypatch, "TMaze", 3)
    resets, _ = _step_then_reset_parity("MiniWorld-TMaze-v0", 16, 20, 5, 3, want_depth=True)
    assert resets >= 48


def test_next_step_is_same_step_shifted_at_full_size():
    """Hallway with 4096 envs (a BASELINE config): engine A auto-resets on the same step, engine B on the next.  Each env has
    its own action queue.  B's reset step shows what A showed on the terminal step (the new episode's first frame and state);
    B's terminal step has A's reward and flags; every other step is the same.  Frames are compared through a 64-bit weighted
    sum per env (on the device), states and flags exactly."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n, steps = 4096, 150
    A = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, seed=123)
    B = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, seed=123, autoreset="next_step")
    A.reset()
    B.reset()
    rng = np.random.default_rng(0)
    queue = np.where(rng.random((n, steps)) < 0.8, 2, rng.integers(0, 3, (n, steps)))
    w = torch.as_tensor(rng.integers(1, 1 << 20, A.obs[0].numel() // 4), dtype=torch.int64, device="cuda")

    def digest(obs):
        return (obs.reshape(n, -1).view(torch.int32).to(torch.int64) * w).sum(1).cpu().numpy()

    keys = ("agent_pos", "agent_dir", "ent_pos", "ent_dir", "step_count", "cam", "light")
    a_hash, a_rew, a_done, a_state = [], [], [], []
    ia = np.zeros(n, np.int64)      # A's record that B's next real step corresponds to
    env_ix = np.arange(n)
    resets = 0
    for t in range(steps):
        o, r, te, tr = A.step(torch.as_tensor(queue[:, t], dtype=torch.int32, device="cuda"))
        a_hash.append(digest(o))
        a_rew.append(r.cpu().numpy())
        a_done.append(np.stack([te.cpu().numpy(), tr.cpu().numpy()]))
        st = A.engine.get_state()
        a_state.append({k: st[k] for k in keys})
        pend = B.reset_pending().cpu().numpy().astype(bool)
        act = np.where(pend, 0, queue[env_ix, ia])
        o, r, te, tr = B.step(torch.as_tensor(act, dtype=torch.int32, device="cuda"))
        h, r, flags, st = digest(o), r.cpu().numpy(), np.stack([te.cpu().numpy(), tr.cpu().numpy()]), B.engine.get_state()
        j = np.where(pend, ia - 1, ia)      # reset step: A's terminal record
        rec_hash = np.array([a_hash[j[i]][i] for i in range(n)])
        rec_done = np.array([a_done[j[i]][:, i] for i in range(n)]).T
        a_terminal = rec_done.any(0)
        # frames and states: every real step whose A record did not end an episode, and every reset step
        cmp = pend | ~a_terminal
        assert np.array_equal(h[cmp], rec_hash[cmp]), t
        for k in keys:
            rec = np.stack([a_state[j[i]][k][i] for i in range(n)])
            assert np.array_equal(st[k][cmp], rec[cmp]), (t, k)
        # rewards and flags: A's on real steps, zero on reset steps
        rec_rew = np.array([a_rew[j[i]][i] for i in range(n)])
        assert np.array_equal(r[~pend], rec_rew[~pend]) and not r[pend].any(), t
        assert np.array_equal(flags[:, ~pend], rec_done[:, ~pend]) and not flags[:, pend].any(), t
        resets += int(pend.sum())
        ia += ~pend
    assert resets >= n // 4
    A.engine.check()
    B.engine.check()
    A.close()
    B.close()


def test_terminal_frame_is_the_references_and_the_next_step_its_reset():
    """OneRoom, seed 7, 4 samples like the reference's frames on llvmpipe: the actions of gl_oneroom_trunc_s7 truncate the episode on
    step 180; the observation of that step is the reference's own frame of it (gl/180/rgb), and the next step installs the world of
    the reference's reset() continuing the stream."""
    import torch
    from miniworld_amd import envs
    from miniworld_amd.vec_env import MiniWorldVecEnv
    from test_gpu_env_api import _assert_same_world
    from test_oracle_vs_reference_gl import load_gl
    _, tr, meta, _ = helpers.load_case("oneroom_trunc_s7")
    frames = load_gl("oneroom_trunc_s7")
    vec = MiniWorldVecEnv("MiniWorld-OneRoom-v0", 2, seed=7, msaa=4, autoreset="next_step")
    vec.reset()
    act = torch.zeros(2, dtype=torch.int32, device="cuda")
    actions = tr["action"]
    assert len(actions) == 180
    for t in range(180):
        act[:] = int(actions[t])
        o, rew, term, trunc = vec.step(act)
        assert bool(term[0].item()) == bool(tr["term"][t]) and bool(trunc[0].item()) == bool(tr["trunc"][t]), t
        assert vec.reset_pending()[0].item() == int(tr["term"][t] or tr["trunc"][t]), t
    assert bool(trunc[0].item())
    assert np.array_equal(o[0].cpu().numpy(), frames[180][1]["rgb"])
    st = vec.engine.get_state()
    assert np.abs(st["agent_pos"][0] - tr["pos"][-1]).max() < 1e-12 and int(st["step_count"][0]) == 180
    act[:] = 2
    o, rew, term, trunc = vec.step(act)
    assert rew[0].item() == 0 and not term[0].item() and not trunc[0].item() and not vec.reset_pending()[0].item()
    h = envs.OneRoom(host_only=True)
    h.reset(seed=7)
    h.reset()
    _assert_same_world(vec, vec.engine.get_state(), 0, h, "reset step")
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("env_id,cls_name", [("MiniWorld-Hallway-v0", "Hallway"), ("MiniWorld-TMaze-v0", "TMaze")])
def test_terminal_frame_equals_the_oracle_render_of_the_terminal_state(env_id, cls_name, monkeypatch):
    """Families without a stored terminal frame: every terminal frame (and depth map) equals the CPU oracle's render of the
    terminal state the device holds between the two steps."""
    import pyoracle
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    _short_episodes(monkeypatch, cls_name, 4)
    n = 8
    vec = MiniWorldVecEnv(env_id, n, seed=60, want_depth=True, autoreset="next_step")
    vec.reset()
    g = torch.Generator(device="cuda").manual_seed(1)
    checked = 0
    for t in range(10):
        o, _, term, trunc = vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
        done = (term | trunc).bool().cpu().numpy()
        if done.any():
            st = vec.engine.get_state()
            for i in np.nonzero(done)[0]:
                want = pyoracle.render(helpers.scene_of_vec_env(vec, st, i))
                assert np.array_equal(o[i].cpu().numpy(), want["rgb"]), (env_id, t, i)
                assert np.array_equal(vec.depth[i].cpu().numpy(), want["depth"]), (env_id, t, i)
                checked += 1
    assert checked >= n
    vec.engine.check()
    vec.close()


def test_abi_edges_of_the_pending_flag(monkeypatch):
    """mw_render between the two steps draws the terminal state; mw_reset and mw_set_state drop a pending reset (the env's next
    step is an ordinary one); mw_get_reset_pending follows term | trunc."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    _short_episodes(monkeypatch, "Hallway", 1)      # every step ends the episode
    n = 6
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, seed=8, want_depth=True, autoreset="next_step")
    vec.reset()
    assert not vec.reset_pending().any()
    act = torch.full((n,), 2, dtype=torch.int32, device="cuda")
    o, _, term, trunc = vec.step(act)
    assert (term | trunc).all() and vec.reset_pending().all()
    terminal, terminal_depth, st_terminal = o.clone(), vec.depth.clone(), vec.engine.get_state()
    out, depth = torch.zeros_like(o), torch.zeros_like(vec.depth)
    vec.engine.render(out, depth)
    assert torch.equal(out, terminal) and torch.equal(depth, terminal_depth)
    assert vec.reset_pending().all()            # rendering and reading the state leave it pending
    # mw_reset of env 0, mw_set_state of env 1 (its terminal state written back): their next step is a step, the others reset
    mask = np.zeros(n, np.uint8)
    mask[0] = 1
    vec.engine.reset(mask, None)
    vec.engine.set_state({k: v[1:2] for k, v in st_terminal.items()}, first=1, count=1)
    assert vec.reset_pending().cpu().numpy().tolist() == [0, 0] + [1] * (n - 2)
    st_before = vec.engine.get_state()
    o, rew, term, trunc = vec.step(act)
    assert bool(trunc[0].item()) and bool(trunc[1].item()) and int(vec.engine.get_state()["step_count"][1]) == 2
    assert not (term | trunc)[2:].any() and not rew[2:].any()
    st = vec.engine.get_state()
    assert (st["step_count"][2:] == 0).all() and (st_before["step_count"][2:] == 1).all()
    assert vec.reset_pending().cpu().numpy().tolist() == [1, 1] + [0] * (n - 2)
    vec.engine.check()
    vec.close()


def test_vector_env_adapter_next_step():
    """MiniWorldVectorEnv(autoreset_mode="next-step"): the instance's metadata, the 5-tuple whose terminal step carries the terminal
    frame and the finished episode's own info (CollectHealth's health <= 0), no final-info keys, and the reset step after it."""
    from miniworld_amd import envs as host_envs
    from miniworld_amd.gymshim import AUTORESET_NEXT_STEP, AUTORESET_SAME_STEP
    from miniworld_amd.vector import MiniWorldVectorEnv
    n = 3
    envs = MiniWorldVectorEnv("MiniWorld-CollectHealth-v0", n, to_numpy=True, seed=21, autoreset_mode="next-step")
    assert envs.metadata["autoreset_mode"] == AUTORESET_NEXT_STEP and MiniWorldVectorEnv.metadata["autoreset_mode"] == AUTORESET_SAME_STEP
    envs.reset(seed=21)
    hosts = []
    for i in range(n):
        h = host_envs.CollectHealth()
        h.reset(seed=21 + i)
        hosts.append(h)
    for t in range(50):                         # turning on the spot: the health runs out on step 50
        a = np.full(n, t % 2, np.int64)
        obs, rew, term, trunc, infos = envs.step(a)
        assert set(infos) == {"health"}
        for i, h in enumerate(hosts):
            hobs, hrew, hterm, htrunc, hi = h.step(int(a[i]))
            assert bool(term[i]) == hterm and bool(trunc[i]) == htrunc and rew[i] == np.float32(hrew), (t, i)
            assert int(infos["health"][i]) == int(hi["health"]), (t, i)
            assert np.array_equal(obs[i], hobs), (t, i)         # the host class renders through the same engine
    assert term.all() and (infos["health"] <= 0).all()
    obs, rew, term, trunc, infos = envs.step(np.full(n, 2, np.int64))
    assert set(infos) == {"health"} and (infos["health"] == 100).all()
    assert not term.any() and not trunc.any() and not rew.any()
    for h in hosts:
        h.close()
    envs.close()


def test_vector_env_adapter_next_step_tmaze_goal_pos(monkeypatch):
    """TMaze's info["goal_pos"] on the step that ends an episode is that episode's box (tmaze.py:89), against the env class's own
    episodes continuing the stream with reset()."""
    from miniworld_amd import envs as host_envs
    from miniworld_amd.vector import MiniWorldVectorEnv
    n = 4
    _short_episodes(monkeypatch, "TMaze", 2)
    envs = MiniWorldVectorEnv("MiniWorld-TMaze-v0", n, to_numpy=True, seed=33, autoreset_mode="next-step")
    envs.reset(seed=33)
    hosts = []
    for i in range(n):
        h = host_envs.TMaze(host_only=True)
        h.reset(seed=33 + i)
        hosts.append(h)
    for episode in range(3):
        for k in range(2):
            _, _, term, trunc, infos = envs.step(np.zeros(n, np.int64))
            assert set(infos) == {"goal_pos"} and bool(trunc.all()) == (k == 1)
        for i, h in enumerate(hosts):
            assert np.array_equal(infos["goal_pos"][i], np.asarray(h.box.pos, np.float64)), (episode, i)
            h.reset()
        _, rew, term, trunc, infos = envs.step(np.full(n, 2, np.int64))       # the reset step: ignored action, the next box
        assert not (term | trunc).any() and not rew.any()
        for i, h in enumerate(hosts):
            assert np.array_equal(infos["goal_pos"][i], np.asarray(h.box.pos, np.float64)), (episode, i)
    envs.close()
