"""Action repeat (mw_step_repeat; MiniWorldVecEnv.step(actions, repeat=K)): up to K env steps per call in one step-kernel launch,
one frame at the end.

The yardstick is never the repeat kernel.  It is the reference's own loop through the plain kernels, the scheme of
tests/test_gpu_autoreset_next_step.py: a second engine C without auto-reset is stepped with single mw_steps, and its host calls
mw_reset(mask, seeds=NULL) + mw_render when an episode ends.  C runs first; every env walks its own list of actions, holding each
one for up to K ticks or until its episode ends, and closes a record per held action: the frame (and depth) at the call's end —
after the reset in same-step mode —, the reward sum float32(sum of the float32 per-step rewards), the last tick's flags, the
ticks it took and the device state.  Engine B then makes step(repeat=K) calls and its j-th call of env i must equal C's j-th
record of env i bit for bit.  In next-step mode C's list gets one more record per finished episode (the reset: reward 0, no
flags, 0 sub-steps, the new world's frame), and B is fed a different action on those calls."""
import ctypes as C_

import numpy as np
import pytest

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


def _actions(rng, n, count, n_actions, p_fwd):
    if p_fwd is None:
        return rng.integers(0, n_actions, (n, count))
    return np.where(rng.random((n, count)) < p_fwd, 2, rng.integers(0, n_actions, (n, count)))


def _reward_sum(rewards):
    """float32(sum of the float32 per-step rewards), the sum in double and in order"""
    s = 0.0
    for r in rewards:
        s += float(r)
    return np.float32(s)


def _reference_records(env_id, n, K, ticks, seed, actions, mode, want_depth, kw):
    """Engine C (no auto-reset, single mw_steps, host resets): the records of every env's completed calls."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    Cv = MiniWorldVecEnv(env_id, n, autoreset=False, seed=seed, want_depth=want_depth, **kw)
    assert Cv.autoreset_mode == "off"
    Cv.reset()
    rbuf, dbuf = torch.zeros_like(Cv.obs), (torch.zeros_like(Cv.depth) if want_depth else None)
    recs = [[] for _ in range(n)]
    call = np.zeros(n, np.int64)            # the env's current call: index into its action list
    sub = np.zeros(n, np.int64)             # ticks of that call so far
    rew = [[] for _ in range(n)]
    clean = np.ones(n, bool)
    env_ix = np.arange(n)
    for _ in range(ticks):
        o, r, te, tr = Cv.step(torch.as_tensor(actions[env_ix, call], dtype=torch.int32, device="cuda"))
        o, d = o.cpu().numpy(), (Cv.depth.cpu().numpy() if want_depth else None)
        r, te, tr = r.cpu().numpy(), te.cpu().numpy(), tr.cpu().numpy()
        st, info = Cv.engine.get_state(), {k: v.cpu().numpy() for k, v in Cv.infos().items()}
        clean &= Cv.frame_clean().cpu().numpy().astype(bool)
        sub += 1
        done = (te | tr).astype(bool)
        if done.any():
            Cv.engine.reset(done.astype(np.uint8), None)
            Cv.engine.render(rbuf, dbuf)
            ro, rd = rbuf.cpu().numpy(), (dbuf.cpu().numpy() if want_depth else None)
            rst, rinfo = Cv.engine.get_state(), {k: v.cpu().numpy() for k, v in Cv.infos().items()}
        for i in range(n):
            rew[i].append(r[i])
            if not done[i] and sub[i] < K:
                continue
            # the call ends here.  Same-step: what it returns of a finished env is the new world's; a world was installed, so
            # the frame is never clean (C, without auto-reset, cannot know that)
            new_world = done[i] and mode == "same_step"
            recs[i].append(dict(
                action=call[i], rgb=(ro if new_world else o)[i], depth=None if d is None else (rd if new_world else d)[i],
                reward=_reward_sum(rew[i]), term=te[i], trunc=tr[i], nsteps=int(sub[i]), state=_rows(rst if new_world else st, i),
                info={k: v[i] for k, v in (rinfo if new_world else info).items()}, clean=bool(clean[i]) and not new_world,
                done=bool(done[i]), terminal_rgb=o[i], terminal_depth=None if d is None else d[i]))
            if done[i] and mode == "next_step":
                recs[i].append(dict(
                    action=None, rgb=ro[i], depth=None if rd is None else rd[i], reward=np.float32(0), term=0, trunc=0, nsteps=0,
                    state=_rows(rst, i), info={k: v[i] for k, v in rinfo.items()}, clean=False, done=False))
            call[i] += 1
            sub[i] = 0
            rew[i] = []
            clean[i] = True
    Cv.engine.check()
    Cv.close()
    return recs


def _repeat_parity(env_id, n, K, ticks, seed, n_actions, mode="same_step", want_depth=False, p_fwd=None, final_obs=False,
                   frame_reuse=True, check_clean=False, **kw):
    """B's step(repeat=K) calls against C's records; returns B's per-call substeps [calls][n], done flags and clean bytes."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    rng = np.random.default_rng(seed)
    actions = _actions(rng, n, ticks + 1, n_actions, p_fwd)
    recs = _reference_records(env_id, n, K, ticks, seed, actions, mode, want_depth, kw)
    calls = min(len(r) for r in recs)
    assert calls >= 2, calls
    B = MiniWorldVecEnv(env_id, n, autoreset=mode, seed=seed, want_depth=want_depth, final_obs=final_obs, frame_reuse=frame_reuse, **kw)
    assert B.frame_reuse == frame_reuse
    B.reset()
    subs, dones, cleans = [], [], []
    for j in range(calls):
        rec = [recs[i][j] for i in range(n)]
        # (a reset call of next-step mode ignores its action: B gets one C never saw there)
        act = np.array([int(actions[i, c["action"]]) if c["action"] is not None else int(rng.integers(0, n_actions)) for i, c in enumerate(rec)])
        if mode == "next_step":
            pend = B.reset_pending().cpu().numpy().astype(bool)
            assert np.array_equal(pend, np.array([c["action"] is None for c in rec])), (env_id, j)
        o, r, te, tr = B.step(torch.as_tensor(act, dtype=torch.int32, device="cuda"), repeat=K)
        o, d = o.cpu().numpy(), (B.depth.cpu().numpy() if want_depth else None)
        r, te, tr, ns = r.cpu().numpy(), te.cpu().numpy(), tr.cpu().numpy(), B.substeps.cpu().numpy()
        st, info = B.engine.get_state(), {k: v.cpu().numpy() for k, v in B.infos().items()}
        cl = B.frame_clean().cpu().numpy()
        fo = B.final_obs.cpu().numpy() if final_obs else None
        fd = B.final_depth.cpu().numpy() if final_obs and want_depth else None
        for i, c in enumerate(rec):
            tag = (env_id, "call", j, "env", i, "nsteps", c["nsteps"])
            assert ns[i] == c["nsteps"], tag + ("substeps", ns[i])
            assert r[i] == c["reward"] and te[i] == c["term"] and tr[i] == c["trunc"], tag + ("reward / flags", r[i], te[i], tr[i], c["reward"], c["term"], c["trunc"])
            assert _same_state(_rows(st, i), c["state"]), tag + ("state",)
            assert np.array_equal(o[i], c["rgb"]), tag + ("rgb",)
            if want_depth:
                assert np.array_equal(d[i], c["depth"]), tag + ("depth",)
            assert info.keys() == c["info"].keys() and all(np.array_equal(info[k][i], c["info"][k]) for k in info), tag + ("info",)
            if check_clean:
                assert bool(cl[i]) == c["clean"], tag + ("frame_clean", cl[i])
            if final_obs and c["done"]:
                assert np.array_equal(fo[i], c["terminal_rgb"]), tag + ("final_obs",)
                if want_depth:
                    assert np.array_equal(fd[i], c["terminal_depth"]), tag + ("final_depth",)
        subs.append(ns.copy())
        dones.append((te | tr).astype(bool))
        cleans.append(cl.astype(bool))
    B.engine.check()
    B.close()
    return np.array(subs), np.array(dones), np.array(cleans)


@pytest.mark.parametrize("spare,K,depth", [("0", 4, False), ("1", 4, False), ("1", 2, True)])
def test_hallway_dense_same_step(spare, K, depth, monkeypatch):
    """The dense K1, 43 envs: five per wavefront and a ragged last one, whose envs stop at different sub-steps; without and with
    spare worlds.  Episodes of 7 steps: at K = 4 truncation lands on sub-step 3 of every second call."""
    monkeypatch.setenv("MW_SPARE", spare)
    _short_episodes(monkeypatch, "Hallway", 7)
    subs, dones, _ = _repeat_parity("MiniWorld-Hallway-v0", 43, K, 30, 900, 3, want_depth=depth, p_fwd=0.6)
    assert dones.sum() >= 43
    if K == 4:
        assert ((subs > 1) & (subs < K)).any()


@pytest.mark.parametrize("spare", ["0", "1"])
def test_hallway_dense_philox(spare, monkeypatch):
    """The dense repeat kernel of the Philox stream (every other case here runs the PCG64 kernels), 7 envs: a full wavefront of five
    and a ragged one of two.  Episodes of 7 steps at K = 4: truncation and the install, with its draws, land on sub-step 3 of every
    second call."""
    monkeypatch.setenv("MW_SPARE", spare)
    _short_episodes(monkeypatch, "Hallway", 7)
    subs, dones, _ = _repeat_parity("MiniWorld-Hallway-v0", 7, 4, 20, 902, 3, p_fwd=0.6, rng="philox")
    assert dones.sum() >= 7
    assert ((subs > 1) & (subs < 4)).any()


def test_maze_wave_per_env_philox(monkeypatch):
    """The wave-per-env repeat kernel of the Philox stream: MazeS3, 3 envs, episodes of 6 steps at K = 4 — every second call ends on
    sub-step 2 and installs a world.  Without spare worlds: the kernel generates the maze itself, from its own stream's draws (with
    them a finished env takes a world the refill kernel made, and this kernel draws nothing)."""
    monkeypatch.setenv("MW_SPARE", "0")
    subs, dones, _ = _repeat_parity("MiniWorld-MazeS3-v0", 3, 4, 18, 78, 3, max_episode_steps=6, rng="philox")
    assert dones.sum() >= 6
    assert ((subs > 1) & (subs < 4)).any()


def test_oneroom_dense_next_step(monkeypatch):
    """Next-step mode, K = 3 on episodes of 2 steps: every real call ends on sub-step 2, every other call is a reset call that
    executes nothing."""
    _short_episodes(monkeypatch, "OneRoom", 2)
    subs, dones, _ = _repeat_parity("MiniWorld-OneRoom-v0", 40, 3, 16, 901, 3, mode="next_step", p_fwd=0.6)
    assert len(subs) >= 8
    # (sub-step 2 truncates; an agent that starts beside the box terminates on sub-step 1)
    assert (subs[0::2] <= 2).all() and (subs[0::2] >= 1).all() and (subs[0::2] == 2).mean() > 0.9 and dones[0::2].all()
    assert (subs[1::2] == 0).all() and not dones[1::2].any()


def test_pickup_objects_domain_rand(monkeypatch):
    """The wave-per-env K1 with meshes and domain randomisation: three draws per executed sub-step, picked objects leave the
    list between sub-steps."""
    _short_episodes(monkeypatch, "PickupObjects", 8)
    subs, dones, _ = _repeat_parity("MiniWorld-PickupObjects-v0", 16, 3, 24, 31, 5, domain_rand=True)
    assert dones.sum() >= 16


def _pair(env_id, n, seed, mode="same_step", **kw):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    B = MiniWorldVecEnv(env_id, n, autoreset=mode, seed=seed, **kw)
    Cv = MiniWorldVecEnv(env_id, n, autoreset=False, seed=seed, **kw)
    B.reset()
    Cv.reset()
    return B, Cv


def test_a_repeated_pickup_picks_the_object_once():
    """PickupObjects, directed: env 0's agent faces its object 0 at pickup distance and every other object of that env is out of
    the list.  Action 4 held for 3 sub-steps picks it up on the first, and the object leaves the list before the second
    (pickupobjects.py:86-88): reward 1, not 2 or 3."""
    import torch
    n, K = 2, 3
    B, Cv = _pair("MiniWorld-PickupObjects-v0", n, 5, domain_rand=True)
    st = Cv.engine.get_state()
    assert _same_state(st, B.engine.get_state())
    r_agent = float(Cv.template.agent.radius)
    assert st["ent_kind"][0, 0] != 0
    st["ent_kind"][0, 1:] = 0
    # the object in the middle of the room, the agent facing it (+x, dir 0) with the object's centre 0.05 m beyond touching: the
    # pickup probe (1.5 radii ahead, 1.2 radii wide) reaches it and no wall
    ext = st["extent"][0]
    st["ent_pos"][0, 0, 0], st["ent_pos"][0, 0, 2] = 0.5 * (ext[0] + ext[1]), 0.5 * (ext[2] + ext[3])
    st["agent_pos"][0] = st["ent_pos"][0, 0] - np.array([r_agent + st["ent_geom"][0, 0, 7] + 0.05, 0.0, 0.0])
    st["agent_pos"][0, 1] = 0.0
    st["agent_dir"][0] = 0.0
    for v in (B, Cv):
        v.engine.set_state(st)
    act = torch.full((n,), 4, dtype=torch.int32, device="cuda")
    picked0 = int(st["num_picked_up"][0])
    rewards, frames = [], []
    for _ in range(K):
        o, r, te, tr = Cv.step(act)
        rewards.append(r.cpu().numpy().copy())
        assert not (te | tr)[0].item()
    rewards = np.array(rewards)
    cst = Cv.engine.get_state()
    # C: the event is the one meant
    assert rewards[:, 0].tolist() == [1.0, 0.0, 0.0], rewards[:, 0]
    assert int(cst["num_picked_up"][0]) == picked0 + 1 and cst["ent_kind"][0, 0] == 0 and cst["carrying"][0] == -1
    o, r, te, tr = B.step(act, repeat=K)
    bst = B.engine.get_state()
    assert r[0].item() == 1.0 and B.substeps.cpu().numpy().tolist() == [K] * n
    assert int(bst["num_picked_up"][0]) == picked0 + 1 and bst["ent_kind"][0, 0] == 0
    assert np.array_equal(r.cpu().numpy(), np.array([_reward_sum(rewards[:, i]) for i in range(n)]))
    assert _same_state(bst, cst)
    assert torch.equal(o, Cv.obs)
    for v in (B, Cv):
        v.engine.check()
        v.close()


def test_collect_health(monkeypatch):
    """MW_TASK_COLLECT: health bookkeeping per sub-step, consumed kits respawn inside the call with their stream draws.  In
    next-step mode, whose stream order is C's own: a same-step engine drops the respawn of a kit consumed on the step that ends
    the episode (mw_step does: the world is replaced), where C's terminal step draws it before the reset."""
    _short_episodes(monkeypatch, "CollectHealth", 7)
    subs, dones, _ = _repeat_parity("MiniWorld-CollectHealth-v0", 12, 3, 30, 13, 8, mode="next_step", p_fwd=0.3)
    assert dones.sum() >= 12


def test_a_kit_is_consumed_and_respawns_inside_the_call():
    """CollectHealth, directed: an agent next to a kit holds action 4 for 3 sub-steps.  Sub-step 1 picks the kit up and, in the
    same step, consumes it (collecthealth.py:82-91: `if action == pickup: if carrying:` runs behind MiniWorldEnv.step's pickup;
    health 100); the respawn — the entity list closes up, the kit re-enters at its end with place_entity's draws — runs inside
    the call, before sub-step 2, and sub-steps 2 and 3 see the new list."""
    import torch
    n, K = 12, 3
    B, Cv = _pair("MiniWorld-CollectHealth-v0", n, 13)
    st = Cv.engine.get_state()
    r_agent = float(Cv.template.agent.radius)
    # the kit with the most room around it: walls and the other entities out of the pickup probe's reach (1.2 radii around a
    # point 1.5 radii ahead of the agent, at most half a radius from the kit's centre)
    best = None
    for i in range(n):
        for s in range(int((st["ent_kind"][i] != 0).sum()) - 1):        # (not the last one: the list has to close up behind it)
            if st["ent_kind"][i, s] == 0 or st["ent_static"][i, s]:
                continue
            p = st["ent_pos"][i, s]
            ext = st["extent"][i]
            room = min(p[0] - ext[0], ext[1] - p[0], p[2] - ext[2], ext[3] - p[2])
            others = [np.hypot(*(st["ent_pos"][i, t, [0, 2]] - p[[0, 2]])) - st["ent_geom"][i, t, 7]
                      for t in range(st["ent_kind"].shape[1]) if t != s and st["ent_kind"][i, t] != 0]
            c = min([room] + others)
            if best is None or c > best[0]:
                best = (c, i, s)
    clear, i, s = best
    assert clear > 1.7 * r_agent + 0.1, best
    st["agent_pos"][i] = st["ent_pos"][i, s] - np.array([r_agent + st["ent_geom"][i, s, 7] + 0.05, 0.0, 0.0])
    st["agent_pos"][i, 1] = 0.0
    st["agent_dir"][i] = 0.0
    for v in (B, Cv):
        v.engine.set_state(st)
    act = torch.full((n,), 4, dtype=torch.int32, device="cuda")
    rewards = []
    Cv.step(act)
    rewards.append(Cv.reward.cpu().numpy().copy())
    # C: the event is the one meant — tick 1 consumed the kit, and the respawn ran behind its frame: the slots behind the kit
    # moved down by one, the kit took the last one at a new place
    c1 = Cv.engine.get_state()
    assert c1["carrying"][i] == -1 and int(Cv.infos()["health"][i].item()) == 100 and rewards[0][i] == 2.0
    last = int((st["ent_kind"][i] != 0).sum()) - 1
    assert s < last, (s, last)
    assert np.array_equal(c1["ent_pos"][i, s:last], st["ent_pos"][i, s + 1:last + 1])
    assert not np.array_equal(c1["ent_pos"][i, last], st["ent_pos"][i, last]) and not np.array_equal(c1["ent_pos"][i, last], st["ent_pos"][i, s])
    for _ in range(K - 1):
        Cv.step(act)
        rewards.append(Cv.reward.cpu().numpy().copy())
    cst = Cv.engine.get_state()
    o, r, te, tr = B.step(act, repeat=K)
    rewards = np.array(rewards)
    assert B.substeps.cpu().numpy().tolist() == [K] * n
    assert np.array_equal(r.cpu().numpy(), np.array([_reward_sum(rewards[:, e]) for e in range(n)]))
    assert _same_state(B.engine.get_state(), cst)
    assert torch.equal(B.infos()["health"], Cv.infos()["health"])
    assert torch.equal(o, Cv.obs)
    for v in (B, Cv):
        v.engine.check()
        v.close()


def test_maze_side_stream_refills():
    """MazeS3 with episodes of 5 steps: the spare worlds' refills run on the side stream across calls, and an env may need a
    spare whose refill is still running or has not started (the wait and inline branches of the refill_mask protocol)."""
    subs, dones, _ = _repeat_parity("MiniWorld-MazeS3-v0", 12, 2, 22, 77, 3, max_episode_steps=5)
    assert dones.sum() >= 24


def test_placement_program_with_program_rules(monkeypatch):
    """Sidewalk: a placement-program family whose env rule lives in the program's tables, with domain randomisation."""
    _short_episodes(monkeypatch, "Sidewalk", 3)
    subs, dones, _ = _repeat_parity("MiniWorld-Sidewalk-v0", 16, 2, 16, 5, 3, domain_rand=True, want_depth=True)
    assert dones.sum() >= 32


def test_final_observations(monkeypatch):
    """final_obs=True: the call takes mw_step's two passes; the finished envs' rows of final_obs hold C's terminal frames, obs
    the new worlds' first frames."""
    _short_episodes(monkeypatch, "Hallway", 5)
    subs, dones, _ = _repeat_parity("MiniWorld-Hallway-v0", 24, 3, 22, 40, 3, final_obs=True, want_depth=True, p_fwd=0.6)
    assert dones.sum() >= 24


def test_frame_reuse_and_the_clean_byte():
    """Frame reuse on: a repeat call is a plain step of the whole batch for the held-frame logic, and the clean byte is the AND
    of the sub-steps' (0 where a world was installed, which C — without auto-reset — does not know).  Forward moves two times in
    three, so that walls block: an env that is blocked on a call's first sub-step is blocked on all of them."""
    subs, dones, cleans = _repeat_parity("MiniWorld-Hallway-v0", 64, 3, 60, 7, 3, p_fwd=0.66, frame_reuse=True, check_clean=True)
    assert cleans.any()


@pytest.mark.parametrize("env_id,n_actions,kw", [("MiniWorld-Hallway-v0", 3, {}), ("MiniWorld-PickupObjects-v0", 5, {"domain_rand": True})])
@pytest.mark.parametrize("mode", [False, "same_step", "next_step"])
def test_repeat_one_equals_mw_step(env_id, n_actions, kw, mode, monkeypatch):
    """mw_step_repeat with repeat = 1 (the repeat kernels) against mw_step (the plain ones): everything bit for bit."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    _short_episodes(monkeypatch, env_id.split("-")[1], 6)
    n = 23
    A = MiniWorldVecEnv(env_id, n, autoreset=mode, seed=3, want_depth=True, **kw)
    B = MiniWorldVecEnv(env_id, n, autoreset=mode, seed=3, want_depth=True, **kw)
    A.reset()
    B.reset()
    ns = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(2)
    for t in range(20):
        act = torch.randint(0, n_actions, (n,), generator=g, device="cuda", dtype=torch.int32)
        pend = A.reset_pending().cpu().numpy()
        A.step(act)
        B.engine.step_repeat(act, 1, B.obs, B.depth, B.reward, B.terminated, B.truncated, ns)
        assert torch.equal(A.obs, B.obs) and torch.equal(A.depth, B.depth), (t, "frame")
        assert torch.equal(A.reward, B.reward) and torch.equal(A.terminated, B.terminated) and torch.equal(A.truncated, B.truncated), t
        assert _same_state(A.engine.get_state(), B.engine.get_state()), t
        assert torch.equal(A.reset_pending(), B.reset_pending()) and torch.equal(A.frame_clean(), B.frame_clean()), t
        assert np.array_equal(ns.cpu().numpy(), 1 - pend.astype(np.int32)), t
    for v in (A, B):
        v.engine.check()
        v.close()


def test_errors_and_no_autoreset(monkeypatch):
    """A repeat outside 1 .. MW_MAX_REPEAT through the raw library call is MW_E_INVALID and touches nothing; without auto-reset an
    env that finishes on sub-step j < K reports j and keeps its terminal state."""
    import torch
    from miniworld_amd import engine as eng
    from miniworld_amd.vec_env import MiniWorldVecEnv
    _short_episodes(monkeypatch, "Hallway", 2)
    n, K = 7, 5
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, autoreset=False, seed=11)
    vec.reset()
    before = vec.engine.get_state()
    obs0 = vec.obs.clone()
    act = torch.zeros(n, dtype=torch.int32, device="cuda")
    ns = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ptr = lambda t: C_.c_void_p(t.data_ptr())
    for bad in (0, 257):
        rc = vec.engine.lib.mw_step_repeat(vec.engine.h, ptr(act), bad, ptr(vec.obs), None, ptr(vec.reward), ptr(vec.terminated),
                                           ptr(vec.truncated), ptr(ns), eng._stream_ptr(vec.engine.device))
        assert rc == -1 and b"repeat" in vec.engine.lib.mw_last_error(vec.engine.h)
        torch.cuda.synchronize()
        assert _same_state(vec.engine.get_state(), before) and torch.equal(vec.obs, obs0) and (ns == -1).all()
    o, r, te, tr = vec.step(act, repeat=K)
    st = vec.engine.get_state()
    assert vec.substeps.cpu().numpy().tolist() == [2] * n and tr.all() and not te.any()
    assert (st["step_count"] == 2).all() and not vec.reset_pending().any()
    # the terminal state: two turns from where the episode began, nothing installed
    ref = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, autoreset=False, seed=11)
    ref.reset()
    ref.step(act)
    ref.step(act)
    assert _same_state(st, ref.engine.get_state()) and torch.equal(o, ref.obs)
    for v in (vec, ref):
        v.engine.check()
        v.close()
