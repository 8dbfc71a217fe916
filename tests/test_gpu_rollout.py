"""Open-loop rollouts (mw_step_plan; MiniWorldVecEnv.rollout(plans, render)): up to T env steps per call in one step-kernel launch,
one action per step, and one frame at the end (render=True) or none (render=False, the frameless call).

The yardstick is never the plan kernel.  It is the scheme of tests/test_gpu_action_repeat.py: a second engine C without auto-reset
is stepped with single mw_steps, and its host calls mw_reset(mask, seeds=NULL) + mw_render when an episode ends.  C runs first; every
env walks its own list of plans, one action per tick, and closes a record per plan: the frame (and depth) at the call's end — after
the reset in same-step mode —, what mw_render draws of C's state right after the call's last tick (the frame's tail applied: a
picked-up object gone), the reward sum float32(sum of the float32 per-step rewards), the per-tick rewards, the last tick's flags,
the ticks it took, the device state and the infos.  Engine B then makes rollout() calls, alternating drawn and frameless ones with
frame reuse and the frame cache at their defaults, and its j-th call of env i must equal C's j-th record of env i bit for bit: the
frame for a drawn call, engine.render behind the call for a frameless one.  In next-step mode C's list gets one more record per
finished episode (the reset: reward 0, no flags, 0 sub-steps, the new world's frame), and B is fed a plan C never saw there."""
import ctypes as C_

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _short_episodes(monkeypatch, cls_name, steps):
    """Episodes of at most `steps` steps for a family whose class fixes max_episode_steps: the batched env reads it from its
    template instance."""
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


def _plans(rng, n, count, T, n_actions, p_fwd):
    """[n][count][T]: env i's list of plans"""
    if p_fwd is None:
        return rng.integers(0, n_actions, (n, count, T))
    return np.where(rng.random((n, count, T)) < p_fwd, 2, rng.integers(0, n_actions, (n, count, T)))


def _reward_sum(rewards):
    """float32(sum of the float32 per-step rewards), the sum in double and in order"""
    s = 0.0
    for r in rewards:
        s += float(r)
    return np.float32(s)


def _drawn(j):
    """B's j-th call draws a frame: D F F D D F F D ... — both kinds meet both halves of every period-2 pattern of calls"""
    return j % 4 in (0, 3)


def _reference_records(env_id, n, T, ticks, seed, plans, mode, want_depth, kw):
    """Engine C (no auto-reset, single mw_steps, host resets): the records of every env's completed calls."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    Cv = MiniWorldVecEnv(env_id, n, autoreset=False, seed=seed, want_depth=want_depth, **kw)
    assert Cv.autoreset_mode == "off"
    Cv.reset()
    zeros = lambda: (torch.zeros_like(Cv.obs), torch.zeros_like(Cv.depth) if want_depth else None)
    (rbuf, rdbuf), (pbuf, pdbuf) = zeros(), zeros()
    recs = [[] for _ in range(n)]
    call = np.zeros(n, np.int64)            # the env's current call: index into its list of plans
    sub = np.zeros(n, np.int64)             # ticks of that call so far
    rew = [[] for _ in range(n)]
    env_ix = np.arange(n)
    host = lambda t: None if t is None else t.cpu().numpy()
    for _ in range(ticks):
        o, r, te, tr = Cv.step(torch.as_tensor(plans[env_ix, call, sub], dtype=torch.int32, device="cuda"))
        o, d, r, te, tr = host(o), host(Cv.depth), host(r), host(te), host(tr)
        st, info = Cv.engine.get_state(), {k: host(v) for k, v in Cv.infos().items()}
        Cv.engine.render(pbuf, pdbuf)           # the state behind the tick, the frame's tail applied
        po, pd = host(pbuf), host(pdbuf)
        sub += 1
        done = (te | tr).astype(bool)
        if done.any():
            Cv.engine.reset(done.astype(np.uint8), None)
            Cv.engine.render(rbuf, rdbuf)
            ro, rd = host(rbuf), host(rdbuf)
            rst, rinfo = Cv.engine.get_state(), {k: host(v) for k, v in Cv.infos().items()}
        for i in range(n):
            rew[i].append(r[i])
            if not done[i] and sub[i] < T:
                continue
            # the call ends here.  Same-step: what it returns of a finished env is the new world's
            new_world = done[i] and mode == "same_step"
            pick = lambda new, old: None if old is None else (new if new_world else old)[i]
            recs[i].append(dict(
                plan=call[i], rgb=pick(ro if new_world else None, o), depth=pick(rd if new_world else None, d),
                render=pick(ro if new_world else None, po), render_depth=pick(rd if new_world else None, pd),
                reward=_reward_sum(rew[i]), step_rewards=np.array(rew[i] + [0.0] * (T - len(rew[i])), np.float32), term=te[i], trunc=tr[i],
                nsteps=int(sub[i]), state=_rows(rst if new_world else st, i), info={k: v[i] for k, v in (rinfo if new_world else info).items()},
                done=bool(done[i])))
            if done[i] and mode == "next_step":
                recs[i].append(dict(
                    plan=None, rgb=ro[i], depth=None if rd is None else rd[i], render=ro[i], render_depth=None if rd is None else rd[i],
                    reward=np.float32(0), step_rewards=np.zeros(T, np.float32), term=0, trunc=0, nsteps=0, state=_rows(rst, i),
                    info={k: v[i] for k, v in rinfo.items()}, done=False))
            call[i] += 1
            sub[i] = 0
            rew[i] = []
    Cv.engine.check()
    Cv.close()
    return recs


def _rollout_parity(env_id, n, T, ticks, seed, n_actions, mode="same_step", want_depth=False, p_fwd=None, **kw):
    """B's rollout() calls, drawn and frameless in turn, against C's records; returns B's per-call substeps [calls][n] and done flags."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    rng = np.random.default_rng(seed)
    plans = _plans(rng, n, ticks + 1, T, n_actions, p_fwd)
    recs = _reference_records(env_id, n, T, ticks, seed, plans, mode, want_depth, kw)
    calls = min(len(r) for r in recs)
    assert calls >= 4, calls
    B = MiniWorldVecEnv(env_id, n, autoreset=mode, seed=seed, want_depth=want_depth, **kw)
    # (frame reuse and the frame cache at their defaults, on: every drawn call also proves the frameless ones before it)
    B.reset()
    fbuf, fdbuf = torch.zeros_like(B.obs), (torch.zeros_like(B.depth) if want_depth else None)
    subs, dones = [], []
    host = lambda t: None if t is None else t.cpu().numpy()
    for j in range(calls):
        rec = [recs[i][j] for i in range(n)]
        # (a reset call of next-step mode ignores its plan: B gets one C never saw there)
        plan = np.stack([plans[i, c["plan"]] if c["plan"] is not None else rng.integers(0, n_actions, T) for i, c in enumerate(rec)], axis=1)
        if mode == "next_step":
            pend = B.reset_pending().cpu().numpy().astype(bool)
            assert np.array_equal(pend, np.array([c["plan"] is None for c in rec])), (env_id, j)
        drawn = _drawn(j)
        o, r, te, tr = B.rollout(torch.as_tensor(plan, dtype=torch.int32, device="cuda"), render=drawn)
        if drawn:
            assert o is B.obs
            o, d = host(o), host(B.depth)
        else:
            assert o is None and not B.frame_clean().any()
            B.engine.render(fbuf, fdbuf)
            o, d = host(fbuf), host(fdbuf)
        r, te, tr, ns, sr = host(r), host(te), host(tr), host(B.substeps), host(B.step_rewards)
        assert sr.shape == (T, n)
        st, info = B.engine.get_state(), {k: host(v) for k, v in B.infos().items()}
        for i, c in enumerate(rec):
            tag = (env_id, "call", j, "drawn" if drawn else "frameless", "env", i, "nsteps", c["nsteps"])
            assert ns[i] == c["nsteps"], tag + ("substeps", ns[i])
            assert r[i] == c["reward"] and te[i] == c["term"] and tr[i] == c["trunc"], tag + ("reward / flags", r[i], te[i], tr[i], c["reward"], c["term"], c["trunc"])
            assert np.array_equal(sr[:, i], c["step_rewards"]), tag + ("step_rewards", sr[:, i], c["step_rewards"])
            assert _same_state(_rows(st, i), c["state"]), tag + ("state",)
            assert np.array_equal(o[i], c["rgb" if drawn else "render"]), tag + ("rgb",)
            if want_depth:
                assert np.array_equal(d[i], c["depth" if drawn else "render_depth"]), tag + ("depth",)
            assert info.keys() == c["info"].keys() and all(np.array_equal(info[k][i], c["info"][k]) for k in info), tag + ("info",)
        subs.append(ns.copy())
        dones.append((te | tr).astype(bool))
    B.engine.check()
    B.close()
    return np.array(subs), np.array(dones)


@pytest.mark.parametrize("spare,depth", [("0", False), ("1", False), ("1", True)])
def test_hallway_dense_same_step(spare, depth, monkeypatch):
    """The dense K1, 43 envs: five per wavefront and a ragged last one, whose envs stop at different sub-steps; without and with
    spare worlds.  Episodes of 7 steps: at T = 4 truncation lands on sub-step 3 of every second call."""
    monkeypatch.setenv("MW_SPARE", spare)
    _short_episodes(monkeypatch, "Hallway", 7)
    subs, dones = _rollout_parity("MiniWorld-Hallway-v0", 43, 4, 30, 900, 3, want_depth=depth, p_fwd=0.6)
    assert dones.sum() >= 43
    assert ((subs > 1) & (subs < 4)).any()


@pytest.mark.parametrize("spare", ["0", "1"])
def test_hallway_dense_philox(spare, monkeypatch):
    """The dense plan kernel of the Philox stream (every other case here runs the PCG64 kernels), 7 envs: a full wavefront of five and
    a ragged one of two.  Episodes of 7 steps at T = 4: truncation and the install, with its draws, land on sub-step 3 of every
    second call, drawn or frameless."""
    monkeypatch.setenv("MW_SPARE", spare)
    _short_episodes(monkeypatch, "Hallway", 7)
    subs, dones = _rollout_parity("MiniWorld-Hallway-v0", 7, 4, 20, 902, 3, p_fwd=0.6, rng="philox")
    assert dones.sum() >= 7
    assert ((subs > 1) & (subs < 4)).any()


def test_maze_wave_per_env_philox(monkeypatch):
    """The wave-per-env plan kernel of the Philox stream: MazeS3, 3 envs, episodes of 6 steps at T = 4 — every second call ends on
    sub-step 2 and installs a world.  Without spare worlds: the kernel generates the maze itself, from its own stream's draws (with
    them a finished env takes a world the refill kernel made, and this kernel draws nothing)."""
    monkeypatch.setenv("MW_SPARE", "0")
    subs, dones = _rollout_parity("MiniWorld-MazeS3-v0", 3, 4, 18, 78, 3, max_episode_steps=6, rng="philox")
    assert dones.sum() >= 6
    assert ((subs > 1) & (subs < 4)).any()


def test_oneroom_dense_next_step(monkeypatch):
    """Next-step mode, T = 3 on episodes of 2 steps: every real call ends on sub-step 1 or 2, every other call is a reset call that
    executes nothing and returns an all-zero step_rewards column (compared in _rollout_parity)."""
    _short_episodes(monkeypatch, "OneRoom", 2)
    subs, dones = _rollout_parity("MiniWorld-OneRoom-v0", 40, 3, 16, 901, 3, mode="next_step", p_fwd=0.6)
    assert len(subs) >= 8
    assert (subs[0::2] <= 2).all() and (subs[0::2] >= 1).all() and dones[0::2].all()
    assert (subs[1::2] == 0).all() and not dones[1::2].any()


def test_pickup_objects_domain_rand(monkeypatch):
    """The wave-per-env K1 with meshes and domain randomisation: three draws per executed sub-step, picked objects leave the list
    between sub-steps and behind the last one of a frameless call."""
    _short_episodes(monkeypatch, "PickupObjects", 8)
    subs, dones = _rollout_parity("MiniWorld-PickupObjects-v0", 16, 3, 24, 31, 5, domain_rand=True)
    assert dones.sum() >= 16


def _pair(env_id, n, seed, mode="same_step", **kw):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    B = MiniWorldVecEnv(env_id, n, autoreset=mode, seed=seed, **kw)
    Cv = MiniWorldVecEnv(env_id, n, autoreset=False, seed=seed, **kw)
    B.reset()
    Cv.reset()
    return B, Cv


def _plan_tensor(rows, n):
    """[T, n]: every env takes the same actions"""
    import torch
    return torch.tensor(rows, dtype=torch.int32, device="cuda")[:, None].repeat(1, n).contiguous()


def test_a_pickup_on_the_last_sub_step_of_a_frameless_call():
    """PickupObjects, directed (the set-up of test_gpu_action_repeat.py's repeated pickup): env 0's agent faces its object 0 at
    pickup distance.  The plan [drop (nothing carried: no move), drop, pickup] picks it up on the LAST sub-step of a frameless call:
    the step kernel itself takes the object out of the list, as the geometry kernel of a drawn call would behind its frame."""
    import torch
    n, T = 2, 3
    B, Cv = _pair("MiniWorld-PickupObjects-v0", n, 5, domain_rand=True)
    st = Cv.engine.get_state()
    assert _same_state(st, B.engine.get_state())
    r_agent = float(Cv.template.agent.radius)
    assert st["ent_kind"][0, 0] != 0
    st["ent_kind"][0, 1:] = 0
    ext = st["extent"][0]
    st["ent_pos"][0, 0, 0], st["ent_pos"][0, 0, 2] = 0.5 * (ext[0] + ext[1]), 0.5 * (ext[2] + ext[3])
    st["agent_pos"][0] = st["ent_pos"][0, 0] - np.array([r_agent + st["ent_geom"][0, 0, 7] + 0.05, 0.0, 0.0])
    st["agent_pos"][0, 1] = 0.0
    st["agent_dir"][0] = 0.0
    for v in (B, Cv):
        v.engine.set_state(st)
    picked0 = int(st["num_picked_up"][0])
    plan = [5, 5, 4]
    rewards = []
    for a in plan:
        o, r, te, tr = Cv.step(torch.full((n,), a, dtype=torch.int32, device="cuda"))
        rewards.append(r.cpu().numpy().copy())
        assert not (te | tr)[0].item()
    rewards = np.array(rewards)
    last_frame = Cv.obs.clone()
    cst = Cv.engine.get_state()
    crender = torch.zeros_like(Cv.obs)
    Cv.engine.render(crender)
    # C: the event is the one meant — the last tick picked, its frame still shows the object, a render of the state does not
    assert rewards[:, 0].tolist() == [0.0, 0.0, 1.0], rewards[:, 0]
    assert int(cst["num_picked_up"][0]) == picked0 + 1 and cst["ent_kind"][0, 0] == 0 and cst["carrying"][0] == -1
    assert not torch.equal(crender[0], last_frame[0])
    o, r, te, tr = B.rollout(_plan_tensor(plan, n), render=False)
    bst = B.engine.get_state()
    assert o is None and r[0].item() == 1.0 and B.substeps.cpu().numpy().tolist() == [T] * n
    assert np.array_equal(B.step_rewards.cpu().numpy(), rewards)
    assert np.array_equal(r.cpu().numpy(), np.array([_reward_sum(rewards[:, i]) for i in range(n)]))
    assert int(bst["num_picked_up"][0]) == picked0 + 1 and bst["ent_kind"][0, 0] == 0
    assert _same_state(bst, cst)
    assert not B.frame_clean().any()
    brender = torch.zeros_like(B.obs)
    B.engine.render(brender)
    assert torch.equal(brender, crender)
    # the following drawn call
    o, r, te, tr = B.rollout(_plan_tensor([0], n))
    Cv.step(torch.zeros(n, dtype=torch.int32, device="cuda"))
    assert torch.equal(o, Cv.obs) and torch.equal(r, Cv.reward) and _same_state(B.engine.get_state(), Cv.engine.get_state())
    for v in (B, Cv):
        v.engine.check()
        v.close()


def test_collect_health(monkeypatch):
    """MW_TASK_COLLECT in next-step mode, whose stream order is C's own: health bookkeeping per sub-step, consumed kits respawn
    inside the call with their stream draws — behind the last sub-step of a frameless call too, a terminal one included."""
    _short_episodes(monkeypatch, "CollectHealth", 7)
    subs, dones = _rollout_parity("MiniWorld-CollectHealth-v0", 12, 3, 30, 13, 8, mode="next_step", p_fwd=0.3)
    assert dones.sum() >= 12


def test_a_kit_consumed_on_the_last_sub_step_of_a_frameless_call_respawns_inside_it():
    """CollectHealth, directed (the set-up of test_gpu_action_repeat.py's kit case): an agent next to a kit takes [drop, drop,
    pickup] in a frameless call.  The last sub-step picks the kit up and consumes it; the respawn, with place_entity's draws from
    the env's stream, runs inside the call: the state behind it and every later call equal C's."""
    import torch
    n, T = 12, 3
    B, Cv = _pair("MiniWorld-CollectHealth-v0", n, 13, mode="next_step")
    st = Cv.engine.get_state()
    r_agent = float(Cv.template.agent.radius)
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
    plan = [5, 5, 4]
    rewards = []
    for a in plan:
        Cv.step(torch.full((n,), a, dtype=torch.int32, device="cuda"))
        rewards.append(Cv.reward.cpu().numpy().copy())
        assert not (Cv.terminated | Cv.truncated).any()
    rewards = np.array(rewards)
    cst = Cv.engine.get_state()
    # C: the event is the one meant — the last tick consumed the kit, and the respawn ran behind its frame: the slots behind the
    # kit moved down by one, the kit took the last one at a new place
    last = int((st["ent_kind"][i] != 0).sum()) - 1
    assert cst["carrying"][i] == -1 and int(Cv.infos()["health"][i].item()) == 100
    assert np.array_equal(cst["ent_pos"][i, s:last], st["ent_pos"][i, s + 1:last + 1])
    assert not np.array_equal(cst["ent_pos"][i, last], st["ent_pos"][i, last]) and not np.array_equal(cst["ent_pos"][i, last], st["ent_pos"][i, s])
    crender = torch.zeros_like(Cv.obs)
    Cv.engine.render(crender)
    o, r, te, tr = B.rollout(_plan_tensor(plan, n), render=False)
    assert o is None and B.substeps.cpu().numpy().tolist() == [T] * n
    assert np.array_equal(B.step_rewards.cpu().numpy(), rewards)
    assert np.array_equal(r.cpu().numpy(), np.array([_reward_sum(rewards[:, e]) for e in range(n)]))
    assert _same_state(B.engine.get_state(), cst)
    assert torch.equal(B.infos()["health"], Cv.infos()["health"])
    brender = torch.zeros_like(B.obs)
    B.engine.render(brender)
    assert torch.equal(brender, crender)
    g = torch.Generator(device="cuda").manual_seed(4)
    for t in range(3):      # later calls: the stream behind the respawn's draws is C's
        act = torch.randint(0, 4, (n,), generator=g, device="cuda", dtype=torch.int32)
        o, r, te, tr = B.rollout(act[None, :], render=t != 1)
        Cv.step(act)
        assert not (Cv.terminated | Cv.truncated).any()
        if o is not None:
            assert torch.equal(o, Cv.obs), t
        assert torch.equal(r, Cv.reward) and _same_state(B.engine.get_state(), Cv.engine.get_state()), t
    for v in (B, Cv):
        v.engine.check()
        v.close()


def test_maze_side_stream_refills():
    """MazeS3 with episodes of 5 steps: the spare worlds' refills run on the side stream across calls, drawn or not, and an env may
    need a spare whose refill is still running or has not started (the wait and inline branches of the refill_mask protocol)."""
    subs, dones = _rollout_parity("MiniWorld-MazeS3-v0", 12, 2, 22, 77, 3, max_episode_steps=5)
    assert dones.sum() >= 24


def test_placement_program_with_program_rules(monkeypatch):
    """Sidewalk: a placement-program family whose env rule lives in the program's tables, with domain randomisation."""
    _short_episodes(monkeypatch, "Sidewalk", 3)
    subs, dones = _rollout_parity("MiniWorld-Sidewalk-v0", 16, 2, 16, 5, 3, domain_rand=True, want_depth=True)
    assert dones.sum() >= 32


@pytest.mark.parametrize("env_id,n_actions,kw", [("MiniWorld-Hallway-v0", 3, {}), ("MiniWorld-PickupObjects-v0", 5, {"domain_rand": True})])
@pytest.mark.parametrize("mode", [False, "same_step", "next_step"])
def test_constant_plans_equal_action_repeat(env_id, n_actions, kw, mode, monkeypatch):
    """A plan whose rows are all equal (the plan kernels) against step(actions, repeat=T) (the repeat kernels), and T = 1 against
    step(actions) (the plain ones), on a twin engine: everything bit for bit."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    _short_episodes(monkeypatch, env_id.split("-")[1], 6)
    n = 23
    A = MiniWorldVecEnv(env_id, n, autoreset=mode, seed=3, want_depth=True, **kw)
    B = MiniWorldVecEnv(env_id, n, autoreset=mode, seed=3, want_depth=True, **kw)
    A.reset()
    B.reset()
    g = torch.Generator(device="cuda").manual_seed(2)
    for t in range(18):
        T = (1, 4, 3)[t % 3]
        act = torch.randint(0, n_actions, (n,), generator=g, device="cuda", dtype=torch.int32)
        pend = A.reset_pending().cpu().numpy()
        A.step(act, repeat=T)
        B.rollout(act[None, :].repeat(T, 1))
        assert torch.equal(A.obs, B.obs) and torch.equal(A.depth, B.depth), (t, "frame")
        assert torch.equal(A.reward, B.reward) and torch.equal(A.terminated, B.terminated) and torch.equal(A.truncated, B.truncated), t
        assert _same_state(A.engine.get_state(), B.engine.get_state()), t
        assert torch.equal(A.reset_pending(), B.reset_pending()) and torch.equal(A.frame_clean(), B.frame_clean()), t
        if T > 1:
            assert torch.equal(A.substeps, B.substeps), t
        else:
            assert np.array_equal(B.substeps.cpu().numpy(), 1 - pend.astype(np.int32)), t
            assert torch.equal(B.step_rewards[0], A.reward), t
        ns = B.substeps.cpu().numpy()
        sr = B.step_rewards.cpu().numpy()
        assert all((sr[ns[i]:, i] == 0).all() for i in range(n)), t
    for v in (A, B):
        v.engine.check()
        v.close()


@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("pad", ["reset", "zero"])
def test_frame_stack_across_frameless_calls(mode, pad, monkeypatch):
    """K = 3: a drawn call, two frameless calls, a drawn call, ...  The first push behind frameless calls rebuilds the stacks of
    exactly the envs that began an episode since their last push — a world installed in any call since then: same-step, the call set
    term | trunc; next-step, the env entered it with reset_pending —, the others gain one frame; frameless calls do not move the
    ring.  The host list is built from a twin engine without a stack."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    _short_episodes(monkeypatch, "Hallway", 5)
    n, K, T = 43, 3, 3
    V = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, autoreset=mode, seed=21, frame_stack=K, stack_pad=pad)
    W = MiniWorldVecEnv("MiniWorld-Hallway-v0", n, autoreset=mode, seed=21)
    V.reset()
    W.reset()
    f0 = W.obs.cpu().numpy()
    blank = np.zeros_like(f0[0])
    rebuilt = lambda f: [f if pad == "reset" else blank] * (K - 1) + [f]
    win = [rebuilt(f0[i]) for i in range(n)]
    assert np.array_equal(V.stack.cpu().numpy(), np.array(win))
    began = np.zeros(n, bool)
    rebuilds = gains = 0
    g = torch.Generator(device="cuda").manual_seed(8)
    for j in range(10):
        drawn = j % 3 == 0
        plans = torch.where(torch.rand((T, n), generator=g, device="cuda") < 0.6, 2, torch.randint(0, 3, (T, n), generator=g, device="cuda")).to(torch.int32)
        pend = W.reset_pending().cpu().numpy().astype(bool)
        pushes = V.engine.stack_window()[1]
        for v in (V, W):
            v.rollout(plans, render=drawn)
        assert torch.equal(V.reward, W.reward) and torch.equal(V.terminated, W.terminated) and torch.equal(V.truncated, W.truncated), j
        began |= pend if mode == "next_step" else (W.terminated | W.truncated).cpu().numpy().astype(bool)
        if not drawn:
            assert V.engine.stack_window()[1] == pushes, j
            continue
        assert V.engine.stack_window()[1] == pushes + 1 and torch.equal(V.obs, W.obs), j
        f = W.obs.cpu().numpy()
        for i in range(n):
            win[i] = rebuilt(f[i]) if began[i] else win[i][1:] + [f[i]]
        rebuilds += int(began.sum())
        gains += int((~began).sum())
        stack = V.stack.cpu().numpy()
        bad = [i for i in range(n) if not np.array_equal(stack[i], np.array(win[i]))]
        assert not bad, (j, bad, began[bad])
        began[:] = False
    assert rebuilds >= n and gains >= 1, (rebuilds, gains)
    for v in (V, W):
        v.engine.check()
        v.close()


@pytest.mark.parametrize("env_id,n,n_actions,eps,kw", [("MiniWorld-Hallway-v0", 43, 3, 7, {"frame_stack": 3}),
                                                      ("MiniWorld-PickupObjects-v0", 16, 5, 8, {"domain_rand": True})])
def test_planner_round_trip(env_id, n, n_actions, eps, kw, monkeypatch):
    """save_state(frames=True), three frameless rollouts of random plans with T = 8 (episodes end inside them), load_state: obs,
    depth, stack and state are what they were at the save, and the next 10 steps equal those of a twin that never planned."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    _short_episodes(monkeypatch, env_id.split("-")[1], eps)
    V = MiniWorldVecEnv(env_id, n, seed=17, want_depth=True, **kw)
    W = MiniWorldVecEnv(env_id, n, seed=17, want_depth=True, **kw)
    V.reset()
    W.reset()
    g = torch.Generator(device="cuda").manual_seed(6)
    acts = lambda *shape: torch.where(torch.rand(shape, generator=g, device="cuda") < 0.5, 2, torch.randint(0, n_actions, shape, generator=g, device="cuda")).to(torch.int32)
    for _ in range(4):
        a = acts(n)
        V.step(a)
        W.step(a)
    snap = V.save_state(frames=True)
    obs0, depth0, st0 = V.obs.clone(), V.depth.clone(), V.engine.get_state()
    stack0 = V.stack.clone() if V.frame_stack else None
    ended = 0
    for _ in range(3):
        o, r, te, tr = V.rollout(acts(8, n), render=False)
        assert o is None
        ended += int((te | tr).sum().item())
    assert ended >= n and not _same_state(V.engine.get_state(), st0)
    assert torch.equal(V.obs, obs0) and torch.equal(V.depth, depth0)        # a frameless call writes no frame
    V.load_state(snap)
    assert torch.equal(V.obs, obs0) and torch.equal(V.depth, depth0) and _same_state(V.engine.get_state(), st0)
    assert _same_state(st0, W.engine.get_state())
    if stack0 is not None:
        assert torch.equal(V.stack, stack0) and torch.equal(V.stack, W.stack)
    for t in range(10):
        a = acts(n)
        V.step(a)
        W.step(a)
        assert torch.equal(V.obs, W.obs) and torch.equal(V.depth, W.depth), t
        assert torch.equal(V.reward, W.reward) and torch.equal(V.terminated, W.terminated) and torch.equal(V.truncated, W.truncated), t
        assert _same_state(V.engine.get_state(), W.engine.get_state()), t
        if stack0 is not None:
            assert torch.equal(V.stack, W.stack), t
    for v in (V, W):
        v.engine.check()
        v.close()


def test_refusals_touch_nothing(monkeypatch):
    """Horizon 0 and MW_MAX_PLAN + 1, null plans, d_depth without d_obs: MW_E_INVALID through the raw library call, nothing launched
    — the state and the stream afterwards are those of a twin that made no call, so the next step is equal."""
    import torch
    from miniworld_amd import engine as eng
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n = 7
    kw = dict(autoreset="same_step", seed=11, want_depth=True, domain_rand=True)
    vec = MiniWorldVecEnv("MiniWorld-PickupObjects-v0", n, **kw)
    twin = MiniWorldVecEnv("MiniWorld-PickupObjects-v0", n, **kw)
    vec.reset()
    twin.reset()
    before = vec.engine.get_state()
    obs0, depth0 = vec.obs.clone(), vec.depth.clone()
    plans = torch.zeros((eng.MAX_PLAN + 1, n), dtype=torch.int32, device="cuda")
    ns = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    sr = torch.full((eng.MAX_PLAN + 1, n), -1.0, dtype=torch.float32, device="cuda")
    ptr = lambda t: None if t is None else C_.c_void_p(t.data_ptr())
    lib, h = vec.engine.lib, vec.engine.h

    def call(d_plans, horizon, obs, depth):
        return lib.mw_step_plan(h, ptr(d_plans), horizon, ptr(obs), ptr(depth), ptr(vec.reward), ptr(sr), ptr(vec.terminated),
                                ptr(vec.truncated), ptr(ns), eng._stream_ptr(vec.engine.device))
    for args, word in (((plans, 0, vec.obs, None), b"horizon"), ((plans, eng.MAX_PLAN + 1, vec.obs, None), b"horizon"),
                       ((plans, 0, None, None), b"horizon"), ((None, 2, vec.obs, None), b"d_plans"), ((None, 2, None, None), b"d_plans"),
                       ((plans, 2, None, vec.depth), b"d_depth")):
        assert call(*args) == -1 and word in lib.mw_last_error(h), args[1:]
        torch.cuda.synchronize()
        assert _same_state(vec.engine.get_state(), before) and torch.equal(vec.obs, obs0) and torch.equal(vec.depth, depth0)
        assert (ns == -1).all() and (sr == -1).all()
    act = torch.full((n,), 2, dtype=torch.int32, device="cuda")
    vec.step(act)
    twin.step(act)
    assert torch.equal(vec.obs, twin.obs) and torch.equal(vec.depth, twin.depth) and torch.equal(vec.reward, twin.reward)
    assert _same_state(vec.engine.get_state(), twin.engine.get_state())
    for v in (vec, twin):
        v.engine.check()
        v.close()
