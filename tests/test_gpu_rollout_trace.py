"""Rollout traces (mw_step_plan_trace; MiniWorldVecEnv.rollout(plans, render, trace=...)): the state behind every sub-step of a plan,
stored by the step kernel of the one launch that runs the plan.

The yardstick is never the trace kernel.  It is the scheme of tests/test_gpu_rollout.py: engine C without auto-reset is stepped with
single mw_steps and keeps get_state() of every tick, taken before its host resets anything; engine B makes traced rollout() calls,
drawn and frameless in turn.  Row k of env i of B's trace must be C's state behind that tick, bit for bit; rows k >= nsteps repeat row
nsteps - 1; an env that executed nothing repeats the state it entered with.  Everything tests/test_gpu_rollout.py compares of a call
— frames, rewards, flags, counts, state, infos — is compared here too, so a traced call is also proven equal to an untraced one.
The carry fixtures (tests/golden/carry, the reference's own step()) are the yardstick of the carried entity's rows."""
import ctypes as C_

import numpy as np
import pytest

import helpers
from test_gpu_rollout import _drawn, _plans, _reward_sum, _rows, _same_state, _short_episodes

pytestmark = pytest.mark.gpu

FIELDS = ("agent_pos", "agent_dir", "carrying", "ent_pos")
SENTINEL = -7


def _trace_row(st, i, slot):
    """env i's row of a trace as get_state() reports it: the four fields, ent_pos of one slot"""
    return {"agent_pos": st["agent_pos"][i].copy(), "agent_dir": st["agent_dir"][i].copy(), "carrying": st["carrying"][i].copy(),
            "ent_pos": st["ent_pos"][i, slot].copy()}


def _same_row(trace, k, i, want, fields=FIELDS):
    return all(np.array_equal(trace[f][k, i], want[f]) for f in fields)


def _reference_records(env_id, n, T, ticks, seed, plans, mode, want_depth, slot, kw):
    """Engine C (no auto-reset, single mw_steps, host resets): the records of every env's completed calls, as in
    tests/test_gpu_rollout.py, and with each the trace rows of its ticks: C's state behind the tick, before the host's reset."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    Cv = MiniWorldVecEnv(env_id, n, autoreset=False, seed=seed, want_depth=want_depth, **kw)
    assert Cv.autoreset_mode == "off"
    Cv.reset()
    zeros = lambda: (torch.zeros_like(Cv.obs), torch.zeros_like(Cv.depth) if want_depth else None)
    (rbuf, rdbuf), (pbuf, pdbuf) = zeros(), zeros()
    recs = [[] for _ in range(n)]
    call = np.zeros(n, np.int64)
    sub = np.zeros(n, np.int64)
    rew = [[] for _ in range(n)]
    rows = [[] for _ in range(n)]
    env_ix = np.arange(n)
    host = lambda t: None if t is None else t.cpu().numpy()
    for _ in range(ticks):
        o, r, te, tr = Cv.step(torch.as_tensor(plans[env_ix, call, sub], dtype=torch.int32, device="cuda"))
        o, d, r, te, tr = host(o), host(Cv.depth), host(r), host(te), host(tr)
        st, info = Cv.engine.get_state(), {k: host(v) for k, v in Cv.infos().items()}
        Cv.engine.render(pbuf, pdbuf)
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
            rows[i].append(_trace_row(st, i, slot))
            if not done[i] and sub[i] < T:
                continue
            new_world = done[i] and mode == "same_step"
            pick = lambda new, old: None if old is None else (new if new_world else old)[i]
            recs[i].append(dict(
                plan=call[i], rgb=pick(ro if new_world else None, o), depth=pick(rd if new_world else None, d),
                render=pick(ro if new_world else None, po), render_depth=pick(rd if new_world else None, pd),
                reward=_reward_sum(rew[i]), step_rewards=np.array(rew[i] + [0.0] * (T - len(rew[i])), np.float32), term=te[i], trunc=tr[i],
                nsteps=int(sub[i]), state=_rows(rst if new_world else st, i), info={k: v[i] for k, v in (rinfo if new_world else info).items()},
                done=bool(done[i]), trace=rows[i]))
            if done[i] and mode == "next_step":
                # the reset call: it executes nothing, its rows are the state the env entered with — the terminal one
                recs[i].append(dict(
                    plan=None, rgb=ro[i], depth=None if rd is None else rd[i], render=ro[i], render_depth=None if rd is None else rd[i],
                    reward=np.float32(0), step_rewards=np.zeros(T, np.float32), term=0, trunc=0, nsteps=0, state=_rows(rst, i),
                    info={k: v[i] for k, v in rinfo.items()}, done=False, trace=[rows[i][-1]]))
            call[i] += 1
            sub[i] = 0
            rew[i] = []
            rows[i] = []
    Cv.engine.check()
    Cv.close()
    return recs


def _trace_parity(env_id, n, T, ticks, seed, n_actions, mode="same_step", want_depth=False, p_fwd=None, slot=0, **kw):
    """B's traced rollout() calls, drawn and frameless in turn, against C's records.  Returns per call: substeps [calls][n], done
    flags, and whether the last row of an env's trace differs from the state the env holds behind the call (a world was installed)."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    rng = np.random.default_rng(seed)
    plans = _plans(rng, n, ticks + 1, T, n_actions, p_fwd)
    recs = _reference_records(env_id, n, T, ticks, seed, plans, mode, want_depth, slot, kw)
    calls = min(len(r) for r in recs)
    assert calls >= 4, calls
    B = MiniWorldVecEnv(env_id, n, autoreset=mode, seed=seed, want_depth=want_depth, **kw)
    B.reset()
    fbuf, fdbuf = torch.zeros_like(B.obs), (torch.zeros_like(B.depth) if want_depth else None)
    subs, dones, moved = [], [], []
    host = lambda t: None if t is None else t.cpu().numpy()
    for j in range(calls):
        rec = [recs[i][j] for i in range(n)]
        plan = np.stack([plans[i, c["plan"]] if c["plan"] is not None else rng.integers(0, n_actions, T) for i, c in enumerate(rec)], axis=1)
        if mode == "next_step":
            pend = B.reset_pending().cpu().numpy().astype(bool)
            assert np.array_equal(pend, np.array([c["plan"] is None for c in rec])), (env_id, j)
        entered = {k: host(v).copy() for k, v in B.state(("agent_pos", "agent_dir", "carrying", "ent_pos")).items()}
        drawn = _drawn(j)
        o, r, te, tr = B.rollout(torch.as_tensor(plan, dtype=torch.int32, device="cuda"), render=drawn, trace=FIELDS, trace_ent=slot)
        assert set(B.trace) == set(FIELDS) and all(B.trace[f].shape[:2] == (T, n) for f in FIELDS)
        trace = {f: host(B.trace[f]) for f in FIELDS}
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
        mv = np.zeros(n, bool)
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
            # the trace: the executed rows are C's states behind those ticks, the others repeat the last one
            m = c["nsteps"]
            assert len(c["trace"]) == max(m, 1)
            for k in range(T):
                want = c["trace"][min(k, len(c["trace"]) - 1)]
                for f in FIELDS:
                    assert np.array_equal(trace[f][k, i], want[f]), tag + ("trace", f, "row", k, trace[f][k, i], want[f])
            if m == 0:      # ... which, for an env that executed nothing, is the state B itself held before the call
                for k in range(T):
                    assert all(np.array_equal(trace[f][k, i], entered[f][i, slot] if f == "ent_pos" else entered[f][i]) for f in FIELDS), tag + ("entered", k)
            mv[i] = not (np.array_equal(trace["agent_pos"][T - 1, i], st["agent_pos"][i]) and trace["agent_dir"][T - 1, i] == st["agent_dir"][i])
        subs.append(ns.copy())
        dones.append((te | tr).astype(bool))
        moved.append(mv)
    B.engine.check()
    B.close()
    return np.array(subs), np.array(dones), np.array(moved)


@pytest.mark.parametrize("spare", ["0", "1"])
def test_hallway_dense_same_step(spare, monkeypatch):
    """The dense trace kernel, 43 envs: five per wavefront and a ragged last one.  Episodes of 7 steps at T = 4: the envs of a wavefront
    stop at different sub-steps — the fill inside the loop and behind it —, and the rows of a terminal sub-step are the terminal state
    although the env holds its next world when the call returns."""
    monkeypatch.setenv("MW_SPARE", spare)
    _short_episodes(monkeypatch, "Hallway", 7)
    subs, dones, moved = _trace_parity("MiniWorld-Hallway-v0", 43, 4, 30, 900, 3, p_fwd=0.6)
    assert dones.sum() >= 43
    assert ((subs > 1) & (subs < 4)).any()
    # within one wavefront (envs 5 w .. 5 w + 4) of one call: an env that stopped early beside one that ran on (rows filled inside the
    # loop), and a whole wavefront that stopped before T (rows filled behind it)
    waves = [subs[:, w:w + 5] for w in range(0, 43, 5)]
    assert any(((wv.min(axis=1) < wv.max(axis=1)) & (wv.min(axis=1) >= 1)).any() for wv in waves)
    assert any((wv.max(axis=1) < 4).any() for wv in waves)
    # a finished env holds a new world behind the call, its trace ends in the old one
    assert (moved & dones).sum() >= 20 and not (moved & ~dones).any()


@pytest.mark.parametrize("spare", ["0", "1"])
def test_hallway_dense_philox(spare, monkeypatch):
    """The dense trace kernel of the Philox stream (every other case here runs the PCG64 kernels), 7 envs: a full wavefront of five and
    a ragged one of two.  Episodes of 7 steps at T = 4: truncation and the install, with its draws, land on sub-step 3 of every
    second call; the rows of that sub-step are the terminal state."""
    monkeypatch.setenv("MW_SPARE", spare)
    _short_episodes(monkeypatch, "Hallway", 7)
    subs, dones, moved = _trace_parity("MiniWorld-Hallway-v0", 7, 4, 20, 902, 3, p_fwd=0.6, rng="philox")
    assert dones.sum() >= 7
    assert ((subs > 1) & (subs < 4)).any()
    assert (moved & dones).any() and not (moved & ~dones).any()


def test_maze_wave_per_env_philox(monkeypatch):
    """The wave-per-env trace kernel of the Philox stream: MazeS3, 3 envs, episodes of 6 steps at T = 4 — every second call ends on
    sub-step 2 and installs a world.  Without spare worlds: the kernel generates the maze itself, from its own stream's draws (with
    them a finished env takes a world the refill kernel made, and this kernel draws nothing)."""
    monkeypatch.setenv("MW_SPARE", "0")
    subs, dones, moved = _trace_parity("MiniWorld-MazeS3-v0", 3, 4, 18, 78, 3, max_episode_steps=6, rng="philox")
    assert dones.sum() >= 6
    assert ((subs > 1) & (subs < 4)).any()
    assert (moved & dones).any()


def test_oneroom_dense_next_step(monkeypatch):
    """Next-step mode, T = 3 on episodes of 2 steps: every second call executes 0 sub-steps and all three of its rows are the state the
    env entered the call with (compared with B.state() before the call in _trace_parity), not the world it installs."""
    _short_episodes(monkeypatch, "OneRoom", 2)
    subs, dones, moved = _trace_parity("MiniWorld-OneRoom-v0", 40, 3, 16, 901, 3, mode="next_step", p_fwd=0.6)
    assert len(subs) >= 8
    assert (subs[0::2] <= 2).all() and (subs[0::2] >= 1).all() and dones[0::2].all()
    assert (subs[1::2] == 0).all() and not dones[1::2].any()
    assert moved[1::2].sum() >= 40 and not moved[0::2].any()      # the reset calls install a world their traces do not show


def test_pickup_objects_domain_rand(monkeypatch):
    """The wave-per-env trace kernel with meshes and domain randomisation, slot 0's position beside the agent's."""
    _short_episodes(monkeypatch, "PickupObjects", 8)
    subs, dones, moved = _trace_parity("MiniWorld-PickupObjects-v0", 16, 3, 24, 31, 5, domain_rand=True)
    assert dones.sum() >= 16


@pytest.mark.parametrize("drawn", [True, False])
def test_pickups_mid_call_and_on_the_last_sub_step(drawn):
    """PickupObjects, directed (the set-up of tests/test_gpu_rollout.py's pickup on the last sub-step): the agents of envs 0 and 1 face
    their object 0 at pickup distance.  Env 0 takes [drop, pickup, drop], env 1 [drop, drop, pickup].  The sub-step that picks the
    object up carries it to the agent's hands — ent_pos of slot 0 moves in that row —, and `carrying` reads -1 in every row: the object
    leaves the list (pickupobjects.py:86-88), as the step kernel stores it.  Against single steps of engine C, drawn and frameless."""
    import torch
    n, T = 16, 3
    from miniworld_amd.vec_env import MiniWorldVecEnv
    kw = dict(seed=5, domain_rand=True)
    B = MiniWorldVecEnv("MiniWorld-PickupObjects-v0", n, autoreset="same_step", **kw)
    Cv = MiniWorldVecEnv("MiniWorld-PickupObjects-v0", n, autoreset=False, **kw)
    B.reset()
    Cv.reset()
    st = Cv.engine.get_state()
    assert _same_state(st, B.engine.get_state())
    r_agent = float(Cv.template.agent.radius)
    for i in (0, 1):
        assert st["ent_kind"][i, 0] != 0
        st["ent_kind"][i, 1:] = 0
        ext = st["extent"][i]
        st["ent_pos"][i, 0, 0], st["ent_pos"][i, 0, 2] = 0.5 * (ext[0] + ext[1]), 0.5 * (ext[2] + ext[3])
        st["agent_pos"][i] = st["ent_pos"][i, 0] - np.array([r_agent + st["ent_geom"][i, 0, 7] + 0.05, 0.0, 0.0])
        st["agent_pos"][i, 1] = 0.0
        st["agent_dir"][i] = 0.0
    for v in (B, Cv):
        v.engine.set_state(st)
    plan = np.full((T, n), 5, np.int32)
    plan[:, 0], plan[:, 1] = [5, 4, 5], [5, 5, 4]
    want, rewards = [], []
    for k in range(T):
        o, r, te, tr = Cv.step(torch.as_tensor(plan[k], device="cuda"))
        assert not (te | tr)[:2].any()
        rewards.append(r.cpu().numpy().copy())
        cst = Cv.engine.get_state()
        want.append([_trace_row(cst, i, 0) for i in range(n)])
    rewards = np.array(rewards)
    # C: the events are the ones meant
    assert rewards[:, 0].tolist() == [0.0, 1.0, 0.0] and rewards[:, 1].tolist() == [0.0, 0.0, 1.0], rewards[:, :2]
    for i, k_pick in ((0, 1), (1, 2)):
        assert np.array_equal(want[k_pick - 1][i]["ent_pos"], st["ent_pos"][i, 0]) and not np.array_equal(want[k_pick][i]["ent_pos"], st["ent_pos"][i, 0])
        assert all(int(want[k][i]["carrying"]) == -1 for k in range(T))
    o, r, te, tr = B.rollout(torch.as_tensor(plan, device="cuda"), render=drawn, trace=FIELDS, trace_ent=0)
    assert (o is B.obs) if drawn else (o is None)
    assert np.array_equal(B.step_rewards.cpu().numpy(), rewards) and B.substeps.cpu().numpy().tolist() == [T] * n
    trace = {f: B.trace[f].cpu().numpy() for f in FIELDS}
    for k in range(T):
        for i in range(n):
            assert _same_row(trace, k, i, want[k][i]), (k, i, {f: trace[f][k, i] for f in FIELDS}, want[k][i])
    assert _same_state(B.engine.get_state(), Cv.engine.get_state())
    if drawn:
        assert torch.equal(B.obs, Cv.obs)
    for v in (B, Cv):
        v.engine.check()
        v.close()


def test_maze_side_stream_refills():
    """MazeS3 with episodes of 5 steps: per-env geometry, the spare worlds installed from the side stream across traced calls."""
    subs, dones, moved = _trace_parity("MiniWorld-MazeS3-v0", 12, 2, 22, 77, 3, max_episode_steps=5)
    assert dones.sum() >= 24
    assert (moved & dones).sum() >= 12


@pytest.mark.parametrize("fam", ["putnext", "roomobjects", "threerooms"])
def test_traced_plans_follow_the_carry_trajectories_at_every_step(fam):
    """The set-up of tests/test_gpu_carry.py::test_frameless_plans_follow_the_carry_trajectories — the reference's own step() on the
    trajectories with fixed step parameters, in frameless chunks of 8 —, looked at inside every chunk, not at its end only: row k of the
    trace against the fixture's pos, dir, carrying and ents_pos[slot] at step t0 + k, for a slot the trajectories carry.  `carrying`
    equal, poses within that file's bound (1e-12: what the oracle and the step kernels hold against these fixtures at chunk ends)."""
    import torch
    from test_gpu_carry import BOUND, _buffers, _engine, _family
    assert BOUND == 1e-12
    cases = _family(fam, only_fixed_params=True)
    n, CH = len(cases), 8
    assert n >= 4
    eng = _engine(cases, n)
    trs = [c[1] for c in cases]
    eng.set_state(helpers.scene_state_arrays([c[0] for c in cases]))
    eng.set_step_params(np.array([[tr[k][0] for k in ("fwd_step", "fwd_drift", "turn_step")] for tr in trs]))
    # the slot most often in hand over the family's trajectories
    held = np.concatenate([tr["carrying"][tr["carrying"] >= 0] for tr in trs])
    assert held.size > 0
    slot = int(np.bincount(held).argmax())
    _, _, rew, term, trunc = _buffers(n)
    ns = torch.zeros(n, dtype=torch.int32, device="cuda")
    sr = torch.zeros((CH, n), dtype=torch.float32, device="cuda")
    trace = {"agent_pos": torch.zeros((CH, n, 3), dtype=torch.float64, device="cuda"), "agent_dir": torch.zeros((CH, n), dtype=torch.float64, device="cuda"),
             "carrying": torch.zeros((CH, n), dtype=torch.int32, device="cuda"), "ent_pos": torch.zeros((CH, n, 3), dtype=torch.float64, device="cuda")}
    T = [len(tr["action"]) for tr in trs]
    worst, in_hand, slot_in_hand, rows = 0.0, 0, 0, 0
    for t0 in range(0, max(T), CH):
        h = min(CH, max(T) - t0)
        plans = np.full((h, n), 7, np.int32)
        want_n = np.zeros(n, np.int32)
        for i in range(n):
            m = max(0, min(h, T[i] - t0))
            plans[:m, i] = trs[i]["action"][t0:t0 + m]
            want_n[i] = m
        eng.step_plan_trace(torch.tensor(plans, device="cuda"), None, None, rew, sr, term, trunc, ns, trace=trace, ent_slot=slot)
        got = {f: t.cpu().numpy() for f, t in trace.items()}
        got_n, got_sr = ns.cpu().numpy(), sr.cpu().numpy()
        for i in range(n):
            m = int(want_n[i])
            if m == 0 or t0 + m > T[i]:
                continue
            assert got_n[i] >= m, (fam, i, t0, got_n[i], m)      # (an episode ends on the last step of its trajectory, if it ends)
            assert np.array_equal(got_sr[:m, i], trs[i]["reward"][t0:t0 + m].astype(np.float32)), (fam, i, t0)
            for k in range(m):
                t, tag = t0 + k, (fam, i, t0, k)
                assert int(got["carrying"][k, i]) == int(trs[i]["carrying"][t]), tag + (got["carrying"][k, i], trs[i]["carrying"][t])
                err = max(np.abs(got["agent_pos"][k, i] - trs[i]["pos"][t]).max(), abs(got["agent_dir"][k, i] - trs[i]["dir"][t]))
                if trs[i]["ents_alive"][t][slot]:
                    err = max(err, np.abs(got["ent_pos"][k, i] - trs[i]["ents_pos"][t][slot]).max())
                assert err < BOUND, tag + (err,)
                worst = max(worst, err)
                rows += 1
                in_hand += int(trs[i]["carrying"][t]) >= 0
                slot_in_hand += int(trs[i]["carrying"][t]) == slot
    print(f"{fam} traced plans: {rows} rows, worst error {worst:.3g}, {in_hand} rows with something in hand, {slot_in_hand} with slot {slot}")
    assert worst < BOUND and in_hand >= 20 and slot_in_hand >= 1, (fam, worst, in_hand, slot_in_hand)
    eng.check()
    eng.close()


def _bufs(T, n, rows_extra=0, fields=FIELDS, fill=0):
    import torch
    shape = {"agent_pos": (3,), "agent_dir": (), "carrying": (), "ent_pos": (3,)}
    return {f: torch.full((T + rows_extra, n) + shape[f], fill, dtype=torch.int32 if f == "carrying" else torch.float64, device="cuda") for f in fields}


@pytest.mark.parametrize("T", [1, 256])
def test_shortest_and_longest_plans_and_single_fields(T):
    """T = 1 and T = MW_MAX_PLAN on 3 Hallway envs (one partly filled dense wavefront), same-step: all four fields against single steps
    of engine C up to each env's episode end and the repeated last row behind it; then each field asked for alone, the other pointers
    NULL, on a twin engine: the same rows, the same state."""
    import torch
    from miniworld_amd import engine as eng
    from miniworld_amd.vec_env import MiniWorldVecEnv
    assert eng.MAX_PLAN == 256
    n, seed = 3, 41
    make = lambda mode: MiniWorldVecEnv("MiniWorld-Hallway-v0", n, autoreset=mode, seed=seed)
    rng = np.random.default_rng(T)
    plan = np.where(rng.random((T, n)) < 0.7, 2, rng.integers(0, 3, (T, n))).astype(np.int32)
    Cv = make(False)
    Cv.reset()
    want, alive = [[] for _ in range(n)], np.ones(n, bool)
    for k in range(T):
        o, r, te, tr = Cv.step(torch.as_tensor(plan[k], device="cuda"))
        st = Cv.engine.get_state()
        for i in np.flatnonzero(alive):
            want[i].append(_trace_row(st, i, 0))
        alive &= ~(te | tr).cpu().numpy().astype(bool)
        if not alive.any():
            break
    Cv.engine.check()
    Cv.close()
    B = make("same_step")
    B.reset()
    B.rollout(torch.as_tensor(plan, device="cuda"), render=False, trace=FIELDS)
    full = {f: B.trace[f].cpu().numpy() for f in FIELDS}
    ns = B.substeps.cpu().numpy()
    assert [len(w) for w in want] == ns.tolist()
    if T == 256:
        assert (ns < T).all() and (ns > 8).any()        # (Hallway's episodes end by step 250: rows behind every env's last one)
    for i in range(n):
        for k in range(T):
            assert _same_row(full, k, i, want[i][min(k, ns[i] - 1)]), (T, i, k)
    after = B.save_state().data.cpu()
    B.engine.check()
    B.close()
    for f in FIELDS:
        V = make("same_step")
        V.reset()
        V.rollout(torch.as_tensor(plan, device="cuda"), render=False, trace=(f,))
        assert set(V.trace) == {f} and np.array_equal(V.trace[f].cpu().numpy(), full[f]), (T, f)
        assert torch.equal(V.save_state().data.cpu(), after), (T, f)
        V.engine.check()
        V.close()


@pytest.mark.parametrize("env_id,n,n_actions,kw", [("MiniWorld-Hallway-v0", 43, 3, {}), ("MiniWorld-PickupObjects-v0", 7, 5, {"domain_rand": True})])
def test_a_trace_stays_inside_its_rows_and_changes_nothing_else(env_id, n, n_actions, kw, monkeypatch):
    """Twin engines, one traced and one not, through drawn and frameless calls: snapshot bytes (state and stream), step_rewards, flags,
    counts and frames stay identical.  The traced engine writes into rows 1 .. T of buffers of T + 2 rows: the row before and the row
    behind keep their sentinel.  (A trace is [T][N] rows of N columns back to back: the column behind the last env of row k is the
    first of row k + 1, so the rows around the trace are the only sentinels the layout allows.)"""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    _short_episodes(monkeypatch, env_id.split("-")[1], 6)
    T = 4
    A = MiniWorldVecEnv(env_id, n, seed=9, want_depth=True, **kw)
    B = MiniWorldVecEnv(env_id, n, seed=9, want_depth=True, **kw)
    A.reset()
    B.reset()
    g = torch.Generator(device="cuda").manual_seed(3)
    ended = 0
    for j in range(8):
        drawn = _drawn(j)
        plans = torch.where(torch.rand((T, n), generator=g, device="cuda") < 0.5, 2, torch.randint(0, n_actions, (T, n), generator=g, device="cuda")).to(torch.int32)
        A.rollout(plans, render=drawn)
        parent = _bufs(T, n, rows_extra=2, fill=SENTINEL)
        sr = torch.full((T + 1, n), float(SENTINEL), dtype=torch.float32, device="cuda")
        B.substeps = torch.zeros(n, dtype=torch.int32, device="cuda") if B.substeps is None else B.substeps
        obs, depth = (B.obs, B.depth) if drawn else (None, None)
        B.engine.step_plan_trace(plans, obs, depth, B.reward, sr, B.terminated, B.truncated, B.substeps, trace={f: t[1:] for f, t in parent.items()}, ent_slot=0)
        for f, t in parent.items():
            assert (t[0] == SENTINEL).all() and (t[T + 1] == SENTINEL).all(), (j, f, "a row outside the trace was written")
            assert not (t[1:T + 1] == SENTINEL).all(dim=0).any(), (j, f, "a column was not written")
        assert (sr[T] == SENTINEL).all() and torch.equal(sr[:T], A.step_rewards), j
        assert torch.equal(A.reward, B.reward) and torch.equal(A.terminated, B.terminated) and torch.equal(A.truncated, B.truncated), j
        assert torch.equal(A.substeps, B.substeps), j
        assert torch.equal(A.save_state().data, B.save_state().data), (j, "state / stream")
        assert torch.equal(A.frame_clean(), B.frame_clean()), j
        if drawn:
            assert torch.equal(A.obs, B.obs) and torch.equal(A.depth, B.depth), j
        ended += int((A.terminated | A.truncated).sum().item())
    assert ended >= n
    for v in (A, B):
        v.engine.check()
        v.close()


def test_refusals_touch_nothing():
    """A null trace, a trace without a field, ent_pos with a slot out of range, and everything mw_step_plan refuses: MW_E_INVALID through
    the raw library call, nothing launched — snapshot bytes and every output buffer as before, and the next step equals a twin's.  And
    ent_pos on a MW_TASK_COLLECT engine."""
    import torch
    from miniworld_amd import engine as eng
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n, T = 7, 2
    kw = dict(autoreset="same_step", seed=11, want_depth=True, domain_rand=True)
    ptr = lambda t: None if t is None else C_.c_void_p(t.data_ptr())

    def refusals(vec, cases):
        lib, h, E = vec.engine.lib, vec.engine.h, int(vec.engine.cfg.max_ents)
        before = vec.save_state().data.clone()
        obs0, depth0 = vec.obs.clone(), vec.depth.clone()
        plans = torch.zeros((eng.MAX_PLAN + 1, n), dtype=torch.int32, device="cuda")
        ns = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        sr = torch.full((eng.MAX_PLAN + 1, n), -1.0, dtype=torch.float32, device="cuda")
        bufs = _bufs(T, n, fill=SENTINEL)

        def view(names, slot=0):
            t = eng.MwPlanTrace()
            for f in names:
                setattr(t, f, bufs[f].data_ptr())
            t.ent_slot = slot
            return C_.byref(t)

        def call(d_plans, horizon, obs, depth, trace):
            return lib.mw_step_plan_trace(h, ptr(d_plans), horizon, ptr(obs), ptr(depth), ptr(vec.reward), ptr(sr), ptr(vec.terminated),
                                          ptr(vec.truncated), ptr(ns), trace, eng._stream_ptr(vec.engine.device))
        for make_args, word in cases(plans, view, E):
            assert call(*make_args) == -1 and word in lib.mw_last_error(h), (word, lib.mw_last_error(h))
            torch.cuda.synchronize()
            assert torch.equal(vec.save_state().data, before) and torch.equal(vec.obs, obs0) and torch.equal(vec.depth, depth0), word
            assert (ns == -1).all() and (sr == -1).all() and all((t == SENTINEL).all() for t in bufs.values()), word

    vec = MiniWorldVecEnv("MiniWorld-PickupObjects-v0", n, **kw)
    twin = MiniWorldVecEnv("MiniWorld-PickupObjects-v0", n, **kw)
    vec.reset()
    twin.reset()
    refusals(vec, lambda plans, view, E: (
        ((plans, T, vec.obs, None, None), b"no trace field"), ((plans, T, None, None, None), b"no trace field"),
        ((plans, T, vec.obs, None, view(())), b"no trace field"), ((plans, T, None, None, view((), 3)), b"no trace field"),
        ((plans, T, vec.obs, None, view(FIELDS, E)), b"ent_slot"), ((plans, T, None, None, view(("ent_pos",), -1)), b"ent_slot"),
        ((plans, 0, vec.obs, None, view(FIELDS)), b"horizon"), ((plans, eng.MAX_PLAN + 1, None, None, view(FIELDS)), b"horizon"),
        ((None, T, vec.obs, None, view(FIELDS)), b"d_plans"), ((None, T, None, None, view(FIELDS)), b"d_plans"),
        ((plans, T, None, vec.depth, view(FIELDS)), b"d_depth")))
    # a frameless call under reset seeds
    seeds = torch.arange(n, dtype=torch.int64, device="cuda")
    vec.engine.set_reset_seeds(seeds)
    refusals(vec, lambda plans, view, E: (((plans, T, None, None, view(FIELDS)), b"reset seeds"),))
    vec.engine.set_reset_seeds(None)
    act = torch.full((n,), 2, dtype=torch.int32, device="cuda")
    vec.step(act)
    twin.step(act)
    assert torch.equal(vec.obs, twin.obs) and torch.equal(vec.depth, twin.depth) and torch.equal(vec.reward, twin.reward)
    assert _same_state(vec.engine.get_state(), twin.engine.get_state())
    for v in (vec, twin):
        v.engine.check()
        v.close()
    ch = MiniWorldVecEnv("MiniWorld-CollectHealth-v0", n, autoreset="next_step", seed=13, want_depth=True)
    ch.reset()
    refusals(ch, lambda plans, view, E: (((plans, T, ch.obs, None, view(FIELDS)), b"MW_TASK_COLLECT"), ((plans, T, None, None, view(("ent_pos",))), b"MW_TASK_COLLECT")))
    ch.rollout(torch.zeros((T, n), dtype=torch.int32, device="cuda"), render=False, trace=True)      # the other fields are CollectHealth's too
    assert tuple(ch.trace["agent_pos"].shape) == (T, n, 3)
    ch.engine.check()
    ch.close()
