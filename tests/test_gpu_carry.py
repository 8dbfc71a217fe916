"""HIP step kernels against the reference's carried-object dynamics (GPU box): tests/golden/carry/*.npz, written by
tools/gen_carry_fixtures.py from the reference's own step() and pinned on the CPU by tests/test_carry_cpu.py.

Batched: env i of one engine replays trajectory i with its own per-step parameters, so the envs a dense wavefront packs side by
side are in different carry states; the threshold cases, single steps whose outcome hangs on a sum of radii that the reference
forms in float32 for mesh entities, run as one batch per family; the frameless plan kernels replay the same trajectories in
chunks; and beyond the fixtures the batched API follows the oracle (helpers.EpisodeMirror) under a scripted carrying policy.
"""
import math

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

FAMILIES = ("putnext", "roomobjects", "threerooms")
BOUND = 1e-12                     # the bound of test_step_matches_reference_trajectory
# N = 6: env i replays trajectory i.  N = 13: the six twice, the second time rotated, and one more — the pairs that share a dense
# wavefront differ from those of N = 6, and the last wavefront is partly empty.
LAYOUTS = {6: [0, 1, 2, 3, 4, 5], 13: [0, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 0, 3]}


def _family(fam, only_fixed_params=False):
    cases = [helpers.load_carry_case(c) for c in helpers.carry_cases(fam + "_")]
    assert len(cases) == 6
    if only_fixed_params:
        cases = [c for c in cases if not int(c[2]["domain_rand"])]
    s0, _, meta, _ = cases[0]
    for c in cases:           # one engine serves them all: shared geometry, one entity table layout, one task
        assert np.array_equal(c[0]["wall_segs"], s0["wall_segs"]) and np.array_equal(c[0]["ents_kind"], s0["ents_kind"])
        assert len(c[0]["mesh_names"]) == len(s0["mesh_names"]) and np.array_equal(c[0]["ents_mesh"], s0["ents_mesh"])
        assert helpers.goals_of(c[2]) == helpers.goals_of(meta) and float(c[2]["agent_radius"]) == float(meta["agent_radius"])
    return cases


def _engine(cases, n):
    s0, _, meta, _ = cases[0]
    g0, g1 = helpers.goals_of(meta)
    return helpers.make_engine_for_scene(s0, n, task=helpers.task_of(meta), goal_ent=g0, goal_ent2=g1, agent_radius=float(meta["agent_radius"]))


def _dense_lanes(s0, task):
    """k1_dense_lanes (mw_policy.h) for an engine that helpers.make_engine_for_scene configures, asked as tests/test_launch_policy_cpu.py does"""
    from test_launch_policy_cpu import LANES, ask, policy_lib
    P, E = len(s0["polys_nv"]), max(1, len(s0["ents_kind"]))
    return ask(policy_lib(), LANES, [P, E, -(-(P + 6 * E) // 16) * 16, task, 16, 75])[1]


def _buffers(n):
    import torch
    return (torch.zeros((n, 60, 80, 3), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"),
            torch.zeros(n, dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"),
            torch.zeros(n, dtype=torch.uint8, device="cuda"))


def _state_error(st, i, tr, t, E, tag):
    """Carried slot, alive flags and step count equal; returns the largest pose difference of env i against step t of tr."""
    assert int(st["carrying"][i]) == int(tr["carrying"][t]), tag
    alive = tr["ents_alive"][t].astype(bool)
    assert np.array_equal(st["ent_kind"][i, :E] != 0, alive), tag
    err = max(np.abs(st["agent_pos"][i] - tr["pos"][t]).max(), abs(st["agent_dir"][i] - tr["dir"][t]))
    if alive.any():
        err = max(err, np.abs(st["ent_pos"][i, :E][alive] - tr["ents_pos"][t][alive]).max(),
                  np.abs(st["ent_dir"][i, :E][alive] - tr["ents_dir"][t][alive]).max())
    return err


def test_the_carrying_families_take_both_forms_of_the_step_kernel():
    """RoomObjects is the carrying family of the dense K1 (several envs per wavefront, one lane per env in intersect); PutNext and
    ThreeRooms take the wave-per-env form."""
    lanes = {fam: _dense_lanes(_family(fam)[0][0], helpers.task_of(_family(fam)[0][2])) for fam in FAMILIES}
    s0 = _family("roomobjects")[0][0]
    assert lanes["roomobjects"] == len(s0["polys_nv"]) + 6 * len(s0["ents_kind"]) and 64 // lanes["roomobjects"] >= 2, lanes      # two envs per wavefront
    assert lanes["putnext"] == 0 and lanes["threerooms"] == 0, lanes


@pytest.mark.parametrize("n", sorted(LAYOUTS))
@pytest.mark.parametrize("fam", FAMILIES)
def test_batched_step_follows_the_carry_trajectories(fam, n):
    """Every env, every step, up to the step that ended its own episode: reward, flags and carried slot equal, poses within 1e-12."""
    cases = _family(fam)
    eng = _engine(cases, n)
    layout = LAYOUTS[n]
    trs = [cases[j][1] for j in layout]
    eng.set_state(helpers.scene_state_arrays([cases[j][0] for j in layout]))
    E = len(cases[0][0]["ents_kind"])
    rgb, act, rew, term, trunc = _buffers(n)
    T = [len(tr["action"]) for tr in trs]
    worst = 0.0
    for t in range(max(T)):
        live = [i for i in range(n) if t < T[i]]
        params = np.array([[trs[i][k][t] for k in ("fwd_step", "fwd_drift", "turn_step")] if t < T[i] else [0.15, 0.0, 15.0] for i in range(n)])
        eng.set_step_params(params)
        act.copy_(act.new_tensor([int(trs[i]["action"][t]) if t < T[i] else 7 for i in range(n)]))
        eng.step(act, rgb, None, rew, term, trunc)
        st = eng.get_state()
        r, te, tu = rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy()
        for i in live:
            tag = (fam, n, i, layout[i], t)
            assert np.float32(trs[i]["reward"][t]) == r[i] and bool(te[i]) == bool(trs[i]["term"][t]) and bool(tu[i]) == bool(trs[i]["trunc"][t]), tag
            assert int(st["step_count"][i]) == t + 1, tag
            worst = max(worst, _state_error(st, i, trs[i], t, E, tag))
    print(f"{fam} N={n}: worst state error {worst:.3g}")
    assert worst < BOUND, (fam, n, worst)
    eng.check()
    eng.close()


@pytest.mark.parametrize("fam", ["roomobjects", "threerooms"])
def test_threshold_cases_are_decided_like_the_reference(fam):
    """All of a family's threshold cases in one batch, one step: blocked or not, picked up or not as the reference decided (the
    float32 sum, where the float64 sum decides the other way), and the state after the step within 1e-12."""
    s0, tr, meta, poke = helpers.load_carry_case("thr_" + fam)
    K = len(poke["kind"])
    eng = helpers.make_engine_for_scene(s0, K, task=helpers.task_of(meta), agent_radius=float(meta["agent_radius"]))
    eng.set_state(helpers.scene_state_arrays([helpers.poked_scene(s0, poke, k) for k in range(K)]))
    eng.set_step_params(np.stack([tr["fwd_step"], tr["fwd_drift"], tr["turn_step"]], axis=1))
    rgb, act, rew, term, trunc = _buffers(K)
    act.copy_(act.new_tensor(tr["action"].astype(np.int32)))
    eng.step(act, rgb, None, rew, term, trunc)
    st = eng.get_state()
    E = len(s0["ents_kind"])
    wrong, worst = [], 0.0
    for k in range(K):
        kind = str(poke["kind"][k])
        got = dict(walk=np.array_equal(st["agent_pos"][k], poke["agent_pos"][k]), carry_move=np.array_equal(st["agent_pos"][k], poke["agent_pos"][k]),
                   carry_turn=st["agent_dir"][k] == poke["agent_dir"][k], pickup=int(st["carrying"][k]) == int(poke["ent"][k][0]))[kind]
        if got != bool(poke["decision"][k]):
            wrong.append((k, kind, bool(poke["sum32"][k] > poke["sum64"][k])))
        else:
            worst = max(worst, _state_error(st, k, tr, k, E, (fam, k)))
    print(f"thr_{fam}: {len(wrong)} of {K} decided differently, worst state error {worst:.3g}")
    assert not wrong, (fam, wrong)
    assert worst < BOUND, (fam, worst)
    eng.check()
    eng.close()


def test_sign_near_threshold_cases_end_the_episode_like_the_reference():
    """near() of Sign's rule (program_rules on the device) with the agent at a distance between the two sums of a key, and the agent
    walking into a key: reward, flags and the agent's pose as the reference's, through the batched API."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    s0, tr, meta, poke = helpers.load_carry_case("thr_sign")
    K, E = len(poke["kind"]), len(s0["ents_kind"])
    vec = MiniWorldVecEnv("MiniWorld-Sign-v0", K, seed=int(meta["seed"]), autoreset=False, **helpers.env_kwargs_of(meta))
    vec.reset()
    st = vec.engine.get_state()
    assert np.array_equal(st["ent_kind"][0, :E], s0["ents_kind"]) and np.array_equal(st["ent_pos"][0, :E], s0["ents_pos"])
    st["ent_pos"][:, :E], st["ent_dir"][:, :E] = poke["ents_pos"], poke["ents_dir"]
    vec.engine.set_state({"agent_pos": poke["agent_pos"], "agent_dir": poke["agent_dir"], "ent_pos": st["ent_pos"], "ent_dir": st["ent_dir"]})
    _, rew, term, trunc = vec.step(torch.tensor(tr["action"].astype(np.int32), device="cuda"))
    st = vec.engine.get_state()
    r, te = rew.cpu().numpy(), term.cpu().numpy().astype(bool)
    near = poke["kind"] == "near"
    assert near.sum() >= 3
    assert np.array_equal(te[near], poke["decision"][near]), (te[near], poke["decision"][near])
    assert np.array_equal(te, tr["term"]) and np.array_equal(r, tr["reward"].astype(np.float32)), (te, tr["term"], r, tr["reward"])
    assert np.abs(st["agent_pos"] - tr["pos"]).max() < BOUND and np.abs(st["agent_dir"] - tr["dir"]).max() < BOUND
    walk = poke["kind"] == "walk"
    assert np.array_equal((st["agent_pos"] == poke["agent_pos"]).all(axis=1)[walk], poke["decision"][walk])
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("fam", FAMILIES)
def test_frameless_plans_follow_the_carry_trajectories(fam):
    """mw_step_plan without a frame, in chunks of 8 steps, on the trajectories with fixed step parameters (a plan has one row of
    them): the executed counts, every step's own reward and the state at each chunk's end are the trajectory's."""
    import torch
    cases = _family(fam, only_fixed_params=True)
    n, CH = len(cases), 8
    assert n >= 4
    eng = _engine(cases, n)
    trs = [c[1] for c in cases]
    eng.set_state(helpers.scene_state_arrays([c[0] for c in cases]))
    eng.set_step_params(np.array([[tr[k][0] for k in ("fwd_step", "fwd_drift", "turn_step")] for tr in trs]))
    for tr in trs:
        assert all(len(np.unique(tr[k])) == 1 for k in ("fwd_step", "fwd_drift", "turn_step"))
    E = len(cases[0][0]["ents_kind"])
    _, _, rew, term, trunc = _buffers(n)
    ns = torch.zeros(n, dtype=torch.int32, device="cuda")
    sr = torch.zeros((CH, n), dtype=torch.float32, device="cuda")
    T = [len(tr["action"]) for tr in trs]
    worst, carried_ends = 0.0, 0
    for t0 in range(0, max(T), CH):
        h = min(CH, max(T) - t0)
        plans = np.full((h, n), 7, np.int32)
        want_n = np.zeros(n, np.int32)
        for i in range(n):
            m = max(0, min(h, T[i] - t0))
            plans[:m, i] = trs[i]["action"][t0:t0 + m]
            want_n[i] = m                   # (an episode ends on the last step of its trajectory, if it ends)
        eng.step_plan(torch.tensor(plans, device="cuda"), None, None, rew, sr, term, trunc, ns)
        st = eng.get_state()
        got_n, got_sr = ns.cpu().numpy(), sr.cpu().numpy()
        for i in range(n):
            m = int(want_n[i])
            if m == 0 or t0 + m > T[i]:
                continue
            te = t0 + m - 1
            tag = (fam, i, t0)
            if t0 + h <= T[i] or trs[i]["term"][te] or trs[i]["trunc"][te]:
                assert got_n[i] == m, (tag, got_n[i], m)
            assert np.array_equal(got_sr[:m, i], trs[i]["reward"][t0:t0 + m].astype(np.float32)), tag
            assert rew.cpu().numpy()[i] == np.float32(trs[i]["reward"][t0:t0 + m].sum()), tag
            if got_n[i] == m:
                assert bool(term[i].item()) == bool(trs[i]["term"][te]) and bool(trunc[i].item()) == bool(trs[i]["trunc"][te]), tag
                worst = max(worst, _state_error(st, i, trs[i], te, E, tag))
                carried_ends += int(trs[i]["carrying"][te]) >= 0
    print(f"{fam} plans: worst state error {worst:.3g}, {carried_ends} chunk ends with something in hand")
    assert worst < BOUND and carried_ends >= 20, (fam, worst, carried_ends)
    eng.check()
    eng.close()


@pytest.mark.parametrize("case", helpers.carry_cases("collecthealth_"))
def test_collecthealth_pickups_follow_the_reference_through_the_env_api(case):
    """CollectHealth's kits are picked up, consumed and respawned from the env's own stream: env 0, generated from the fixture's seed
    on the device, reproduces the reference's rewards, flags and the agent's pose at every step."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    s0, tr, meta, _ = helpers.load_carry_case(case)
    vec = MiniWorldVecEnv("MiniWorld-CollectHealth-v0", 3, seed=int(meta["seed"]), autoreset=False)
    vec.reset()
    st = vec.engine.get_state(0, 1)
    assert np.array_equal(st["agent_pos"][0], s0["agent_pos"])
    act = torch.zeros(3, dtype=torch.int32, device="cuda")
    worst = 0.0
    for t in range(len(tr["action"])):
        act[:] = int(tr["action"][t])
        _, rew, term, trunc = vec.step(act)
        assert np.float32(tr["reward"][t]) == rew[0].item(), (case, t)
        assert bool(term[0].item()) == bool(tr["term"][t]) and bool(trunc[0].item()) == bool(tr["trunc"][t]), (case, t)
        st = vec.engine.get_state(0, 1)
        assert int(st["carrying"][0]) == -1, (case, t)
        worst = max(worst, np.abs(st["agent_pos"][0] - tr["pos"][t]).max(), abs(st["agent_dir"][0] - tr["dir"][t]))
    assert worst < BOUND, (case, worst)
    assert (tr["event"] & 4).sum() >= 2
    vec.engine.check()
    vec.close()


def _scripted_action(m, rng, mem):
    """The fixtures' policy, from a mirror's state: walk to the nearest movable entity and pick it up; with something in hand, draw
    from actions 0-7 (tools/gen_carry_fixtures.py: POLICY)."""
    pos, d, carrying, _, alive, epos, _ = m.state()
    if carrying >= 0:
        return int(rng.choice(8, p=[0.2, 0.2, 0.40, 0.06, 0.02, 0.10, 0.01, 0.01]))
    if mem["wander"] > 0:
        mem["wander"] -= 1
        return int(rng.choice([0, 1, 2, 2, 3]))
    ok = alive & (m.sc["ents_static"] == 0)
    if not ok.any() or rng.random() < 0.05:
        return int(rng.integers(0, 8))
    dist = np.where(ok, np.hypot(epos[:, 0] - pos[0], epos[:, 2] - pos[2]), np.inf)
    k = int(np.argmin(dist))
    diff = (math.atan2(-(epos[k, 2] - pos[2]), epos[k, 0] - pos[0]) - d + math.pi) % (2 * math.pi) - math.pi
    if abs(diff) > math.radians(10):
        return 0 if diff > 0 else 1
    if dist[k] < 2.5 * float(m.h.agent.radius) + float(m.sc["ents_radius"][k]):
        mem["wander"] = 4               # (whether it succeeds or a wall vetoes it: move on, or carry it away)
        return 4
    return 2


@pytest.mark.parametrize("env_id,cls_name,dr,task", [("MiniWorld-RoomObjects-v0", "RoomObjects", True, 0), ("MiniWorld-PutNext-v0", "PutNext", False, 3)])
def test_vec_env_follows_the_oracle_under_the_carrying_policy(env_id, cls_name, dr, task):
    """Beyond the fixtures: 70 envs generated on the device, 150 steps of the scripted carrying policy computed per env from its CPU
    mirror (reference-exact generator + the oracle's dynamics, which tests/test_carry_cpu.py pins on the reference).  The device's
    state equals the mirror's at every step, rewards and flags included, across PutNext's auto-resets."""
    import torch
    from miniworld_amd import envs
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n, steps, seed = 70, 150, 4200
    vec = MiniWorldVecEnv(env_id, n, seed=seed, domain_rand=dr)
    vec.reset()
    mirrors = [helpers.EpisodeMirror(getattr(envs, cls_name), seed + i, dr, task) for i in range(n)]
    rng = np.random.default_rng(9)
    mem = [{"wander": 0} for _ in range(n)]
    worst, carried, mesh_carried = 0.0, 0, 0
    for t in range(steps):
        a = np.array([_scripted_action(m, rng, mem[i]) for i, m in enumerate(mirrors)], np.int32)
        _, rew, term, trunc = vec.step(torch.tensor(a, device="cuda"))
        got = torch.stack([rew, term.float(), trunc.float()]).cpu().numpy()
        for i, m in enumerate(mirrors):
            r, te, tr = m.step(a[i])
            assert np.float32(r) == got[0, i] and te == bool(got[1, i]) and tr == bool(got[2, i]), (env_id, t, i)
        st = vec.engine.get_state()
        for i, m in enumerate(mirrors):
            pos, d, carrying, count, alive, epos, edir = m.state()
            E = len(alive)
            assert int(st["step_count"][i]) == count and int(st["carrying"][i]) == carrying, (env_id, t, i)
            assert np.array_equal(st["ent_kind"][i, :E] != 0, alive), (env_id, t, i)
            worst = max(worst, np.abs(st["agent_pos"][i] - pos).max(), abs(st["agent_dir"][i] - d),
                        np.abs(st["ent_pos"][i, :E] - epos).max(), np.abs(st["ent_dir"][i, :E] - edir).max())
            carried += carrying >= 0
            mesh_carried += carrying >= 0 and int(m.sc["ents_kind"][carrying]) == 2
    print(f"{env_id}: worst state error {worst:.3g}, {carried} env-steps carrying, {mesh_carried} of them a mesh entity")
    assert worst < BOUND, (env_id, worst)
    assert carried >= 1000 and (cls_name != "RoomObjects" or mesh_carried >= 300), (carried, mesh_carried)
    vec.engine.check()
    vec.close()
