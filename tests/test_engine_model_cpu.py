"""The CPU model of the stepping API (tests/engine_model.py) checked without a GPU: against the reference-derived fixtures, against
hand-written loops over the host classes, and the fuzzer's generator (tests/api_fuzz.py) run on the model alone until its sequences
reach the coverage conditions the GPU fuzzer (tests/test_gpu_api_fuzz.py) asserts again."""
import collections

import numpy as np
import pytest

import api_fuzz
import engine_model
import helpers
import pyoracle
from conftest import golden_cases
from test_gpu_frame_cache import _short_episodes


def _vec(monkeypatch, cls_name, n, seed, task, episode=7, **kw):
    from miniworld_amd import envs
    _short_episodes(monkeypatch, cls_name, episode)
    mv = engine_model.ModelVec(getattr(envs, cls_name), n, seed=seed, task=task, **kw)
    mv.reset()
    return mv


def _actions(rng, n_actions, shape):
    return np.where(rng.random(shape) < 0.3, 4 % n_actions, rng.integers(0, n_actions, shape))


def _outputs(mv):
    out = {"obs": mv.obs.copy(), "reward": mv.reward.copy(), "terminated": mv.terminated.copy(), "truncated": mv.truncated.copy(),
           "pending": mv.pending.copy(), "state": [e.key()[1:] for e in mv.envs]}
    if mv.depth is not None:
        out["depth"] = mv.depth.copy()
    if mv.K:
        out["stack"] = mv.stack_array()
    return out


def _same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k] if k == "state" else np.array_equal(a[k], b[k]), (tag, k)


# ---------------------------------------------------------------------------------------------------------------- 1. the fixtures

@pytest.mark.parametrize("case", golden_cases())
def test_model_env_reproduces_the_reference_trajectory_and_frames(case):
    """What test_oracle_cpu.py asserts of the oracle, of a ModelEnv driven with the fixture's actions and recorded per-step
    parameters: rewards, flags, carried slot and entity lists identical, poses within 1e-12, the stored frames bit for bit."""
    s0, tr, meta, obs = helpers.load_case(case)
    rule = helpers.rule_of(meta)
    if rule == "api_only":
        pytest.skip("the env's Python rule moves entities (CollectHealth respawn): covered through the env API")
    g0, g1 = helpers.goals_of(meta)
    m = engine_model.ModelEnv.from_scene(s0, helpers.task_of(meta), int(min(float(s0["max_episode_steps"]), 2 ** 30)), g0, g1,
                                         float(meta.get("agent_radius", 0.4)))
    meshes = helpers.golden_meshes(s0)
    poke = meta.get("poke", np.array([-1.0]))
    worst, shown = 0.0, 0

    def frame(f):
        out = pyoracle.render(m.frame_scene(), meshes=meshes)
        assert np.array_equal(out["rgb"], obs[f]["rgb"]) and np.array_equal(out["z16"], obs[f]["z16"]), (case, "frame", f)
        return 1
    if 0 in obs:
        shown += frame(0)
    for t in range(len(tr["action"])):
        if int(poke[0]) == t:
            m.dyn.ents[int(poke[1])].pos[:] = [float(x) for x in poke[2:5]]
        r, te, tu = m.substep(tr["action"][t], (tr["fwd_step"][t], tr["fwd_drift"][t], tr["turn_step"][t]))
        if rule == "engine":
            assert r == tr["reward"][t] and te == tr["term"][t], (case, t)
        assert tu == tr["trunc"][t], (case, t)
        pos, d, carrying, count, alive, epos, edir = m.state()
        assert carrying == tr["carrying"][t] and count == t + 1, (case, t)
        assert np.array_equal(alive, tr["ents_alive"][t].astype(bool)), (case, t)
        worst = max(worst, np.abs(pos - tr["pos"][t]).max(), abs(d - tr["dir"][t]))
        if alive.any():
            worst = max(worst, np.abs(epos[alive] - tr["ents_pos"][t][alive]).max())
        if t + 1 in obs:
            shown += frame(t + 1)
    assert worst < 1e-12, (case, worst)
    assert shown == len(obs), (case, "a stored frame was not compared", sorted(obs))


# ---------------------------------------------------------------------------------------------------------------- 2. repeat, rollout

@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("cls_name,task,n_actions,dr", [("Hallway", 1, 3, False), ("PickupObjects", 2, 5, True)])
def test_repeat_and_rollout_equal_their_single_steps(monkeypatch, mode, cls_name, task, n_actions, dr):
    """One env per batch, so that the single-step twin can stop where the env stops: step(a, repeat=k) is k step(a) with a break on
    done, rollout(plans) the same over the plan's rows, with one push for the call; the reward is the sum (these families pay one
    reward that is no float per episode, so the sum of the single steps' floats is the double sum rounded once); trace rows are the
    states behind the single steps (read from the next-step twin, which keeps its terminal state), rows not executed repeat the last."""
    rng = np.random.default_rng(5)
    early = 0
    for seed in (11, 12):
        kw = dict(autoreset=mode, domain_rand=dr, want_depth=True, frame_stack=2)
        A, B = (_vec(monkeypatch, cls_name, 1, seed, task, **kw) for _ in range(2))
        for call in range(14):
            tag = (cls_name, mode, seed, call)
            T = int(rng.choice([1, 2, 5])) if call % 2 == 0 else int(rng.integers(1, 5))
            plan = np.repeat(_actions(rng, n_actions, (1, 1)), T, 0) if call % 2 == 0 else _actions(rng, n_actions, (T, 1))
            if call % 2 == 0:
                A.step(plan[0], repeat=T)
            else:
                A.rollout(plan, trace=True)
            stack0 = list(B.stack[0])

            def row():
                ag = B.envs[0].dyn.ag
                return (np.array(ag.pos[:]), float(ag.dir), int(ag.carrying))
            total, n, rows, step_r, done = 0.0, 0, [row()], np.zeros(T, np.float32), False
            if B.pending[0]:
                B.step(plan[0])                 # the reset step: nothing is executed, the rows hold the state it entered with
            else:
                rows = []
                for k in range(T):
                    B.step(plan[k])
                    total += float(B.reward[0])
                    step_r[k] = B.reward[0]
                    n += 1
                    rows.append(row())
                    done = bool(B.terminated[0] or B.truncated[0])
                    if done:
                        break
                early += n < T
                if not (done and mode == "same_step"):      # (a new episode's stack is the twin's own already)
                    B.stack[0] = stack0[1:] + [B.obs[0].copy()]
                B.reward[0] = np.float32(total)
            rows += [rows[-1]] * (T - len(rows))
            assert A.substeps[0] == n and np.array_equal(A.step_rewards[:, 0], step_r), tag
            _same(_outputs(A), _outputs(B), tag)
            if call % 2 == 1 and mode == "next_step":
                for k in range(T):
                    assert np.array_equal(A.trace["agent_pos"][k, 0], rows[k][0]) and A.trace["agent_dir"][k, 0] == rows[k][1] \
                        and A.trace["carrying"][k, 0] == rows[k][2], tag + (k,)
    assert early > 0, "no call ended an episode before its last sub-step: the stop rule was not met"


# ---------------------------------------------------------------------------------------------------------------- 3. the auto-reset modes

@pytest.mark.parametrize("mode", ["same_step", "next_step", "seeds"])
@pytest.mark.parametrize("cls_name,task,n_actions,dr", [("Hallway", 1, 3, False), ("PickupObjects", 2, 5, True)])
def test_autoreset_modes_equal_step_then_reset_over_the_host_class(monkeypatch, mode, cls_name, task, n_actions, dr):
    """`obs = env.step(a); if done: obs = env.reset(...)` written out over the host class, the oracle's step and the env's own stream —
    reset() for the same-step and next-step modes, reset(seed=next_seed[i]) for the seeded one, with one of the caller's writes."""
    from miniworld_amd import envs
    from miniworld_amd.scene import scene_from_env
    n, seed, steps = 3, 40, 30
    mv = _vec(monkeypatch, cls_name, n, seed, task, autoreset=mode, domain_rand=dr, final_obs=mode != "next_step")
    cls = getattr(envs, cls_name)
    rng = np.random.default_rng(9)
    acts = _actions(rng, n_actions, (steps, n))
    meshes = {}

    class Hand:
        def __init__(self, i):
            self.h = cls(host_only=True, domain_rand=dr)
            self.h.reset(seed=seed + i)
            self.world()
            self.pending = False

        def world(self):
            h = self.h
            self.sc = scene_from_env(h)
            self.dyn = pyoracle.Dynamics(self.sc, task, int(h.max_episode_steps), num_objs=len(self.sc["ents_kind"]),
                                         max_forward_step=float(h.max_forward_step), agent_radius=float(h.agent.radius))
            from miniworld_amd.objmesh import ObjMesh
            for name in [str(m) for m in self.sc["mesh_names"]]:
                m = ObjMesh.get(name)
                meshes[name] = {"verts": m.verts, "norms": m.norms, "texcs": m.texcs, "colors": m.colors}

        def frame(self, first):
            sc = dict(self.sc)
            if not first:
                E, ents = len(sc["ents_kind"]), self.dyn.render_ents
                sc["agent_pos"], sc["agent_dir"] = np.array(self.dyn.ag.pos[:]), np.float64(self.dyn.ag.dir)
                sc["ents_pos"] = np.array([ents[k].pos[:] for k in range(E)]).reshape(E, 3)
                sc["ents_dir"] = np.array([ents[k].dir for k in range(E)])
                sc["ents_kind"] = np.where([bool(ents[k].alive) for k in range(E)], sc["ents_kind"], 0).astype(np.int32)
            return pyoracle.render(sc, meshes=meshes)["rgb"]

        def step(self, a):
            rand = self.h.np_random if dr else None
            p = [self.h.params.sample(rand, k) for k in ("forward_step", "forward_drift", "turn_step")]
            return self.dyn.step(int(a), *p)

    hands = [Hand(i) for i in range(n)]
    next_seed = [seed + n + i for i in range(n)]
    ends = 0
    for t in range(steps):
        if mode == "seeds" and t == 5:
            mv.next_seed[1] = next_seed[1] = 777         # the caller's write wins
        mv.step(acts[t])
        for i, hd in enumerate(hands):
            tag = (cls_name, mode, t, i)
            if hd.pending:          # next-step: this call is the reset
                hd.h.reset()
                hd.world()
                hd.pending = False
                want = (hd.frame(True), 0.0, False, False)
            else:
                r, te, tr = hd.step(acts[t, i])
                want = (hd.frame(False), r, te, tr)
                if te or tr:
                    ends += 1
                    if mode == "next_step":
                        hd.pending = True
                    else:
                        assert np.array_equal(mv.final_obs[i], want[0]), tag
                        if mode == "seeds":
                            hd.h.reset(seed=next_seed[i])
                            assert mv.episode_seed[i] == next_seed[i], tag
                            next_seed[i] += n
                        else:
                            hd.h.reset()
                        hd.world()
                        want = (hd.frame(True),) + want[1:]
            assert np.array_equal(mv.obs[i], want[0]), tag
            assert mv.reward[i] == np.float32(want[1]) and bool(mv.terminated[i]) == want[2] and bool(mv.truncated[i]) == want[3], tag
            assert bool(mv.pending[i]) == hd.pending, tag
            if mode == "seeds":
                assert mv.next_seed[i] == next_seed[i], tag
    assert ends >= 6, ends


# ---------------------------------------------------------------------------------------------------------------- 4. records

@pytest.mark.parametrize("frames", [False, True])
def test_save_mutate_load_returns_the_saved_state(monkeypatch, frames):
    """A record is independent of everything the batch does afterwards — steps through episode ends, the stream, the stacks — and a
    loaded batch continues as the saved one did; without frames the loaded envs show a redraw of their state and new stacks."""
    n, steps = 3, 12
    mv = _vec(monkeypatch, "PickupObjects", n, 60, 2, autoreset="seeds", domain_rand=True, want_depth=True, frame_stack=3)
    rng = np.random.default_rng(3)
    for a in _actions(rng, 5, (5, n)):
        mv.step(a)
    snap = mv.save_state(frames=frames)
    at_save = _outputs(mv)
    seeds_at_save = mv.episode_seed.copy(), mv.next_seed.copy()       # (the batch's, not the records': the caller's to put back)
    acts = _actions(rng, 5, (steps, n))

    def play():
        out = []
        for a in acts:
            mv.step(a, repeat=2)
            out.append(_outputs(mv))
        return out
    first = play()
    assert (mv.terminated | mv.truncated).any() or any((o["terminated"] | o["truncated"]).any() for o in first)
    for again in range(2):
        mv.load_state(snap)
        mv.episode_seed[:], mv.next_seed[:] = seeds_at_save
        now = _outputs(mv)
        for k in ("state", "pending") + (("obs", "depth", "stack") if frames else ()):
            assert now[k] == at_save[k] if k == "state" else np.array_equal(now[k], at_save[k]), (again, k)
        if not frames:
            for i, e in enumerate(mv.envs):
                want = pyoracle.render(e.scene_now(), meshes=mv._meshes)
                assert np.array_equal(mv.obs[i], want["rgb"]) and np.array_equal(mv.depth[i], want["depth"])
                assert all(np.array_equal(f, want["rgb"]) for f in mv.stack[i])
            mv.load_state(snap)
        replay = play()
        for t, (a, b) in enumerate(zip(first, replay)):
            if not frames:      # (the stacks started anew; they agree again once K frames were pushed)
                a, b = ({k: v for k, v in o.items() if k != "stack" or t >= 2} for o in (a, b))
            _same(a, b, (again, t))


def test_a_masked_load_and_a_fork_move_only_what_they_name(monkeypatch):
    n = 4
    mv = _vec(monkeypatch, "Hallway", n, 70, 1, autoreset="next_step", frame_stack=2)
    rng = np.random.default_rng(4)
    for a in _actions(rng, 3, (4, n)):
        mv.step(a)
    snap = mv.save_state([2, 0], capacity=n, frames=True)           # record 0 = env 2, record 1 = env 0
    before = _outputs(mv)
    for a in _actions(rng, 3, (3, n)):
        mv.step(a)
    moved = _outputs(mv)
    mv.load_state_where(snap, [0, 1, 0, 1], [9, 0, 9, 1], True)      # env 1 := env 2 then, env 3 := env 0 then
    now = _outputs(mv)
    for i, src in ((1, 2), (3, 0)):
        assert now["state"][i] == before["state"][src] and np.array_equal(now["obs"][i], before["obs"][src])
        assert np.array_equal(now["stack"][i], before["stack"][src])
    for i in (0, 2):
        assert now["state"][i] == moved["state"][i] and np.array_equal(now["obs"][i], moved["obs"][i])
    mv.fork([3, 3, 0, 1], frames=True)
    forked = _outputs(mv)
    for j, s in enumerate([3, 3, 0, 1]):
        assert forked["state"][j] == now["state"][s] and np.array_equal(forked["stack"][j], now["stack"][s])


# ---------------------------------------------------------------------------------------------------------------- 5. stacks

@pytest.mark.parametrize("pad", ["reset", "zero"])
def test_stack_and_final_stack_equal_a_plain_deque(monkeypatch, pad):
    n, K = 3, 3
    mv = _vec(monkeypatch, "Hallway", n, 80, 1, autoreset="same_step", final_obs=True, frame_stack=K, stack_pad=pad)
    zero = np.zeros_like(mv.obs[0])

    def new(frame):
        return collections.deque([frame.copy() if pad == "reset" else zero] * (K - 1) + [frame.copy()], maxlen=K)
    dq = [new(mv.obs[i]) for i in range(n)]
    rng = np.random.default_rng(6)
    ends = 0
    for t, a in enumerate(_actions(rng, 3, (24, n))):
        mv.step(a, repeat=1 + t % 2)                # one push per call, whatever repeat is
        for i in range(n):
            if mv.terminated[i] or mv.truncated[i]:
                ends += 1
                assert np.array_equal(mv.final_stack[i], np.array(list(dq[i])[1:] + [mv.final_obs[i]])), (pad, t, i)
                dq[i] = new(mv.obs[i])
            else:
                dq[i].append(mv.obs[i].copy())
            assert np.array_equal(mv.stack_array()[i], np.array(dq[i])), (pad, t, i)
    assert ends >= 4


# ---------------------------------------------------------------------------------------------------------------- 6. the generator's coverage

@pytest.mark.parametrize("cfg_name", list(api_fuzz.CONFIGS))
def test_the_fuzzers_sequences_reach_their_coverage_conditions(monkeypatch, cfg_name, capsys):
    cfg = api_fuzz.CONFIGS[cfg_name]
    if cfg["episode"]:
        _short_episodes(monkeypatch, cfg["cls"], cfg["episode"])
    kinds, cov = collections.Counter(), collections.Counter()
    for seed in api_fuzz.SEEDS:
        mv, ops, k = api_fuzz.run_model(cfg_name, seed)
        kinds.update(k)
        cov.update(mv.cov)
        assert eval(api_fuzz.format_ops(ops[:5])) == ops[:5], "an op log must read back as the ops it lists"
    with capsys.disabled():
        print(f"\n[api fuzz coverage] {cfg_name}: {dict(cov)} ops {dict(kinds)}")
    assert api_fuzz.coverage_failures(cfg_name, kinds, cov) == []


def test_an_op_list_replays_to_the_same_model():
    """the helper a regression case is cut with: a prefix of a logged sequence, applied as data"""
    name = "mazes3_same_step"
    mv, ops, _ = api_fuzz.run_model(name, 1, n_ops=25)
    again, _, _ = api_fuzz.run_model(name, 1, ops=ops)
    _same(_outputs(mv), _outputs(again), name)
