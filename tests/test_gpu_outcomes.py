"""The step that ENDS an episode, in the forms and modes of the batched env where it had only been compared with the CPU model:
step(repeat=K), the traced rollout, the three auto-reset forms and PickupObjects' steps in the emptied room (GPU box).

Every expected value is the reference's own, from tests/golden/out_*.npz (tools/gen_outcome_fixtures.py: the unmodified reference
driven by a scripted expert until its outcome — a GOTO success, Sign's +1, Sidewalk's box, all objects collected, a box put next,
an episode that terminates and truncates in one step).  A batch of three, seeded seed, seed + 1, seed + 2 and all given env 0's
actions: env 0 IS the fixture's episode, the other two end theirs at other steps (or not at all), so a dense wavefront holds envs
in different phases.  The short cases carry the forms; Maze and the other long ones are left to the plain parametrized tests."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

N = 3
FORWARD = 2
FORM_CASES = ["out_hallway_s7", "out_mazes2_s0", "out_oneroom_len_t_s1", "out_sign_box_s0", "out_sign_key_s1", "out_sidewalk_s0",
              "out_sidewalk_street_box", "out_pickup_all_s0", "out_putnext_s3"]
REPEATS = (2, 3)
HORIZON = 4


def end_of(tr, meta):
    return len(tr["action"]) - int(meta["after"])


def repeat_phases(actions, end, K):
    """the positions p (0 = first) the terminal sub-step can take in a step(repeat=K) call under the fixture's own actions: a call
    repeats ONE action, so the p steps before the terminal one must have taken it too"""
    return [p for p in range(K) if end - 1 - p >= 0 and len(set(int(a) for a in actions[end - 1 - p:end])) == 1]


def _vec(case, **more):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    s0, tr, meta, obs = helpers.load_case(case)
    vec = MiniWorldVecEnv("MiniWorld-%s-v0" % str(meta["env"]), N, seed=int(meta["seed"]), **helpers.env_kwargs_of(meta), **more)
    assert vec.rng_mode == "pcg64"
    return vec, tr, meta, obs, end_of(tr, meta)


def _act(a):
    import torch
    return torch.full((N,), int(a), dtype=torch.int32, device="cuda")


def _replay(vec, meta, actions):
    """the fixture's episode from its start: reset(seed) and single steps"""
    vec.reset(seed=int(meta["seed"]))
    for a in actions:
        vec.step(_act(a))


def _pose_error(st, tr, t):
    return max(np.abs(st["agent_pos"][0] - tr["pos"][t]).max(), abs(st["agent_dir"][0] - tr["dir"][t]))


@pytest.mark.parametrize("case", FORM_CASES)
def test_repeat_call_that_holds_the_terminal_substep(case):
    """step(a, repeat=K) with the terminal sub-step first, in the middle and last in its call, as far as the fixture's actions allow
    (tests/test_outcome_fixtures_cpu.py asserts that the cases together allow every position): the reward is float32 of the double
    sum of the reference's rewards of the executed sub-steps, the flags are the terminal step's, `substeps` counts what ran, and
    the env stands where the reference's terminal step left it."""
    vec, tr, meta, obs, end = _vec(case, autoreset=False)
    done = 0
    for K in REPEATS:
        for p in repeat_phases(tr["action"], end, K):
            first = end - 1 - p
            _replay(vec, meta, tr["action"][:first])
            o, rew, term, trunc = vec.step(_act(tr["action"][end - 1]), repeat=K)
            tag = (case, K, p)
            want = np.float32(sum(float(x) for x in tr["reward"][first:end]))
            print(tag, "reward", rew[0].item(), "want", want, "substeps", vec.substeps[0].item())
            assert rew[0].item() == want, tag
            assert bool(term[0].item()) == bool(tr["term"][end - 1]) and bool(trunc[0].item()) == bool(tr["trunc"][end - 1]), tag
            assert vec.substeps[0].item() == p + 1, tag
            st = vec.engine.get_state()
            assert _pose_error(st, tr, end - 1) < 1e-12 and int(st["step_count"][0]) == end, tag
            assert np.array_equal(o[0].cpu().numpy(), obs[end]["rgb"]), tag + ("the terminal frame",)
            done += 1
    assert done >= 2, (case, "no repeat call was checked")
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("case", FORM_CASES)
def test_traced_rollout_that_holds_the_terminal_step(case):
    """rollout(plans[4, N], trace=True) with the terminal step in each of its four rows: step_rewards rows are the reference's rewards
    and zero behind the end, the trace rows its poses within the suite's 1e-12 (rows behind the end repeat the terminal one)."""
    import torch
    vec, tr, meta, obs, end = _vec(case, autoreset=False)
    for q in range(min(HORIZON, end)):
        first = end - 1 - q
        _replay(vec, meta, tr["action"][:first])
        plan = [int(a) for a in tr["action"][first:end]] + [FORWARD] * (HORIZON - 1 - q)
        plans = torch.tensor(plan, dtype=torch.int32, device="cuda")[:, None].repeat(1, N).contiguous()
        o, rew, term, trunc = vec.rollout(plans, trace=True)
        tag = (case, q)
        rows = vec.step_rewards[:, 0].cpu().numpy()
        want = np.zeros(HORIZON, np.float32)
        want[:q + 1] = tr["reward"][first:end]
        print(tag, "step_rewards", rows, "want", want)
        assert np.array_equal(rows, want), tag
        assert rew[0].item() == np.float32(sum(float(x) for x in tr["reward"][first:end])), tag
        assert bool(term[0].item()) == bool(tr["term"][end - 1]) and bool(trunc[0].item()) == bool(tr["trunc"][end - 1]), tag
        assert vec.substeps[0].item() == q + 1, tag
        pos, d, carry = (vec.trace[k][:, 0].cpu().numpy() for k in ("agent_pos", "agent_dir", "carrying"))
        for k in range(HORIZON):
            t = min(first + k, end - 1)
            assert np.abs(pos[k] - tr["pos"][t]).max() < 1e-12 and abs(d[k] - tr["dir"][t]) < 1e-12 and carry[k] == tr["carrying"][t], tag + (k,)
        assert np.array_equal(o[0].cpu().numpy(), obs[end]["rgb"]), tag + ("the terminal frame",)
    vec.engine.check()
    vec.close()


def _assert_next_world(vec, case, tag):
    """env 0 holds s1/: the world the reference's env.reset() built behind the fixture's last step, and shows its first frame"""
    import pyoracle
    from test_outcome_fixtures_cpu import next_world_of
    d = np.load(helpers.GOLDEN + "/" + case + ".npz")
    s1 = {k[3:]: d[k] for k in d.files if k.startswith("s1/")}
    st = vec.engine.get_state()
    helpers.assert_world_equal(helpers.world_of_scene(helpers.scene_of_vec_env(vec, st, 0)), next_world_of(case), tag)
    assert int(st["step_count"][0]) == 0 and int(st["carrying"][0]) == -1, tag
    want = pyoracle.render(s1, meshes=helpers.golden_meshes(s1))["rgb"]
    assert np.array_equal(vec.obs[0].cpu().numpy(), want), tag + ("the next world's first frame",)


@pytest.mark.parametrize("mode,final_obs", [("same_step", False), ("same_step", True), ("next_step", False)])
@pytest.mark.parametrize("case", FORM_CASES)
def test_autoreset_across_the_outcome_installs_the_references_next_world(case, mode, final_obs):
    """The fixture's episode under the same-step auto-reset (without and with final_obs) and the next-step one: reward and flags of the
    ending step, the terminal observation bit-equal to the fixture's terminal frame where the mode returns one (final_obs; the
    next-step mode's own observation), and the world installed behind it bit-equal to s1/ — the stream's continuity across an
    outcome, against the reference itself and not against the host classes.  (Without domain randomisation the steps that
    out_pickup_all_s0 takes past its end draw nothing, so its s1/ is also the world behind the terminal step.)"""
    vec, tr, meta, obs, end = _vec(case, autoreset=mode, final_obs=final_obs)
    assert not bool(meta["domain_rand"])
    vec.reset()
    for t in range(end):
        o, rew, term, trunc = vec.step(_act(tr["action"][t]))
        if t < end - 1:
            assert rew[0].item() == np.float32(tr["reward"][t]) and not term[0].item() and not trunc[0].item(), (case, mode, t)
    tag = (case, mode, final_obs)
    print(tag, "reward", rew[0].item(), "want", np.float32(tr["reward"][end - 1]), "flags", term[0].item(), trunc[0].item())
    assert rew[0].item() == np.float32(tr["reward"][end - 1]), tag
    assert bool(term[0].item()) == bool(tr["term"][end - 1]) and bool(trunc[0].item()) == bool(tr["trunc"][end - 1]), tag
    if mode == "next_step":
        assert np.array_equal(o[0].cpu().numpy(), obs[end]["rgb"]), tag + ("the terminal frame",)
        assert vec.reset_pending()[0].item() == 1, tag
        o, rew, term, trunc = vec.step(_act(FORWARD))
        assert rew[0].item() == 0 and not term[0].item() and not trunc[0].item(), tag
    elif final_obs:
        assert np.array_equal(vec.final_obs[0].cpu().numpy(), obs[end]["rgb"]), tag + ("the terminal frame",)
    _assert_next_world(vec, case, tag)
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("case", ["out_pickup_all_s0", "out_pickup_all_dr_s1"])
def test_pickupobjects_steps_in_the_emptied_room(case):
    """PickupObjects past its last pickup (no auto-reset: the caller steps on): no mesh entity is left, the frames are the
    fixture's bit for bit and come from the raster kernels that drew the populated room, and the engine's checks stay clean."""
    vec, tr, meta, obs, end = _vec(case, autoreset=False)
    after = int(meta["after"])
    assert after >= 3
    vec.reset()
    populated = None
    for t in range(end + after):
        o, rew, term, trunc = vec.step(_act(tr["action"][t]))
        if t == 0:
            populated = vec.engine.raster_path()
        assert rew[0].item() == np.float32(tr["reward"][t]), (case, t)
        assert bool(term[0].item()) == bool(tr["term"][t]) and bool(trunc[0].item()) == bool(tr["trunc"][t]), (case, t)
        if t + 1 in obs:
            assert np.array_equal(o[0].cpu().numpy(), obs[t + 1]["rgb"]), (case, t + 1)
        if t >= end:
            assert vec.engine.raster_path() == populated, (case, t, vec.engine.raster_path(), populated)
    st = vec.engine.get_state()
    assert not st["ent_kind"][0].any() and _pose_error(st, tr, end + after - 1) < 1e-12
    vec.engine.check()
    vec.close()
