"""A coverage condition on tests/golden/out_*.npz (tools/gen_outcome_fixtures.py): every (family, outcome) of REQUIRED has a
fixture, and the last executed step of each fixture shows the outcome its meta/outcome names — recomputed here in plain Python
from the recorded arrays, so a regenerated file cannot quietly lose what it is there for.  The parametrized tests over
conftest.golden_cases() (oracle, model, step kernel, renderer, both env APIs) then pin every layer on these episodes."""
import numpy as np
import pytest

import helpers
from conftest import golden_cases

PICKUP, DROP = 4, 5

# (env class, domain randomisation, outcome)
REQUIRED = [
    ("Hallway", False, "success"), ("Hallway", True, "success"), ("OneRoomS6", False, "success"), ("OneRoomS6Fast", False, "success"),
    ("MazeS2", False, "success"), ("MazeS3Fast", False, "success"), ("Maze", False, "success"), ("FourRooms", False, "success"),
    ("FourRooms", True, "success"), ("TMazeLeft", False, "success"), ("TMazeRight", False, "success"), ("YMazeRight", False, "success"),
    ("WallGap", False, "success"),
    ("OneRoom", False, "success_and_truncated"), ("OneRoom", False, "truncated_one_short"),
    ("Sign", False, "sign_plus_box"), ("Sign", False, "sign_plus_key"),
    ("Sidewalk", False, "success"), ("Sidewalk", False, "street_and_box"),
    ("PickupObjects", False, "all_collected"), ("PickupObjects", True, "all_collected"),
    ("PutNext", False, "put_next"),
    ("CollectHealth", False, "health_out"), ("CollectHealth", False, "kits_then_health_out"),
]

OUTCOME_CASES = [c for c in golden_cases() if c.startswith("out_")]


def success_reward(step_count, max_episode_steps):
    """MiniWorldEnv._reward (miniworld.py)"""
    return 1.0 - 0.2 * (step_count / max_episode_steps)


def kits_taken(tr, end):
    """CollectHealth: the pickup steps behind which a kit stands somewhere else (consumed and re-placed), and the rewards the
    health bookkeeping (collecthealth.py: -2 a step, 100 again with a kit, 2 while positive, else -100 and the end) gives"""
    health, rewards, taken = 100, [], 0
    for t in range(end):
        health -= 2
        if tr["action"][t] == PICKUP and t > 0 and not np.array_equal(tr["ents_pos"][t][:, [0, 2]], tr["ents_pos"][t - 1][:, [0, 2]]):
            health, taken = 100, taken + 1
        rewards.append(2.0 if health > 0 else -100.0)
    return taken, rewards


def outcome_holds(outcome, tr, meta, end, max_steps):
    """Does step `end` (the count of executed steps) of the trajectory show `outcome`, and no earlier step an end?"""
    r, te, tu = float(tr["reward"][end - 1]), bool(tr["term"][end - 1]), bool(tr["trunc"][end - 1])
    if np.any(tr["term"][:end - 1]) or np.any(tr["trunc"][:end - 1]):
        return False
    if outcome == "success":
        return te and not tu and end < max_steps and r == success_reward(end, max_steps)
    if outcome == "success_and_truncated":
        return te and tu and end == max_steps and r == success_reward(end, max_steps) == 1 - 0.2
    if outcome == "truncated_one_short":
        return not te and tu and end == max_steps and r == 0.0
    if outcome in ("sign_plus_box", "sign_plus_key"):
        kw = helpers.env_kwargs_of(meta)
        return te and not tu and r == 1.0 and kw.get("goal", 0) == (outcome == "sign_plus_key") and tr["action"][end - 1] != 3
    if outcome == "street_and_box":
        in_street = tr["pos"][:end, 0] > 0.0                    # (sidewalk.py: the street is the room x in 0 .. 6)
        return te and not tu and bool(in_street[-1]) and not in_street[:-1].any() and r == 0 + success_reward(end, max_steps)
    if outcome == "all_collected":
        n = len(tr["ents_alive"][0])
        return te and not tu and r == 1.0 and int(np.sum(tr["reward"][:end] == 1.0)) == n and not tr["ents_alive"][end - 1].any() \
            and tr["ents_alive"][end - 2].sum() == 1
    if outcome == "put_next":
        return te and not tu and r == success_reward(end, max_steps) and tr["action"][end - 1] == DROP \
            and (tr["carrying"][:end - 1] == int(meta["goal_ent"])).any() and tr["carrying"][end - 1] == -1
    if outcome in ("health_out", "kits_then_health_out"):
        taken, rewards = kits_taken(tr, end)
        return te and not tu and r == -100.0 and rewards == [float(x) for x in tr["reward"][:end]] \
            and (taken == 0 and end == 50 if outcome == "health_out" else taken >= 4)
    raise KeyError(outcome)


def _end_of(tr, meta):
    return len(tr["action"]) - int(meta["after"])


def test_every_family_outcome_has_a_fixture():
    have = set()
    for case in OUTCOME_CASES:
        s0, tr, meta, obs = helpers.load_case(case)
        have.add((str(meta["env"]), bool(meta["domain_rand"]), str(meta["outcome"])))
    assert sorted(set(REQUIRED) - have) == []
    assert sorted(have - set(REQUIRED)) == [], "a fixture whose outcome the table does not list"


@pytest.mark.parametrize("case", OUTCOME_CASES)
def test_the_last_executed_step_shows_the_outcome(case):
    s0, tr, meta, obs = helpers.load_case(case)
    end = _end_of(tr, meta)
    assert end == int(meta["end"]) and end >= 1
    assert outcome_holds(str(meta["outcome"]), tr, meta, end, float(s0["max_episode_steps"])), (case, tr["reward"][end - 1])
    # the aimed length is the one the batched env is given
    if "max_episode_steps" in helpers.env_kwargs_of(meta):
        assert helpers.env_kwargs_of(meta)["max_episode_steps"] == int(s0["max_episode_steps"])


@pytest.mark.parametrize("case", OUTCOME_CASES)
def test_the_stored_frames_are_first_middle_terminal_and_the_next_world_is_there(case):
    d = np.load(helpers.GOLDEN + "/" + case + ".npz")
    s0, tr, meta, obs = helpers.load_case(case)
    end, after = _end_of(tr, meta), int(meta["after"])
    assert sorted(obs) == sorted({0, end // 2, end, end + after})
    s1 = {k[3:]: d[k] for k in d.files if k.startswith("s1/")}
    assert sorted(s1) == sorted(s0)
    assert int(s1["step_count"]) == 0 and not np.array_equal(s1["agent_pos"], s0["agent_pos"])
    if after:       # PickupObjects: the steps past the end run in a room with no mesh entity (and no entity at all) left
        assert not tr["ents_alive"][end - 1:].any() and not obs[end + after]["ents_kind"].any()
        assert obs[end]["ents_kind"].sum() > 0, "the terminal frame still shows the object its step removed behind the render"


def next_world_of(case):
    """s1/ as helpers.world_of_scene compares worlds"""
    d = np.load(helpers.GOLDEN + "/" + case + ".npz")
    return helpers.world_of_scene({k[3:]: d[k] for k in d.files if k.startswith("s1/")})


@pytest.mark.parametrize("case", [c for c in OUTCOME_CASES if c != "out_collecthealth_kits_s1"])
def test_the_host_class_continues_the_stream_into_the_references_next_world(case):
    """engine_model.ModelEnv (host world generator, the oracle's step, the per-step draws from the env's own stream) seeded like the
    fixture and given its actions; reset() behind the last step must build s1/, the world the reference built there.  (The respawns of
    out_collecthealth_kits_s1 draw from the stream inside the rule, which the model does not hold: the batched env covers it.)"""
    import engine_model
    from miniworld_amd import envs
    from miniworld_amd.scene import scene_from_env
    s0, tr, meta, obs = helpers.load_case(case)
    kw = helpers.env_kwargs_of(meta)
    dr = kw.pop("domain_rand", False)
    cls = getattr(envs, str(meta["env"]))
    if str(meta["env"]) == "Sign":          # (takes no domain_rand argument, sign.py:92-98)
        cls = lambda host_only, domain_rand, **k: getattr(envs, "Sign")(host_only=host_only, **k)     # noqa: E731
    m = engine_model.ModelEnv(cls, int(meta["seed"]), dr, helpers.task_of(meta), **kw)
    for t in range(len(tr["action"])):
        m.substep(int(tr["action"][t]))
        if dr:
            assert abs(m.dyn.ag.dir - tr["dir"][t]) < 1e-12, (case, t)
    m.reset()
    helpers.assert_world_equal(helpers.world_of_scene(scene_from_env(m.h)), next_world_of(case), case)


def test_the_form_cases_allow_every_position_of_the_terminal_substep():
    """tests/test_gpu_outcomes.py puts the terminal sub-step first, in the middle and last in a step(repeat=K) call as far as a
    fixture's own actions allow (a call repeats one action); together its cases must allow every position, in more than one family"""
    from test_gpu_outcomes import FORM_CASES, REPEATS, end_of, repeat_phases
    assert set(FORM_CASES) <= set(OUTCOME_CASES)
    allowed = {}
    for case in FORM_CASES:
        s0, tr, meta, obs = helpers.load_case(case)
        for K in REPEATS:
            for p in repeat_phases(tr["action"], end_of(tr, meta), K):
                allowed.setdefault((K, p), set()).add(str(meta["env"]))
    for K in REPEATS:
        for p in range(K):
            assert len(allowed.get((K, p), ())) >= 2, (K, p, allowed)
