"""The device generators' placement tests against the reference's float32 sums of radii (GPU box): tests/golden/placement/*.npz,
written by tools/gen_placement_fixtures.py from the reference's own reset() and pinned on the CPU by tests/test_placement_cpu.py.

Every fixture is a world whose generation hangs on one test of place_entity: the candidate's distance to an entity lies strictly
between the float32 sum of the two radii — what the reference forms where a MeshEnt takes part (miniworld.py:960) — and their
float64 sum.  A generator that adds the other way takes the other decision there, draws on, and ends with another world
(test_placement_cpu.py shows that for every mesh case); the control cases (boxes and the agent only: the reference adds in double)
fail for a generator that adds in float32 everywhere, and the RoomObjects one, where the agent's radius 1.5 is exact in float32, for
one that decides by the value instead of the kind.  Batches of three, seeded with the case's seed - 1: the crafted env is the middle one.
The state the device holds is compared with the fixture by exact equality, in the fields _assert_same_world (test_gpu_env_api.py)
compares, through every way an episode can start: the plain reset, the unseeded reset and K1's same-step install (spare worlds off
and on: the refill kernel's copy of the generator), reset_where, the seeded auto-reset, a level bank — and CollectHealth's respawn
kernel, which places a kit AFTER the agent (the agent branch of the device's test).

Only the PCG64 stream has a reference to compare with; the Philox stream's worlds are the engine's own and are not covered here."""
import pytest

import helpers

pytestmark = pytest.mark.gpu

N, MID = 3, 1
CASES = helpers.placement_cases()
META = {c: helpers.load_placement_case(c)[2] for c in CASES}
RESET_CASES = [c for c in CASES if not c.startswith("respawn")]
SECOND_EPISODE = [c for c in RESET_CASES if int(META[c]["resets_before"]) == 1]
# one plain mesh case per site of the device code: gen_place (PickupObjects), prog_blocked in the dense K1's family (RoomObjects)
# and in a wave-per-env family (CollectHealth)
SEEDED = [next(c for c in RESET_CASES if c.startswith(p) and not int(META[c]["resets_before"]) and not int(META[c]["domain_rand"]))
          for p in ("pickupobjects", "roomobjects", "collecthealth")]


def _vec(name, seed=None, episode_steps=None, monkeypatch=None, **more):
    """A batch of three of the case's family and constructor arguments, seeded so that env MID gets the case's seed (or with `seed`).
    episode_steps: the engine's max_episode_steps (the families' constructors fix their own: RoomObjects' episodes never end)."""
    from miniworld_amd import vec_env
    meta = META[name]
    if episode_steps is not None:
        real = vec_env.build_config

        def short_episodes(*a, **k):
            setup = real(*a, **k)
            setup.cfg.max_episode_steps = episode_steps
            return setup
        monkeypatch.setattr(vec_env, "build_config", short_episodes)
    vec = vec_env.MiniWorldVecEnv("MiniWorld-%s-v0" % str(meta["env"]), N, seed=int(meta["seed"]) - 1 if seed is None else seed,
                                  **helpers.env_kwargs_of(meta), **more)
    assert vec.rng_mode == "pcg64"
    return vec


def _dense_lanes(vec):
    """k1_dense_lanes (mw_policy.h) of this engine's configuration, asked as tests/test_launch_policy_cpu.py does"""
    from test_launch_policy_cpu import LANES, ask, policy_lib
    c = vec.engine.cfg
    return ask(policy_lib(), LANES, [c.max_polys, c.max_ents, c.max_visible, c.task, 16, 75])[1]


def _assert_fixture_world(vec, name, env=MID):
    st = vec.engine.get_state()
    got = helpers.world_of_scene(helpers.scene_of_vec_env(vec, st, env))
    helpers.assert_world_equal(got, helpers.load_placement_case(name)[0], (name, env))
    vec.engine.check()


def _turn(vec, steps):
    import torch
    act = torch.zeros(N, dtype=torch.int32, device="cuda")      # turn left: no move, no pickup, and without DR no draw
    for _ in range(steps):
        out = vec.step(act)
    return out


def test_the_cases_take_both_forms_of_the_step_kernel():
    """RoomObjects packs into the dense K1 (the env's leading lane installs a world); PickupObjects, CollectHealth and PutNext take the
    wave-per-env form."""
    lanes = {}
    for name in SEEDED + [c for c in RESET_CASES if c.startswith("putnext")][:1]:
        vec = _vec(name, autoreset=False)
        lanes[str(META[name]["env"])] = _dense_lanes(vec)
        vec.close()
    assert lanes["RoomObjects"] > 0 and 64 // lanes["RoomObjects"] >= 2, lanes
    assert lanes["PickupObjects"] == 0 and lanes["CollectHealth"] == 0 and lanes["PutNext"] == 0, lanes


@pytest.mark.parametrize("name", RESET_CASES)
def test_reset_holds_the_fixture_world(name):
    """MiniWorldVecEnv(..., seed=, **kwargs).reset(), and for the second-episode cases engine.reset(None, None) behind it."""
    vec = _vec(name, autoreset=False)
    vec.reset()
    for _ in range(int(META[name]["resets_before"])):
        vec.engine.reset(None, None)
    _assert_fixture_world(vec, name)
    vec.close()


@pytest.mark.parametrize("spare", ["0", "1"])
@pytest.mark.parametrize("how", ["reset", "install"])
@pytest.mark.parametrize("name", SECOND_EPISODE)
def test_second_episode_holds_the_fixture_world(name, how, spare, monkeypatch):
    """The episode after reset(seed), where the deciding test lies: through the unseeded reset and through K1's same-step install at
    the end of a two-step episode of turns, without spare worlds (the generator runs in the reset kernel / inside K1) and with
    them (it ran in the refill blocks, the episode's end copies the spare in)."""
    monkeypatch.setenv("MW_SPARE", spare)
    if how == "reset":
        vec = _vec(name, autoreset=False)
        vec.reset()
        vec.engine.reset(None, None)
    else:
        vec = _vec(name, episode_steps=2, monkeypatch=monkeypatch)
        vec.reset()
        _, _, term, trunc = _turn(vec, 2)
        assert bool(trunc.bool().all()) and not bool(term.bool().any())
    _assert_fixture_world(vec, name)
    vec.close()


@pytest.mark.parametrize("name", SEEDED)
def test_reset_where_holds_the_fixture_world(name):
    vec = _vec(name, seed=1000, autoreset=False)
    vec.reset()
    vec.reset_where([0, 1, 0], [0, int(META[name]["seed"]), 0])
    _assert_fixture_world(vec, name)
    vec.close()


@pytest.mark.parametrize("name", SEEDED)
def test_seeded_auto_reset_holds_the_fixture_world(name, monkeypatch):
    """autoreset="seeds" (mw_set_reset_seeds): the env whose episode ends starts the episode of next_seed[i] in that step."""
    vec = _vec(name, seed=1000, episode_steps=2, monkeypatch=monkeypatch, autoreset="seeds")
    vec.reset()
    vec.next_seed[MID] = int(META[name]["seed"])
    _, _, _, trunc = _turn(vec, 2)
    assert bool(trunc.bool().all()) and int(vec.episode_seed[MID]) == int(META[name]["seed"])
    _assert_fixture_world(vec, name)
    vec.close()


@pytest.mark.parametrize("name", SEEDED)
def test_a_level_of_the_seed_holds_the_fixture_world(name):
    """A level bank whose record 1 is the case's seed (make_levels: the seeded reset, then the snapshot), played by every env."""
    s = int(META[name]["seed"])
    vec = _vec(name, seed=1000, autoreset="levels")
    vec.set_levels(vec.make_levels([s + 7, s, s + 11]))
    vec.next_level.fill_(1)
    vec.reset()
    assert vec.level.tolist() == [1] * N
    for env in (0, MID):
        _assert_fixture_world(vec, name, env)
    vec.close()


def test_respawn_holds_the_fixture_world():
    """CollectHealth's respawn (mw_collect_respawn_kernel): from the injected state one pickup step consumes kit 0 and places it again,
    after the agent in the list; its first candidate lies between the two sums of the kit's radius and the agent's, the reference
    rejects it (the float32 sum is the larger one) and draws on."""
    import torch
    name = "respawn_0"
    _, case, meta, poke = helpers.load_placement_case(name)
    assert str(case["other"]) == "Agent" and bool(case["ref_rejects"])
    vec = _vec(name, autoreset=False)
    assert _dense_lanes(vec) == 0
    vec.reset()
    st = vec.engine.get_state()
    E = len(poke["ents_dir"])
    st["agent_pos"][MID], st["agent_dir"][MID] = poke["agent_pos"], poke["agent_dir"]
    st["ent_pos"][MID, :E], st["ent_dir"][MID, :E] = poke["ents_pos"], poke["ents_dir"]
    vec.engine.set_state(st)
    vec.step(torch.tensor([0, int(poke["action"]), 0], dtype=torch.int32, device="cuda"))
    assert int(vec.infos()["health"][MID]) == 100          # the kit was consumed
    _assert_fixture_world(vec, name)
    vec.close()
