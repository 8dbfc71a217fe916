"""Every argument check of MiniWorldVecEnv as a row of a table, over the stub engine (helpers.stub_engine), CPU tensors: a label, the
env the call is made on, the call, and what comes of it — the exception's type (ValueError, RuntimeError, or KeyError for an unknown
id) or None for a call that is accepted — with the library calls made meanwhile, by name: none before a refusal, unless the row says
otherwise (the constructor's frame_cache check comes after the assets are uploaded).  The rows were read off vec_env.py before it was
split into modules and its scalar checks became one helper per rule; the accepting rows pin what a uniform rule would be tempted to
refuse (integer-valued arguments, numpy scalars) and the library calls they lead to.  Three things changed with the helpers, and only
their rows were flipped (marked "was:" below): a bool is no number anywhere (nav_field's cell, margin and reach took True as 1), a
margin or reach that is no number is a ValueError like every other argument (it was the TypeError of the comparison), and a numpy
real scalar that is no Python float (np.float32, np.int64) is a number for every real argument, as it was for margin and reach.

Not covered: a snapshot on another device in set_levels and load_state is moved, not refused; the one refusal of that kind,
save_state(into=<a snapshot elsewhere>), is reached with a tensor on the "meta" device.  Engine's own tensor checks (EngineError) are
tests/test_engine_refusals_cpu.py's."""
import math

import numpy as np
import pytest
import torch

from helpers import stub_engine

N = 4
HALLWAY = "MiniWorld-Hallway-v0"
ENVS = {"plain": (HALLWAY, {}),
        "stack": (HALLWAY, dict(frame_stack=2)),
        "levels": (HALLWAY, dict(autoreset="levels")),
        "banked": (HALLWAY, dict(autoreset="levels")),          # "levels" after set_levels
        "seeds": (HALLWAY, dict(autoreset="seeds")),
        "collect": ("MiniWorld-CollectHealth-v0", {})}
RETURNS = {"mw_snapshot_bytes": 4096, "mw_snapshot_frames_bytes": 8192}
F64, F32, I32, I64, U8 = torch.float64, torch.float32, torch.int32, torch.int64, torch.uint8


def mod():
    from miniworld_amd import vec_env
    return vec_env


def eng():
    from miniworld_amd import engine
    return engine


def new(env_id=HALLWAY, **kw):
    return mod().MiniWorldVecEnv(env_id, N, seed=3, **kw)


def z(shape, dtype=F64):
    return torch.zeros(shape, dtype=dtype)


def plans(T=3, n=N):
    return z((T, n), I64)


def snap(frames=False, flags=0, stack=0, count=1, capacity=4, device="cpu"):
    return mod().EnvSnapshot(torch.zeros(64, dtype=U8, device=device), count, capacity, z(64, U8) if frames else None, flags, stack)


def no_goal(v, call):
    """`call` on an env whose configuration names no goal entity"""
    keep, v.engine.cfg.goal_ent = v.engine.cfg.goal_ent, -1
    try:
        return call()
    finally:
        v.engine.cfg.goal_ent = keep


def field(v):
    return v.nav_field(target=0)


def points():
    return z((N, 3))


BUILD = ["mw_nav_build"]
CAST = ["mw_ray_cast"]
V, R, K = ValueError, RuntimeError, KeyError
CONSTRUCTED = ["mw_upload_texture"] * 3 + ["mw_set_geometry", "mw_set_obs_layout", "mw_set_frame_reuse"]      # what Hallway's constructor calls before frame_cache is looked at

# (label, env, call(v), exception type or None, library calls by name)
TABLE = [
    # ---- the constructor
    ("frame_stack True", None, lambda v: new(frame_stack=True), V, []),
    ("frame_stack 1", None, lambda v: new(frame_stack=1), V, []),
    ("frame_stack 17", None, lambda v: new(frame_stack=17), V, []),
    ("frame_stack 2.0", None, lambda v: new(frame_stack=2.0), V, []),
    ("frame_stack '3'", None, lambda v: new(frame_stack="3"), V, []),
    ("stack_pad", None, lambda v: new(stack_pad="edge"), V, []),
    ("autoreset unknown", None, lambda v: new(autoreset="sometimes"), V, []),
    ("autoreset 1", None, lambda v: new(autoreset=1), V, []),
    ("final_obs next_step", None, lambda v: new(autoreset="next_step", final_obs=True), V, []),
    ("final_obs levels", None, lambda v: new(autoreset="levels", final_obs=True), V, []),
    ("final_obs off", None, lambda v: new(autoreset=False, final_obs=True), V, []),
    ("obs_layout", None, lambda v: new(obs_layout="chw"), V, []),
    ("env_id unknown", None, lambda v: new("MiniWorld-Nowhere-v0"), K, []),
    ("rng unknown", None, lambda v: new(rng="mt19937"), V, []),
    ("frame_cache True", None, lambda v: new(frame_cache=True), V, CONSTRUCTED),
    ("frame_cache -1", None, lambda v: new(frame_cache=-1), V, CONSTRUCTED),
    ("frame_cache 9", None, lambda v: new(frame_cache=9), V, CONSTRUCTED),
    ("frame_cache 2.0", None, lambda v: new(frame_cache=2.0), V, CONSTRUCTED),
    ("frame_cache np.int64(2) accepted", None, lambda v: new(frame_cache=np.int64(2)), None, CONSTRUCTED + ["mw_set_frame_cache"]),
    ("frame_stack np.int64(2) accepted", None, lambda v: new(frame_stack=np.int64(2)), None, CONSTRUCTED + ["mw_set_frame_cache", "mw_set_frame_stack"]),
    # ---- reset, reset_where
    ("reset seeds negative", "seeds", lambda v: v.reset(seed=-1), V, []),
    ("reset seeds past 2^63", "seeds", lambda v: v.reset(seed=2 ** 63 - 2 * N + 1), V, []),
    ("reset levels before set_levels", "levels", lambda v: v.reset(), R, []),
    ("reset_where negative in a list", "plain", lambda v: v.reset_where([1, 0, 0, 0], [-1, 0, 0, 0]), V, []),
    ("reset_where 2^64 in a list", "plain", lambda v: v.reset_where([1, 0, 0, 0], [2 ** 64, 0, 0, 0]), V, []),
    ("reset_where negative in a host tensor", "plain", lambda v: v.reset_where([1, 0, 0, 0], torch.tensor([5, -1, 0, 0])), V, []),
    ("reset_where 2^64 - 1 accepted", "plain", lambda v: v.reset_where([1, 0, 0, 0], [2 ** 64 - 1, 0, 0, 0]), None, ["mw_reset_where", "mw_render"]),
    # ---- step, rollout
    ("step levels before set_levels", "levels", lambda v: v.step(z(N, I64)), R, []),
    ("rollout levels before set_levels", "levels", lambda v: v.rollout(plans()), R, []),
    ("rollout trace a string", "plain", lambda v: v.rollout(plans(), trace="agent_pos"), V, []),
    ("rollout trace empty", "plain", lambda v: v.rollout(plans(), trace=()), V, []),
    ("rollout trace unknown name", "plain", lambda v: v.rollout(plans(), trace=("agent_pos", "velocity")), V, []),
    ("rollout trace ent_pos on CollectHealth", "collect", lambda v: v.rollout(plans(), trace=("ent_pos",)), V, []),
    ("rollout trace_ent True", "plain", lambda v: v.rollout(plans(), trace=("ent_pos",), trace_ent=True), V, []),
    ("rollout trace_ent -1", "plain", lambda v: v.rollout(plans(), trace=("ent_pos",), trace_ent=-1), V, []),
    ("rollout trace_ent max_ents", "plain", lambda v: v.rollout(plans(), trace=("ent_pos",), trace_ent=int(v.engine.cfg.max_ents)), V, []),
    ("rollout trace_ent 0.0", "plain", lambda v: v.rollout(plans(), trace=("ent_pos",), trace_ent=0.0), V, []),
    ("rollout trace_ent np.int64(0) accepted", "plain", lambda v: v.rollout(plans(), trace=("ent_pos",), trace_ent=np.int64(0)), None, ["mw_step_plan_trace"]),
    ("rollout trace_ent unread without ent_pos", "plain", lambda v: v.rollout(plans(), trace=True, trace_ent=-1), None, ["mw_step_plan_trace"]),
    ("rollout plans 1-D", "plain", lambda v: v.rollout(z(N, I64)), V, []),
    ("rollout plans of another N", "plain", lambda v: v.rollout(plans(n=N + 1)), V, []),
    ("rollout T 0", "plain", lambda v: v.rollout(plans(T=0)), V, []),
    ("rollout T 257", "plain", lambda v: v.rollout(plans(T=257)), V, []),
    ("rollout render=False with seeds", "seeds", lambda v: v.rollout(plans(), render=False), V, []),
    # ---- make_levels, set_levels
    ("make_levels 2-D", "plain", lambda v: v.make_levels([[1, 2]]), V, []),
    ("make_levels empty", "plain", lambda v: v.make_levels([]), V, []),
    ("make_levels floats", "plain", lambda v: v.make_levels([1.0, 2.0]), V, []),
    ("make_levels negative", "plain", lambda v: v.make_levels([1, -2]), V, []),
    ("make_levels negative tensor", "plain", lambda v: v.make_levels(torch.tensor([1, -2])), V, []),
    ("set_levels in another mode", "plain", lambda v: v.set_levels(snap(frames=True)), R, []),
    ("set_levels without frame records", "levels", lambda v: v.set_levels(snap()), V, []),
    ("set_levels frames of another configuration", "levels", lambda v: v.set_levels(snap(frames=True, flags=eng().SNAPF_DEPTH)), V, []),
    ("set_levels frames of another stack depth", "levels", lambda v: v.set_levels(snap(frames=True, flags=eng().SNAPF_STACK, stack=3)), V, []),
    ("set_levels no records", "levels", lambda v: v.set_levels(snap(frames=True, count=0)), V, []),
    # ---- save_state, load_state
    ("save_state records without into", "plain", lambda v: v.save_state(records=[0, 1, 2, 3]), V, []),
    ("save_state capacity below the count", "plain", lambda v: v.save_state(capacity=N - 1), V, []),
    ("save_state into with capacity", "plain", lambda v: v.save_state([0], into=snap(), records=[0], capacity=4), V, []),
    ("save_state into without records", "plain", lambda v: v.save_state([0], into=snap()), V, []),
    ("save_state into frames of another configuration", "plain", lambda v: v.save_state([0], into=snap(frames=True, flags=eng().SNAPF_DEPTH), records=[0]), V, []),
    ("save_state into records of another length", "plain", lambda v: v.save_state([0, 1], into=snap(), records=[0]), V, []),
    ("save_state into records 2-D", "plain", lambda v: v.save_state([0, 1], into=snap(), records=[[0, 1]]), V, []),
    ("save_state into more than the capacity", "plain", lambda v: v.save_state([0, 1], into=snap(capacity=1), records=[0, 1]), V, []),
    ("save_state into a snapshot elsewhere", "plain", lambda v: v.save_state([0], into=snap(device="meta"), records=[0]), V, []),
    ("load_state frames=True without frame records", "plain", lambda v: v.load_state(snap(), frames=True), V, []),
    ("load_state frames of another configuration", "plain", lambda v: v.load_state(snap(frames=True, flags=eng().SNAPF_STACK, stack=2)), V, []),
    # ---- state, set_state_where
    ("state unknown field", "plain", lambda v: v.state(("agent_pos", "velocity")), V, []),
    ("state no field", "plain", lambda v: v.state(()), V, []),
    ("set_state_where no field", "plain", lambda v: v.set_state_where([1, 0, 0, 0]), V, []),
    ("set_state_where unknown field", "plain", lambda v: v.set_state_where([1, 0, 0, 0], velocity=[0.0] * N), V, []),
    # ---- nav_field
    ("nav_field into no NavField", "plain", lambda v: v.nav_field(into={}), V, []),
    ("nav_field into with a target", "plain", lambda v: v.nav_field(target=0, into=field(v)), V, BUILD),       # (the build is field()'s)
    ("nav_field into with a cell", "plain", lambda v: v.nav_field(cell=0.5, into=field(v)), V, BUILD),
    ("nav_field into with a margin", "plain", lambda v: v.nav_field(margin=0.1, into=field(v)), V, BUILD),
    ("nav_field into with a reach", "plain", lambda v: v.nav_field(reach=1.0, into=field(v)), V, BUILD),
    ("nav_field into with obstacles", "plain", lambda v: v.nav_field(obstacles="walls+entities", into=field(v)), V, BUILD),
    ("nav_field obstacles", "plain", lambda v: v.nav_field(obstacles="entities"), V, []),
    ("nav_field cell 0", "plain", lambda v: v.nav_field(cell=0), V, []),
    ("nav_field cell -1", "plain", lambda v: v.nav_field(cell=-1.0), V, []),
    ("nav_field cell inf", "plain", lambda v: v.nav_field(cell=math.inf), V, []),
    ("nav_field cell nan", "plain", lambda v: v.nav_field(cell=math.nan), V, []),
    ("nav_field cell '0.25'", "plain", lambda v: v.nav_field(cell="0.25"), V, []),
    ("nav_field cell True", "plain", lambda v: v.nav_field(cell=True), V, []),                                  # was: None, BUILD
    ("nav_field cell np.float32", "plain", lambda v: v.nav_field(cell=np.float32(0.5)), None, BUILD),          # was: V, []
    ("nav_field cell 1 accepted", "plain", lambda v: v.nav_field(cell=1), None, BUILD),
    ("nav_field cell np.float64 accepted", "plain", lambda v: v.nav_field(cell=np.float64(0.5)), None, BUILD),
    ("nav_field margin -1", "plain", lambda v: v.nav_field(margin=-1.0), V, []),
    ("nav_field margin nan", "plain", lambda v: v.nav_field(margin=math.nan), V, []),
    ("nav_field margin inf", "plain", lambda v: v.nav_field(margin=math.inf), V, []),
    ("nav_field margin '1'", "plain", lambda v: v.nav_field(margin="1"), V, []),                                # was: TypeError, []
    ("nav_field margin True", "plain", lambda v: v.nav_field(margin=True), V, []),                              # was: None, BUILD
    ("nav_field margin 0 accepted", "plain", lambda v: v.nav_field(margin=0), None, BUILD),
    ("nav_field margin np.float32 accepted", "plain", lambda v: v.nav_field(margin=np.float32(0.1)), None, BUILD),
    ("nav_field no goal entity", "plain", lambda v: no_goal(v, lambda: v.nav_field()), V, []),
    ("nav_field points float32", "plain", lambda v: v.nav_field(target=z((N, 3), F32), reach=1.0), V, []),
    ("nav_field points of another shape", "plain", lambda v: v.nav_field(target=z((N, 2)), reach=1.0), V, []),
    ("nav_field points without reach", "plain", lambda v: v.nav_field(target=points()), V, []),
    ("nav_field points reach 0", "plain", lambda v: v.nav_field(target=points(), reach=0.0), V, []),
    ("nav_field points reach -1", "plain", lambda v: v.nav_field(target=points(), reach=-1.0), V, []),
    ("nav_field points reach inf", "plain", lambda v: v.nav_field(target=points(), reach=math.inf), V, []),
    ("nav_field points reach 'far'", "plain", lambda v: v.nav_field(target=points(), reach="far"), V, []),      # was: TypeError, []
    ("nav_field points reach True", "plain", lambda v: v.nav_field(target=points(), reach=True), V, []),        # was: None, BUILD
    ("nav_field points reach 1 accepted", "plain", lambda v: v.nav_field(target=points(), reach=1), None, BUILD),
    ("nav_field points reach np.float32 accepted", "plain", lambda v: v.nav_field(target=points(), reach=np.float32(0.5)), None, BUILD),
    ("nav_field slot -1", "plain", lambda v: v.nav_field(target=-1), V, []),
    ("nav_field slot max_ents", "plain", lambda v: v.nav_field(target=int(v.engine.cfg.max_ents)), V, []),
    ("nav_field slot with reach", "plain", lambda v: v.nav_field(target=0, reach=1.0), V, []),
    ("nav_field slot np.int64 accepted", "plain", lambda v: v.nav_field(target=np.int64(0)), None, BUILD),
    ("nav_field target a name", "plain", lambda v: v.nav_field(target="box"), V, []),
    ("nav_field target 0.0", "plain", lambda v: v.nav_field(target=0.0), V, []),
    ("nav_field target True", "plain", lambda v: v.nav_field(target=True), V, []),
    ("nav_field too many cells", "plain", lambda v: v.nav_field(cell=0.01), V, []),
    ("nav_field mask float", "plain", lambda v: v.nav_field(mask=z(N)), V, []),
    ("nav_field mask of another length", "plain", lambda v: v.nav_field(mask=z(N + 1, U8)), V, []),
    ("nav_field mask a list", "plain", lambda v: v.nav_field(mask=[1, 0, 1, 0]), V, []),
    ("nav_field mask bool accepted", "plain", lambda v: v.nav_field(mask=z(N, torch.bool)), None, BUILD),
    # ---- nav_query
    ("nav_query no NavField", "plain", lambda v: v.nav_query(None), V, []),
    ("nav_query pos float32", "plain", lambda v: v.nav_query(field(v), pos=z((N, 3), F32)), V, BUILD),
    ("nav_query pos of another shape", "plain", lambda v: v.nav_query(field(v), pos=z((N, 2))), V, BUILD),
    # ---- seen_map, seen_update
    ("seen_map obstacles", "plain", lambda v: v.seen_map(obstacles="entities"), V, []),
    ("seen_map max_range 0", "plain", lambda v: v.seen_map(max_range=0), V, []),
    ("seen_map max_range -1", "plain", lambda v: v.seen_map(max_range=-1.0), V, []),
    ("seen_map max_range inf", "plain", lambda v: v.seen_map(max_range=math.inf), V, []),
    ("seen_map max_range True", "plain", lambda v: v.seen_map(max_range=True), V, []),
    ("seen_map max_range '10'", "plain", lambda v: v.seen_map(max_range="10"), V, []),
    ("seen_map max_range 5 accepted", "plain", lambda v: v.seen_map(max_range=5), None, []),
    ("seen_map fov 0", "plain", lambda v: v.seen_map(fov=0.0), V, []),
    ("seen_map fov 7", "plain", lambda v: v.seen_map(fov=7.0), V, []),
    ("seen_map fov nan", "plain", lambda v: v.seen_map(fov=math.nan), V, []),
    ("seen_map fov True", "plain", lambda v: v.seen_map(fov=True), V, []),
    ("seen_map fov '1'", "plain", lambda v: v.seen_map(fov="1"), V, []),
    ("seen_map fov 2 pi accepted", "plain", lambda v: v.seen_map(fov=2 * math.pi), None, []),
    ("seen_map fov 3 accepted", "plain", lambda v: v.seen_map(fov=3), None, []),
    ("seen_map like no NavField", "plain", lambda v: v.seen_map(like=object()), V, []),
    ("seen_map like with a cell", "plain", lambda v: v.seen_map(cell=0.5, like=field(v)), V, BUILD),
    ("seen_map cell 0", "plain", lambda v: v.seen_map(cell=0.0), V, []),
    ("seen_map cell True", "plain", lambda v: v.seen_map(cell=True), V, []),
    ("seen_map cell inf", "plain", lambda v: v.seen_map(cell=math.inf), V, []),
    ("seen_map cell '1'", "plain", lambda v: v.seen_map(cell="1"), V, []),
    ("seen_map cell 1 accepted", "plain", lambda v: v.seen_map(cell=1), None, []),
    ("seen_map too many cells", "plain", lambda v: v.seen_map(cell=0.01), V, []),
    ("seen_update no SeenMap", "plain", lambda v: v.seen_update(field(v)), V, BUILD),
    ("seen_update clear float", "plain", lambda v: v.seen_update(v.seen_map(), clear=z(N)), V, []),
    ("seen_update clear of another length", "plain", lambda v: v.seen_update(v.seen_map(), clear=z(N + 1, U8)), V, []),
    ("seen_update clear a list", "plain", lambda v: v.seen_update(v.seen_map(), clear=[1, 0, 0, 0]), V, []),
    ("seen_update mask float", "plain", lambda v: v.seen_update(v.seen_map(), mask=z(N)), V, []),
    ("seen_update mask 2-D", "plain", lambda v: v.seen_update(v.seen_map(), mask=z((N, 1), U8)), V, []),
    ("seen_update bool flags accepted", "plain", lambda v: v.seen_update(v.seen_map(), clear=z(N, torch.bool), mask=z(N, torch.bool)), None, ["mw_seen_update"]),
    # ---- raycast, lidar
    ("raycast neither direction nor offsets", "plain", lambda v: v.raycast(), V, []),
    ("raycast both direction and offsets", "plain", lambda v: v.raycast(direction=z((N, 2, 2)), offsets=z(2)), V, []),
    ("raycast offsets float32", "plain", lambda v: v.raycast(offsets=z(3, F32)), V, []),
    ("raycast offsets 2-D", "plain", lambda v: v.raycast(offsets=z((N, 3))), V, []),
    ("raycast direction float32", "plain", lambda v: v.raycast(direction=z((N, 3, 2), F32)), V, []),
    ("raycast direction of another shape", "plain", lambda v: v.raycast(direction=z((N, 3, 3))), V, []),
    ("raycast direction strided", "plain", lambda v: v.raycast(direction=z((N, 3, 4))[..., ::2]), V, []),
    ("raycast no rays", "plain", lambda v: v.raycast(offsets=z(0)), V, []),
    ("raycast 4097 rays", "plain", lambda v: v.raycast(offsets=z(4097)), V, []),
    ("raycast origin of another shape", "plain", lambda v: v.raycast(offsets=z(3), origin=z((N, 2, 3))), V, []),
    ("raycast max_t 0", "plain", lambda v: v.raycast(offsets=z(3), max_t=0), V, []),
    ("raycast max_t inf", "plain", lambda v: v.raycast(offsets=z(3), max_t=math.inf), V, []),
    ("raycast max_t True", "plain", lambda v: v.raycast(offsets=z(3), max_t=True), V, []),
    ("raycast max_t '1'", "plain", lambda v: v.raycast(offsets=z(3), max_t="1"), V, []),
    ("raycast max_t 2 accepted", "plain", lambda v: v.raycast(offsets=z(3), max_t=2), None, CAST),
    ("raycast radius -1", "plain", lambda v: v.raycast(offsets=z(3), radius=-1.0), V, []),
    ("raycast radius inf", "plain", lambda v: v.raycast(offsets=z(3), radius=math.inf), V, []),
    ("raycast radius True", "plain", lambda v: v.raycast(offsets=z(3), radius=True), V, []),
    ("raycast radius 0 accepted", "plain", lambda v: v.raycast(offsets=z(3), radius=0), None, CAST),
    ("raycast obstacles", "plain", lambda v: v.raycast(offsets=z(3), obstacles="entities"), V, []),
    ("raycast mask float", "plain", lambda v: v.raycast(offsets=z(3), mask=z(N)), V, []),
    ("raycast mask of another length", "plain", lambda v: v.raycast(offsets=z(3), mask=z(N - 1, U8)), V, []),
    ("raycast into no dict", "plain", lambda v: v.raycast(offsets=z(3), into=[z((N, 3))]), V, []),
    ("raycast into of the other mode", "plain", lambda v: v.raycast(offsets=z(3), into={"t": z((N, 3)), "hit": z((N, 3), I32)}), V, []),
    ("raycast into of another R", "plain", lambda v: v.raycast(direction=z((N, 3, 2)), into={"t": z((N, 2)), "hit": z((N, 2), I32)}), V, []),
    ("raycast into of another dtype", "plain", lambda v: v.raycast(direction=z((N, 3, 2)), into={"t": z((N, 3)), "hit": z((N, 3), I64)}), V, []),
    ("lidar rays 0", "plain", lambda v: v.lidar(rays=0), V, []),
    ("lidar rays 4097", "plain", lambda v: v.lidar(rays=4097), V, []),
    ("lidar rays True", "plain", lambda v: v.lidar(rays=True), V, []),
    ("lidar rays 8.0", "plain", lambda v: v.lidar(rays=8.0), V, []),
    ("lidar rays np.int64 accepted", "plain", lambda v: v.lidar(rays=np.int64(8)), None, CAST),
    ("lidar fov 0", "plain", lambda v: v.lidar(fov=0), V, []),
    ("lidar fov 7", "plain", lambda v: v.lidar(fov=7.0), V, []),
    ("lidar fov True", "plain", lambda v: v.lidar(fov=True), V, []),
    ("lidar fov 3 accepted", "plain", lambda v: v.lidar(fov=3), None, CAST),
    ("lidar max_range 0", "plain", lambda v: v.lidar(max_range=0.0), V, []),
    ("lidar radius -1", "plain", lambda v: v.lidar(radius=-1.0), V, []),
    ("lidar obstacles", "plain", lambda v: v.lidar(obstacles="entities"), V, []),
]


@pytest.fixture(scope="module")
def stub():
    """(the recording library, the envs of ENVS by name, made on first use)"""
    patch = pytest.MonkeyPatch()
    lib, made = stub_engine(patch, returns=RETURNS), {}

    def env(name):
        if name not in made:
            made[name] = new(ENVS[name][0], **ENVS[name][1])
            if name == "banked":
                made[name].set_levels(made[name].make_levels([1, 2, 3]))
        return made[name]
    yield lib, env
    patch.undo()


def test_the_labels_are_distinct():
    assert len({row[0] for row in TABLE}) == len(TABLE)


@pytest.mark.parametrize("label,env,call,raises,calls", TABLE, ids=[row[0] for row in TABLE])
def test_an_argument_is_refused_or_accepted_as_recorded(label, env, call, raises, calls, stub):
    lib, make = stub
    v = make(env) if env else None
    before = len(lib.calls)
    if raises is None:
        call(v)
    else:
        with pytest.raises(raises) as info:
            call(v)
        assert type(info.value) is raises, (label, info.value)
    assert [name for name, _ in lib.calls[before:] if name not in RETURNS] == calls, label


def test_a_bank_is_needed_only_until_it_is_set(stub):
    lib, make = stub
    v = make("banked")
    before = len(lib.calls)
    v.step(torch.zeros(N, dtype=I64))
    assert [name for name, _ in lib.calls[before:] if name not in RETURNS] == ["mw_step", "mw_snapshot_load_where", "mw_snapshot_load_frames_where"]
