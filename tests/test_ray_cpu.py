"""Ray casts (mw_ray_cast; MiniWorldVecEnv.raycast / lidar) without a GPU.

The arithmetic the kernels inline (miniworld_amd/csrc/mw_ray.h) runs on the host in a program of its own
(tests/hostcheck/ray_cast.cpp), built with the address and undefined-behaviour sanitizers, on worlds the host classes generate; its t
and hit are compared, exactly, with the restatement of tests/ray_reference.py, and the restatement's geometric property check is
applied to them.  Beside that: the ABI names, the launch policy's choice of form, the argument errors of the two vec-env methods over
a stub engine, and the smoothed follower of examples/expert_smooth.py on the oracle's dynamics."""
import math
import os
import re

import numpy as np
import pytest

import nav_reference as nav
import ray_reference as ref
from helpers import stub_engine
from query_checks import (CSRC, ROOT, build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, host_world as _host_world,
                          launch_of, run, world_lines)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("ray_cast", tmp_path_factory.mktemp("ray_cast"))


def _run(program, tmp_path, w, max_t, radius, flags, offsets, origins, dirs):
    lines = [f"{float(max_t)!r} {float(radius)!r} {flags}"] + world_lines(w, carry=True, pose=True, extent=False)
    lines.append(str(len(offsets)))
    lines.append(" ".join(repr(float(v)) for v in offsets))
    lines.append(str(len(origins)))
    lines += [" ".join(repr(float(v)) for v in (*o, *d)) for o, d in zip(origins, dirs)]
    rows = [line.split() for line in run(program, tmp_path / "world.txt", lines)]
    assert len(rows) == len(offsets) + len(origins)
    t = np.array([float.fromhex(x[0]) for x in rows])
    hit = np.array([int(x[1]) for x in rows], np.int32)
    d = np.array([[float.fromhex(x[2]), float.fromhex(x[3])] for x in rows])
    return t, hit, d


def _explicit_rays(rng, w, n=200):
    """origins inside and outside the extent and on walls, directions of any length, a zero direction, NaN rows"""
    ext = w["extent"]
    span = max(ext[1] - ext[0], ext[3] - ext[2])
    o = np.zeros((n, 3))
    o[:, 0], o[:, 2] = rng.uniform(ext[0], ext[1], n), rng.uniform(ext[2], ext[3], n)
    o[:, 1] = rng.uniform(0, 1, n)
    o[100:140, 0] = rng.uniform(ext[0] - span, ext[1] + span, 40)
    o[100:140, 2] = rng.uniform(ext[2] - span, ext[3] + span, 40)
    segs = w["segs"]
    for k in range(140, 170):       # on a wall
        s, u = segs[rng.integers(0, len(segs))], rng.uniform(0, 1)
        o[k, 0], o[k, 2] = s[0] + u * (s[2] - s[0]), s[1] + u * (s[3] - s[1])
    ang = rng.uniform(0, 2 * math.pi, n)
    ln = np.exp(rng.uniform(math.log(0.01), math.log(30.0), n))
    d = np.stack([np.cos(ang) * ln, np.sin(ang) * ln], axis=1)
    d[170:176] = 0.0
    d[176, 0], d[177, 1], o[178, 0], o[179, 2] = np.nan, np.nan, np.nan, np.nan
    return o, d


WORLDS = ["MazeS2", "FourRooms", "YMaze", "Sidewalk", "ThreeRooms"]


@pytest.mark.parametrize("cls_name", WORLDS)
def test_casts_equal_the_restatement_and_hold_the_property(program, tmp_path, cls_name):
    rng = np.random.default_rng(2400)
    offsets = ref.lidar_offsets(256, 2 * math.pi)
    seen_ent = misses = hits = zeros = 0
    for seed in (0, 1):
        env, sc, w = _host_world(cls_name, seed)
        o, d = _explicit_rays(rng, w)
        fan_d = ref.fan_directions(w["agent"][2], offsets)
        fan_o = np.tile([[w["agent"][0], w["agent"][1]]], (len(offsets), 1))
        all_o, all_d = np.concatenate([fan_o, o[:, [0, 2]]]), np.concatenate([fan_d, d])
        for radius in (0.0, 0.2, w["agent_radius"]):
            for entities in (False, True):
                for max_t in (1.5, 100.0):
                    t, hit, used = _run(program, tmp_path, w, max_t, radius, 1 if entities else 0, offsets, o, d)
                    assert np.array_equal(used, all_d, equal_nan=True)          # the fan's directions, bit for bit
                    want_t, want_hit = ref.cast(w, all_o, all_d, max_t, radius, entities)
                    assert np.array_equal(hit, want_hit), ("hits that differ", np.nonzero(hit != want_hit)[0][:8].tolist())
                    assert np.array_equal(t, want_t), ("t that differ", np.nonzero(t != want_t)[0][:8].tolist())
                    assert not np.signbit(t).any()
                    checked, excused = ref.check_property(w, all_o, all_d, t, hit, radius, entities)
                    assert excused <= ref.EXCUSED_SHARE * len(t), (excused, len(t))
                    # NaN rows: max_t and nothing; a zero direction hits only what its origin is inside
                    assert (t[256 + 176:256 + 180] == max_t).all() and (hit[256 + 176:256 + 180] == -1).all()
                    zero = slice(256 + 170, 256 + 176)
                    assert ((hit[zero] == -1) | (t[zero] == 0.0)).all()
                    seen_ent += int((hit >= ref.RAY_ENT).sum())
                    misses += int((hit < 0).sum())
                    hits += int(((hit >= 0) & (t > 0)).sum())
                    zeros += int(((hit >= 0) & (t == 0)).sum())
                    if not entities:
                        assert (hit < ref.RAY_ENT).all()
                    if max_t == 100.0 and cls_name != "Sidewalk":
                        assert (hit[:256] >= 0).all()       # a closed floor plan: every ray of the fan meets something
    assert misses and hits and zeros
    if cls_name in ("ThreeRooms", "Sidewalk"):
        assert seen_ent, "no ray met an entity"


def test_a_swept_disc_never_gets_farther_than_the_ray(program, tmp_path):
    env, sc, w = _host_world("FourRooms", 0)
    offsets = ref.lidar_offsets(64, 2 * math.pi)
    t0, _, _ = _run(program, tmp_path, w, 50.0, 0.0, 0, offsets, [], [])
    t1, _, _ = _run(program, tmp_path, w, 50.0, 0.3, 0, offsets, [], [])
    assert (t1 <= t0).all() and (t1 < t0).any()


def test_two_walls_that_share_an_end_circle_tie_to_the_lower_index(program, tmp_path):
    """a corner: the disc swept straight at the shared endpoint meets the end circle of both walls at the same t"""
    w = {"segs": np.array([[0.0, 0.0, 4.0, 0.0], [0.0, 0.0, 0.0, 4.0]]), "kind": np.zeros(1, np.int32), "pos": np.zeros((1, 3)), "radius": np.zeros(1),
         "carry": -1, "agent_radius": 0.4, "max_forward_step": 0.17, "agent": (-3.0, -3.0, 0.0)}
    t, hit, _ = _run(program, tmp_path, w, 100.0, 0.5, 0, [], [[-3.0, 0.0, -3.0]], [[1.0, 1.0]])
    wt, wh = ref.cast(w, [[-3.0, -3.0]], [[1.0, 1.0]], 100.0, 0.5, False)
    assert hit[0] == 0 and wh[0] == 0 and t[0] == wt[0] and abs(t[0] - (3.0 - 0.5 / math.sqrt(2))) < 1e-12
    # ... and in the other order of the walls the answer is the same t, still the lower index
    w["segs"] = w["segs"][::-1].copy()
    t2, hit2, _ = _run(program, tmp_path, w, 100.0, 0.5, 0, [], [[-3.0, 0.0, -3.0]], [[1.0, 1.0]])
    assert hit2[0] == 0 and t2[0] == t[0]


# ---------------------------------------------------------------------------------------------------------------- the interface

def test_header_declares_the_entry_point():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    text = " ".join(header.split())
    proto = ("int mw_ray_cast(mw_engine *e, const mw_ray_params *params, const uint8_t *d_mask, const double *d_origin /* [N][R][3] (y is not read) or "
             "NULL = the env's agent position for all its rays */, const double *d_dir /* [N][R][2] = (dx, dz), any length, or NULL */, const double "
             "*d_offsets /* [R], radians, shared by all envs: the fan; exactly one of d_dir / d_offsets is non-null */, double *d_t /* [N][R] */, "
             "int32_t *d_hit /* [N][R] or NULL */, double *d_dir_out /* [N][R][2] or NULL */, void *stream);")
    assert proto in text
    for cite in ("intersect_circle_segs (math.py:30-62)", "MiniWorldEnv.intersect (miniworld.py:937-963)"):
        assert cite in text[text.index("---- ray casts"):], cite
    struct = header[header.index("typedef struct mw_ray_params {"):header.index("} mw_ray_params;")]
    assert tuple(re.findall(r"(\w+);", struct)) == tuple(n for n, _ in engine.MwRayParams._fields_) == ("max_t", "radius", "rays", "flags")
    assert (engine.RAY_ENTITIES, engine.RAY_ENT, engine.RAY_MAX) == (1, 0x10000, 4096)
    for k, v in (("MW_RAY_ENTITIES", 1), ("MW_RAY_ENT", "0x10000"), ("MW_RAY_MAX", 4096)):
        assert re.search(rf"#define {k} {v}\b", header), k
    check_units_built("mw_ray.hip", "mw_engine_ray.hip")
    for k in ("mw_ray_lanes_kernel", "mw_ray_waves_kernel"):
        check_kernel(k, "mw_ray.hip")
    check_does_not_wait("mw_engine_ray.hip")


def test_library_exports_the_entry_point_and_refuses_a_null_engine():
    from miniworld_amd import engine
    check_refuses_null_engine("mw_ray_cast", engine.MwRayParams(1.0, 0.0, 4, 0), None, None, None, None, None, None, None, None)


def _policy(program, n, r, max_segs, max_ents):
    return launch_of(program, n, r, max_segs, max_ents, names=("per_lane", "grid", "threads", "lds", "fits", "threshold"))


def test_policy_chooses_the_form_from_the_ray_count(program):
    src = open(os.path.join(CSRC, "mw_policy.h")).read()
    thr = int(re.search(r"constexpr int kRayPerLaneFrom = (\d+);", src).group(1))
    assert _policy(program, 1, 1, 1, 1)["threshold"] == thr and 1 < thr <= 4096
    for n, segs, ents in ((1024, 256, 1), (4096, 8, 1), (67, 64, 35)):
        for r in (1, 3, thr - 1):
            p = _policy(program, n, r, segs, ents)
            assert (p["per_lane"], p["grid"], p["threads"], p["lds"], p["fits"]) == (0, -(-n * r // 4), 256, 0, 1), (n, r, p)
        for r in (thr, thr + 1, 257, 4096):
            p = _policy(program, n, r, segs, ents)
            assert (p["per_lane"], p["grid"], p["fits"]) == (1, n, 1), (n, r, p)
            assert p["threads"] == min(256, -(-r // 64) * 64) and p["lds"] == -(-(48 * segs + 32 * ents) // 16) * 16
    # the Maze's 256 segments are 12 KB; what does not fit 64 KiB is flagged, not launched
    assert _policy(program, 3, 64, 256, 1)["lds"] == 12320
    assert _policy(program, 3, 64, 1364, 1)["fits"] == 1 and _policy(program, 3, 64, 1365, 1)["fits"] == 0 and _policy(program, 3, 1, 1365, 1)["fits"] == 1


def test_vec_env_argument_errors_and_calls(monkeypatch):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    n0 = len(lib.calls)
    d = torch.zeros((5, 3, 2), dtype=torch.float64)
    r = vec.raycast(direction=d)
    assert [c[0] for c in lib.calls[n0:]] == ["mw_ray_cast"]
    assert set(r) == {"t", "hit"} and r["t"].dtype == torch.float64 and r["hit"].dtype == torch.int32 and tuple(r["t"].shape) == tuple(r["hit"].shape) == (5, 3)
    assert (r["t"] == 1.0).all() and (r["hit"] == -1).all()
    args = lib.calls[-1][1]
    p = args[1]._obj
    assert (p.max_t, p.radius, p.rays, p.flags) == (1.0, 0.0, 3, 0)
    assert args[2] is None and args[3] is None and args[4].value == d.data_ptr() and args[5] is None
    assert args[6].value == r["t"].data_ptr() and args[7].value == r["hit"].data_ptr() and args[8] is None
    off = torch.tensor([-0.5, 0.0, 0.5, 1.0], dtype=torch.float64)
    o = torch.zeros((5, 4, 3), dtype=torch.float64)
    mask = torch.tensor([1, 0, 0, 1, 0], dtype=torch.uint8)
    f = vec.raycast(offsets=off, origin=o, max_t=7.5, radius=0.25, obstacles="walls+entities", mask=mask)
    assert set(f) == {"t", "hit", "dir"} and tuple(f["dir"].shape) == (5, 4, 2) and (f["t"] == 7.5).all()
    args = lib.calls[-1][1]
    p = args[1]._obj
    assert (p.max_t, p.radius, p.rays, p.flags) == (7.5, 0.25, 4, engine.RAY_ENTITIES)
    assert args[2].value == mask.data_ptr() and args[3].value == o.data_ptr() and args[4] is None and args[5].value == off.data_ptr()
    assert args[8].value == f["dir"].data_ptr()
    flags = mask.bool()
    assert vec.raycast(offsets=off, into=f, mask=flags) is f
    assert lib.calls[-1][1][6].value == f["t"].data_ptr() and lib.calls[-1][1][2].value == flags.data_ptr()
    n0 = len(lib.calls)
    big = torch.zeros((5, engine.RAY_MAX + 1, 2), dtype=torch.float64)
    for kw in (dict(), dict(direction=d, offsets=off), dict(direction=d.float()), dict(direction=d[:4]), dict(direction=torch.zeros((5, 3, 3), dtype=torch.float64)),
               dict(direction=d.tolist()), dict(direction=big), dict(direction=d[:, :0]), dict(offsets=off.float()), dict(offsets=off[None]),
               dict(offsets=torch.zeros(0, dtype=torch.float64)), dict(direction=d, origin=o), dict(direction=d, origin=o[:, :3].float()),
               dict(direction=d, max_t=0.0), dict(direction=d, max_t=float("inf")), dict(direction=d, max_t=float("nan")), dict(direction=d, max_t=-1.0),
               dict(direction=d, radius=-0.1), dict(direction=d, radius=float("inf")), dict(direction=d, radius=float("nan")),
               dict(direction=d, obstacles="entities"), dict(direction=d, mask=torch.zeros(4, dtype=torch.uint8)), dict(direction=d, mask=torch.zeros(5)),
               dict(direction=d, mask=[1, 0, 0, 0, 0]), dict(direction=d, into=f), dict(offsets=off, into=r), dict(direction=d, into=r["t"]),
               dict(direction=d, into={"t": r["t"], "hit": r["hit"].to(torch.int64)})):
        with pytest.raises(ValueError):
            vec.raycast(**kw)
    assert len(lib.calls) == n0         # nothing reached the library
    # the lidar: the fan's offsets, built once per (rays, fov) and kept
    n0 = len(lib.calls)
    s = vec.lidar()
    assert [c[0] for c in lib.calls[n0:]] == ["mw_ray_cast"]
    assert tuple(s["t"].shape) == (5, 64) and tuple(s["dir"].shape) == (5, 64, 2)
    p = lib.calls[-1][1][1]._obj
    assert (p.max_t, p.radius, p.rays, p.flags) == (10.0, 0.0, 64, engine.RAY_ENTITIES)
    offs = vec._lidar_bufs[(64, 2 * math.pi)][0]
    assert offs.tolist() == [k * 2 * math.pi / 64 for k in range(64)] and lib.calls[-1][1][5].value == offs.data_ptr()
    assert vec.lidar() is s and vec._lidar_bufs[(64, 2 * math.pi)][0] is offs
    fov = math.radians(90)
    s2 = vec.lidar(rays=5, fov=fov, max_range=4.0, radius=0.1, obstacles="walls")
    assert vec._lidar_bufs[(5, fov)][0].tolist() == [-fov / 2 + k * fov / 4 for k in range(5)] and s2 is not s
    p = lib.calls[-1][1][1]._obj
    assert (p.max_t, p.radius, p.rays, p.flags) == (4.0, 0.1, 5, 0)
    assert vec.lidar(rays=1, fov=1.0) and vec._lidar_bufs[(1, 1.0)][0].tolist() == [0.0]
    for kw in (dict(rays=0), dict(rays=engine.RAY_MAX + 1), dict(rays=2.5), dict(fov=0.0), dict(fov=7.0), dict(max_range=0.0), dict(radius=-1.0),
               dict(obstacles="none")):
        with pytest.raises(ValueError):
            vec.lidar(**kw)
    assert "turn_left" in MiniWorldVecEnv.lidar.__doc__


# ---------------------------------------------------------------------------------------------------------------- the follower

def test_smoothed_follower_reaches_the_box_on_the_oracles_dynamics():
    """MazeS3, reset(seed=0 .. 15): the expert of examples/expert_smooth.py — K = 6 cells of lookahead down the restatement's field, a
    swept disc of agent_radius + 0.05 cast (the restatement's) at each, the farthest free one the aim, the next cell's centre after a
    blocked forward move until one succeeds — stepped by the oracle's dynamics, reaches the box within max_episode_steps in all 16,
    and in fewer steps overall than the plain follower of tests/test_nav_cpu.py."""
    import pyoracle
    K, MARGIN = 6, 0.05
    total = {False: 0, True: 0}
    for casts in (False, True):
        for seed in range(16):
            env, sc, w = _host_world("MazeS3", seed)
            ents = [e for e in env.entities if e is not env.agent]
            goal = ents.index(env.box)
            f = nav.field(w, 0.25, goal)
            tx, tz, _ = nav.target_of(w, goal, None)
            dyn = pyoracle.Dynamics(sc, pyoracle.TASK_GOTO, int(env.max_episode_steps), goal_ent=goal, num_objs=len(w["kind"]),
                                    max_forward_step=w["max_forward_step"], agent_radius=w["agent_radius"])
            fwd, turn = float(env.params.get_max("forward_step")), float(env.params.get_max("turn_step"))
            done, steps, stuck = False, 0, False
            while not done and steps < int(env.max_episode_steps):
                p = [dyn.ag.pos[0], dyn.ag.pos[1], dyn.ag.pos[2]]
                way, x, z = [], p[0], p[2]
                for _ in range(K if casts else 1):
                    c, _, x, z = nav.query(f, w["extent"], 0.25, (tx, tz), x, z)
                    way.append((x, z))
                    if len(way) == 1:
                        assert c >= 0, (seed, steps, p)
                aim = way[0]
                if casts and not stuck:
                    _, hit = ref.cast(w, [[p[0], p[2]]] * K, [[x - p[0], z - p[2]] for x, z in way], 1.0, w["agent_radius"] + MARGIN, False)
                    free = np.nonzero(hit < 0)[0]
                    if len(free):
                        aim = way[int(free[-1])]
                a = nav.follow(p, dyn.ag.dir, aim[0], aim[1], math.radians(turn))
                rew, term, trunc = dyn.step(a, fwd, 0.0, turn)
                steps += 1
                if a == nav.FORWARD:
                    stuck = (dyn.ag.pos[0], dyn.ag.pos[2]) == (p[0], p[2])
                done = term or trunc
            assert done and term and rew > 0, (casts, seed, steps)
            total[casts] += steps
    print("steps over the 16 mazes: plain", total[False], "smoothed", total[True])
    assert total[True] < total[False]
