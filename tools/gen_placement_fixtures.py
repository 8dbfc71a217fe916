"""Generates tests/golden/placement/*.npz from the reference itself (FIXTURE TOOLING): placement tests that hang on a sum of radii.

place_entity's rejection sampling (miniworld.py:872-905) asks MiniWorldEnv.intersect whether a candidate position is free; its
entity test is `d < radius + ent2.radius` (miniworld.py:960).  A MeshEnt's radius is an np.float32, and under NumPy 2's promotion
rules `python_float + np.float32` is formed in float32, so that sum differs in the last float32 bit from the one a double addition
gives.  A candidate whose distance falls between the two sums is accepted by one and rejected by the other, and from there on the
env's random stream, this world and every later episode differ.  The window is about 3e-8 m wide: no seed hits it by chance.

The cases are AIMED.  The room size is a constructor argument, and every sampled position is continuous in it as long as no earlier
accept / reject decision changes.  The reference's unmodified classes run under the GL stubs (tools/refshim.py) with env.intersect
wrapped by a recorder that restates each call's tests in the reference's own expressions, checks them against the call's result and
notes the random stream's state at the call (a function of the number of draws so far alone: two runs whose states agree at every
call made the same decisions).  For a seed with a mixed-precision test of small margin the size is moved until the margin changes sign,
then bisected until the distance lies strictly between the two sums; a step that changes an earlier decision ends the attempt.

  <family>_<k>.npz    meta/env, meta/kwargs (repr), meta/domain_rand, meta/seed, meta/resets_before (unseeded reset() calls between
                      reset(seed) and the crafted episode), meta/numpy, meta/site; case/dist, case/sum32, case/sum64, case/test_index
                      (the deciding test's number among the entity tests of the crafted reset), case/placed and case/other (class
                      names), case/r_placed, case/r_other (their radii), case/mesh (a MeshEnt takes part), case/ref_rejects (what the
                      reference decided); w/*: the resulting world (world_of).
  putnext_<k>.npz, roomobjects_control_0.npz
                      controls (meta/site "control"): boxes and the agent only, where the reference adds in double and the float32 sum
                      differs as a number; in the RoomObjects one a radius (the agent's 1.5) is exact in float32 all the same.
  respawn_0.npz       CollectHealth's respawn (collecthealth.py:86-87): poke/agent_pos, poke/agent_dir, poke/ents_pos, poke/ents_dir is the
                      state before one pickup step, w/* the world after it.

Which directions exist is arithmetic, not luck: a pair of radii has ONE float32 sum and ONE float64 sum, so every pair decides in one
direction only, and two MeshEnts of one class (r + r is exact in both formats) never differ.  possible_directions() derives from the
reference's own radii what each kind of case can show; main() asks for all of that and the tool refuses to write otherwise.
  * PickupObjects, mesh against mesh: Ball + Key is the only pair that differs: one direction.
  * CollectHealth: MedKit + agent is the only pair that differs: one direction, at reset and in the respawn — where the kit is placed
    after the agent, so that case runs the agent branch of the device's test.
  * Sign, Sidewalk, ThreeRooms: Sign's agent is sampled in x 3.6..5.4, z 3.6..6.4 whatever the size and its keys stand at fixed spots
    2.6 m and more away; Sidewalk's cones stand more than 1 m from anything sampled (the sums are 0.74 and 0.90); ThreeRooms takes no continuous constructor argument.
    None of them can be aimed: no case.

Files are written with fixed zip timestamps: a second run reproduces them byte for byte.

Usage (build container only):  python tools/gen_placement_fixtures.py
"""
import io
import itertools
import math
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refscene  # noqa: E402
import refshim  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "placement")
MAX_SEEDS = 600                   # seeds 1 .. 599: a test batch seeded with seed - 1 holds the case in its middle env
MAX_MARGIN = 0.10                 # a test further than this from its threshold is not tried
LARGEST_GOLDEN = 1257859          # bytes of the largest file in tests/golden/ (gl_maze_s0.npz)
BASE_SIZES = {"PickupObjects": (12, 11.5, 12.5), "RoomObjects": (10, 9.5, 10.5), "CollectHealth": (16, 15.5), "PutNext": (12, 11.5)}

def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy stamps the members with the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            z.writestr(info, buf.getvalue())


# ---------------------------------------------------------------------------------------------- recording intersect

def is_mesh(ent):
    return hasattr(ent, "mesh")


def both_sums(r0, r1):
    """(float32 sum, float64 sum) of two radii as numbers, whatever their types."""
    return float(np.float32(r0) + np.float32(r1)), float(r0) + float(r1)


class Recorder:
    """Wraps env.intersect: per call the stream's state, whether a wall was hit, and the entity tests up to the first hit."""

    def __init__(self, env):
        from miniworld.math import intersect_circle_segs
        self.env, self.calls, self.segs = env, [], intersect_circle_segs
        self.orig = env.intersect
        env.intersect = self

    def __call__(self, ent, pos, radius):
        env = self.env
        call = {"rng": env.np_random.bit_generator.state["state"]["state"], "pos": np.array(pos, np.float64), "tests": []}
        p = np.array([pos[0], 0, pos[2]])
        call["wall"] = bool(self.segs(p, radius, env.wall_segs))
        hit = None
        if not call["wall"]:
            for ent2 in env.entities:
                if ent2 is ent:
                    continue
                px, _, pz = ent2.pos
                d = np.linalg.norm(np.array([px, 0, pz]) - p)
                s = radius + ent2.radius                                   # the reference's expression (miniworld.py:960)
                s32, s64 = both_sums(radius, ent2.radius)
                mixed = is_mesh(ent) or is_mesh(ent2)
                assert float(s) == (s32 if mixed else s64), (type(ent).__name__, type(ent2).__name__, float(s), s32, s64)
                call["tests"].append({"placed": ent, "other": ent2, "d": float(d), "s32": s32, "s64": s64, "mixed": mixed, "hit": bool(d < s)})
                if d < s:
                    hit = ent2
                    break
        res = self.orig(ent, pos, radius)
        assert (res is True) == call["wall"] and (call["wall"] or res is hit), "the recorder's restatement disagrees with intersect"
        self.calls.append(call)
        return res

    def tests(self):
        return [(ci, t) for ci, c in enumerate(self.calls) for t in c["tests"]]

    def signature(self, upto):
        """The decisions before entity test number `upto`: the stream's state, the wall answer and the hits of every call so far."""
        sig, n = [], 0
        for c in self.calls:
            hits = []
            for t in c["tests"]:
                if n == upto:
                    return sig + [(c["rng"], c["wall"], tuple(hits))]
                hits.append(t["hit"])
                n += 1
            sig.append((c["rng"], c["wall"], tuple(hits)))
        return None


def run(cls, kwargs, seed, resets_before):
    """reset(seed) and `resets_before` unseeded resets; the recorder holds the calls of the last one."""
    env = refshim.make_env(cls, **kwargs)
    rec = Recorder(env)
    env.reset(seed=seed)
    for _ in range(resets_before):
        del rec.calls[:]
        env.reset()
    return env, rec


# ---------------------------------------------------------------------------------------------- the world a case leaves

def world_of(env):
    """What tests/test_gpu_env_api.py::_assert_same_world compares, as arrays: poses, kinds, mesh names, geometry, per-episode
    parameters, and the texture variant of every room polygon (drawn under domain randomisation)."""
    sc = refscene.scene_from_ref_env(env)
    room = [i for i in range(len(sc["polys_nv"])) if not sc["polys_nv"][i] & 0x100]
    names = [str(n) for n in sc["mesh_names"]]
    return {
        "agent_pos": sc["agent_pos"], "agent_dir": sc["agent_dir"],
        "cam": np.array([sc["cam_height"], sc["cam_fwd_disp"], sc["cam_pitch"], sc["cam_fov_y"]], np.float64),
        "light": np.concatenate([sc["sky"], sc["light_pos"], sc["light_color"], sc["light_ambient"]]).astype(np.float64),
        "ents_kind": sc["ents_kind"], "ents_pos": sc["ents_pos"], "ents_dir": sc["ents_dir"], "ents_size": sc["ents_size"],
        "ents_color": sc["ents_color"], "ents_scale": sc["ents_scale"], "ents_radius": sc["ents_radius"],
        "ents_mesh_name": np.array([names[m] if m >= 0 else "" for m in sc["ents_mesh"]]),
        "polys_tex_name": np.array([str(sc["tex_names"][sc["polys_tex"][i]]) for i in room]),
    }


def pack(env, cls, kwargs, seed, resets_before, site, t, index):
    out = {"w/" + k: v for k, v in world_of(env).items()}
    out["meta/env"] = np.array(cls)
    out["meta/kwargs"] = np.array(repr({k: v for k, v in kwargs.items() if k != "domain_rand"}))
    out["meta/domain_rand"] = np.int32(bool(kwargs.get("domain_rand", False)))
    out["meta/seed"] = np.int64(seed)
    out["meta/resets_before"] = np.int32(resets_before)
    out["meta/numpy"] = np.array(np.__version__)
    out["meta/site"] = np.array(site)
    out["case/dist"], out["case/sum32"], out["case/sum64"] = np.float64(t["d"]), np.float64(t["s32"]), np.float64(t["s64"])
    out["case/test_index"] = np.int32(index)
    out["case/placed"], out["case/other"] = np.array(type(t["placed"]).__name__), np.array(type(t["other"]).__name__)
    out["case/r_placed"], out["case/r_other"] = np.float64(t["placed"].radius), np.float64(t["other"].radius)
    out["case/mesh"] = np.bool_(t["mixed"])
    out["case/ref_rejects"] = np.bool_(t["hit"])
    return out


# ---------------------------------------------------------------------------------------------- aiming

def kind_of(cls, t, control):
    """The kind of case a test would make, or None."""
    placed, other = t["placed"], t["other"]
    if control:
        return None if t["mixed"] else "control"
    if not t["mixed"]:
        return None
    if cls != "PickupObjects":
        return cls
    agent = type(placed).__name__ == "Agent"
    if agent:
        return "agent_mesh"
    if is_mesh(placed) and is_mesh(other):
        return "mesh_mesh"
    if is_mesh(placed) and type(other).__name__ == "Box":
        return "mesh_box"
    return None                 # a box placed against a mesh: the same sums as mesh_box, not asked for


def aim(cls, kwargs, seed, resets_before, wanted, control=False, pair_ok=lambda t: True):
    """Tries the tests of one seed's crafted episode; returns (kind, direction, packed case) or None.  wanted(kind, ref_rejects) says
    whether such a case is still needed."""
    env0, rec0 = run(cls, kwargs, seed, resets_before)
    tests = rec0.tests()
    order = sorted(range(len(tests)), key=lambda g: abs(tests[g][1]["d"] - 0.5 * (tests[g][1]["s32"] + tests[g][1]["s64"])))
    for g in order:
        t = tests[g][1]
        lo, hi = min(t["s32"], t["s64"]), max(t["s32"], t["s64"])
        mid = 0.5 * (lo + hi)
        m0 = t["d"] - mid
        kind = kind_of(cls, t, control)
        # between the sums the reference rejects where its own sum is the larger one: float32 for a mixed pair, float64 for a control
        rejects = (t["s32"] > t["s64"]) if t["mixed"] else (t["s64"] > t["s32"])
        if kind is None or not lo < hi or abs(m0) > MAX_MARGIN or not wanted(kind, rejects) or not pair_ok(t):
            continue
        if any(abs(tests[h][1]["d"] - tests[h][1]["s64"]) < 3 * abs(m0) for h in range(g)):
            continue            # an earlier decision would flip first
        sig0 = rec0.signature(g)

        def margin(size):
            env, rec = run(cls, dict(kwargs, size=size), seed, resets_before)
            tt = rec.tests()
            if len(tt) <= g or rec.signature(g) != sig0:
                return None, None, None
            return tt[g][1]["d"] - mid, env, tt[g][1]
        s0, found = float(kwargs["size"]), None
        # distances grow about in proportion to the room: d(size + delta) ~ d * (1 + delta / size)
        guess = -m0 * s0 / t["d"]
        for delta in (f * guess for f in (1.25, 2.0, 4.0, -1.25, -4.0)):
            m1, _, _ = margin(s0 + delta)
            if m1 is not None and (m1 > 0) != (m0 > 0):
                found = s0 + delta
                break
        if found is None:
            continue
        a, b, ma = s0, found, m0
        for _ in range(70):
            c = 0.5 * (a + b)
            mc, env, tc = margin(c)
            if mc is None or c in (a, b):
                break
            if lo < tc["d"] < hi:
                assert tc["s32"] == t["s32"] and tc["s64"] == t["s64"] and tc["hit"] == rejects, (cls, seed, tc)
                return kind, rejects, pack(env, cls, dict(kwargs, size=c), seed, resets_before, "", tc, g)
            if (mc > 0) == (ma > 0):
                a, ma = c, mc
            else:
                b = c
    return None


def possible_directions(cls, kind):
    """The directions (True: the reference rejects between the sums) that the pairs of radii of one kind of case can show."""
    env = refshim.make_env(cls)
    env.reset(seed=0)
    ents = {}
    for s in range(8):          # (PickupObjects draws its objects' classes: a few seeds show them all)
        env.reset(seed=s)
        for e in env.entities:
            ents[(type(e).__name__, float(e.radius))] = e
    out = set()
    for placed, other in itertools.permutations(ents.values(), 2):
        t = {"placed": placed, "other": other, "mixed": is_mesh(placed) or is_mesh(other)}
        s32, s64 = both_sums(placed.radius, other.radius)
        if kind_of(cls, t, False) == kind and s32 != s64:
            out.add(s32 > s64)
    return out


def collect(cls, site, kinds, need, control=False):
    """Scans seeds (and base sizes) until every (kind, direction, flag) of `need` has a case; returns {name: case}."""
    have = {}

    def attempt(key, kwargs, resets_before, wanted):
        for size in BASE_SIZES[cls]:
            for seed in range(1, MAX_SEEDS):
                got = aim(cls, dict(kwargs, size=size), seed, resets_before, wanted, control)
                if got:
                    kind, rejects, case = got
                    case["meta/site"] = np.array(site + ":" + kind)
                    have[key if key else (kind, rejects)] = case
                    return True
        return False
    for kind, rejects in need["plain"]:
        if not attempt(None, {}, 0, lambda k, r: k == kind and r == rejects):
            sys.exit(f"refusing to write: no {cls} case of kind {kind}, reference {'rejects' if rejects else 'accepts'}")
    for flag, kwargs, resets_before in need["flags"]:
        if not attempt(flag, kwargs, resets_before, lambda k, r: k in kinds):
            sys.exit(f"refusing to write: no {cls} case with {flag}")
    return have


# ---------------------------------------------------------------------------------------------- CollectHealth's respawn

def respawn_case(size=16):
    """A kit respawns (collecthealth.py:86-87) with the agent in the list: its first candidate lies at a distance of the agent strictly
    between the sums of the kit's radius (np.float32) and the agent's (Python float).  The agent is moved there, and kit 0 in front of it."""
    for seed in range(1, MAX_SEEDS):
        def prepared(agent_pos, agent_dir):
            env = refshim.make_env("CollectHealth", size=size)
            env.reset(seed=seed)
            rec = Recorder(env)
            ag = env.agent
            ag.pos, ag.dir = np.array(agent_pos, np.float64), float(agent_dir)
            kit = [e for e in env.entities if e is not ag][0]
            kit.pos = ag.pos + ag.dir_vec * 1.5 * ag.radius
            return env, rec, kit
        centre = np.array([size / 2, 0.0, size / 2])
        env, rec, kit = prepared(centre, 0.0)
        env.step(env.actions.pickup)
        if len(rec.calls) < 2 or rec.calls[0]["wall"] or env.health != 100:
            continue
        cand = rec.calls[1]["pos"] * [1, 0, 1]           # call 0 is the pickup probe, call 1 the respawn's first candidate
        u = centre - cand
        if np.linalg.norm(u) < 3.0:
            continue
        u /= np.linalg.norm(u)
        theta = math.atan2(-u[2], u[0])                   # facing the centre, away from the candidate: dir_vec = (cos, 0, -sin)
        s32, s64 = both_sums(kit.radius, env.agent.radius)
        lo, hi = min(s32, s64), max(s32, s64)
        pos = cand + u * (0.5 * (lo + hi))
        for _ in range(64):
            d = float(np.linalg.norm(np.array([pos[0], 0, pos[2]]) - cand))
            if lo < d < hi:
                break
            pos[0] = np.nextafter(pos[0], pos[0] + (1 if (d < lo) == (u[0] > 0) else -1))
        else:
            continue
        env, rec, kit = prepared(pos, theta)
        ents0 = [e for e in env.entities if e is not env.agent]
        poke = {"agent_pos": np.array(env.agent.pos, np.float64), "agent_dir": np.float64(env.agent.dir),
                "ents_pos": np.array([e.pos for e in ents0], np.float64), "ents_dir": np.array([e.dir for e in ents0], np.float64)}
        env.step(env.actions.pickup)
        if env.health != 100 or len(rec.calls) < 3 or rec.calls[1]["wall"] or not np.array_equal(rec.calls[1]["pos"] * [1, 0, 1], cand):
            continue
        t = rec.calls[1]["tests"][-1]
        if t["other"] is not env.agent or not lo < t["d"] < hi or any(abs(x["d"] - x["s32"]) < 1e-3 for x in rec.calls[1]["tests"][:-1]):
            continue
        assert t["hit"] == (s32 > s64) and t["mixed"] and t["placed"] is kit
        index = sum(len(c["tests"]) for c in rec.calls[:1]) + len(rec.calls[1]["tests"]) - 1
        out = pack(env, "CollectHealth", {"size": size}, seed, 0, "prog_blocked:agent:respawn", t, index)
        out.update({"poke/" + k: v for k, v in poke.items()})
        out["poke/action"] = np.int32(env.actions.pickup)
        return out
    sys.exit("refusing to write: no respawn case")


# ---------------------------------------------------------------------------------------------- the set

def main():
    assert np.lib.NumpyVersion(np.__version__) >= "2.0.0", "the reference's float32 sums are NumPy 2's (NEP 50); this is numpy " + np.__version__
    files = {}

    def add(prefix, cases):
        for k, (key, c) in enumerate(sorted(cases.items(), key=lambda kv: str(kv[0]))):
            files[f"{prefix}_{k}"] = c
            print(f"{prefix}_{k}", key, "seed", int(c["meta/seed"]), str(c["meta/kwargs"]), "dr", int(c["meta/domain_rand"]), "resets_before",
                  int(c["meta/resets_before"]), str(c["meta/site"]), str(c["case/placed"]), "against", str(c["case/other"]),
                  "reference", "rejects" if c["case/ref_rejects"] else "accepts", float(c["case/dist"]), float(c["case/sum32"]), float(c["case/sum64"]))
    kinds = ("mesh_box", "mesh_mesh", "agent_mesh")
    plain = [(k, d) for k in kinds for d in sorted(possible_directions("PickupObjects", k))]
    assert len(plain) == 5, plain          # mesh_box and agent_mesh both ways, mesh_mesh one way (Ball + Key)
    add("pickupobjects", collect("PickupObjects", "gen_place", kinds,
                                 {"plain": plain, "flags": [("domain_rand", {"domain_rand": True}, 0), ("second_episode", {}, 1)]}))
    plain = [("RoomObjects", d) for d in sorted(possible_directions("RoomObjects", "RoomObjects"))]
    assert len(plain) == 2, plain
    add("roomobjects", collect("RoomObjects", "prog_blocked", ("RoomObjects",),
                               {"plain": plain, "flags": [("domain_rand", {"domain_rand": True}, 0), ("second_episode", {}, 1)]}))
    plain = [("CollectHealth", d) for d in sorted(possible_directions("CollectHealth", "CollectHealth"))]
    assert plain == [("CollectHealth", True)], plain       # MedKit + agent: the float32 sum is the larger one
    add("collecthealth", collect("CollectHealth", "prog_blocked", ("CollectHealth",), {"plain": plain, "flags": []}))
    # controls: boxes and the agent only, where the reference itself adds in double; two cases
    ctl = {}
    for seed in range(1, MAX_SEEDS):
        got = aim("PutNext", {"size": 12}, seed, 0, lambda k, r: True, control=True)
        if got:
            got[2]["meta/site"] = np.array("control")
            ctl[len(ctl)] = got[2]
            if len(ctl) == 2:
                break
    if len(ctl) != 2:
        sys.exit(f"refusing to write: {len(ctl)} control cases")
    add("putnext", ctl)
    # a control that tells "by kind" from "by value": RoomObjects' agent has radius 1.5, a Python float that float32 holds exactly,
    # and meets a box — the reference adds in double
    def exact_in_float32(t):
        return any(float(np.float32(e.radius)) == float(e.radius) for e in (t["placed"], t["other"]))
    for seed in range(1, MAX_SEEDS):
        got = aim("RoomObjects", {"size": 10}, seed, 0, lambda k, r: True, control=True, pair_ok=exact_in_float32)
        if got:
            got[2]["meta/site"] = np.array("control")
            add("roomobjects_control", {0: got[2]})
            break
    else:
        sys.exit("refusing to write: no control with a radius that float32 holds exactly")
    files["respawn_0"] = respawn_case()
    c = files["respawn_0"]
    print("respawn_0 seed", int(c["meta/seed"]), float(c["case/dist"]), float(c["case/sum32"]), float(c["case/sum64"]))
    # every case discriminates
    for name, c in files.items():
        lo, hi = sorted((float(c["case/sum32"]), float(c["case/sum64"])))
        assert lo < float(c["case/dist"]) < hi, name
    os.makedirs(OUT, exist_ok=True)
    for name, f in files.items():
        path = os.path.join(OUT, name + ".npz")
        save_npz(path, f)
        assert os.path.getsize(path) < LARGEST_GOLDEN // 50, (name, os.path.getsize(path))
        print(name + ".npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
