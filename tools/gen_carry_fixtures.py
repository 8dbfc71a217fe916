"""Generates tests/golden/carry/*.npz from the reference itself (FIXTURE TOOLING): carried-object dynamics.

Runs the reference's unmodified world generation and dynamics under the GL stubs (tools/refshim.py) with the recording of
tools/gen_golden.py, and stores, without rendered frames:

  <family>_<i>.npz        six trajectories each of PutNext, RoomObjects and ThreeRooms (the last two of each with
                          domain_rand=True) of a scripted carrying policy: walk to the nearest movable entity, pick it up, then
                          draw actions 0-7 with the probabilities of POLICY; toggle and done appear at about 1 % throughout.
                          (After a drop the nearest entity is the dropped one; three times in ten another one is sought, as it is
                          after a move or a pickup that failed.)
                          Beside the keys of gen_golden.py: tr/event (a bit mask per step, EV_*), meta/ent_class (the class name of
                          every entity), meta/numpy and meta/policy_seed.
  collecthealth_<i>.npz   two CollectHealth trajectories of the same policy in which kits are picked up (rule "api_only").
  thr_<family>.npz        threshold cases (RoomObjects, ThreeRooms, Sign): single steps from full starting states (poke/agent_pos,
                          poke/agent_dir, poke/carrying, poke/ents_pos, poke/ents_dir; row k of tr/* is the reference's state after
                          the one step of case k).  Each places an entity, or the agent for near(), at a distance strictly between
                          the float64 sum and the float32 sum of the radii that decide the step (poke/sum64, poke/sum32, poke/dist;
                          poke/kind names the site, poke/decision is what the reference did).

Why the two sums differ: a MeshEnt's radius (Ball, Key, MedKit, the duckie) derives from ObjMesh.max_coords and is an np.float32,
and under NumPy 2's promotion rules `python_float + np.float32` is evaluated in float32 (miniworld.py:611, :960, :975).

The set has to hold the event counts of REQUIRED; the generator counts them from the reference's own states, replaces the
poorest trajectory of a family by the next seed's until they hold, and refuses to write otherwise.  Files are written with
fixed zip timestamps: a second run reproduces them byte for byte.

Usage (build container only):  python tools/gen_carry_fixtures.py
"""
import io
import math
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402
import refscene  # noqa: E402
import refshim  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "carry")
POLICY = [0.2, 0.2, 0.40, 0.06, 0.02, 0.10, 0.01, 0.01]      # actions 0-7 while carrying
STEPS = 300
FAMILIES = ("PutNext", "RoomObjects", "ThreeRooms")
PER_FAMILY, DR_FROM = 6, 4                                    # trajectories per family; index of the first randomised one
MAX_SEEDS = 40
EV_TURN_UNDONE, EV_MOVE_BLOCKED_BY_CARRY, EV_PICKUP, EV_DROP, EV_PICKUP_WALL_VETO, EV_PICKUP_TWO_IN_REACH, EV_MOVE_BLOCKED = (
    1, 2, 4, 8, 16, 32, 64)
REQUIRED = {"turn_undone": 100, "move_blocked_by_carry": 100, "pickup": 60, "drop": 60, "turn_undone_per_family": 40,
            "carried_steps_per_class": 100, "pickup_wall_veto": 1, "pickup_two_in_reach": 1, "threshold_cases": 40}
LARGEST_GOLDEN = 1257859                                       # bytes of the largest file in tests/golden/ (gl_maze_s0.npz)


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


# ---------------------------------------------------------------------------------------------- the scripted policy

def _wrap(a):
    return (a + math.pi) % (2 * math.pi) - math.pi


def choose_action(env, rng, st):
    ag = env.agent
    if ag.carrying:
        return int(rng.choice(8, p=POLICY))
    u = rng.random()
    if u < 0.02:
        return 6 if u < 0.01 else 7                            # toggle, done
    if st["wander"] > 0:
        st["wander"] -= 1
        return int(rng.choice([0, 1, 2, 2, 3]))
    movable = [e for e in env.entities if e is not ag and not e.is_static]
    rest = [e for e in movable if e is not st["avoid"]] or movable
    tgt = st["target"] = min(rest, key=lambda e: float(np.linalg.norm(e.pos - ag.pos)))
    v = tgt.pos - ag.pos
    d = math.hypot(v[0], v[2])
    diff = _wrap(math.atan2(-v[2], v[0]) - ag.dir)              # dir_vec = (cos dir, 0, -sin dir)
    if abs(diff) > math.radians(10):
        return 0 if diff > 0 else 1
    if d < 2.5 * ag.radius + tgt.radius:                        # the pickup probe reaches 2.7 * radius + the entity's
        return 4
    return 2


def pickup_probe(env):
    """What the reference's pickup would meet (miniworld.py:695-698, 937-961), in its own expressions: (wall, entities in reach)."""
    from miniworld.math import intersect_circle_segs
    ag = env.agent
    test_pos = ag.pos + ag.dir_vec * 1.5 * ag.radius
    radius = 1.2 * ag.radius
    px, _, pz = test_pos
    pos = np.array([px, 0, pz])
    wall = bool(intersect_circle_segs(pos, radius, env.wall_segs))
    reach = []
    for ent2 in env.entities:
        if ent2 is ag:
            continue
        px, _, pz = ent2.pos
        if np.linalg.norm(np.array([px, 0, pz]) - pos) < radius + ent2.radius:
            reach.append(ent2)
    return wall, reach


def run_trajectory(cls, seed, domain_rand):
    kwargs = {"domain_rand": True} if domain_rand else {}
    env = refshim.make_env(cls, **kwargs)
    log = gen_golden.log_param_draws(env)
    env.reset(seed=seed)
    s0 = refscene.scene_from_ref_env(env)
    ents0 = [e for e in env.entities if e is not env.agent]
    policy_seed = 5000 + seed
    rng = np.random.default_rng(policy_seed)
    tr = {k: [] for k in gen_golden.TR_KEYS}
    events = []
    st = {"wander": 0, "avoid": None, "target": None}
    for t in range(STEPS):
        ag = env.agent
        a = choose_action(env, rng, st)
        pos0, dir0, carry0 = np.array(ag.pos, np.float64), float(ag.dir), ag.carrying
        dv0, rv0 = ag.dir_vec, ag.right_vec
        ev = 0
        if a == 4 and carry0 is None:
            wall, reach = pickup_probe(env)
            if wall and any(not e.is_static for e in reach):
                ev |= EV_PICKUP_WALL_VETO
            if not wall and len(reach) >= 2:
                ev |= EV_PICKUP_TWO_IN_REACH
        del log[:]
        obs, rew, term, trunc, info = env.step(a)
        gen_golden.record_step(tr, env, ents0, a, rew, term, trunc, log)
        same_pos = np.array_equal(np.asarray(ag.pos, np.float64), pos0)
        if a in (0, 1) and carry0 is not None and float(ag.dir) == dir0:
            ev |= EV_TURN_UNDONE
        if a in (2, 3) and same_pos:
            ev |= EV_MOVE_BLOCKED
            if carry0 is not None:
                # nothing moved: the agent's own test of this step (miniworld.py:631) can be asked again
                fwd = tr["fwd_step"][-1] * (1 if a == 2 else -1)
                if not env.intersect(ag, pos0 + dv0 * fwd + rv0 * tr["fwd_drift"][-1], ag.radius):
                    ev |= EV_MOVE_BLOCKED_BY_CARRY
        picked = carry0 is None and (ag.carrying is not None or (cls == "CollectHealth" and a == 4 and info.get("health") == 100))
        if picked:
            ev |= EV_PICKUP
            st["avoid"] = None
        if carry0 is not None and ag.carrying is None:
            ev |= EV_DROP
            # the nearest movable entity is now the one just dropped: mostly it is picked up again, sometimes another one is sought
            st["avoid"] = carry0 if rng.random() < 0.3 else None
        if carry0 is None and ((a == 2 and same_pos) or (a == 4 and not picked)):
            # out of reach from here (a wall in the way, or in the probe's circle): roam a little, then seek another entity
            st["wander"] = int(rng.integers(3, 12))
            st["avoid"] = st["target"]
        events.append(ev)
        if term or trunc:
            break
    out = gen_golden.pack_case(s0, tr, env, ents0, cls, kwargs, seed, POLICY, np.array([-1, 0, 0, 0, 0], np.float64))
    out["tr/event"] = np.array(events, np.int32)
    out["meta/ent_class"] = np.array([type(e).__name__ for e in ents0])
    out["meta/numpy"] = np.array(np.__version__)
    out["meta/policy_seed"] = np.int32(policy_seed)
    return out


def count_events(case):
    ev = case["tr/event"]
    n = {name: int(np.count_nonzero(ev & bit)) for name, bit in (
        ("turn_undone", EV_TURN_UNDONE), ("move_blocked_by_carry", EV_MOVE_BLOCKED_BY_CARRY), ("pickup", EV_PICKUP), ("drop", EV_DROP),
        ("pickup_wall_veto", EV_PICKUP_WALL_VETO), ("pickup_two_in_reach", EV_PICKUP_TWO_IN_REACH))}
    n["actions"] = set(int(a) for a in case["tr/action"])
    n["carried"] = {}
    for c in case["tr/carrying"]:
        if c >= 0:
            k = str(case["meta/ent_class"][c])
            n["carried"][k] = n["carried"].get(k, 0) + 1
    return n


def total(counts, key):
    return sum(c[key] for c in counts)


def check_counts(files):
    """The counts REQUIRED names, over the trajectories; returns the list of what is missing."""
    counts = {name: count_events(c) for name, c in files.items()}
    traj = [counts[n] for n in counts if not n.startswith("collecthealth")]
    missing = []
    for key in ("turn_undone", "move_blocked_by_carry", "pickup", "drop", "pickup_wall_veto", "pickup_two_in_reach"):
        if total(traj, key) < REQUIRED[key]:
            missing.append((key, total(traj, key)))
    for fam in FAMILIES:
        n = total([counts[k] for k in counts if k.startswith(fam.lower() + "_")], "turn_undone")
        if n < REQUIRED["turn_undone_per_family"]:
            missing.append((fam + " turn_undone", n))
    for k in ("Ball", "Key", "MeshEnt"):
        n = sum(c["carried"].get(k, 0) for c in traj)
        if n < REQUIRED["carried_steps_per_class"]:
            missing.append(("carried " + k, n))
    acts = set().union(*[c["actions"] for c in traj])
    if not {6, 7} <= acts:
        missing.append(("actions", sorted(acts)))
    return missing, counts


def family_trajectories(cls):
    """Six trajectories (the last two randomised) from seeds 0, 1, ...; one that ends within 100 steps or picks up fewer than three
    times is passed over.  While the family's counts are short, the poorest one is replaced by the next seed's."""
    seeds = iter(range(MAX_SEEDS))

    def next_case(domain_rand):
        for seed in seeds:
            c = run_trajectory(cls, seed, domain_rand)
            if len(c["tr/action"]) >= 100 and count_events(c)["pickup"] >= 3:
                return c
        sys.exit(f"refusing to write: {cls} ran out of seeds")

    def score(c):
        n = count_events(c)
        return n["turn_undone"] + n["move_blocked_by_carry"]
    cases = [next_case(i >= DR_FROM) for i in range(PER_FAMILY)]
    while True:
        n = [count_events(c) for c in cases]
        if total(n, "turn_undone") >= REQUIRED["turn_undone_per_family"] and total(n, "move_blocked_by_carry") >= 34 \
                and total(n, "pickup") >= 20 and total(n, "drop") >= 20:
            break
        worst = min(range(PER_FAMILY), key=lambda i: score(cases[i]))
        cases[worst] = next_case(worst >= DR_FROM)
    segs = [c["s0/wall_segs"] for c in cases]
    assert all(np.array_equal(s, segs[0]) for s in segs), f"{cls}: the trajectories do not share wall_segs"
    E = [len(c["s0/ents_kind"]) for c in cases]
    assert len(set(E)) == 1, f"{cls}: entity counts differ {E}"
    return cases


def collecthealth_trajectories():
    out, seed = [], 0
    while len(out) < 2 and seed < MAX_SEEDS:
        c = run_trajectory("CollectHealth", seed, False)
        if count_events(c)["pickup"] >= 2:
            out.append(c)
        seed += 1
    assert len(out) == 2, "CollectHealth: no two seeds with kits picked up"
    return out


# ---------------------------------------------------------------------------------------------- threshold cases

class Thresholds:
    """Single steps of one reference env whose outcome hangs on a sum of radii that float32 and float64 round differently."""

    def __init__(self, cls, seed, **kwargs):
        self.cls, self.seed, self.kwargs = cls, seed, kwargs
        self.env = refshim.make_env(cls, **kwargs)
        self.log = gen_golden.log_param_draws(self.env)
        self.env.reset(seed=seed)
        self.s0 = refscene.scene_from_ref_env(self.env)
        self.ents0 = [e for e in self.env.entities if e is not self.env.agent]
        self.base_pos = [np.array(e.pos, np.float64) for e in self.ents0]
        self.base_dir = [float(e.dir) for e in self.ents0]
        self.fwd = float(self.env.params.sample(None, "forward_step"))
        self.turn = float(self.env.params.sample(None, "turn_step"))
        self.rng = np.random.default_rng(7000 + seed)
        self.tr = {k: [] for k in gen_golden.TR_KEYS}
        self.poke = {k: [] for k in ("agent_pos", "agent_dir", "carrying", "ents_pos", "ents_dir", "kind", "ent", "dist", "sum64", "sum32",
                                     "decision")}

    def install(self, state):
        env = self.env
        env.agent.pos, env.agent.dir = np.array(state["agent_pos"], np.float64), float(state["agent_dir"])
        env.agent.carrying = self.ents0[state["carrying"]] if state["carrying"] >= 0 else None
        for e, p, d in zip(self.ents0, state["ents_pos"], state["ents_dir"]):
            e.pos, e.dir = np.array(p, np.float64), float(d)
        env.step_count = 0

    def blank(self):
        return {"agent_pos": np.zeros(3), "agent_dir": 0.0, "carrying": -1, "ents_pos": [p.copy() for p in self.base_pos],
                "ents_dir": list(self.base_dir)}

    # Each builder returns (state, action, the distance as the reference will compute it) for a wanted distance d.
    def build_walk(self, m, phi, d):
        """The agent one forward step away from a spot at distance d of mesh entity m, walking towards it (miniworld.py:631, :960)."""
        st = self.blank()
        u = np.array([math.cos(phi), 0.0, math.sin(phi)])
        st["agent_pos"] = self.base_pos[m] * [1, 0, 1] + u * (d + self.fwd)
        st["agent_dir"] = math.atan2(u[2], -u[0])
        self.install(st)
        ag = self.env.agent
        nxt = ag.pos + ag.dir_vec * self.fwd + ag.right_vec * 0.0
        return st, 2, float(np.linalg.norm(self.base_pos[m] * [1, 0, 1] - nxt * [1, 0, 1]))

    def build_pickup(self, m, phi, d):
        """The pickup probe's centre at distance d of mesh entity m (miniworld.py:697-698, :960)."""
        st = self.blank()
        ar = self.env.agent.radius
        u = np.array([math.cos(phi), 0.0, math.sin(phi)])
        st["agent_pos"] = self.base_pos[m] * [1, 0, 1] + u * (d + 1.5 * ar)
        st["agent_dir"] = math.atan2(u[2], -u[0])
        self.install(st)
        ag = self.env.agent
        test_pos = ag.pos + ag.dir_vec * 1.5 * ag.radius
        return st, 4, float(np.linalg.norm(self.base_pos[m] * [1, 0, 1] - test_pos * [1, 0, 1]))

    def build_carry(self, turn, c, x, p, theta, d):
        """The agent at p carries c; entity x lies at distance d of where the step would put c (miniworld.py:636-638 / 659-661, :960)."""
        st = self.blank()
        st["agent_pos"], st["agent_dir"], st["carrying"] = np.array(p, np.float64), theta, c
        self.install(st)
        env, ag = self.env, self.env.agent
        ce = self.ents0[c]
        st["ents_pos"][c] = np.array(env._get_carry_pos(ag.pos, ce), np.float64)
        st["ents_dir"][c] = theta
        if turn:
            ag.dir = theta + self.turn * (math.pi / 180)        # turn_agent's own expressions (miniworld.py:652-659)
            cp = env._get_carry_pos(ag.pos, ce)
        else:
            nxt = ag.pos + ag.dir_vec * self.fwd + ag.right_vec * 0.0
            cp = env._get_carry_pos(nxt, ce)
        xp = cp * [1, 0, 1] + ag.dir_vec * d
        st["ents_pos"][x] = np.array(xp, np.float64)
        return st, (0 if turn else 2), float(np.linalg.norm(xp * [1, 0, 1] - cp * [1, 0, 1]))

    def build_near(self, m, phi, d):
        """The agent at distance d of mesh entity m, turning on the spot (miniworld.py:974-975; sign.py:160-170)."""
        st = self.blank()
        u = np.array([math.cos(phi), 0.0, math.sin(phi)])
        st["agent_pos"] = self.base_pos[m] + u * d
        st["agent_dir"] = float(self.rng.uniform(-math.pi, math.pi))
        return st, 0, float(np.linalg.norm(self.base_pos[m] - st["agent_pos"]))

    def step(self, state, action):
        self.install(state)
        env, ag = self.env, self.env.agent
        del self.log[:]
        res = env.step(action)
        return res

    def outcome(self, kind, state, action, m):
        obs, rew, term, trunc, info = self.step(state, action)
        ag = self.env.agent
        if kind == "pickup":
            return ag.carrying is self.ents0[m]
        if kind == "carry_turn":
            return float(ag.dir) == float(state["agent_dir"])
        if kind == "near":
            return bool(term)
        return np.array_equal(np.asarray(ag.pos, np.float64), state["agent_pos"])

    def add(self, kind, build, sum64, sum32, ents):
        """Stores the case built at the midpoint of the two sums, if that step really hangs on them: just below both the reference
        decides one way, just above both the other, and between them as the float32 sum says, where the float64 sum says otherwise."""
        lo, hi = min(sum64, sum32), max(sum64, sum32)
        if not lo < hi:
            return False
        for d, want in ((lo - 1e-6, True), (hi + 1e-6, False)):
            st, a, _ = build(d)
            if self.outcome(kind, st, a, ents[0]) != want:
                return False
        st, a, dist = build(0.5 * (lo + hi))
        if not lo < dist < hi:
            return False
        decision = self.outcome(kind, st, a, ents[0])
        assert (dist < sum64) != (dist < sum32) and decision == (dist < sum32), (self.cls, kind, ents, dist, sum64, sum32, decision)
        obs_state = st
        self.install(obs_state)
        del self.log[:]
        obs, rew, term, trunc, info = self.env.step(a)
        gen_golden.record_step(self.tr, self.env, self.ents0, a, rew, term, trunc, self.log)
        for k in ("agent_pos", "agent_dir", "carrying"):
            self.poke[k].append(st[k])
        self.poke["ents_pos"].append(np.array(st["ents_pos"], np.float64))
        self.poke["ents_dir"].append(np.array(st["ents_dir"], np.float64))
        self.poke["kind"].append(kind)
        self.poke["ent"].append(list(ents))
        self.poke["dist"].append(dist)
        self.poke["sum64"].append(sum64)
        self.poke["sum32"].append(sum32)
        self.poke["decision"].append(decision)
        return True

    def is_mesh(self, i):
        return hasattr(self.ents0[i], "mesh")

    def movable(self):
        return [i for i, e in enumerate(self.ents0) if not e.is_static]

    def free_spot(self):
        env = self.env
        room = env.rooms[0]
        m = 1.2 * env.agent.radius + 1.0
        return np.array([self.rng.uniform(room.min_x + m, room.max_x - m), 0.0, self.rng.uniform(room.min_z + m, room.max_z - m)])

    def generate(self, per_site, carry_pairs=True, sites=("walk", "pickup", "carry_move", "carry_turn")):
        env = self.env
        ar = env.agent.radius
        meshes = [i for i in range(len(self.ents0)) if self.is_mesh(i)]
        for kind in sites:
            if kind in ("walk", "pickup", "near"):
                for m in meshes:
                    e = self.ents0[m]
                    if kind == "walk":
                        s32, s64, b = float(ar + e.radius), float(ar) + float(e.radius), self.build_walk
                    elif kind == "pickup":
                        s32, s64, b = float(1.2 * ar + e.radius), 1.2 * float(ar) + float(e.radius), self.build_pickup
                    else:
                        s32 = float(e.radius + env.agent.radius + 1.1 * env.max_forward_step)
                        s64 = float(e.radius) + float(env.agent.radius) + 1.1 * float(env.max_forward_step)
                        b = self.build_near
                    got = 0
                    for _ in range(40):
                        phi = float(self.rng.uniform(-math.pi, math.pi))
                        got += self.add(kind, lambda d: b(m, phi, d), s64, s32, (m, -1))
                        if got == per_site:
                            break
            else:
                mov = self.movable()
                for c in mov:
                    for x in [i for i in range(len(self.ents0)) if i != c and type(self.ents0[i]).__name__ != "ImageFrame"]:
                        if not (self.is_mesh(c) or self.is_mesh(x)):
                            continue
                        ce, xe = self.ents0[c], self.ents0[x]
                        s32, s64 = float(ce.radius + xe.radius), float(ce.radius) + float(xe.radius)
                        got = 0
                        for _ in range(40):
                            p, theta = self.free_spot(), float(self.rng.uniform(-math.pi, math.pi))
                            got += self.add(kind, lambda d: self.build_carry(kind == "carry_turn", c, x, p, theta, d), s64, s32, (c, x))
                            if got == per_site:
                                break

    def pack(self):
        K = len(self.poke["kind"])
        out = gen_golden.pack_case(self.s0, self.tr, self.env, self.ents0, self.cls, self.kwargs, self.seed, POLICY,
                                   np.array([-1, 0, 0, 0, 0], np.float64))
        out["poke/agent_pos"] = np.array(self.poke["agent_pos"], np.float64).reshape(K, 3)
        out["poke/agent_dir"] = np.array(self.poke["agent_dir"], np.float64)
        out["poke/carrying"] = np.array(self.poke["carrying"], np.int32)
        out["poke/ents_pos"] = np.array(self.poke["ents_pos"], np.float64)
        out["poke/ents_dir"] = np.array(self.poke["ents_dir"], np.float64)
        out["poke/kind"] = np.array(self.poke["kind"])
        out["poke/ent"] = np.array(self.poke["ent"], np.int32).reshape(K, 2)
        for k in ("dist", "sum64", "sum32"):
            out["poke/" + k] = np.array(self.poke[k], np.float64)
        out["poke/decision"] = np.array(self.poke["decision"], bool)
        out["meta/ent_class"] = np.array([type(e).__name__ for e in self.ents0])
        out["meta/numpy"] = np.array(np.__version__)
        out["meta/policy_seed"] = np.int32(7000 + self.seed)
        return out


def threshold_files():
    files = {}
    for cls, seed, kwargs, per_site, sites in (("RoomObjects", 1, {}, 2, ("walk", "pickup", "carry_move", "carry_turn")),
                                               ("ThreeRooms", 0, {}, 1, ("walk", "pickup", "carry_move", "carry_turn")),
                                               ("Sign", 0, {}, 3, ("near", "walk"))):
        th = Thresholds(cls, seed, **kwargs)
        th.generate(per_site, sites=sites)
        files["thr_" + cls.lower()] = th.pack()
    kinds = np.concatenate([f["poke/kind"] for f in files.values()])
    above = np.concatenate([f["poke/sum32"] > f["poke/sum64"] for f in files.values()])
    assert len(kinds) >= REQUIRED["threshold_cases"], len(kinds)
    assert above.any() and not above.all(), "the threshold cases show one polarity only"
    for k in ("walk", "pickup", "carry_move", "carry_turn", "near"):
        assert (kinds == k).any(), k
    assert (files["thr_sign"]["poke/kind"] == "near").any()
    return files


def main():
    assert np.lib.NumpyVersion(np.__version__) >= "2.0.0", "the reference's float32 sums are NumPy 2's (NEP 50); this is numpy " + np.__version__
    files = {}
    for cls in FAMILIES:
        for i, c in enumerate(family_trajectories(cls)):
            files[f"{cls.lower()}_{i}"] = c
    for i, c in enumerate(collecthealth_trajectories()):
        files[f"collecthealth_{i}"] = c
    missing, counts = check_counts(files)
    for name, n in counts.items():
        print(name, "seed", int(files[name]["meta/seed"]), "dr", int(files[name]["meta/domain_rand"]), "steps", len(files[name]["tr/action"]),
              {k: v for k, v in n.items() if k != "actions"})
    if missing:
        sys.exit(f"refusing to write: the set lacks {missing}")
    thr = threshold_files()
    for name, f in thr.items():
        kinds, n = np.unique(f["poke/kind"], return_counts=True)
        print(name, dict(zip(kinds.tolist(), n.tolist())), "sum32 above sum64:", int((f["poke/sum32"] > f["poke/sum64"]).sum()), "of", len(f["poke/kind"]))
    files.update(thr)
    os.makedirs(OUT, exist_ok=True)
    for name, f in files.items():
        path = os.path.join(OUT, name + ".npz")
        save_npz(path, f)
        assert os.path.getsize(path) < LARGEST_GOLDEN, (name, os.path.getsize(path))
        print(name + ".npz", os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
