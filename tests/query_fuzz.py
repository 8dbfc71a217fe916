"""The world queries asked behind the ops of the stepping-API fuzzer ("The API model and its fuzzer").  Plain Python and
numpy, no torch and no engine: tests/test_query_fuzz_cpu.py runs it on the model alone, tests/test_gpu_query_fuzz.py applies the same
ops to the engine as well.

`Driver` draws the state ops of a sequence from api_fuzz.Generator — the same configs, the same stream — and between them inserts ops
of its own, drawn from a second, independent stream: frameless rollouts ({"kind": "rollout", ..., "render": False}) and queries
({"kind": "query", "what": ..., ...}).  A query op is complete in itself, like every op: its shapes, its mask and the `clear` bytes of a
persistent map are plain values in it.  `Mirror` answers a query op through the restatements (tests/*_reference.py, as they are) from
a `source` of worlds and poses: ModelSource here, the engine's host routes in the GPU module.  The persistent maps (the seen map, the
scan map) live in the Mirror for the whole sequence.

The clear rule: an update of a persistent map passes clear = 1 for exactly the envs whose model world_id differs from the one that
map's last update of the env met — an auto-reset, reset_where, a load or a fork that brought another world, a next-step install.  A
pose that jumps inside the same world keeps the map.

A restatement may decline a case it cannot judge exactly (nav_reference.field: a cell centre within rounding of a threshold).  The
driver drops such a query — it is not logged and counts for nothing but `dropped` — and the dropped share is capped (DROP_CAP)."""
import collections
import math

import numpy as np

import api_fuzz
import depth_reference
import ego_reference
import label_reference
import nav_reference as nav
import ray_reference as ray
import scan_reference
import seen_reference

N_OPS = 48                      # state ops per sequence
SEEDS = (1, 2, 3, 4)
P_HOT, P_COLD = 0.7, 0.15       # a query behind an op that can change what a query sees / behind any other op
P_FRAMELESS = 0.3               # a frameless rollout behind a state op
P_MASK = 0.25                   # a query with a mask
DROP_CAP = 0.05

MSAA = 8                        # the engine's default sample count, the model's frames' own
CELL, RAY_RANGE, SEEN_RANGE, POINT_REACH = 0.5, 6.0, 4.0, 0.6
WALLS_ENTS = "walls+entities"
EGO = {"ego9": dict(size=9, frame="north", anchor="bottom"), "ego17": dict(size=17, frame="heading", anchor="centre")}
EGO_CELL, EGO_RANGE, DEPTH_SIZE = 0.25, 10.0, 17
ENTITY_AWARE = ("raycast", "lidar", "nav", "seen", "ego9", "ego17", "scan")
BEHIND = ("load_list", "load_masked", "load_whole", "fork", "reset_where", "set_ent_pos", "repeat_ended", "frameless")


# The stepping fuzzer's configs, and one of this driver's own: the only family whose pickups take an entity out of the list, in a mode
# that takes frameless rollouts (api_fuzz's PickupObjects config is seeded, which refuses them) — the path on which the step kernel
# itself applies the removal behind the last sub-step of a frameless plan.
CONFIGS = dict(api_fuzz.CONFIGS)
CONFIGS["pickup_same_step"] = dict(cls="PickupObjects", env_id="MiniWorld-PickupObjects-v0", n=3, task=2, n_actions=5, episode=8, cache=False,
                                   kw=dict(autoreset="same_step"))


def fuzz_seed(cfg_name, seed):
    return 1000 * (1 + list(CONFIGS).index(cfg_name)) + 37 * seed


def make_model(cfg_name, seed):
    """api_fuzz.make_model over this module's configs"""
    import engine_model
    from miniworld_amd import envs
    cfg = CONFIGS[cfg_name]
    mv = engine_model.ModelVec(getattr(envs, cfg["cls"]), cfg["n"], seed=fuzz_seed(cfg_name, seed), task=cfg["task"], **cfg["kw"])
    mv.reset()
    return mv


def make_generator(cfg_name, seed):
    """api_fuzz.Generator(cfg_name, seed); for a config of this module alone the same object, set up as its constructor would"""
    if cfg_name in api_fuzz.CONFIGS:
        return api_fuzz.Generator(cfg_name, seed)
    g = api_fuzz.Generator.__new__(api_fuzz.Generator)
    g.cfg = CONFIGS[cfg_name]
    g.rng = np.random.default_rng([seed, list(CONFIGS).index(cfg_name)])
    g.kinds = api_fuzz.op_kinds(g.cfg)
    w = np.array([api_fuzz.WEIGHTS[k] for k in g.kinds], float)
    g.p, g.last_turn, g.queue = w / w.sum(), [0] * g.cfg["n"], []
    return g


class Declined(Exception):
    """a restatement refused to judge a near-tie"""


def query_kinds(cfg):
    return ["raycast", "lidar", "nav", "seen", "ego9", "ego17", "label", "scan"] + (["depth"] if cfg["kw"].get("want_depth") else [])


def world_of_model(e):
    """the restatements' world (nav_reference.world_of_scene's keys) of a ModelEnv: the scene a frame drawn now shows, the carried slot"""
    w = nav.world_of_scene(e.scene_now())
    w["carry"] = int(e.dyn.ag.carrying)
    return w


def pose_of_model(e):
    ag = e.dyn.ag
    return (float(ag.pos[0]), float(ag.pos[2]), float(ag.dir))


class ModelSource:
    """what a Mirror reads, from the model batch"""

    def __init__(self, mv):
        self.mv = mv

    def worlds(self):
        return [world_of_model(e) for e in self.mv.envs]

    def poses(self):
        return [pose_of_model(e) for e in self.mv.envs]

    def scene(self, i):
        return self.mv.envs[i].scene_now()

    def meshes(self):
        out = {}
        for e in self.mv.envs:
            out.update(e.meshes())
        return out

    def depth(self, i):
        return self.mv.depth[i]

    def cam(self, i):
        sc = self.mv.envs[i].sc
        return tuple(float(sc[k]) for k in ("cam_height", "cam_fwd_disp", "cam_pitch", "cam_fov_y"))


def default_fov(fov_y_deg, width, height):
    """MiniWorldVecEnv.default_fov(): the horizontal field of view of the default camera"""
    return 2.0 * math.atan(math.tan(math.radians(float(fov_y_deg)) / 2.0) * float(width) / float(height))


def setup_of_model(mv):
    """the values the queries' defaults take from the engine's configuration, from the model: (extent of the template world, the default
    horizontal field of view, the agent's height)"""
    e = mv.envs[0]
    return (np.asarray(e.sc["extent"], np.float64), default_fov(e.h.params.params["cam_fov_y"].default, mv.W, mv.H), float(e.sc["agent_height"]))


def _nav_field(w, op, i):
    target = op["target"] if op["points"] is None else tuple(op["points"][i])
    try:
        return nav.field(w, CELL, target, reach=None if op["points"] is None else POINT_REACH, entities=True)
    except AssertionError as err:
        if "the exact comparison would hang" in str(err):       # (a near-tie; anything else a restatement raises is a failure)
            raise Declined(str(err)) from None
        raise


def _fan(w, pose, op):
    offs = ray.lidar_offsets(op["rays"], 2 * math.pi)
    dirs = ray.fan_directions(pose[2], offs)
    t, hit = ray.cast(w, np.tile(np.array([[pose[0], pose[1]]]), (len(offs), 1)), dirs, RAY_RANGE, op.get("radius", 0.0),
                      op.get("obstacles", WALLS_ENTS) == WALLS_ENTS)
    return t, hit, dirs


class Mirror:
    """The restatements behind a sequence's query ops, with the persistent maps.  `answer(op, source)`: per env the dict of every output
    the device call of the op writes, None for an env under a zero mask byte."""

    def __init__(self, n, extent, fov, agent_height):
        self.n, self.fov, self.cos_half, self.top = n, fov, seen_reference.cos_half_of(fov), agent_height
        self.gx, self.gz = nav.grid_shape(extent, CELL)
        self.seen = [seen_reference.Map(self.gx, self.gz) for _ in range(n)]
        self.scan = [np.zeros((2, self.gz, self.gx), np.uint8) for _ in range(n)]
        self.scan_count = [np.zeros(2, np.int64) for _ in range(n)]

    def answer(self, op, source):
        what, mask = op["what"], op.get("mask")
        worlds, poses = source.worlds(), source.poses()
        on = [mask is None or bool(mask[i]) for i in range(self.n)]
        if what == "nav":       # (all fields first: a declined env drops the query before anything is kept)
            fields = [_nav_field(worlds[i], op, i) if on[i] else None for i in range(self.n)]
        meshes = source.meshes() if what == "label" else None
        out = []
        for i in range(self.n):
            if not on[i]:
                out.append(None)
                continue
            w, pose = worlds[i], poses[i]
            if what in ("raycast", "lidar"):
                t, hit, dirs = _fan(w, pose, op)
                out.append({"t": t, "hit": hit, "dir": dirs})
            elif what == "nav":
                txz = (float(w["pos"][0][0]), float(w["pos"][0][2])) if op["points"] is None else (float(op["points"][i][0]), float(op["points"][i][2]))
                cost, nxt, wx, wz = nav.query(fields[i], w["extent"], CELL, txz, pose[0], pose[1])
                out.append({"field": fields[i], "cost": cost, "next": nxt, "waypoint": (wx, wz)})
            elif what == "seen":
                assert seen_reference.covers(w["extent"], CELL, self.gx, self.gz), "the template's grid does not cover this world"
                m = self.seen[i]
                seen_reference.update(m, w, CELL, pose, SEEN_RANGE, self.cos_half, True, clear=bool(op["clear"][i]))
                out.append({"seen": m.seen.copy(), "count": m.count, "new": m.new})
            elif what in EGO:
                g = EGO[what]
                planes, _ = ego_reference.window(w, pose, g["size"], EGO_CELL, g["size"] / 2 if g["anchor"] == "bottom" else 0.0, g["frame"] == "north",
                                                 ("wall", "entity", "visible"), EGO_CELL / 2, EGO_CELL / 2, EGO_RANGE, self.cos_half, True)
                out.append({"planes": planes})
            elif what == "label":
                sc = source.scene(i)
                f = label_reference.label_frame(sc, op["width"], op["height"], MSAA, meshes=meshes)
                out.append({"cls": f["cls"], "code": f["code"]})
            elif what == "depth":
                out.append({"planes": depth_reference.window(source.depth(i), pose, source.cam(i), MSAA, DEPTH_SIZE, EGO_CELL, 0.0, False, min_range=0.05,
                                                             max_range=8.0, floor_tol=0.1, top=self.top)})
            elif what == "scan":
                assert seen_reference.covers(w["extent"], CELL, self.gx, self.gz), "the template's grid does not cover this world"
                t, hit, dirs = _fan(w, pose, {"rays": 65})
                free, obstacle = scan_reference.sets(pose[:2], t, dirs, RAY_RANGE, w["extent"][0], w["extent"][2], CELL, self.gx, self.gz)
                new = scan_reference.update(self.scan[i], self.scan_count[i], free, obstacle, clear=bool(op["clear"][i]))
                out.append({"map": self.scan[i].copy(), "count": self.scan_count[i].copy(), "new": new, "t": t, "hit": hit, "dir": dirs})
            else:
                raise ValueError(what)
        return out


def probe(op, w, pose, i):
    """what an entity-aware query says of one world, without the persistent maps: to tell whether another entity list would have shown"""
    what = op["what"]
    if what in ("raycast", "lidar", "scan"):
        t, hit, _ = _fan(w, pose, op if what != "scan" else {"rays": 65})
        return t.tobytes() + hit.tobytes()
    if what == "nav":
        try:
            return _nav_field(w, op, i).tobytes()
        except Declined:
            return None
    if what == "seen":
        return seen_reference.visible(w, CELL, *nav.grid_shape(w["extent"], CELL), pose, SEEN_RANGE, seen_reference.cos_half_of(op["fov"]), True)[0].tobytes()
    g = EGO[what]
    return ego_reference.window(w, pose, g["size"], EGO_CELL, g["size"] / 2 if g["anchor"] == "bottom" else 0.0, g["frame"] == "north",
                                ("wall", "entity", "visible"), EGO_CELL / 2, EGO_CELL / 2, EGO_RANGE, seen_reference.cos_half_of(op["fov"]), True)[0].tobytes()


class Driver:
    """One sequence on the model: `ops()` yields every op behind its application to the model, `answers` then holds the restatement's
    answer to a query op from the model's own worlds and poses.  `replay(ops)` does the same from a logged list."""

    def __init__(self, cfg_name, seed, p_hot=P_HOT, p_cold=P_COLD, p_frameless=P_FRAMELESS, answer=True):
        """answer=False (the GPU module, which feeds the restatements from the engine instead): only the queries whose restatement can
        decline are answered on the model, since a declined query is dropped"""
        self.cfg_name, self.seed, self.cfg, self.answer = cfg_name, seed, CONFIGS[cfg_name], answer
        self.p_hot, self.p_cold, self.p_frameless = p_hot, p_cold, p_frameless
        self.mv, self.bank = make_model(cfg_name, seed), [None] * api_fuzz.BANK
        self.gen = make_generator(cfg_name, seed)
        self.rng = np.random.default_rng([seed, list(CONFIGS).index(cfg_name), 77])
        self.kinds = query_kinds(self.cfg)
        self.extent, self.fov, self.top = setup_of_model(self.mv)
        self.mirror = Mirror(self.mv.N, self.extent, self.fov, self.top)
        self.source = ModelSource(self.mv)
        self.counts, self.log, self.answers = collections.Counter(), [], None
        n = self.mv.N
        ids = [e.world_id for e in self.mv.envs]
        self.map_world = {"seen": list(ids), "scan": list(ids)}       # the world each persistent map's last update of the env met
        self.asked_world = list(ids)                                    # ... and the last query of any kind
        self.left_slots = [set() for _ in range(n)]                     # the slots that left the env's list since a query last met it
        self.left_tail = [set() for _ in range(n)]                      # ... of them, behind the LAST sub-step of a frameless rollout
        self.hot, self.behind = False, set()

    # ---------------------------------------------------------------- the model's side of an op
    def _alive(self, i):
        e = self.mv.envs[i]
        return [bool(e.dyn.ents[k].alive) for k in range(e.E)]

    def _held(self):
        return [(int(e.dyn.ag.carrying), sum(self._alive(i))) for i, e in enumerate(self.mv.envs)]

    def _state_op(self, op):
        """applies a state op to the model; notes what a query directly behind it stands behind"""
        mv, kind = self.mv, op["kind"]
        held, was = self._held(), [(e.world_id, self._alive(i)) for i, e in enumerate(mv.envs)]
        api_fuzz.apply_model(mv, self.bank, op)
        for i, (e, (world, alive)) in enumerate(zip(mv.envs, was)):
            now = self._alive(i)
            self.left_slots[i] = set() if e.world_id != world else {k for k in range(e.E) if not now[k] and (k in self.left_slots[i] or alive[k])}
            # (the model's _left: the last executed sub-step took an entity out — in a frameless call the step kernel's own tail)
            tail = kind == "rollout" and not op.get("render", True) and e.world_id == world and bool(mv._left[i])
            self.left_tail[i] = (self.left_tail[i] | ({k for k in range(e.E) if alive[k] and not now[k]} if tail else set())) & self.left_slots[i]
        tags, hot = set(), False
        if kind == "load_state":
            tags.add("load_" + op["form"])
        elif kind in ("fork", "reset_where"):
            tags.add(kind)
        elif kind == "set_state_where":
            hot = True
            if "ent_pos" in op:
                tags.add("set_ent_pos")
        elif kind in ("step", "rollout"):
            ended = bool((mv.terminated | mv.truncated).any())
            hot = ended or held != self._held() or op.get("repeat", 1) > 1
            if kind == "step" and op["repeat"] > 1 and ended:
                tags.add("repeat_ended")
            if kind == "rollout" and not op.get("render", True):
                tags.add("frameless")
        self.behind, self.hot = tags, hot or bool(tags)
        self.log.append(op)

    def _ask(self, op):
        """a query op on the model: the restatement's answer (None: declined, the query is dropped) and the coverage it counts for"""
        mv, c, what = self.mv, self.counts, op["what"]
        c["drawn"] += 1
        try:
            answers = self.mirror.answer(op, self.source) if self.answer or what == "nav" else ()
        except Declined:        # (only a navigation field declines, before anything is kept: the persistent maps are as they were)
            c["dropped"] += 1
            return None
        c["asked:" + what] += 1
        for tag in self.behind:
            c["behind:" + tag] += 1
        n, on = mv.N, [op.get("mask") is None or bool(op["mask"][i]) for i in range(mv.N)]
        c["world_changed"] += any(mv.envs[i].world_id != self.asked_world[i] for i in range(n))
        c["pending"] += bool(mv.pending.any())
        if "clear" in op:
            c["clear_bits"] += sum(1 for i in range(n) if on[i] and op["clear"][i])
        if what in ENTITY_AWARE and op.get("obstacles", WALLS_ENTS) == WALLS_ENTS:
            worlds, poses = self.source.worlds(), self.source.poses()
            carrying = [i for i in range(n) if on[i] and worlds[i]["carry"] >= 0]
            left = [(i, sorted(self.left_slots[i])) for i in range(n) if on[i] and self.left_slots[i]]
            c["carrying"] += bool(carrying)
            c["left"] += bool(left)
            # would the comparison have seen a stale list?  The restatement again, with the carried slot an obstacle / the slot re-listed
            is_now = {i: probe(op, worlds[i], poses[i], i) for i in set(carrying) | {i for i, _ in left}}
            c["carrying_matters"] += any(is_now[i] is not None and probe(op, dict(worlds[i], carry=-1), poses[i], i) != is_now[i] for i in carrying)
            matters = []
            for i, ks in left:
                kind = worlds[i]["kind"].copy()
                kind[ks] = np.asarray(mv.envs[i].sc["ents_kind"])[ks]
                if is_now[i] is not None and probe(op, dict(worlds[i], kind=kind), poses[i], i) != is_now[i]:
                    matters.append(i)
            c["left_matters"] += bool(matters)
            c["left_tail"] += any(self.left_tail[i] for i, _ in left)
            c["left_tail_matters"] += any(self.left_tail[i] for i in matters)
        self.asked_world = [e.world_id for e in mv.envs]
        for i in range(n):
            if on[i]:
                self.left_slots[i], self.left_tail[i] = set(), set()
        self.log.append(op)
        return answers

    # ---------------------------------------------------------------- drawing the inserted ops
    def _action(self, i):
        """as Generator._action, from this driver's own stream: a pickup where one would find something, else uniform"""
        rng, na, d = self.rng, self.cfg["n_actions"], self.mv.envs[i].dyn
        if na >= 5 and d.ag.carrying < 0:
            s, c = math.sin(d.ag.dir), math.cos(d.ag.dir)
            if d.intersect(-1, d.ag.pos[0] + c * 1.5 * d.ag.radius, d.ag.pos[2] - s * 1.5 * d.ag.radius, 1.2 * d.ag.radius) > 0 and rng.random() < 0.9:
                return 4
        return int(rng.integers(0, na))

    def _draw_frameless(self):
        """1 - 4 sub-steps; an env that could pick something up now turns on the spot first and picks up with its LAST sub-step: the
        removal then falls to the frameless call's own tail"""
        rng, n = self.rng, self.mv.N
        T = int(rng.choice([1, 1, 2, 3, 4]))
        last = [self._action(i) for i in range(n)]
        plans = [[(int(rng.integers(0, 2)) if last[i] == 4 else int(rng.integers(0, self.cfg["n_actions"]))) for i in range(n)] for _ in range(T - 1)] + [last]
        return {"kind": "rollout", "plans": plans, "trace": [None, True][int(rng.integers(0, 2))], "render": False}

    def _draw_query(self):
        rng, mv, n = self.rng, self.mv, self.mv.N
        asked = [self.counts["drawn:" + k] for k in self.kinds]
        least = [k for k, a in zip(self.kinds, asked) if a == min(asked)]
        what = least[int(rng.integers(0, len(least)))]
        self.counts["drawn:" + what] += 1
        op = {"kind": "query", "what": what}
        if what in ("raycast", "lidar"):
            op.update(rays=int(rng.choice([65, 5])), obstacles=[WALLS_ENTS, "walls"][int(rng.random() < 0.3)],
                      radius=[0.0, float(mv.envs[0].dyn.ag.radius)][int(rng.integers(0, 2))])
        elif what == "nav":
            e_ok = all(e.E > 0 and bool(e.dyn.ents[0].alive) and e.dyn.ag.carrying != 0 for e in mv.envs)
            op.update(target=0 if e_ok else None, points=None if e_ok else [[float(v) for v in e.dyn.ag.pos[:]] for e in mv.envs])
        elif what in ("seen", "scan"):
            op["clear"] = [int(e.world_id != self.map_world[what][i]) for i, e in enumerate(mv.envs)]
        elif what == "label":
            op.update(width=mv.W, height=mv.H)
        if what in ("seen", "ego9", "ego17"):
            op["fov"] = self.fov
        if what != "lidar" and rng.random() < P_MASK:
            op["mask"] = (rng.random(n) < 0.6).astype(int).tolist()
        return op

    def _query(self, op):
        self.answers = self._ask(op)
        if self.answers is None:
            return False
        if op["what"] in self.map_world:        # the envs this update met: their map now belongs to the world they are in
            for i, e in enumerate(self.mv.envs):
                if op.get("mask") is None or op["mask"][i]:
                    self.map_world[op["what"]][i] = e.world_id
        return True

    def _inserted(self):
        if self.rng.random() < (self.p_hot if self.hot else self.p_cold):
            op = self._draw_query()
            if self._query(op):
                yield op

    # ---------------------------------------------------------------- a sequence
    def ops(self, n_ops=N_OPS):
        for _ in range(n_ops):
            op = self.gen.draw(self.mv, self.bank)
            self._state_op(op)
            yield op
            yield from self._inserted()
            if self.cfg["kw"]["autoreset"] != "seeds" and self.rng.random() < self.p_frameless:
                op = self._draw_frameless()
                self._state_op(op)
                yield op
                yield from self._inserted()

    def replay(self, ops):
        """the ops of a log (or of a regression case) as data: nothing is drawn"""
        for op in ops:
            if op["kind"] == "query":
                assert self._query(op), ("a logged query was declined", op)
            else:
                self._state_op(op)
            yield op


def run_model(cfg_name, seed, n_ops=N_OPS, ops=None, **kw):
    """A sequence on the model alone: the driver behind it (its .mv, .log, .counts)."""
    d = Driver(cfg_name, seed, **kw)
    for _ in (d.ops(n_ops) if ops is None else d.replay(ops)):
        pass
    return d


def coverage_failures(cfg_name, counts):
    """The conditions a config's sequences must reach together (counts: the drivers' counts, summed over the seeds): those missed."""
    cfg = CONFIGS[cfg_name]
    need = {"asked:" + k: 8 for k in query_kinds(cfg)}
    need.update({"behind:" + k: 1 for k in BEHIND if k != "frameless" or cfg["kw"]["autoreset"] != "seeds"})
    need.update(world_changed=5, clear_bits=5)
    if cfg["cls"] == "PutNext":     # (PickupObjects takes what was picked up out of the world within the step: no env carries behind an op)
        need.update(carrying=3, carrying_matters=2)
    if cfg["cls"] == "PickupObjects":
        need.update(left=2, left_matters=1)
        if cfg["kw"]["autoreset"] != "seeds":       # ... and behind the last sub-step of a frameless rollout, where no frame's tail follows
            need.update(left_tail=2, left_tail_matters=1)
    if cfg["kw"]["autoreset"] == "next_step":
        need["pending"] = 2
    bad = [f"{k} {counts[k]} < {v}" for k, v in need.items() if counts[k] < v]
    if counts["dropped"] > DROP_CAP * counts["drawn"]:
        bad.append(f"dropped {counts['dropped']} of {counts['drawn']} queries: more than {DROP_CAP:.0%}")
    return bad
