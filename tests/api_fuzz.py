"""The seeded op generator of the stepping-API fuzzer, its configurations and its coverage conditions ("The API model and
its fuzzer").  No torch here: tests/test_engine_model_cpu.py runs the generator against the model alone, tests/test_gpu_api_fuzz.py
applies the same ops to the engine as well.

An op is a dict of plain Python values — {"kind": ..., lists, ints, floats} — complete in itself: applying a list of ops needs no
generator, so a failing prefix printed by the fuzzer can be pasted into a regression case as it stands."""
import collections
import math

import numpy as np

import engine_model

N_OPS = 120
SEEDS = (1, 2, 3)
BANK = 3            # snapshot slots

#   cls / env_id: the family; n: envs; episode: max_episode_steps (through _short_episodes, or the Maze's own argument);
#   kw: MiniWorldVecEnv's and the model's arguments; cache: the accelerated engine caches frames (the revisit conditions apply)
CONFIGS = {
    "hallway_seeds_final_stack_depth": dict(cls="Hallway", env_id="MiniWorld-Hallway-v0", n=7, task=1, n_actions=3, episode=8, cache=True,
                                            kw=dict(autoreset="seeds", final_obs=True, frame_stack=3, want_depth=True)),
    "hallway_next_step_zero_pad_81x61": dict(cls="Hallway", env_id="MiniWorld-Hallway-v0", n=7, task=1, n_actions=3, episode=7, cache=False,
                                             kw=dict(autoreset="next_step", frame_stack=3, stack_pad="zero", obs_width=81, obs_height=61)),
    "putnext_same_step": dict(cls="PutNext", env_id="MiniWorld-PutNext-v0", n=6, task=3, n_actions=8, episode=9, cache=True,
                              kw=dict(autoreset="same_step")),
    "pickup_dr_seeds_depth": dict(cls="PickupObjects", env_id="MiniWorld-PickupObjects-v0", n=5, task=2, n_actions=5, episode=8, cache=False,
                                  kw=dict(autoreset="seeds", domain_rand=True, want_depth=True)),
    "mazes3_same_step": dict(cls="MazeS3", env_id="MiniWorld-MazeS3-v0", n=3, task=1, n_actions=3, episode=None, cache=False,
                             kw=dict(autoreset="same_step", max_episode_steps=9)),
}

# op kind -> weight; "next_seed" is drawn in the "seeds" mode only (there is nothing to write in the others)
WEIGHTS = {"step": 30, "rollout": 10, "reset_where": 6, "next_seed": 5, "set_state_where": 10, "save_state": 9, "load_state": 11,
           "fork": 4, "state": 3, "render_top_view": 3, "get_visible_ents": 3, "frame_clean": 3, "frame_source": 3}
STATE_EXTRA = ("cam", "light", "num_picked_up", "ent_mesh", "ent_static", "ent_geom", "extent")


def op_kinds(cfg):
    return [k for k in WEIGHTS if k != "next_seed" or cfg["kw"]["autoreset"] == "seeds"]


def fuzz_seed(cfg_name, seed):
    """the seed of the env batch of (config, fuzz seed)"""
    return 1000 * (1 + list(CONFIGS).index(cfg_name)) + 37 * seed


def make_model(cfg_name, seed):
    """the model batch, reset; call under _short_episodes for the families whose class fixes the episode length"""
    from miniworld_amd import envs
    cfg = CONFIGS[cfg_name]
    kw = dict(cfg["kw"])
    mv = engine_model.ModelVec(getattr(envs, cfg["cls"]), cfg["n"], seed=fuzz_seed(cfg_name, seed), task=cfg["task"], **kw)
    mv.reset()
    return mv


class Generator:
    """Draws the ops of one sequence.  It looks at the model (for legal poses to write, for what the bank holds) and never at the
    engine."""

    def __init__(self, cfg_name, seed):
        self.cfg = CONFIGS[cfg_name]
        self.rng = np.random.default_rng([seed, list(CONFIGS).index(cfg_name)])
        self.kinds = op_kinds(self.cfg)
        w = np.array([WEIGHTS[k] for k in self.kinds], float)
        self.p = w / w.sum()
        self.last_turn = [0] * self.cfg["n"]
        self.queue = []             # ops decided ahead: the turns around an entity write (draw())

    # ---------------------------------------------------------------- actions
    def _action(self, mv, i):
        """biased as tests/test_gpu_frame_cache.py biases its actions: many turns, half of them undoing the env's last one, so that
        states return; the rest uniform (moves into walls and boxes are blocked: clean frames), and a pickup more often than not
        where the model says that one would find something (miniworld.py:695-702)"""
        rng, na = self.rng, self.cfg["n_actions"]
        u = rng.random()
        if na >= 5:
            d = mv.envs[i].dyn
            s, c = math.sin(d.ag.dir), math.cos(d.ag.dir)
            hit = d.intersect(-1, d.ag.pos[0] + c * 1.5 * d.ag.radius, d.ag.pos[2] - s * 1.5 * d.ag.radius, 1.2 * d.ag.radius)
            if d.ag.carrying < 0 and hit > 0 and rng.random() < 0.6:
                return 4
        if u < 0.45:
            a = 1 - self.last_turn[i] if rng.random() < 0.5 else int(rng.integers(0, 2))
            self.last_turn[i] = a
            return a
        if na >= 5 and u < 0.65:
            return 4
        if na > 5 and u < 0.72:
            return 5
        return int(rng.integers(0, na))

    def _actions(self, mv):
        return [self._action(mv, i) for i in range(self.cfg["n"])]

    def _mask(self, p):
        m = (self.rng.random(self.cfg["n"]) < p).astype(int)
        if not m.any():
            m[self.rng.integers(0, len(m))] = 1
        return m.tolist()

    # ---------------------------------------------------------------- legal poses
    def _pose(self, mv, i, stay=0.0):
        """a free agent pose for env i: in front of one of its entities, another env's, or its own jittered; every candidate is
        checked with the oracle's intersect in env i's world, and the env's own pose is what remains when none passes"""
        rng, e = self.rng, mv.envs[i]
        ag = e.dyn.ag
        for _ in range(0 if rng.random() < stay else 8):
            how = rng.random()
            movable = [k for k in range(e.E) if e.dyn.ents[k].alive and k != ag.carrying]
            if how < 0.4 and movable:
                k = movable[rng.integers(0, len(movable))]
                en = e.dyn.ents[k]
                th = float(rng.uniform(-math.pi, math.pi))
                d = float(en.radius) + float(ag.radius) + float(rng.uniform(0.02, 0.25))
                x, z = en.pos[0] - d * math.cos(th), en.pos[2] + d * math.sin(th)       # dir_vec = (cos, 0, -sin): facing the entity
            elif how < 0.7:
                o = mv.envs[rng.integers(0, mv.N)].dyn.ag
                x, z, th = o.pos[0], o.pos[2], float(o.dir)
            else:
                x, z = ag.pos[0] + float(rng.uniform(-0.4, 0.4)), ag.pos[2] + float(rng.uniform(-0.4, 0.4))
                th = float(ag.dir) + float(rng.uniform(-1, 1))
            if e.free_for_agent(x, z):
                return [float(x), float(ag.pos[1]), float(z)], th
        return [float(v) for v in ag.pos[:]], float(ag.dir)

    def _ent_row(self, mv, i):
        """env i's entity positions with one entity (alive, not carried) moved a little, to a place its own intersect calls free"""
        rng, e = self.rng, mv.envs[i]
        row = [[float(v) for v in e.dyn.ents[k].pos[:]] for k in range(e.E)]
        movable = [k for k in range(e.E) if e.dyn.ents[k].alive and k != e.dyn.ag.carrying]
        for _ in range(8 if movable else 0):
            k = movable[rng.integers(0, len(movable))]
            x, z = row[k][0] + float(rng.uniform(-0.3, 0.3)), row[k][2] + float(rng.uniform(-0.3, 0.3))
            if e.free_for_entity(k, x, z):
                row[k][0], row[k][2] = x, z
                break
        return row

    # ---------------------------------------------------------------- one op
    def draw(self, mv, bank):
        rng, cfg, n = self.rng, self.cfg, self.cfg["n"]
        if self.queue:
            what = self.queue.pop(0)
            if what in (0, 1):
                return {"kind": "step", "actions": [what] * n, "repeat": 1}
            mask = self._mask(0.6)
            return {"kind": "set_state_where", "mask": mask, "agent": {i: self._pose(mv, i, 1.0) for i in range(n) if mask[i]},
                    "ent_pos": {i: self._ent_row(mv, i) for i in range(n) if mask[i]}}
        kind = self.kinds[rng.choice(len(self.kinds), p=self.p)]
        filled = [s for s in range(BANK) if bank[s] is not None]
        if kind == "load_state" and not filled:
            kind = "save_state"
        if kind == "step":
            return {"kind": kind, "actions": self._actions(mv), "repeat": int(rng.choice([1, 1, 2, 5]))}
        if kind == "rollout":
            trace = [None, None, True, ["agent_pos", "ent_pos"]][rng.integers(0, 4)]
            return {"kind": kind, "plans": [self._actions(mv) for _ in range(int(rng.integers(1, 5)))], "trace": trace}
        if kind == "reset_where":
            return {"kind": kind, "mask": self._mask(0.3), "seeds": [int(s) for s in rng.integers(0, 2 ** 31, n)]}
        if kind == "next_seed":
            envs = np.flatnonzero(self._mask(0.4)).tolist()
            return {"kind": kind, "envs": envs, "values": [int(s) for s in rng.integers(0, 2 ** 31, len(envs))]}
        if kind == "set_state_where":
            mask = self._mask(0.3)
            # half of the writes that move an entity leave the agent where it stands: the poses it returns to afterwards are
            # poses it was drawn in with the entity elsewhere
            ents = rng.random() < 0.4 and mv.envs[0].E > 0
            if ents and rng.random() < 0.5:
                # left, right, the write with every agent where it stands, left, right: the poses behind the write are poses that
                # were drawn, with the entity elsewhere, two frames before it
                self.queue = [1, "write", 0, 1]
                return {"kind": "step", "actions": [0] * n, "repeat": 1}
            op = {"kind": kind, "mask": mask, "agent": {i: self._pose(mv, i, 0.5 if ents else 0.1) for i in range(n) if mask[i]}}
            if ents:
                op["ent_pos"] = {i: self._ent_row(mv, i) for i in range(n) if mask[i]}
            return op
        if kind == "save_state":
            s = int(rng.integers(0, BANK))
            if bank[s] is not None and rng.random() < 0.4:
                # into an existing snapshot: over records it holds, and at most one appended
                snap = bank[s]
                m = int(rng.integers(1, min(n, snap.count + (snap.count < snap.capacity)) + 1))
                recs = rng.permutation(snap.count)[:m].tolist()
                if len(recs) < m:
                    recs.append(snap.count)
                elif snap.count < snap.capacity and rng.random() < 0.5:
                    recs[-1] = snap.count
                return {"kind": kind, "slot": s, "into": True, "envs": rng.permutation(n)[:m].tolist(), "records": [int(r) for r in recs]}
            envs = None if rng.random() < 0.4 else rng.permutation(n)[:int(rng.integers(1, n + 1))].tolist()
            return {"kind": kind, "slot": s, "into": False, "envs": envs, "frames": bool(rng.random() < 0.5)}
        if kind == "load_state":
            s = filled[rng.integers(0, len(filled))]
            snap = bank[s]
            frames = [None, False, True][rng.integers(0, 3)] if snap.with_frames else [None, False][rng.integers(0, 2)]
            form = ["list", "masked", "whole"][rng.integers(0, 3)]
            if form == "whole":
                return {"kind": kind, "slot": s, "form": form, "frames": frames}
            if form == "list":
                m = int(rng.integers(1, n + 1))
                return {"kind": kind, "slot": s, "form": form, "frames": frames, "envs": rng.permutation(n)[:m].tolist(),
                        "records": [int(r) for r in rng.integers(0, snap.count, m)]}
            return {"kind": kind, "slot": s, "form": form, "frames": bool(frames), "mask": self._mask(0.4),
                    "records": [int(r) for r in rng.integers(0, snap.count, n)]}
        if kind == "fork":
            return {"kind": kind, "src": [int(j) for j in rng.integers(0, n, n)], "frames": bool(rng.random() < 0.5)}
        if kind == "state":
            k = int(rng.integers(0, len(STATE_EXTRA) + 1))
            return {"kind": kind, "fields": None if k == 0 else ["agent_pos", "ent_kind"] + list(STATE_EXTRA[:k])}
        if kind == "render_top_view":
            return {"kind": kind, "render_agent": bool(rng.random() < 0.5)}
        return {"kind": kind}


def state_write_arrays(op, n, E):
    """set_state_where's arrays of an op: rows of the unmasked envs are NaN (they are not read)"""
    pos, d = np.full((n, 3), np.nan), np.full(n, np.nan)
    for i, (p, th) in op["agent"].items():
        pos[int(i)], d[int(i)] = p, th
    out = {"agent_pos": pos, "agent_dir": d}
    if "ent_pos" in op:
        ep = np.full((n, E, 3), np.nan)
        for i, row in op["ent_pos"].items():
            ep[int(i)] = 0.0
            ep[int(i), :len(row)] = row
        out["ent_pos"] = ep
    return out


def apply_model(mv, bank, op):
    """the op on the model batch; `bank` holds the model's snapshots, slot by slot"""
    kind = op["kind"]
    if kind == "reset":         # (not drawn by the generator: for regression cases)
        mv.reset(op["seed"])
    elif kind == "step":
        mv.step(op["actions"], repeat=op["repeat"])
    elif kind == "rollout":
        mv.rollout(np.array(op["plans"]), trace=op["trace"])
    elif kind == "reset_where":
        mv.reset_where(op["mask"], op["seeds"])
    elif kind == "next_seed":
        mv.next_seed[op["envs"]] = op["values"]
    elif kind == "set_state_where":
        mv.set_state_where(op["mask"], **state_write_arrays(op, mv.N, max(1, mv.envs[0].E)))
    elif kind == "save_state":
        s = op["slot"]
        if op["into"]:
            mv.save_state(op["envs"], into=bank[s], records=op["records"])
        else:
            bank[s] = mv.save_state(op["envs"], capacity=mv.N, frames=op["frames"])
    elif kind == "load_state":
        snap = bank[op["slot"]]
        if op["form"] == "masked":
            mv.load_state_where(snap, op["mask"], op["records"], op["frames"])
        else:
            mv.load_state(snap, op.get("envs"), op.get("records"), op["frames"])
    elif kind == "fork":
        mv.fork(op["src"], frames=op["frames"])
    # state() and the side calls read: nothing of the model changes


def run_model(cfg_name, seed, n_ops=N_OPS, ops=None):
    """A sequence on the model alone: (model, ops, op-kind counts).  `ops`: apply these instead of drawing."""
    mv, bank = make_model(cfg_name, seed), [None] * BANK
    gen, log = Generator(cfg_name, seed), []
    for t in range(n_ops if ops is None else len(ops)):
        op = gen.draw(mv, bank) if ops is None else ops[t]
        apply_model(mv, bank, op)
        log.append(op)
    return mv, log, collections.Counter(op["kind"] for op in log)


def coverage_failures(cfg_name, kinds, cov):
    """The coverage conditions a config's three sequences must reach together (kinds, cov: their summed op counts and model
    bookkeeping); returns the list of those missed."""
    cfg = CONFIGS[cfg_name]
    mode, bad = cfg["kw"]["autoreset"], []
    for k in op_kinds(cfg):
        if kinds[k] < 5:
            bad.append(f"op {k} drawn {kinds[k]} < 5 times")
    need = {"ends": 10, "early_ends": 2, "loads_on_moved": 3}
    if mode == "next_step":
        need["hit_pending"] = 2
    if cfg["cls"] == "PutNext":
        need["hit_carrying"] = 2
    if cfg["cls"] == "PickupObjects":
        need["hit_after_pickup"] = 1
    if cfg["cache"]:
        need.update(revisits=15, identical=15)
    for k, v in need.items():
        if cov[k] < v:
            bad.append(f"{k} {cov[k]} < {v}")
    return bad


def format_ops(ops):
    return "[\n" + "".join(f"  {op!r},\n" for op in ops) + "]"
