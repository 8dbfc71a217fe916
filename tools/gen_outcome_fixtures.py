"""Generates tests/golden/out_*.npz: reference episodes that REACH their outcome (FIXTURE TOOLING).

tools/gen_golden.py drives the reference with random policies, which almost never finish a task.  Here the unmodified reference
(under tools/refshim.py's GL stubs) is driven by a scripted expert: waypoints from a grid search over the env's own wall
segments (tests/nav_reference.py's occupancy and Dijkstra), a turn to within half a turn step, forward, and pickup / drop where
the case says so.  The expert decides from the live reference state only, so the per-step draws of domain randomisation do not
matter to it.  Every case runs twice: once to find the actions, once to record them with the three stored frames known (first,
middle, terminal).

A file has gen_golden.py's layout (s0/ tr/ obs/ meta/: conftest.golden_cases() lists it, every test parametrized over that list
runs it) and
  * meta/outcome   what the last executed step shows, by tests/test_outcome_fixtures_cpu.py's outcome_holds (asserted here too),
  * meta/after     how many steps were taken past the episode's end (PickupObjects: the emptied room),
  * s1/...         the reference's scene after env.reset() WITHOUT a seed behind the last step: the next world of the same stream.
A frame stored for step t is the scene the reference's step() rendered: it is snapshotted inside a wrapped env.render_obs, so a
step whose rule removes an object behind the render (pickupobjects.py:86-88) still shows it, as the reference's observation does.
Files are written with fixed zip timestamps: a second run reproduces them byte for byte.

Usage (where the reference tree exists):  python tools/gen_outcome_fixtures.py [case ...] [--check]
"""
import io
import math
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import gen_golden  # noqa: E402
import nav_reference as nav  # noqa: E402
import pyoracle  # noqa: E402
import refscene  # noqa: E402
import refshim  # noqa: E402
from test_outcome_fixtures_cpu import outcome_holds  # noqa: E402  (the plain-Python statement of every outcome)

OUT = os.path.join(HERE, "..", "tests", "golden")
MAX_FILE_BYTES = 78 * 1024          # the largest trajectory fixture before these
TURN_LEFT, TURN_RIGHT, FORWARD, BACK, PICKUP, DROP = range(6)

# (case name, env class, kwargs, seed, script, script arguments, outcome, steps past the end)
CASES = [
    ("out_hallway_s7", "Hallway", {}, 7, "goto", {}, "success", 0),
    ("out_hallway_dr_s1", "Hallway", {"domain_rand": True}, 1, "goto", {}, "success", 0),
    ("out_onerooms6_s0", "OneRoomS6", {}, 0, "goto", {}, "success", 0),
    ("out_onerooms6fast_s0", "OneRoomS6Fast", {}, 0, "goto", {}, "success", 0),
    ("out_mazes2_s0", "MazeS2", {}, 0, "goto", {}, "success", 0),
    ("out_mazes3fast_s0", "MazeS3Fast", {}, 0, "goto", {}, "success", 0),
    ("out_maze_s0", "Maze", {}, 0, "goto", {}, "success", 0),
    ("out_fourrooms_s0", "FourRooms", {}, 0, "goto", {}, "success", 0),
    ("out_fourrooms_dr_s1", "FourRooms", {"domain_rand": True}, 1, "goto", {}, "success", 0),
    ("out_tmazeleft_s0", "TMazeLeft", {}, 0, "goto", {}, "success", 0),
    ("out_tmazeright_s0", "TMazeRight", {}, 0, "goto", {}, "success", 0),
    ("out_ymazeright_s0", "YMazeRight", {}, 0, "goto", {}, "success", 0),
    ("out_wallgap_s0", "WallGap", {}, 0, "goto", {}, "success", 0),
    # aimed episode length: max_episode_steps = the expert's success step T (filled in by main) and T - 1
    ("out_oneroom_len_t_s1", "OneRoom", {"max_episode_steps": "T"}, 1, "goto", {}, "success_and_truncated", 0),
    ("out_oneroom_len_tm1_s1", "OneRoom", {"max_episode_steps": "T-1"}, 1, "goto", {}, "truncated_one_short", 0),
    ("out_sign_box_s0", "Sign", {"goal": 0, "color_index": 0}, 0, "sign", {}, "sign_plus_box", 0),
    ("out_sign_key_s1", "Sign", {"goal": 1, "color_index": 2}, 1, "sign", {}, "sign_plus_key", 0),
    ("out_sidewalk_s0", "Sidewalk", {}, 0, "sidewalk", {}, "success", 0),
    ("out_sidewalk_street_box", "Sidewalk", {}, None, "street_box", {}, "street_and_box", 0),
    ("out_pickup_all_s0", "PickupObjects", {}, 0, "collect", {}, "all_collected", 3),
    ("out_pickup_all_dr_s1", "PickupObjects", {"domain_rand": True}, 1, "collect", {}, "all_collected", 3),
    ("out_putnext_s3", "PutNext", {}, 3, "putnext", {}, "put_next", 0),
    ("out_collecthealth_none_s0", "CollectHealth", {}, 0, "idle", {}, "health_out", 0),
    ("out_collecthealth_kits_s1", "CollectHealth", {}, 1, "kits", {"kits": 4}, "kits_then_health_out", 0),
]
STREET_BOX_SEEDS = 200


# ------------------------------------------------------------------------------------------------ the expert

def _ents(env):
    return [e for e in env.entities if e is not env.agent]


class Navigator:
    """Waypoints towards one entity over a grid of the env's wall segments; fields are kept per (target, obstacles) key."""

    def __init__(self, env, cell=0.25, extra_segs=(), inflate=None):
        self.env, self.cell, self.inflate = env, cell, inflate or {}
        segs = np.asarray(env.wall_segs, np.float64)[:, :, [0, 2]].reshape(-1, 4)
        if len(extra_segs):
            segs = np.concatenate([segs, np.asarray(extra_segs, np.float64).reshape(-1, 4)])
        self.segs = segs
        self.extent = np.array([env.min_x, env.max_x, env.min_z, env.max_z], np.float64)
        self.shape = nav.grid_shape(self.extent, cell)
        self.fields = {}

    def _world(self, target):
        env = self.env
        ents = _ents(env)
        kind = np.array([0 if type(e).__name__ in ("ImageFrame", "TextFrame") else 1 for e in ents])
        radius = np.array([float(e.radius) + self.inflate.get(id(e), 0.0) for e in ents])
        carry = ents.index(env.agent.carrying) if env.agent.carrying is not None else -1
        return {"segs": self.segs, "extent": self.extent, "kind": kind, "pos": np.array([e.pos for e in ents], np.float64).reshape(-1, 3),
                "radius": radius, "carry": carry, "agent_radius": float(env.agent.radius), "max_forward_step": float(env.max_forward_step)}, ents.index(target)

    def field(self, target):
        w, slot = self._world(target)
        key = (slot, w["carry"], w["pos"].tobytes())
        if key not in self.fields:
            gx, gz = self.shape
            blocked, _ = nav.occupancy(w, self.cell, gx, gz, self.cell / 2, True, slot)
            x, z = nav.centres(self.extent, self.cell, gx, gz)
            X, Z = np.meshgrid(x, z)
            d = np.sqrt((w["pos"][slot][0] - X) ** 2 + (w["pos"][slot][2] - Z) ** 2)
            reach = float(target.radius) + w["agent_radius"] + 1.1 * w["max_forward_step"]
            cost = nav.dijkstra(blocked, (d < reach) & ~blocked)
            f = np.where(cost != np.iinfo(np.int64).max, np.minimum(cost, nav.UNREACHED - 1), nav.UNREACHED)
            f[blocked] = nav.BLOCKED
            self.fields = {key: (f.astype(np.uint16), blocked)}
        return self.fields[key]

    def _clear(self, blocked, x0, z0, x1, z1):
        n = max(2, int(math.hypot(x1 - x0, z1 - z0) / (self.cell / 2)) + 1)
        gz, gx = blocked.shape
        for s in np.linspace(0.0, 1.0, n):
            i = int(math.floor((x0 + s * (x1 - x0) - self.extent[0]) / self.cell))
            j = int(math.floor((z0 + s * (z1 - z0) - self.extent[2]) / self.cell))
            if not (0 <= i < gx and 0 <= j < gz) or blocked[j, i]:
                return False
        return True

    def waypoint(self, target, lookahead=12):
        """(x, z) to head for: the target itself once its reach is entered, else the farthest cell in free sight down the field"""
        f, blocked = self.field(target)
        pos = self.env.agent.pos
        x, z = float(pos[0]), float(pos[2])
        txz = (float(target.pos[0]), float(target.pos[2]))
        cost, nxt, wx, wz = nav.query(f, self.extent, self.cell, txz, x, z)
        if cost <= 0:
            return txz
        best = (wx, wz)
        for _ in range(lookahead):
            cost, nxt, nx, nz = nav.query(f, self.extent, self.cell, txz, wx, wz)
            if cost <= 0 or not self._clear(blocked, x, z, nx, nz):
                break
            wx, wz = nx, nz
            best = (wx, wz)
        return best


def _turn_step(env):
    return math.radians(float(env.params.sample(None, "turn_step")))           # (no stream: the parameter's default)


def _head_for(env, wx, wz):
    return nav.follow(env.agent.pos, float(env.agent.dir), wx, wz, _turn_step(env))


def _would_pick(env, target):
    test_pos = env.agent.pos + env.agent.dir_vec * 1.5 * env.agent.radius
    return env.intersect(env.agent, test_pos, 1.2 * env.agent.radius) is target


def script_goto(env, args):
    navi = Navigator(env)
    while True:
        yield _head_for(env, *navi.waypoint(env.box))


def script_sign(env, args):
    """towards the object the sign names, with a wide berth round the five others (touching one ends the episode with -1)"""
    target = env._objects[env._goal][env._color_index]
    others = {id(o): 1.1 * env.max_forward_step + 0.3 for pair in env._objects for o in pair if o is not target}
    navi = Navigator(env, inflate=others)
    while True:
        yield _head_for(env, *navi.waypoint(target))


def script_sidewalk(env, args):
    """along the sidewalk: the kerb (x = 0, z in 0 .. 12) counts as a wall"""
    navi = Navigator(env, extra_segs=[[0.0, 0.0, 0.0, 12.0]])
    while True:
        yield _head_for(env, *navi.waypoint(env.box))


def script_collect(env, args):
    navi = Navigator(env)
    while True:
        live = [e for e in _ents(env) if not e.is_static]
        if not live:
            yield FORWARD           # the emptied room: the steps past the end
            continue
        target = min(live, key=lambda e: float(np.linalg.norm(e.pos - env.agent.pos)))
        yield PICKUP if _would_pick(env, target) else _head_for(env, *navi.waypoint(target))


def script_putnext(env, args):
    navi = Navigator(env)
    red, yellow = env.red_box, env.yellow_box
    while True:
        if env.agent.carrying is None:
            yield PICKUP if _would_pick(env, red) else _head_for(env, *navi.waypoint(red))
        else:
            d = math.hypot(red.pos[0] - yellow.pos[0], red.pos[2] - yellow.pos[2])
            if math.sqrt(d * d + yellow.pos[1] ** 2) < red.radius + yellow.radius + 1.1 * env.max_forward_step:
                yield DROP
            else:
                yield _head_for(env, *navi.waypoint(yellow))


def script_idle(env, args):
    while True:
        yield TURN_LEFT


def script_kits(env, args):
    navi = Navigator(env)
    taken = 0
    while True:
        if taken >= args["kits"]:
            yield TURN_LEFT
            continue
        target = min(_ents(env), key=lambda e: float(np.linalg.norm(e.pos - env.agent.pos)))
        if _would_pick(env, target):
            taken += 1
            yield PICKUP
        else:
            yield _head_for(env, *navi.waypoint(target))


def street_box_plan(env):
    """Sidewalk: an action list whose LAST forward step both enters the street (x > 0) and comes within `near` of the box, with no
    earlier step doing either — two straight legs on headings the turn step allows, searched on the plain kinematics (no wall or
    entity is within reach on such a path; the reference run that records the case is what decides).  None if the seed has none."""
    a, box = env.agent, env.box
    step, turn = float(env.params.sample(None, "forward_step")), _turn_step(env)
    near = box.radius + a.radius + 1.1 * env.max_forward_step
    touch = box.radius + a.radius
    bx, bz = float(box.pos[0]), float(box.pos[2])
    best = None
    for kg in range(-12, 13):
        g = float(a.dir) + kg * turn
        ug = np.array([math.cos(g), -math.sin(g)])
        for kh in range(-12, 13):
            h = float(a.dir) + kh * turn
            uh = np.array([math.cos(h), -math.sin(h)])
            if uh[0] <= 1e-9:
                continue
            for m in range(0, 90):
                q = np.array([a.pos[0], a.pos[2]]) + m * step * ug
                if not (-3 + a.radius + 0.05 < q[0] < -1e-6 and a.radius + 0.05 < q[1] < 12 - a.radius - 0.05):
                    break
                if math.hypot(q[0] - bx, q[1] - bz) < near + 1e-6:
                    break
                for n in range(1, 40):
                    p = q + n * step * uh
                    d = math.hypot(p[0] - bx, p[1] - bz)
                    if p[0] > 1e-6:
                        if d < near - 1e-6 and d > touch + 0.02:
                            cost = abs(kg) + m + abs(kh - kg) + n
                            if best is None or cost < best[0]:
                                best = (cost, kg, m, kh, n)
                        break
                    if d < near + 1e-6 or not (a.radius + 0.05 < p[1] < 12 - a.radius - 0.05):
                        break
    if best is None:
        return None
    _, kg, m, kh, n = best

    def turns(k):
        return [TURN_LEFT if k > 0 else TURN_RIGHT] * abs(k)
    return turns(kg) + [FORWARD] * m + turns(kh - kg) + [FORWARD] * n


SCRIPTS = {"goto": script_goto, "sign": script_sign, "sidewalk": script_sidewalk, "collect": script_collect, "putnext": script_putnext,
           "idle": script_idle, "kits": script_kits}


# ------------------------------------------------------------------------------------------------ running a case

def _make(cls, kwargs, seed):
    env = refshim.make_env(cls, **kwargs)
    log = gen_golden.log_param_draws(env)
    env.reset(seed=seed)
    return env, log


def find_actions(cls, kwargs, seed, script, args, after, plan=None):
    """first run: the expert's actions up to the episode's end, then `after` more"""
    env, _ = _make(cls, kwargs, seed)
    gen = iter(plan) if plan is not None else SCRIPTS[script](env, args)
    actions, end = [], None
    for _ in range(int(min(float(env.max_episode_steps), 4000)) + after):
        try:
            a = int(next(gen))
        except StopIteration:
            break
        _, _, term, trunc, _ = env.step(a)
        actions.append(a)
        if end is None and (term or trunc):
            end = len(actions)
        if end is not None and len(actions) == end + after:
            break
    return actions, end


def record(name, cls, kwargs, seed, actions, end, outcome, after):
    """second run: gen_golden.run_case's recording of the given actions, frames snapshotted inside render_obs"""
    import helpers
    env, log = _make(cls, kwargs, seed)
    s0 = refscene.scene_from_ref_env(env)
    ents0 = _ents(env)
    frames = sorted({0, end // 2, end, end + after})
    tr = {k: [] for k in gen_golden.TR_KEYS}
    scenes = {0: s0}
    orig_render = env.render_obs
    shot = {}

    def render_obs(*a, **k):
        if env.step_count in frames:
            shot["scene"] = refscene.scene_from_ref_env(env)
            shot["pos"] = np.array([e.pos for e in ents0], np.float64).reshape(len(ents0), 3)
            shot["dir"] = np.array([e.dir for e in ents0], np.float64)
            shot["alive"] = np.array([any(e is x for x in env.entities) for e in ents0])
        return orig_render(*a, **k)
    env.render_obs = render_obs
    for t, a in enumerate(actions):
        del log[:]
        obs, rew, term, trunc, info = env.step(a)
        gen_golden.record_step(tr, env, ents0, a, rew, term, trunc, log)
        if (t + 1) in frames:
            sc = shot["scene"]
            full = dict(s0)
            full.update({k: sc[k] for k in ("agent_pos", "agent_dir", "agent_carrying", "step_count")})
            full["ents_pos"], full["ents_dir"] = shot["pos"], shot["dir"]
            full["ents_kind"] = np.where(shot["alive"], s0["ents_kind"], 0).astype(np.int32)
            scenes[t + 1] = sc if cls == "CollectHealth" else full      # (respawned kits move to the list's end: the live order)
    out = gen_golden.pack_case(s0, tr, env, ents0, cls, kwargs, seed, int(env.action_space.n), np.array([-1, 0, 0, 0, 0], np.float64))
    out["meta/outcome"], out["meta/after"], out["meta/end"] = np.array(outcome), np.int32(after), np.int32(end)
    shows = outcome_holds(outcome, {k[3:]: v for k, v in out.items() if k.startswith("tr/")}, {k[5:]: v for k, v in out.items() if k.startswith("meta/")},
                          end, float(env.max_episode_steps))
    assert shows, (name, "the run does not show", outcome, tr["reward"][end - 1])
    meshes = helpers.golden_meshes(s0)
    for e in ents0:          # the committed mesh arrays are the reference's own
        if hasattr(e, "mesh"):
            assert np.array_equal(refscene.ref_mesh_arrays(e.mesh)["verts"], meshes[refscene.mesh_name_of(e)]["verts"]), name
    for k, sc in scenes.items():
        r = pyoracle.render(sc, meshes=meshes)
        out[f"obs/{k}/rgb"], out[f"obs/{k}/z16"] = r["rgb"], r["z16"]
        out[f"obs/{k}/top_rgb"] = pyoracle.render(sc, meshes=meshes, view="top", render_agent=True)["rgb"]
        for key in ("agent_pos", "agent_dir", "ents_pos", "ents_dir", "ents_kind"):
            out[f"obs/{k}/{key}"] = sc[key]
    out["meta/frames"] = np.array(sorted(scenes), np.int32)
    env.render_obs = orig_render
    env.reset()                                   # no seed: the stream goes on
    for k, v in refscene.scene_from_ref_env(env).items():
        out["s1/" + k] = v
    return out


def npz_bytes(arrays):
    """np.savez_compressed with fixed member timestamps"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue(), compresslevel=9)
    return buf.getvalue()


def build_case(name, cls, kwargs, seed, script, args, outcome, after, success_t):
    kwargs = dict(kwargs)
    if kwargs.get("max_episode_steps") in ("T", "T-1"):
        kwargs["max_episode_steps"] = success_t[(cls, seed)] - (kwargs["max_episode_steps"] == "T-1")
    plan = None
    if script == "street_box":
        for seed in range(STREET_BOX_SEEDS):
            env, _ = _make(cls, kwargs, seed)
            plan = street_box_plan(env)
            if plan is not None:
                actions, end = find_actions(cls, kwargs, seed, script, args, after, plan)
                if end == len(plan):
                    break
                plan = None
        if plan is None:
            raise RuntimeError(f"{name}: none of {STREET_BOX_SEEDS} seeds allows the step")
    actions, end = find_actions(cls, kwargs, seed, script, args, after, plan)
    assert end is not None and len(actions) == end + after, (name, "the episode did not end", len(actions))
    return npz_bytes(record(name, cls, kwargs, seed, actions, end, outcome, after)), seed, end


def main():
    argv = sys.argv[1:]
    check = "--check" in argv
    only = {a for a in argv if not a.startswith("--")}
    success_t = {}
    for cls, seed in {(c[1], c[3]) for c in CASES if c[2].get("max_episode_steps") in ("T", "T-1")}:
        success_t[(cls, seed)] = find_actions(cls, {}, seed, "goto", {}, 0)[1]
    total, bad = 0, []
    for case in CASES:
        name = case[0]
        path = os.path.join(OUT, name + ".npz")
        if only and name not in only:
            continue
        data, seed, end = build_case(*case, success_t)
        assert len(data) <= MAX_FILE_BYTES, (name, len(data))
        total += len(data)
        if check:
            with open(path, "rb") as f:
                same = f.read() == data
            bad += [] if same else [name]
        else:
            with open(path, "wb") as f:
                f.write(data)
        print(f"{name}: seed={seed} end={end} bytes={len(data)}" + (" (checked)" if check else ""))
    assert total < 1.5 * 2 ** 20, total
    print("total", total, "bytes")
    if bad:
        raise SystemExit(f"not reproduced byte for byte: {bad}")


if __name__ == "__main__":
    main()
