"""Shared test helpers: golden fixtures -> neutral scenes -> engine state."""
import os

import numpy as np

from engine_model import ModelEnv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_case(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    s0 = {k[3:]: d[k] for k in d.files if k.startswith("s0/")}
    tr = {k[3:]: d[k] for k in d.files if k.startswith("tr/")}
    meta = {k[5:]: d[k] for k in d.files if k.startswith("meta/")}
    obs = {}
    for k in d.files:
        if k.startswith("obs/"):
            _, fr, key = k.split("/")
            obs.setdefault(int(fr), {})[key] = d[k]
    return s0, tr, meta, obs


def carry_cases(prefix=""):
    """Names of the carried-object fixtures (tests/golden/carry/, tools/gen_carry_fixtures.py) that start with `prefix`."""
    return sorted(f[:-4] for f in os.listdir(os.path.join(GOLDEN, "carry")) if f.endswith(".npz") and f.startswith(prefix))


def load_carry_case(name):
    """(s0, tr, meta, poke) of a carried-object fixture; poke: the starting states of a threshold file's single steps, else empty."""
    d = np.load(os.path.join(GOLDEN, "carry", name + ".npz"))
    return tuple({k[len(p):]: d[k] for k in d.files if k.startswith(p)} for p in ("s0/", "tr/", "meta/", "poke/"))


def placement_cases(prefix=""):
    """Names of the placement fixtures (tests/golden/placement/, tools/gen_placement_fixtures.py) that start with `prefix`."""
    return sorted(f[:-4] for f in os.listdir(os.path.join(GOLDEN, "placement")) if f.endswith(".npz") and f.startswith(prefix))


def load_placement_case(name):
    """(world, case, meta, poke) of a placement fixture; poke: the state before the respawn case's one step, else empty."""
    d = np.load(os.path.join(GOLDEN, "placement", name + ".npz"))
    return tuple({k[len(p):]: d[k] for k in d.files if k.startswith(p)} for p in ("w/", "case/", "meta/", "poke/"))


def world_of_scene(sc):
    """The w/ arrays of a placement fixture from a neutral scene (scene.scene_from_env of a host env, scene_of_vec_env of a
    device env): what test_gpu_env_api._assert_same_world compares — poses, kinds, mesh names, a box's size and colour, a
    mesh's scale and radius, the per-episode parameters — and the texture variant of every room polygon."""
    live = np.asarray(sc["ents_kind"]) != 0
    box = (np.asarray(sc["ents_kind"])[live] == 1)[:, None]
    names = [str(n) for n in sc["mesh_names"]]
    room = [i for i in range(len(sc["polys_nv"])) if not sc["polys_nv"][i] & 0x100]
    return {
        "agent_pos": np.asarray(sc["agent_pos"], np.float64), "agent_dir": np.float64(sc["agent_dir"]),
        "cam": np.array([sc["cam_height"], sc["cam_fwd_disp"], sc["cam_pitch"], sc["cam_fov_y"]], np.float64),
        "light": np.concatenate([sc["sky"], sc["light_pos"], sc["light_color"], sc["light_ambient"]]).astype(np.float64),
        "ents_kind": np.asarray(sc["ents_kind"])[live], "ents_pos": np.asarray(sc["ents_pos"])[live], "ents_dir": np.asarray(sc["ents_dir"])[live],
        "ents_size": np.where(box, np.asarray(sc["ents_size"])[live], 0.0), "ents_color": np.where(box, np.asarray(sc["ents_color"])[live], 1.0),
        "ents_scale": np.asarray(sc["ents_scale"])[live], "ents_radius": np.asarray(sc["ents_radius"])[live],
        "ents_mesh_name": np.array([names[m] if m >= 0 else "" for m in np.asarray(sc["ents_mesh"])[live]]),
        "polys_tex_name": np.array([str(sc["tex_names"][sc["polys_tex"][i]]) for i in room]),
    }


def assert_world_equal(got, want, tag):
    """Exact equality, field by field."""
    assert sorted(got) == sorted(want), (tag, sorted(got), sorted(want))
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (tag, k, got[k], want[k])


def poked_scene(s0, poke, k):
    """Scene s0 with the starting state of threshold case k substituted."""
    sc = dict(s0)
    sc["agent_pos"], sc["agent_dir"], sc["agent_carrying"] = poke["agent_pos"][k], poke["agent_dir"][k], poke["carrying"][k]
    sc["ents_pos"], sc["ents_dir"] = poke["ents_pos"][k], poke["ents_dir"][k]
    return sc


def golden_meshes(scene):
    """mesh name -> arrays dict for oracle.pyoracle.render, from tests/golden/meshes.npz."""
    d = np.load(os.path.join(GOLDEN, "meshes.npz"))
    out = {}
    for name in [str(m) for m in scene.get("mesh_names", [])]:
        base = name.split("_")[0]
        base = base if f"{base}/verts" in d.files else name        # ball / key geometry is stored once per shape
        m = {k: d[f"{base}/{k}"] for k in ("verts", "norms", "texcs")}
        kd = d["kd:" + name] if ("kd:" + name) in d.files else np.ones(3)
        m["colors"] = np.broadcast_to(kd.astype(np.float32), m["verts"].shape).copy()
        out[name] = m
    return out


def frame_scene(s0, frame):
    """Scene s0 with the agent/entity state of a stored frame substituted."""
    sc = dict(s0)
    for k in ("agent_pos", "agent_dir", "ents_pos", "ents_dir", "ents_kind"):
        sc[k] = frame[k]
    return sc


def task_of(meta):
    if rule_of(meta) != "engine":
        return 0
    return {"PickupObjects": 2, "PutNext": 3, "RoomObjects": 0, "ThreeRooms": 0}.get(str(meta["env"]), 1)


def rule_of(meta):
    """"engine": the env's reward / termination rule is one of K1's task rules; "host": it is Python on top
    of the engine's physics (C-level tests compare poses only); "api_only": the host also moves entities."""
    return str(meta["rule"]) if "rule" in meta else "engine"


def env_kwargs_of(meta):
    import ast
    kw = ast.literal_eval(str(meta["kwargs"])) if "kwargs" in meta else {}
    if bool(meta["domain_rand"]):
        kw["domain_rand"] = True
    return kw


def goals_of(meta):
    return int(meta.get("goal_ent", 0)), int(meta.get("goal_ent2", -1))


# ------------------------------------------------------------------ the engine without a device (CPU tests)

class RecordingLib:
    """Stands in for libmwengine.so: every entry point succeeds and is written down — `calls`, (name, args) in order; `returns` maps an
    entry point's name to what it returns instead of 0 (mw_snapshot_bytes -> 4096); `engines` are the Engines opened on it."""

    def __init__(self, returns=None):
        self.calls, self.engines, self.returns = [], [], dict(returns or {})

    def __getattr__(self, name):
        if not name.startswith("mw_"):
            raise AttributeError(name)
        rc = self.returns.get(name, 0)

        def call(*args):
            self.calls.append((name, args))
            return rc
        return call


def stub_engine(monkeypatch, returns=None):
    """engine.Engine without a device: the real class over a RecordingLib, tensors on the CPU.  Only Engine._open() is replaced (the
    library, the device, the handle); every host attribute is the real __init__'s.  Returns the library."""
    import torch
    from miniworld_amd import engine
    lib = RecordingLib(returns)

    def open_(self):
        lib.engines.append(self)
        self.lib, self.device, self.h = lib, torch.device("cpu"), 1
    monkeypatch.setattr(engine.Engine, "_open", open_)
    monkeypatch.setattr(engine.Engine, "close", lambda self: None)
    monkeypatch.setattr(engine, "_stream_ptr", lambda device=None: None)       # (no HIP stream without a device)
    return lib


# ------------------------------------------------------------------ engine glue (GPU tests)

def make_engine_for_scene(s0, n_envs, task=1, max_episode_steps=None, domain_rand=False, max_visible=None,
                          goal_ent=0, goal_ent2=-1, agent_radius=0.4, msaa=8, width=80, height=60):
    """Engine with the scene's shared geometry / textures uploaded (state not yet set)."""
    from miniworld_amd import engine as eng
    from miniworld_amd import assets
    cfg = eng.MwConfig()
    E = max(1, len(s0["ents_kind"]))
    P, S = len(s0["polys_nv"]), len(s0["wall_segs"])
    cfg.device_id = 0
    cfg.num_envs = n_envs
    cfg.obs_width, cfg.obs_height, cfg.msaa = width, height, msaa
    cfg.max_ents, cfg.max_polys, cfg.max_segs = E, P, S
    cfg.max_visible = max_visible or -(-(P + 6 * E) // 16) * 16
    cfg.shared_geometry = 1
    cfg.task = task
    cfg.goal_ent, cfg.goal_ent2 = goal_ent, goal_ent2
    cfg.num_objs = len(s0["ents_kind"])
    mes = max_episode_steps if max_episode_steps is not None else s0["max_episode_steps"]
    cfg.max_episode_steps = int(min(float(mes), 2 ** 30))
    cfg.domain_rand = int(domain_rand)
    cfg.generator = eng.GEN_NONE
    cfg.autoreset = eng.AUTORESET_OFF
    cfg.agent_radius = agent_radius
    eng.fill_ranges(cfg)
    cfg.max_forward_step = float(s0["max_forward_step"])
    e = eng.Engine(cfg)
    for i, name in enumerate([str(t) for t in s0["tex_names"]]):
        e.upload_texture(i, assets.texture_rgb_bottom_up(name))
    polys = np.zeros(P, eng.POLY_DTYPE)
    polys["v"], polys["uv"], polys["n"] = s0["polys_v"], s0["polys_uv"], s0["polys_n"]
    polys["nv"], polys["tex"] = s0["polys_nv"], s0["polys_tex"]
    polys["rgb"] = s0["polys_rgb"] if "polys_rgb" in s0 else 1.0
    if "polys_xf" in s0:
        polys["xf"] = s0["polys_xf"]
    e.set_geometry(-1, polys, s0["wall_segs"])
    from miniworld_amd.scene import upload_scene_meshes
    tex_ids = {str(t): i for i, t in enumerate(s0["tex_names"])}
    e._test_mesh_map = upload_scene_meshes(e, s0, {}, tex_ids)
    return e


def scene_state_arrays(scenes, E=None):
    """Stack neutral scenes (same entity table layout) into mw_set_state arrays."""
    n = len(scenes)
    E = max(1, len(scenes[0]["ents_kind"])) if E is None else E
    Es = len(scenes[0]["ents_kind"])
    st = {
        "agent_pos": np.array([s["agent_pos"] for s in scenes], np.float64),
        "agent_dir": np.array([s["agent_dir"] for s in scenes], np.float64),
        "cam": np.array([[s["cam_height"], s["cam_fwd_disp"], s["cam_pitch"], s["cam_fov_y"]] for s in scenes], np.float64),
        "light": np.array([np.concatenate([s["sky"], s["light_pos"], s["light_color"], s["light_ambient"]]) for s in scenes], np.float64),
        "carrying": np.array([int(s.get("agent_carrying", -1)) for s in scenes], np.int32),
        "step_count": np.array([int(s.get("step_count", 0)) for s in scenes], np.int32),
        "num_picked_up": np.zeros(n, np.int32),
        "ent_kind": np.zeros((n, E), np.int32),
        "ent_mesh": np.full((n, E), -1, np.int32),
        "ent_static": np.zeros((n, E), np.int32),
        "ent_pos": np.zeros((n, E, 3), np.float64),
        "ent_dir": np.zeros((n, E), np.float64),
        "ent_geom": np.zeros((n, E, 9), np.float64),
        "extent": np.array([s.get("extent", np.zeros(4)) for s in scenes], np.float64),
    }
    for i, s in enumerate(scenes):
        if Es == 0:
            continue
        st["ent_kind"][i, :Es] = s["ents_kind"]
        st["ent_mesh"][i, :Es] = s["ents_mesh"]       # scene mesh index == engine mesh id (upload order)
        st["ent_static"][i, :Es] = s["ents_static"]
        st["ent_pos"][i, :Es] = s["ents_pos"]
        st["ent_dir"][i, :Es] = s["ents_dir"]
        st["ent_geom"][i, :Es, 0:3] = s["ents_size"]
        st["ent_geom"][i, :Es, 3:6] = s["ents_color"]
        st["ent_geom"][i, :Es, 6] = s["ents_scale"]
        st["ent_geom"][i, :Es, 7] = s["ents_radius"]
        st["ent_geom"][i, :Es, 8] = s["ents_height"]
    return st


def depth_from_z16(z16):
    """FrameBuffer.get_depth_map's own numpy expression (opengl.py:426-431) on a u16 map."""
    z_near, z_far = 0.04, 100.0
    depth_map = z16.astype(np.float32) / 65535
    clip_z = (depth_map - 0.5) * 2.0
    world_z = -2 * z_far * z_near / (clip_z * (z_far - z_near) - (z_far + z_near))
    return world_z.astype(np.float32)


# ------------------------------------------------------------------ batched env -> oracle scenes

def vec_env_meshes(vec):
    """mesh name -> arrays for pyoracle.render, for every mesh resident in the batched env's engine."""
    from miniworld_amd.objmesh import ObjMesh
    out = {}
    for name in vec.mesh_ids:
        m = ObjMesh.get(name)
        out[name] = {"verts": m.verts, "norms": m.norms, "texcs": m.texcs, "colors": m.colors}
    return out


def scene_of_vec_env(vec, st, i, row=None):
    """Neutral scene (oracle input) of env i of a MiniWorldVecEnv, from what the DEVICE holds: the state arrays `st`
    (mw_get_state; `row` = env i's row in them, default i) and, for envs with their own geometry set (Maze, texture
    domain randomisation), the polygons read back with mw_get_geometry."""
    from miniworld_amd.scene import scene_from_env
    row = i if row is None else row
    sc = scene_from_env(vec.template)
    names = sorted(vec.mesh_ids, key=vec.mesh_ids.get)
    sc["agent_pos"], sc["agent_dir"] = st["agent_pos"][row], st["agent_dir"][row]
    sc["cam_height"], sc["cam_fwd_disp"], sc["cam_pitch"], sc["cam_fov_y"] = st["cam"][row]
    sc["sky"], sc["light_pos"] = st["light"][row, 0:3], st["light"][row, 3:6]
    sc["light_color"], sc["light_ambient"] = st["light"][row, 6:9], st["light"][row, 9:12]
    sc["ents_kind"], sc["ents_mesh"] = st["ent_kind"][row], st["ent_mesh"][row]
    sc["ents_pos"], sc["ents_dir"] = st["ent_pos"][row], st["ent_dir"][row]
    sc["ents_size"], sc["ents_color"] = st["ent_geom"][row, :, 0:3], st["ent_geom"][row, :, 3:6]
    sc["ents_scale"], sc["ents_radius"], sc["ents_height"] = st["ent_geom"][row, :, 6], st["ent_geom"][row, :, 7], st["ent_geom"][row, :, 8]
    sc["ents_static"] = st["ent_static"][row]
    sc["mesh_names"] = np.array(names)
    sc["mesh_tex"] = np.full(len(names), -1, np.int32)         # ball / key meshes are untextured
    if not vec.engine.cfg.shared_geometry:
        polys, segs = vec.engine.get_geometry(i)
        sc["polys_v"], sc["polys_uv"], sc["polys_n"] = polys["v"], polys["uv"], polys["n"]
        sc["polys_nv"], sc["polys_tex"], sc["polys_rgb"] = polys["nv"], polys["tex"], polys["rgb"]
        sc["polys_xf"] = polys["xf"]
        sc["wall_segs"] = segs
        ids = vec.tex_ids
        sc["tex_names"] = np.array(sorted(ids, key=ids.get))
    return sc


class EpisodeMirror(ModelEnv):
    """One environment of a device batch replayed on the CPU from the same seed, with nothing of the engine in it: engine_model.ModelEnv
    (host world generator, the C oracle's dynamics, the per-step domain-randomisation draws from the env's own numpy stream) with
    the same-step auto-reset folded into step(): an episode's end continues that stream with reset() exactly like the device's
    same-step auto-reset."""

    def step(self, action):
        r, te, tr = self.substep(action)
        if te or tr:
            self.reset()
        return r, te, tr
