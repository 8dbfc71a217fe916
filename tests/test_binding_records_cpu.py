"""The Python binding's behaviour as two records (tests/golden/vec_env_configs.json, tests/golden/binding_calls.json), without a GPU:
the mw_config and the asset lists MiniWorldVecEnv builds for every family, and the library calls a scripted session makes — the entry
points in order, integers and floats by value, pointers as null / non-null (their positions are the binding's own declared argument
types), structs passed by reference as their bytes (one whose members are pointers: member by member).  Both were recorded over the
stub engine of helpers.py before engine.py and vec_env.py were split up, so a difference is a change of behaviour.

Both files are written compactly and expanded here.  A config case lists the members in which it differs from the case it is `like`
(the first case lists every member).  In the call record the entries behind an operation of the session are a block, written once
however many sessions make them, a session is its operations with their blocks, and a struct's bytes are zlib-compressed base64 under
the SHA-1 of the bytes."""
import base64
import ctypes as C
import hashlib
import json
import os
import zlib

import pytest

from helpers import GOLDEN, stub_engine

CONFIGS = os.path.join(GOLDEN, "vec_env_configs.json")
CALLS = os.path.join(GOLDEN, "binding_calls.json")
RETURNS = {"mw_snapshot_bytes": 4096, "mw_snapshot_frames_bytes": 8192}
AUTORESETS = (True, False, "same_step", "next_step", "levels", "seeds")
SESSION_ENVS = (("MiniWorld-Hallway-v0", False), ("MiniWorld-Maze-v0", True), ("MiniWorld-PickupObjects-v0", True),
                ("MiniWorld-FourRooms-v0", True), ("MiniWorld-CollectHealth-v0", False))
SESSION_MODES = {"same_step": dict(autoreset="same_step", final_obs=True, frame_stack=3),
                 "next_step": dict(autoreset="next_step", want_depth=True),
                 "levels": dict(autoreset="levels"),
                 "seeds": dict(autoreset="seeds")}


def argtypes_of(name):
    from miniworld_amd import engine
    return engine.SIGNATURES[name][0]


def tree(obj):
    """a ctypes value as plain names, lists and numbers"""
    if isinstance(obj, C.Structure):
        return {f[0]: tree(getattr(obj, f[0])) for f in obj._fields_}
    if isinstance(obj, C.Array):
        return [tree(x) for x in obj]
    return obj


# ------------------------------------------------------------------ record 1: configs

def config_cases():
    from miniworld_amd.vec_env import _KIND
    cases = [(f"{env_id} dr={int(dr)}", env_id, dict(domain_rand=dr)) for env_id in _KIND for dr in (False, True)]
    hallway = "MiniWorld-Hallway-v0"
    cases.append((f"{hallway} msaa=4", hallway, dict(msaa=4)))
    cases += [(f"{hallway} autoreset={a!r}", hallway, dict(autoreset=a)) for a in AUTORESETS]
    cases.append((f"{hallway} device_id=1", hallway, dict(device_id=1)))
    return cases


def capture_config(install, env_id, kwargs):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = install()
    vec = MiniWorldVecEnv(env_id, 4, seed=3, **kwargs)
    uploads = [name for name, _ in lib.calls if name in ("mw_upload_texture", "mw_upload_mesh")]
    textures, meshes = sorted(vec.tex_ids, key=vec.tex_ids.get), sorted(vec.mesh_ids, key=vec.mesh_ids.get)
    assert [vec.tex_ids[t] for t in textures] == list(range(len(textures))) and uploads.count("mw_upload_texture") == len(textures)
    assert [vec.mesh_ids[m] for m in meshes] == list(range(len(meshes))) and uploads.count("mw_upload_mesh") == len(meshes)
    return {"config": tree(vec.engine.cfg), "textures": textures, "meshes": meshes}


def _differences(want, got, path=""):
    if isinstance(want, dict) and isinstance(got, dict) and sorted(want) == sorted(got):
        return [d for k in want for d in _differences(want[k], got[k], f"{path}.{k}" if path else k)]
    if isinstance(want, list) and isinstance(got, list) and len(want) == len(got):
        return [d for k, (w, g) in enumerate(zip(want, got)) for d in _differences(w, g, f"{path}[{k}]")]
    return [] if want == got and type(want) is type(got) else [f"{path}: recorded {want!r}, now {got!r}"]


def load_configs():
    """label -> {"config": every member, "textures", "meshes"}: each case's own members over those of the case it is like"""
    cases, out = json.load(open(CONFIGS)), {}

    def flat(label):
        own = dict(cases[label])
        return {**(flat(own.pop("like")) if "like" in own else {}), **own}
    for label in cases:
        members = flat(label)
        out[label] = {"config": {k[len("config."):]: v for k, v in members.items() if k.startswith("config.")},
                      "textures": members["textures"], "meshes": members["meshes"]}
    return out


@pytest.fixture(scope="module")
def recorded_configs():
    return load_configs()


def test_every_case_of_the_config_record_is_still_a_case(recorded_configs):
    from miniworld_amd.vec_env import _KIND
    assert sorted(recorded_configs) == sorted(label for label, _, _ in config_cases())
    assert len(_KIND) == 23 and len(recorded_configs) == 2 * 23 + 8


@pytest.mark.parametrize("label", [c[0] for c in config_cases()])
def test_the_config_of_a_family_is_the_recorded_one(label, recorded_configs, monkeypatch):
    _, env_id, kwargs = next(c for c in config_cases() if c[0] == label)
    got = json.loads(json.dumps(capture_config(lambda: stub_engine(monkeypatch), env_id, kwargs)))
    assert _differences(recorded_configs[label], got) == []


# ------------------------------------------------------------------ record 2: call sequences

class CallLog:
    """the session's entries: {"op": label} markers, {"raises": type} for a refusal, and one entry per library call"""

    def __init__(self, lib, blobs):
        self.lib, self.blobs, self.entries, self.seen = lib, blobs, [], 0

    def _struct(self, obj):
        if any(t is C.c_void_p for _, t in obj._fields_):       # (addresses differ from run to run: member by member)
            return {n: (("ptr" if getattr(obj, n) else "null") if t is C.c_void_p else tree(getattr(obj, n))) for n, t in obj._fields_}
        raw = bytes(obj)
        key = hashlib.sha1(raw).hexdigest()[:16]
        self.blobs[key] = raw.hex()
        return {"bytes": key}

    def _arg(self, a, ctype):
        if issubclass(ctype, C._Pointer):
            obj = getattr(a, "_obj", None)
            if isinstance(obj, C.Structure):
                return {type(obj).__name__: self._struct(obj)}
            return "null" if a is None else "ptr"
        if ctype in (C.c_void_p, C.c_char_p):
            return "ptr" if (a.value if isinstance(a, C.c_void_p) else a) else "null"
        return float(a) if ctype is C.c_double else int(a)

    def flush(self):
        for name, args in self.lib.calls[self.seen:]:
            types = argtypes_of(name)
            assert len(types) == len(args), (name, len(types), len(args))
            self.entries.append({"call": name, "args": [self._arg(a, t) for a, t in zip(args, types)]})
        self.seen = len(self.lib.calls)

    def do(self, label, fn):
        self.entries.append({"op": label})
        try:
            return fn()
        except (ValueError, RuntimeError, KeyError) as exc:
            self.entries.append({"raises": type(exc).__name__})
        finally:
            self.flush()


def run_session(install, env_id, domain_rand, mode_kwargs, blobs):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = install()
    log = CallLog(lib, blobs)
    do = log.do
    N = 4
    vec = do("construct", lambda: MiniWorldVecEnv(env_id, N, seed=3, domain_rand=domain_rand, **mode_kwargs))
    E = vec.engine.E
    actions = torch.tensor([0, 1, 2, 2])
    plans = torch.tensor([[2, 0, 1, 2]] * 8, dtype=torch.int64)
    if vec.autoreset_mode == "levels":      # (reset and step need a bank in this mode; the other modes meet these two at the end)
        bank = do("make_levels", lambda: vec.make_levels([10, 11, 12, 13, 14]))
        do("set_levels", lambda: vec.set_levels(bank))
    do("reset", lambda: vec.reset())
    do("step", lambda: vec.step(actions))
    do("step repeat=3", lambda: vec.step(actions, repeat=3))
    do("stack", lambda: vec.stack)
    do("rollout", lambda: vec.rollout(plans))
    do("rollout trace=True", lambda: vec.rollout(plans, trace=True))
    do("rollout trace=ent_pos", lambda: vec.rollout(plans[:5], trace=("ent_pos",)))
    do("rollout render=False", lambda: vec.rollout(plans, render=False))
    snap = do("save_state", lambda: vec.save_state())
    fsnap = do("save_state frames", lambda: vec.save_state([3, 1, 0], capacity=4, frames=True))
    do("save_state into", lambda: vec.save_state([2, 0], into=fsnap, records=[1, 3]))
    do("save_state into plain", lambda: vec.save_state(torch.tensor([1]), into=snap, records=torch.tensor([2])))
    do("load_state", lambda: vec.load_state(snap))
    do("load_state indices", lambda: vec.load_state(snap, envs=[1, 2], records=[0, 0]))
    do("load_state frames", lambda: vec.load_state(fsnap, envs=[0, 1, 2]))
    do("load_state frames=False", lambda: vec.load_state(fsnap, envs=[0, 1, 2], frames=False))
    do("fork", lambda: vec.fork(torch.tensor([0, 0, 2, 2])))
    do("fork frames", lambda: vec.fork([1, 1, 3, 3], frames=True))
    do("state", lambda: vec.state())
    do("state fields", lambda: vec.state(("extent", "agent_pos")))
    do("set_state_where list", lambda: vec.set_state_where([1, 0, 1, 0], agent_dir=[0.0, 0.5, 1.0, 1.5]))
    do("set_state_where bool", lambda: vec.set_state_where(torch.tensor([True, False, False, True]), agent_pos=torch.zeros((N, 3), dtype=torch.float64),
                                                           ent_pos=torch.zeros((N, E, 3), dtype=torch.float64)))
    do("reset_where", lambda: vec.reset_where([0, 1, 1, 0], [7, 8, 9, 10]))
    do("reset_where tensors", lambda: vec.reset_where(torch.tensor([True, False, False, False]), torch.tensor([5, 6, 7, 8])))
    field = do("nav_field slot", lambda: vec.nav_field(target=0))
    do("nav_field points", lambda: vec.nav_field(target=torch.zeros((N, 3), dtype=torch.float64), reach=0.5, cell=0.5, obstacles="walls+entities"))
    do("nav_field into", lambda: vec.nav_field(into=field, mask=torch.tensor([True, False, True, False])))
    do("nav_query", lambda: vec.nav_query(field))
    do("nav_query pos", lambda: vec.nav_query(field, pos=torch.zeros((N, 3), dtype=torch.float64)))
    rays = do("raycast direction", lambda: vec.raycast(direction=torch.ones((N, 5, 2), dtype=torch.float64), origin=torch.zeros((N, 5, 3), dtype=torch.float64),
                                                        radius=0.1, obstacles="walls+entities"))
    do("raycast offsets", lambda: vec.raycast(offsets=torch.zeros(3, dtype=torch.float64), max_t=4.0, mask=torch.tensor([1, 1, 0, 0], dtype=torch.uint8)))
    do("raycast into", lambda: vec.raycast(direction=torch.ones((N, 5, 2), dtype=torch.float64), into=rays))
    do("lidar", lambda: vec.lidar(rays=8))
    do("lidar again", lambda: vec.lidar(rays=8))
    do("default_fov", lambda: vec.default_fov())
    seen = do("seen_map", lambda: vec.seen_map(cell=0.5, max_range=6.0, fov=2.0, obstacles="walls+entities"))
    seen_like = do("seen_map like", lambda: vec.seen_map(like=field))
    do("seen_update", lambda: vec.seen_update(seen))
    do("seen_update clear", lambda: vec.seen_update(seen, clear=torch.tensor([1, 0, 0, 1], dtype=torch.uint8)))
    do("seen_update bool mask", lambda: vec.seen_update(seen_like, mask=torch.tensor([True, False, True, False])))
    do("infos", lambda: vec.infos())
    do("final_infos", lambda: vec.final_infos())
    do("reset_pending", lambda: vec.reset_pending())
    do("frame_source", lambda: vec.frame_source())
    do("frame_clean", lambda: vec.frame_clean())
    do("render_top_view", lambda: vec.render_top_view())
    do("get_visible_ents", lambda: vec.get_visible_ents())
    bank = do("make_levels", lambda: vec.make_levels([10, 11, 12, 13, 14]))
    do("set_levels", lambda: vec.set_levels(bank))
    do("step after set_levels", lambda: vec.step(actions))
    return log.entries


def session_cases():
    return [(f"{env_id} dr={int(dr)} {mode}", env_id, dr, kwargs) for env_id, dr in SESSION_ENVS for mode, kwargs in SESSION_MODES.items()]


def load_calls():
    """{"blobs": SHA-1 prefix -> hex bytes, "sessions": label -> entries}: every operation's marker followed by its block's entries"""
    rec = json.load(open(CALLS))
    blobs = {k: zlib.decompress(base64.b64decode(v)).hex() for k, v in rec["blobs"].items()}
    assert all(hashlib.sha1(bytes.fromhex(v)).hexdigest()[:16] == k for k, v in blobs.items())
    sessions = {label: [e for op, block in ops for e in [{"op": op}] + rec["blocks"][block]]
                for label, ops in rec["sessions"].items()}
    return {"blobs": blobs, "sessions": sessions}


@pytest.fixture(scope="module")
def recorded_calls():
    return load_calls()


def test_every_session_of_the_call_record_is_still_a_session(recorded_calls):
    assert sorted(recorded_calls["sessions"]) == sorted(c[0] for c in session_cases())


def _blob_differences(want_hex, got_hex, struct):
    from miniworld_amd import engine
    cls = getattr(engine, struct)
    return _differences(tree(cls.from_buffer_copy(bytes.fromhex(want_hex))), tree(cls.from_buffer_copy(bytes.fromhex(got_hex))), struct)


@pytest.mark.parametrize("label", [c[0] for c in session_cases()])
def test_a_session_makes_the_recorded_library_calls(label, recorded_calls, monkeypatch):
    _, env_id, dr, kwargs = next(c for c in session_cases() if c[0] == label)
    blobs = {}
    got = json.loads(json.dumps(run_session(lambda: stub_engine(monkeypatch, returns=RETURNS), env_id, dr, kwargs, blobs)))
    want = recorded_calls["sessions"][label]
    for k, (w, g) in enumerate(zip(want, got)):
        if w != g:
            where = next((e["op"] for e in reversed(want[:k + 1]) if "op" in e), "?")
            detail = _differences(w, g)
            for wa, ga in zip(w.get("args", []), g.get("args", [])):       # a struct's bytes differ: name the members
                if isinstance(wa, dict) and isinstance(ga, dict) and wa != ga and list(wa) == list(ga) and "bytes" in list(wa.values())[0]:
                    name = list(wa)[0]
                    detail = _blob_differences(recorded_calls["blobs"][wa[name]["bytes"]], blobs[ga[name]["bytes"]], name)
            pytest.fail(f"entry {k} (in {where!r}): recorded {w.get('call') or w}, now {g.get('call') or g}: {detail}")
    assert len(got) == len(want)
    assert all(recorded_calls["blobs"][k] == v for k, v in blobs.items())
