"""The world queries fuzzed behind the ops of the stepping API (tests/query_fuzz.py; DESIGN §5, "The API model and its fuzzer").

One accelerated engine per sequence (frame_reuse=True, frame_cache=4: every shortcut between a step and the entity list).  Behind
every op: the stepping fuzzer's own comparison with the model (tests/test_gpu_api_fuzz.py's `differences`, as it is; a frameless rollout
must also leave vec.obs every byte), then the worlds the queries read — the engine's host routes against the model's scene: segments,
listed slots, carried slot, kinds, radii and extent exactly, entity positions and poses within POSE_BAR.  On a query op the device call, then
the restatement fed from the ENGINE's host-route world and poses (they agree with the model to 1e-12, not to the bit, and the
restatements are exact), every output bit for bit; the rows under a zero mask byte keep every byte.

A failure prints the config, the seed, the op's index and the ops up to it as a list that replay() takes as it stands."""
import collections
import math

import numpy as np
import pytest

import api_fuzz
import nav_reference as nav
import query_checks
import query_fuzz
import ray_reference as ray
from query_fuzz import CELL, EGO, EGO_CELL, RAY_RANGE, SEEN_RANGE, WALLS_ENTS
from test_gpu_api_fuzz import POSE_BAR, apply_engine, differences
from test_gpu_frame_cache import _short_episodes

pytestmark = pytest.mark.gpu

SEEDS, N_OPS = query_fuzz.SEEDS, query_fuzz.N_OPS
ACCELERATED = dict(frame_reuse=True, frame_cache=4)
_covered = collections.defaultdict(dict)        # config -> seed -> the driver's counts


def _episodes(monkeypatch, cfg_name):
    cfg = query_fuzz.CONFIGS[cfg_name]
    if cfg["episode"]:
        _short_episodes(monkeypatch, cfg["cls"], cfg["episode"])


class EngineSource:
    """what a Mirror reads, from the engine's host routes; refresh() behind every op"""

    def __init__(self, vec):
        self.vec = vec
        self.refresh()

    def refresh(self):
        vec = self.vec
        self.st = vec.engine.get_state()
        self._worlds = [nav.world_of_engine(vec.engine, self.st, i) for i in range(vec.num_envs)]
        self._poses = query_checks.poses(vec)

    def worlds(self):
        return self._worlds

    def poses(self):
        return self._poses

    def scene(self, i):
        from helpers import scene_of_vec_env
        return scene_of_vec_env(self.vec, self.st, i)

    def meshes(self):
        from helpers import vec_env_meshes
        return vec_env_meshes(self.vec)

    def depth(self, i):
        return self.vec.depth[i].cpu().numpy()

    def cam(self, i):
        return tuple(self.st["cam"][i])


def world_differences(src, mv):
    """the worlds the queries read, engine against model: the list of what differs"""
    bad = []
    for i, (w, pose) in enumerate(zip(src.worlds(), src.poses())):
        e = mv.envs[i]
        m, mpose = query_fuzz.world_of_model(e), query_fuzz.pose_of_model(e)
        listed = ray.listed_slots(w)
        if w["segs"].shape != m["segs"].shape:
            bad.append(f"env {i}: {len(w['segs'])} segments, the model has {len(m['segs'])}")
        elif not np.array_equal(w["segs"], m["segs"]):
            bad.append(f"env {i}: segments off by {float(np.abs(w['segs'] - m['segs']).max()):.3g}")
        if listed != ray.listed_slots(m):
            bad.append(f"env {i}: listed slots {listed}, the model lists {ray.listed_slots(m)}")
            listed = sorted(set(listed) & set(ray.listed_slots(m)))
        if int(w["carry"]) != int(m["carry"]):
            bad.append(f"env {i}: carried slot {w['carry']}, the model carries {m['carry']}")
        if not np.array_equal(np.asarray(w["extent"], np.float64), m["extent"]):
            bad.append(f"env {i}: extent {list(w['extent'])}, the model's {list(m['extent'])}")
        if (w["agent_radius"], w["max_forward_step"]) != (m["agent_radius"], m["max_forward_step"]):
            bad.append(f"env {i}: agent radius / forward step {w['agent_radius']!r} {w['max_forward_step']!r}, the model's {m['agent_radius']!r} {m['max_forward_step']!r}")
        slots = listed + ([int(w["carry"])] if w["carry"] >= 0 else [])
        if slots:
            if not np.array_equal(np.asarray(w["radius"], np.float64)[slots], m["radius"][slots]):
                bad.append(f"env {i}: radii {np.asarray(w['radius'])[slots].tolist()}, the model's {m['radius'][slots].tolist()}")
            if not np.array_equal(np.asarray(w["kind"])[slots], m["kind"][slots]):
                bad.append(f"env {i}: kinds {np.asarray(w['kind'])[slots].tolist()}, the model's {m['kind'][slots].tolist()}")
            err = float(np.abs(np.asarray(w["pos"], np.float64)[slots] - m["pos"][slots]).max())
            if not err < POSE_BAR:
                bad.append(f"env {i}: entity positions off by {err:.3g}")
        err = max(abs(float(a) - b) for a, b in zip(pose, mpose))
        if not err < POSE_BAR:
            bad.append(f"env {i}: pose off by {err:.3g}")
    return bad


def _u8(a):
    return None if a is None else query_checks.dev(np.asarray(a, np.uint8))


def _same_bits(got, want):
    g = np.ascontiguousarray(got)
    w = np.asarray(want)
    return w.size == g.size and g.tobytes() == np.ascontiguousarray(w.astype(g.dtype).reshape(g.shape)).tobytes()


def ask_engine(vec, held, mirror, op):
    """the device call of a query op: name -> the tensor of every output it wrote, and a snapshot of each from before the call"""
    import torch
    what, mask = op["what"], _u8(op.get("mask"))

    def keep(name, make):
        if name not in held:
            held[name] = make()
        return held[name]

    def snap(outs):
        return outs, {k: v.clone() for k, v in outs.items()}
    if what in ("raycast", "lidar"):
        if what == "lidar":
            outs, before = snap(vec.lidar(op["rays"], 2 * math.pi, RAY_RANGE, op["radius"], op["obstacles"]))
            return outs, before
        offs = torch.tensor(ray.lidar_offsets(op["rays"], 2 * math.pi), dtype=torch.float64, device="cuda")
        kw = dict(offsets=offs, max_t=RAY_RANGE, radius=op["radius"], obstacles=op["obstacles"])
        if mask is None:
            return snap(vec.raycast(**kw))
        out = vec.raycast(**kw)
        out["t"].fill_(-7.0), out["hit"].fill_(-7), out["dir"].fill_(-7.0)
        outs, before = snap(out)
        assert vec.raycast(mask=mask, into=out, **kw) is out
        return outs, before
    if what == "nav":
        if op["points"] is None:
            fld = vec.nav_field(target=op["target"], cell=CELL, obstacles=WALLS_ENTS, mask=mask)
        else:
            fld = vec.nav_field(target=query_checks.dev(np.array(op["points"], np.float64)), reach=query_fuzz.POINT_REACH, cell=CELL, obstacles=WALLS_ENTS, mask=mask)
        assert (fld.gx, fld.gz) == (mirror.gx, mirror.gz)
        q = vec.nav_query(fld)
        outs = {"field": fld.field.view(torch.int16), "cost": q["cost"], "next": q["next"], "waypoint": q["waypoint"]}
        # (a new field: the rows of a masked build that were not built hold 0xFFFF; the query's rows are all written)
        return outs, {"field": torch.full_like(outs["field"], -1)}
    if what == "seen":
        m = keep("seen", lambda: vec.seen_map(cell=CELL, max_range=SEEN_RANGE, obstacles=WALLS_ENTS))
        assert (m.gx, m.gz, m.cos_half) == (mirror.gx, mirror.gz, mirror.cos_half)
        outs, before = snap({"seen": m.seen, "count": m.count, "new": m.new})
        vec.seen_update(m, clear=_u8(op["clear"]), mask=mask)
        return outs, before
    if what in EGO:
        g = EGO[what]
        w = keep(what, lambda: vec.ego_window(size=g["size"], frame=g["frame"], anchor=g["anchor"], obstacles=WALLS_ENTS))
        assert (w.cell, w.back, w.wall_radius, w.entity_pad, w.max_range, w.cos_half, tuple(w.names)) == (
            EGO_CELL, g["size"] / 2 if g["anchor"] == "bottom" else 0.0, EGO_CELL / 2, EGO_CELL / 2, query_fuzz.EGO_RANGE, mirror.cos_half, ("wall", "entity", "visible"))
        outs, before = snap({"planes": w.planes})
        vec.ego_update(w, mask=mask)
        return outs, before
    if what == "label":
        f = keep("label", lambda: vec.label_frame())
        assert tuple(f.cls.shape[1:]) == (op["height"], op["width"]) and int(vec.engine.cfg.msaa) == query_fuzz.MSAA
        outs, before = snap({"cls": f.cls, "code": f.code})
        vec.label_update(f, mask=mask)
        return outs, before
    if what == "depth":
        w = keep("depth", lambda: vec.depth_window(size=query_fuzz.DEPTH_SIZE))
        assert (w.cell, w.back, w.frame, w.min_range, w.max_range, w.floor_tol, w.top) == (EGO_CELL, 0.0, "heading", 0.05, 8.0, 0.1, mirror.top)
        outs, before = snap({"planes": w.planes})
        vec.depth_update(w, mask=mask)
        return outs, before
    if what == "scan":
        m = keep("scan", lambda: vec.scan_map(cell=CELL, rays=65, max_range=RAY_RANGE))
        assert (m.gx, m.gz, m.obstacles, m.fov) == (mirror.gx, mirror.gz, WALLS_ENTS, 2 * math.pi)
        outs, before = snap({"map": m.map, "count": m.count, "new": m.new})
        vec.scan_map_update(m, clear=_u8(op["clear"]), mask=mask)
        scan = vec.lidar(65, m.fov, RAY_RANGE, obstacles=WALLS_ENTS)         # the beams the update cast: the same call again
        outs.update(t=scan["t"], hit=scan["hit"], dir=scan["dir"])
        return outs, before
    raise ValueError(what)


def query_differences(vec, held, mirror, src, op):
    """the device call of a query op against the restatement fed from the engine's own world and poses: the list of what differs
    (None: the restatement declined the case on the engine's floats)"""
    try:
        want = mirror.answer(op, src)
    except query_fuzz.Declined:
        return None
    outs, before = ask_engine(vec, held, mirror, op)
    got = {k: query_checks.host(v) for k, v in outs.items()}
    was = {k: query_checks.host(v) for k, v in before.items()}
    bad = []
    for i, w in enumerate(want):
        for name in got:
            if w is None:
                if name in was and not np.array_equal(got[name][i], was[name][i]):
                    bad.append(f"{op['what']}.{name}: env {i} is masked off and was written")
            elif not _same_bits(got[name][i], w[name]):
                g, x = np.asarray(got[name][i]), np.asarray(w[name]).reshape(np.asarray(got[name][i]).shape)
                bad.append(f"{op['what']}.{name}: env {i}, {int((g != x).sum())} of {g.size} values differ, the first at {np.argwhere(g != x)[:4].tolist()}")
    return bad


def replay(cfg_name, seed, ops=None, n_ops=N_OPS):
    """One sequence on the model and on the accelerated engine, compared behind every op.  `ops`: apply these instead of drawing (the
    list a failure printed, or a prefix of it cut down to a regression case).  Call under _episodes as the fuzzer's cases do.
    Returns the driver's counts."""
    from miniworld_amd.vec_env import MiniWorldVecEnv
    cfg = query_fuzz.CONFIGS[cfg_name]
    d = query_fuzz.Driver(cfg_name, seed, answer=False)
    mv = d.mv
    vec = MiniWorldVecEnv(cfg["env_id"], cfg["n"], seed=query_fuzz.fuzz_seed(cfg_name, seed), **ACCELERATED, **cfg["kw"])
    try:
        assert (vec.frame_reuse, vec.frame_cache) == (True, 4)
        vec.reset()
        bank, held, src = [None] * api_fuzz.BANK, {}, EngineSource(vec)
        fov, top = vec.default_fov(), float(vec.engine.cfg.agent_height)
        assert abs(fov - d.fov) < POSE_BAR and abs(top - d.top) < POSE_BAR, ("the queries' defaults", fov, d.fov, top, d.top)
        mirror = query_fuzz.Mirror(mv.N, d.extent, fov, top)

        def where(t, op):
            return (f"{cfg_name} seed {seed}, op {t} ({op['kind']}{' ' + op['what'] if op['kind'] == 'query' else ''})", f"\nthe ops up to it:\n{api_fuzz.format_ops(d.log)}")
        bad = differences(vec, mv, {"kind": "reset"}) + world_differences(src, mv)
        assert not bad, f"{cfg_name} seed {seed}, after reset(): {bad}"
        for t, op in enumerate(d.ops(n_ops) if ops is None else d.replay(ops)):
            head, tail = where(t, op)
            if op["kind"] == "query":
                bad = query_differences(vec, held, mirror, src, op)
                # (declined on the model's floats it would have been dropped; declined on the engine's alone it was never compared)
                assert bad is not None, f"{head}: the restatement declined the engine's floats, not the model's{tail}"
                assert not bad, f"{head}: the device differs from the restatement of its own world: {bad}{tail}"
                continue
            frameless = op["kind"] == "rollout" and not op.get("render", True)
            obs = vec.obs.clone() if frameless else None
            apply_engine(vec, bank, op)
            src.refresh()
            bad = differences(vec, mv, op)
            if frameless and not bool((vec.obs == obs).all()):
                bad.append("obs: a frameless rollout wrote it")
            assert not bad, f"{head} differs from the model: {bad}{tail}"
            bad = world_differences(src, mv)
            assert not bad, f"{head}: the world the queries read differs from the model's: {bad}{tail}"
        vec.engine.check()
    finally:
        vec.close()
    return d.counts


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("cfg_name", list(query_fuzz.CONFIGS))
def test_query_fuzz(monkeypatch, cfg_name, seed):
    _episodes(monkeypatch, cfg_name)
    _covered[cfg_name][seed] = replay(cfg_name, seed)


@pytest.mark.parametrize("cfg_name", list(query_fuzz.CONFIGS))
def test_the_sequences_met_what_they_are_for(monkeypatch, cfg_name):
    """The coverage conditions over the config's seeds, on the model's counts of the sequences that ran above (a seed that did not run
    here — a selection by hand — is run on the model alone: the ops do not depend on the engine)."""
    _episodes(monkeypatch, cfg_name)
    counts = collections.Counter()
    for seed in SEEDS:
        counts.update(_covered[cfg_name][seed] if seed in _covered[cfg_name] else query_fuzz.run_model(cfg_name, seed).counts)
    assert query_fuzz.coverage_failures(cfg_name, counts) == [], (cfg_name, dict(counts))
    assert counts["dropped"] <= query_fuzz.DROP_CAP * counts["drawn"], dict(counts)
