"""Label frames on the GPU (mw_label_frame; MiniWorldVecEnv.label_frame / label_update) against the brute-force restatement of
tests/label_reference.py — numpy in the documented order of operations, fed by the scenes the device holds (helpers.scene_of_vec_env) —
bit for bit in all five outputs: families with shared and per-env geometry, polygon chunks, Boxes, static frames and mesh objects, the
sample counts and a frame of two bands, both mesh modes.  Then the engine's own depth frame as the independent check of the labels, the
mask, that nothing in the engine changes, and the carried object."""
import numpy as np
import pytest

import label_reference as ref
from depth_reference import z16_of
from helpers import scene_of_vec_env, vec_env_meshes
from query_checks import vec_env

pytestmark = pytest.mark.gpu
N = 8
MISS_CAP, INTERIOR_FLOOR = 0.005, 0.70         # tests/test_label_cpu.py's caps


def _vec(env_id, n=N, **kw):
    return vec_env(env_id, n, **kw)


def _walk(vec, steps, seed):
    import torch
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        vec.step(torch.as_tensor(rng.integers(0, 3, vec.num_envs), dtype=torch.int32, device="cuda"))      # turns and forward moves


def _want(vec, mode, envs=None, **kw):
    """the restatement's frames of the scenes the device holds"""
    st = vec.engine.get_state()
    meshes = vec_env_meshes(vec)
    H, W = int(vec.obs.shape[1]), int(vec.obs.shape[2])
    return {i: ref.label_frame(scene_of_vec_env(vec, st, i), W, H, int(vec.engine.cfg.msaa), meshes=meshes, mode=mode, **kw)
            for i in (range(vec.num_envs) if envs is None else envs)}


def _same(f, want):
    got = {k: getattr(f, k).cpu().numpy() for k in ("cls", "code", "depth", "ent_pixels", "ent_box")}
    for i, w in want.items():
        E = len(w["ent_pixels"])         # (the engine may have more slots than the scene: the rest are empty)
        for k in ("cls", "code"):
            assert np.array_equal(got[k][i], w[k]), (i, k, np.argwhere(got[k][i] != w[k])[:8].tolist())
        assert np.array_equal(got["depth"][i].view(np.uint32), w["depth"].view(np.uint32)), (i, "depth", np.argwhere(got["depth"][i] != w["depth"])[:8].tolist())
        assert np.array_equal(got["ent_pixels"][i][:E], w["ent_pixels"]) and not got["ent_pixels"][i][E:].any(), (i, got["ent_pixels"][i], w["ent_pixels"])
        assert np.array_equal(got["ent_box"][i][:E], w["ent_box"]), (i, got["ent_box"][i], w["ent_box"])


CONFIGS = [("MiniWorld-Hallway-v0", 8, {}), ("MiniWorld-OneRoom-v0", 8, dict(domain_rand=True)), ("MiniWorld-MazeS3-v0", 4, {}), ("MiniWorld-Sign-v0", 8, {}),
           ("MiniWorld-PickupObjects-v0", 8, dict(domain_rand=True)), ("MiniWorld-Sidewalk-v0", 8, {}),
           ("MiniWorld-PickupObjects-v0", 8, dict(domain_rand=True, msaa=4)), ("MiniWorld-Hallway-v0", 8, dict(msaa=1)), ("MiniWorld-Sidewalk-v0", 8, dict(msaa=1)),
           ("MiniWorld-PickupObjects-v0", 8, dict(obs_width=84, obs_height=84)), ("MiniWorld-Sign-v0", 8, dict(obs_width=81, obs_height=61, msaa=4))]


@pytest.mark.parametrize("env_id,n,kw", CONFIGS, ids=[f"{c[0].split('-')[1]}-{'-'.join(f'{k}{v}' for k, v in c[2].items()) or 'plain'}" for c in CONFIGS])
def test_kernel_equals_the_restatement(env_id, n, kw):
    vec = _vec(env_id, n, **kw)
    _walk(vec, 12, 3500)
    has_mesh = bool((vec.state(("ent_kind",))["ent_kind"] == 2).any())
    seen = set()
    for mode in ("exact", "bounds") if has_mesh else ("exact",):
        f = vec.label_frame(meshes=mode, depth=True, stats=True)
        assert vec.label_update(f) is f.cls
        want = _want(vec, mode)
        _same(f, want)
        seen |= set(np.unique(f.cls.cpu().numpy()).tolist())
    assert ref.WALL in seen or ref.FLOOR in seen, seen
    print(env_id, kw, "classes", sorted(seen))
    vec.engine.check()
    vec.close()


def test_unpruned_mesh_phase_gives_the_same_bits():
    from miniworld_amd import engine
    vec = _vec("MiniWorld-PickupObjects-v0", 4)
    _walk(vec, 12, 3501)
    f, g = vec.label_frame(depth=True, stats=True), vec.label_frame(depth=True, stats=True)
    vec.label_update(f)
    vec.engine.label_frame(engine.MwLabelParams(g.near, g.far, engine.LABEL_MESH_EXACT | engine.LABEL_UNPRUNED, 0), g.cls, g.code, g.depth, g.ent_pixels, g.ent_box)
    for k in ("cls", "code", "depth", "ent_pixels", "ent_box"):
        assert (getattr(f, k) == getattr(g, k)).all(), k
    assert (f.cls == ref.MESH).any()
    vec.close()


@pytest.mark.parametrize("env_id,kw", [("MiniWorld-PickupObjects-v0", dict(domain_rand=True)), ("MiniWorld-FourRooms-v0", {}), ("MiniWorld-Sidewalk-v0", dict(msaa=4))])
def test_the_engines_own_depth_frame_agrees_with_the_labels(env_id, kw):
    vec = _vec(env_id, want_depth=True, **kw)
    _walk(vec, 12, 3502)
    f = vec.label_frame(depth=True)
    vec.label_update(f)
    H, W = int(vec.obs.shape[1]), int(vec.obs.shape[2])
    code, t = f.code.cpu().numpy(), f.depth.cpu().numpy().astype(np.float64)
    z16 = z16_of(vec.depth.cpu().numpy().reshape(N, H, W))
    for i in range(N):
        bad, inner = ref.against_frame(dict(code=code[i], t=t[i]), z16[i])
        print(f"{env_id} env {i}: {bad} of {inner} interior pixels miss the engine's depth, {inner} of {W * H} interior")
        assert inner >= INTERIOR_FLOOR * W * H, (env_id, i, inner)
        assert bad <= MISS_CAP * inner, (env_id, i, bad, inner)
    vec.close()


def test_a_masked_env_keeps_every_byte():
    import torch
    vec = _vec("MiniWorld-PickupObjects-v0")
    mask = np.array([1, 0, 1, 0, 0, 1, 1, 0], np.uint8)
    f = vec.label_frame(depth=True, stats=True)
    f.cls.fill_(0xAB); f.code.fill_(0x5A5A5A5A); f.depth.fill_(-3.0); f.ent_pixels.fill_(-7); f.ent_box.fill_(-9)
    vec.label_update(f, mask=torch.as_tensor(mask, device="cuda"))
    off = torch.as_tensor(mask == 0, device="cuda")
    assert (f.cls[off] == 0xAB).all() and (f.code[off] == 0x5A5A5A5A).all() and (f.depth[off] == -3.0).all()
    assert (f.ent_pixels[off] == -7).all() and (f.ent_box[off] == -9).all()
    _same(f, _want(vec, "exact", envs=[int(i) for i in np.nonzero(mask)[0]]))
    vec.close()


def test_nothing_in_the_engine_changes():
    import torch
    from miniworld_amd.engine import STATE_FIELDS
    a, b = _vec("MiniWorld-PickupObjects-v0", domain_rand=True), _vec("MiniWorld-PickupObjects-v0", domain_rand=True)
    rng = np.random.default_rng(3503)
    fa, fb = a.label_frame(depth=True, stats=True), a.label_frame(meshes="bounds")
    for k in range(6):
        act = torch.as_tensor(rng.integers(0, a.n_actions, N), dtype=torch.int32, device="cuda")
        ra, rb = a.step(act), b.step(act)
        for x, y in zip(ra, rb):
            assert torch.equal(x, y), k
        sa, sb = a.state(tuple(STATE_FIELDS)), b.state(tuple(STATE_FIELDS))
        for name in sa:
            assert torch.equal(sa[name], sb[name]), (k, name)
        a.label_update(fa)
        a.label_update(fb)
        assert torch.equal(a.obs, b.obs), k
    a.engine.check()
    a.close(); b.close()


def test_the_carried_object_is_labelled():
    """RoomObjects: every agent is put 0.6 m (1.5 agent radii: where pickup looks) before its env's first mesh object and picks it up; an
    agent whose reach meets a wall or another object first tries again from the next of four sides"""
    import math
    import torch
    vec = _vec("MiniWorld-RoomObjects-v0")
    st = vec.state(("agent_pos", "ent_kind", "ent_pos"))
    slot = int(np.nonzero((st["ent_kind"].cpu().numpy() == 2).all(0))[0][0])          # (the family's entity table is the same in every env)
    target = st["ent_pos"][:, slot].clone()
    for side in range(4):
        d = side * math.pi / 2
        todo = vec.state(("carrying",))["carrying"] != slot
        pos = st["agent_pos"].clone()
        pos[:, 0], pos[:, 2] = target[:, 0] - 0.6 * math.cos(d), target[:, 2] + 0.6 * math.sin(d)
        vec.set_state_where(todo.to(torch.uint8), agent_pos=pos, agent_dir=torch.full((N,), d, dtype=torch.float64, device="cuda"))
        vec.step(torch.where(todo, 4, 0).to(torch.int32))        # pickup; the others turn on the spot
    carrying = vec.state(("carrying",))["carrying"].cpu().numpy()
    held = [i for i in range(N) if carrying[i] == slot]
    assert len(held) >= N // 2, carrying
    f = vec.label_frame(depth=True, stats=True)
    vec.label_update(f)
    _same(f, _want(vec, "exact", envs=held))
    pixels = f.ent_pixels.cpu().numpy()
    print("carried slot", slot, "pixels per env", pixels[:, slot].tolist())
    assert all(pixels[i, slot] > 20 for i in held)
    assert all(((f.slot[i] == slot).sum() == pixels[i, slot]).item() for i in held)
    vec.close()
