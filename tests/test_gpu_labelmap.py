"""Object maps on the GPU (mw_label_project; MiniWorldVecEnv.object_window / object_update / object_map / object_map_update) against the
restatement of tests/objectmap_reference.py — numpy in the documented order of operations, fed by the engine's own label and depth
tensors and the poses, cameras and extents of vec.state() — bit for bit: plane, map, cells and pos at every step.  Then the frame sizes
and sample counts that take another path, the largest launch (above 64 KiB of LDS), mask and clear, synthetic label images through an
int32 tensor and `depth=` (the one-cell window is the atomic-contention path), the geometry — a sensed cell lies on its object, and
where the privileged entity plane is empty no object is sensed —, the refusals and the adapter's key."""
import math

import numpy as np
import pytest

import objectmap_reference as ref
from query_checks import dev as _dev, teleport, vec_env, worlds

pytestmark = pytest.mark.gpu
N = 4
BASE = ref.RAY_ENT


# PickupObjects: env i plays the world of seed + i, and those of seeds 3 .. 6 each hold a ball or a box, 0.9 m high — a key, 0.35 m
# high, lies below the view of a camera 1.5 m up from 1.5 m away (seed 2's world holds keys alone)
SEEDS = {"MiniWorld-PickupObjects-v0": 3}


def _vec(env_id, n=N, **kw):
    kw.setdefault("want_depth", True)
    kw.setdefault("seed", SEEDS.get(env_id, 0))
    return vec_env(env_id, n, **kw)


def _state(vec):
    """per env: pose (x, z, dir), cam (height, fwd_disp, pitch, fov_y), extent"""
    st = vec.state(("agent_pos", "agent_dir", "cam", "extent"))
    pos, d, cam, ext = (st[k].cpu().numpy() for k in ("agent_pos", "agent_dir", "cam", "extent"))
    return [((pos[i, 0], pos[i, 2], d[i]), tuple(cam[i]), tuple(ext[i])) for i in range(vec.num_envs)]


def _sensor(o):
    return dict(min_range=o.min_range, max_range=o.max_range, floor_tol=o.floor_tol, top=o.top)


def _inputs(vec, labels, depth):
    """what the binding projects: (code int32[N, H, W], base, depth float32[N, H, W]) on the host"""
    import torch
    H, W = vec.obs.shape[1], vec.obs.shape[2]
    if torch.is_tensor(labels):
        code, base = labels, 0
    else:
        code, base = labels.code, BASE
        if depth is None and labels.depth is not None:
            depth = labels.depth
    depth = vec.depth if depth is None else depth
    return code.cpu().numpy(), base, depth.cpu().numpy().reshape(vec.num_envs, H, W)


def _window_both(vec, w, labels, depth=None, mask=None):
    """one object_update on the device and through the restatement: equal for the envs under the mask, every byte kept for the others"""
    msaa = int(vec.engine.cfg.msaa)
    code, base, frames = _inputs(vec, labels, depth)
    before = w.plane.cpu().numpy()
    assert vec.object_update(w, labels, depth=depth, mask=_dev(mask)) is w.plane
    got = w.plane.cpu().numpy()
    out = []
    for i, (pose, cam, _) in enumerate(_state(vec)):
        if mask is not None and not mask[i]:
            assert np.array_equal(got[i], before[i]), (i, "a masked-off env's plane moved")
            out.append(None)
            continue
        want = ref.window(frames[i], code[i], base, pose, cam, msaa, w.size, w.cell, w.back, w.frame == "north", **_sensor(w))
        assert np.array_equal(got[i], want), (i, w.size, w.back, w.frame, "cells that differ", np.argwhere(got[i] != want)[:8].tolist())
        out.append(want)
    return out


def _mirror(m, garbage=0):
    return [ref.Map(m.gx, m.gz, m.ids, garbage) for _ in range(m.map.shape[0])]


def _map_both(vec, m, mirror, labels, depth=None, clear=None, mask=None):
    """one object_map_update on the device and on `mirror` (a ref.Map per env) through the restatement"""
    msaa = int(vec.engine.cfg.msaa)
    code, base, frames = _inputs(vec, labels, depth)
    assert vec.object_map_update(m, labels, depth=depth, clear=_dev(clear), mask=_dev(mask)) is m.cells
    maps, cells, pos = m.map.cpu().numpy(), m.cells.cpu().numpy(), m.pos.cpu().numpy()
    for i, (pose, cam, ext) in enumerate(_state(vec)):
        if mask is None or mask[i]:
            ref.map_update(mirror[i], frames[i], code[i], base, pose, cam, msaa, ext, m.cell, bool(clear is not None and clear[i]), **_sensor(m))
        assert np.array_equal(maps[i], mirror[i].map), (i, "map", np.argwhere(maps[i] != mirror[i].map)[:8].tolist())
        assert np.array_equal(cells[i], mirror[i].cells), (i, "cells", cells[i], mirror[i].cells)
        assert ref.same_bits(pos[i], mirror[i].pos), (i, "pos", pos[i], mirror[i].pos)


def _objects(vec):
    """per env: [(slot, x, z, radius, height)] of the listed entities, from the host route"""
    st = vec.engine.get_state()
    return [[(k, float(st["ent_pos"][i][k][0]), float(st["ent_pos"][i][k][2]), float(st["ent_geom"][i][k][7]), float(st["ent_geom"][i][k][8]))
             for k in range(st["ent_kind"].shape[1]) if int(st["ent_kind"][i][k])] for i in range(vec.num_envs)]


def _seg_dist(ax, az, bx, bz, x, z):
    dx, dz = bx - ax, bz - az
    t = min(1.0, max(0.0, ((x - ax) * dx + (z - az) * dz) / (dx * dx + dz * dz)))
    return math.hypot(ax + t * dx - x, az + t * dz - z)


def _crosses(ax, az, bx, bz, s):
    """whether the stretch a -> b meets the wall segment s = (cx, cz, dx, dz)"""
    side = lambda px, pz, qx, qz, rx, rz: (qx - px) * (rz - pz) - (qz - pz) * (rx - px)
    return (side(ax, az, bx, bz, s[0], s[1]) * side(ax, az, bx, bz, s[2], s[3]) <= 0.0
            and side(s[0], s[1], s[2], s[3], ax, az) * side(s[0], s[1], s[2], s[3], bx, bz) <= 0.0)


def _face_an_object(vec, distance):
    """Teleports every agent `distance` metres from an object of its world, facing it — the lowest slot that reaches into the camera's
    view from there (0.75 m high or more), from the first of eight directions that stands half a metre inside the extent with no wall
    across the line of sight and no other object within 0.3 m of it.  Returns the slot per env."""
    objects, states, walls = _objects(vec), _state(vec), [w["segs"] for w in worlds(vec)]
    xs, zs, ds, slots = [], [], [], []
    for i in range(vec.num_envs):
        x0, x1, z0, z1 = states[i][2]
        found = None
        for s, ex, ez, _, height in objects[i]:
            if height < 0.75:
                continue
            for k in range(8):
                d = k * math.pi / 4
                x, z = ex - distance * math.cos(d), ez + distance * math.sin(d)
                inside = x0 + 0.5 <= x <= x1 - 0.5 and z0 + 0.5 <= z <= z1 - 0.5
                clear = not any(_crosses(x, z, ex, ez, [float(v) for v in seg]) for seg in walls[i])
                if inside and clear and all(o[0] == s or _seg_dist(x, z, ex, ez, o[1], o[2]) > o[3] + 0.3 for o in objects[i]):
                    found = (x, z, d, s)
                    break
            if found:
                break
        assert found, (i, objects[i])
        xs.append(found[0]); zs.append(found[1]); ds.append(found[2]); slots.append(found[3])
    teleport(vec, (np.array(xs), np.array(zs)))
    import torch
    vec.set_state_where(torch.ones(vec.num_envs, dtype=torch.uint8, device="cuda"), agent_dir=torch.as_tensor(np.array(ds), dtype=torch.float64, device="cuda"))
    return slots


SHAPES = [(S, a, f) for S in (1, 2, 33, 128) for a in ("centre", "bottom") for f in ("heading", "north")]


@pytest.mark.parametrize("env_id,domain_rand", [("MiniWorld-Hallway-v0", False), ("MiniWorld-FourRooms-v0", False), ("MiniWorld-PickupObjects-v0", False),
                                                ("MiniWorld-Hallway-v0", True)])
def test_walk_equals_the_restatement_at_every_step(env_id, domain_rand):
    import torch
    vec = _vec(env_id, domain_rand=domain_rand)
    rng = np.random.default_rng(3700)
    # 128 x 128 cells of 0.1 m: the largest window; the others at the default cell
    windows = [vec.object_window(size=S, cell=0.1 if S == 128 else 0.25, anchor=a, frame=f) for S, a, f in SHAPES]
    field = vec.nav_field()
    own, envs = vec.object_map(like=field), vec.object_map(like=field)
    assert (own.gx, own.gz, own.ids) == (field.gx, field.gz, min(int(vec.engine.cfg.max_ents), 255))
    mirror_own, mirror_envs = _mirror(own), _mirror(envs)
    labels = vec.label_frame(meshes="bounds", depth=True)
    _face_an_object(vec, 2.5)           # the walk starts where an object is in view
    object_cells = counted = 0
    for k in range(6):
        vec.step(torch.as_tensor(rng.integers(0, 3, N), dtype=torch.int32, device="cuda"))
        vec.label_update(labels)
        for j, w in enumerate(windows if k == 0 else windows[k::5]):
            # once with the label frame's own depth, once with the env's depth map
            for want in _window_both(vec, w, labels, depth=vec.depth if (j + k) % 2 else None):
                object_cells += int((want != 0).sum())
        _map_both(vec, own, mirror_own, labels)
        _map_both(vec, envs, mirror_envs, labels, depth=vec.depth)
        counted += int(own.cells.sum()) + int(envs.cells.sum())
    assert object_cells > 0 and counted > 0
    vec.engine.check()
    vec.close()


@pytest.mark.parametrize("width,height,msaa", [(21, 13, 8), (21, 13, 1), (80, 60, 4)])
def test_other_frame_sizes_and_sample_counts(width, height, msaa):
    """21 x 13 = 273 pixels: a multiple of neither the lane count nor 4 (scalar loads, a ragged last round); 4 and 1 samples: the depth is
    taken elsewhere in the pixel"""
    import torch
    vec = _vec("MiniWorld-Hallway-v0", obs_width=width, obs_height=height, msaa=msaa)
    rng = np.random.default_rng(3701)
    w, wn = vec.object_window(size=33), vec.object_window(size=9, cell=0.5, anchor="bottom", frame="north")
    m = vec.object_map()
    mirror = _mirror(m)
    labels = vec.label_frame(depth=True)
    _face_an_object(vec, 2.5)
    cells = 0
    for k in range(3):
        vec.step(torch.as_tensor(rng.integers(0, 2, N), dtype=torch.int32, device="cuda"))
        vec.label_update(labels)
        cells += sum(int((p != 0).sum()) for p in _window_both(vec, w, labels, depth=vec.depth if k == 1 else None))
        _window_both(vec, wn, labels)
        _map_both(vec, m, mirror, labels, depth=vec.depth if k == 2 else None)
    assert cells > 0
    vec.engine.check()
    vec.close()


def _hand_built(vec, gx, gz, cell, ids):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import ObjectMap
    return ObjectMap(torch.zeros((N, gz, gx), dtype=torch.uint8, device="cuda"), torch.zeros((N, ids), dtype=torch.int32, device="cuda"),
                     torch.zeros((N, ids, 3), dtype=torch.float64, device="cuda"), engine.MwNavParams(cell, 0.0, 0.0, gx, gz, 0, 0), ids, 0.05, 8.0, 0.1, 1.6)


def test_the_largest_launch_and_one_cell_more():
    from miniworld_amd import engine
    vec = _vec("MiniWorld-Hallway-v0")
    ext = _state(vec)[0][2]
    cell = max(ext[1] - ext[0], ext[3] - ext[2]) / 127.0         # 128 x 128 cells over the extent: 64 KiB of keys
    labels = vec.label_frame(depth=True)
    slots = _face_an_object(vec, 2.0)
    vec.label_update(labels)
    for ids in (255, 1):            # 255: 3060 bytes of sums behind the keys, 68 596 bytes of LDS
        m = _hand_built(vec, 128, 128, cell, ids)
        mirror = _mirror(m)
        _map_both(vec, m, mirror, labels, clear=np.ones(N, np.uint8))
        _map_both(vec, m, mirror, labels)
        assert all(int(m.cells[i, slots[i]]) > 0 for i in range(N) if slots[i] < ids)
    vec.engine.check()
    more = _hand_built(vec, 145, 113, cell, 255)         # 16385 cells
    more.map.fill_(0xAB)
    with pytest.raises(engine.EngineError, match="use a larger cell"):
        vec.object_map_update(more, labels)
    assert (more.map == 0xAB).all() and not more.cells.any()
    vec.engine.check()
    vec.close()


def test_a_masked_env_keeps_every_byte():
    import torch
    vec = _vec("MiniWorld-Hallway-v0")
    mask = np.array([1, 0, 1, 0], np.uint8)
    labels = vec.label_frame(depth=True)
    _face_an_object(vec, 2.0)
    vec.label_update(labels)
    w = vec.object_window(size=9)
    w.plane.fill_(0xAB)
    _window_both(vec, w, labels, mask=mask)
    assert (w.plane.cpu().numpy()[mask == 0] == 0xAB).all() and not (w.plane.cpu().numpy()[mask == 1] == 0xAB).any()
    m = vec.object_map()
    m.map.fill_(0xAB)
    m.cells.view(torch.uint8).fill_(0xAB)
    m.pos.view(torch.uint8).fill_(0xAB)
    mirror = _mirror(m, 0xAB)
    # clear under the mask rewrites rows 0 and 2; clear outside it does nothing: the mask wins
    _map_both(vec, m, mirror, labels, clear=np.array([1, 1, 1, 0], np.uint8), mask=mask)
    maps, cells, pos = m.map.cpu().numpy(), m.cells.cpu().numpy(), m.pos.cpu().numpy()
    assert (maps[mask == 0] == 0xAB).all() and (cells[mask == 0] == -0x54545455).all() and (pos[mask == 0].view(np.uint8) == 0xAB).all()
    assert not (maps[mask == 1] == 0xAB).any() and (cells[mask == 1] >= 0).all() and cells[mask == 1].sum() > 0
    # without clear the bytes out of view stay, garbage as they are
    _map_both(vec, m, mirror, labels, mask=1 - mask)
    assert (m.map.cpu().numpy()[mask == 0] == 0xAB).any()
    vec.engine.check()
    vec.close()


def test_clear_behind_same_step_auto_reset_restarts_the_finished_envs_maps():
    import torch
    vec = _vec("MiniWorld-MazeS3-v0", max_episode_steps=4)
    m = vec.object_map()
    mirror = _mirror(m)
    labels = vec.label_frame()          # no depth of its own: the env's
    vec.label_update(labels)
    _map_both(vec, m, mirror, labels)
    rng = np.random.default_rng(3702)
    finished = 0
    for k in range(9):
        actions = rng.integers(0, 2, N)           # turns: nobody reaches the box, every episode ends at its step limit
        _, _, term, trunc = vec.step(torch.as_tensor(actions, dtype=torch.int32, device="cuda"))[:4]
        done = (term | trunc).bool()
        finished += int(done.sum())
        vec.label_update(labels)
        _map_both(vec, m, mirror, labels, clear=done.cpu().numpy().astype(np.uint8))
        # a restarted map holds this frame alone
        fresh = _mirror(m)
        _map_both(vec, vec.object_map(), fresh, labels)
        d = done.cpu().numpy()
        assert all(np.array_equal(mirror[i].map, fresh[i].map) for i in range(N) if d[i])
    assert finished >= 2 * N
    vec.engine.check()
    vec.close()


def _codes(fill, **regions):
    """a label image [N, 60, 80] of `fill` with id in columns lo .. hi - 1: _codes(-1, id3=(30, 50)); the caller's own: base 0"""
    code = np.full((N, 60, 80), fill, np.int32)
    for name, (lo, hi) in regions.items():
        code[:, :, lo:hi] = int(name[2:])
    return code


def test_synthetic_labels_through_a_tensor_and_the_depth_argument():
    import torch
    vec = _vec("MiniWorld-Hallway-v0")
    flat = lambda v: torch.full((N, 60, 80, 1), v, dtype=torch.float32, device="cuda")
    depth = flat(2.0)
    ahead, behind = 0.3, 0.3 + math.pi
    a, b = _dev(_codes(-1, id3=(30, 50))), _dev(_codes(-1))
    m = vec.object_map(ids=5)
    mirror = _mirror(m)
    x, z = np.full(N, 5.0), np.full(N, 0.1)
    # A puts id 3 into some cells; C, looking the other way, leaves them; B, from A's pose, sees them empty; A again; clear with C
    seen = []
    for direction, labels, clear in ((ahead, a, 1), (behind, b, 0), (ahead, b, 0), (ahead, a, 0), (behind, b, 1)):
        teleport(vec, (x, z), direction)
        _map_both(vec, m, mirror, labels, depth=depth, clear=np.full(N, clear, np.uint8))
        seen.append((m.map.cpu().numpy().copy(), m.cells.cpu().numpy().copy(), m.pos.cpu().numpy().copy()))
    held = seen[0][0] == 4
    assert held.any(axis=(1, 2)).all() and (seen[0][1][:, 3] == held.sum(axis=(1, 2))).all() and not np.isnan(seen[0][2][:, 3]).any()
    assert np.isnan(seen[0][2][:, [0, 1, 2, 4]]).all()          # n == 0: NaN positions
    assert np.array_equal(seen[1][0], seen[0][0]) and np.array_equal(seen[1][1], seen[0][1])
    assert not seen[2][0].any() and not seen[2][1].any() and np.isnan(seen[2][2]).all()
    assert np.array_equal(seen[3][0], seen[0][0]) and not seen[4][0].any()
    # an id from K on is mapped, not counted
    few = vec.object_map(ids=3)
    teleport(vec, (x, z), ahead)
    _map_both(vec, few, _mirror(few), a, depth=depth)
    assert (few.map == 4).any() and not few.cells.any() and few.pos.isnan().all()
    # one cell for all 4800 pixels — every lane's atomicMin on one address —, and the lowest of the ids in it wins
    one = vec.object_window(size=1, cell=20.0)
    invalid = [255, 300, -1, -BASE - 1, np.iinfo(np.int32).min, np.iinfo(np.int32).max]
    for values, byte in (([7, 2, 200, 254] + invalid, 1 + 2), (invalid, 0), ([254] + invalid, 255), ([0], 1)):
        rng = np.random.default_rng(3703)
        codes = rng.permutation(np.resize(np.array(values, np.int64), N * 4800)).astype(np.int32).reshape(N, 60, 80)
        got = _window_both(vec, one, _dev(codes), depth=depth)
        assert all(g.tolist() == [[byte]] for g in got), (values, got)
    # ... the same conflict with a label frame's base: ids are code - RAY_ENT, and a wall's code is no object
    frame = vec.label_frame()
    frame.code.copy_(_dev(np.resize(np.array([BASE + 7, BASE + 2, BASE + 255, BASE - 1, 3, -1], np.int32), (N, 60, 80))))
    assert all(g.tolist() == [[3]] for g in _window_both(vec, one, frame, depth=depth))
    # depths that are no point leave the window all 0 and every byte of an uncleared map as it was
    w = vec.object_window(size=33)
    nan, inf = float("nan"), float("inf")
    full = _dev(_codes(3))
    for bad in (nan, inf, 0.0, -3.0, 100.0, 0.049, 8.000001):
        w.plane.fill_(0x5A)
        _window_both(vec, w, full, depth=flat(bad))
        assert not w.plane.any(), bad
        m.map.fill_(0x11)
        for r in mirror:
            r.map[:] = 0x11
        _map_both(vec, m, mirror, full, depth=flat(bad))
        assert (m.map == 0x11).all() and not m.cells.any(), bad
    # ... and a frame with each of them somewhere, per env another, under random ids
    rng = np.random.default_rng(3704)
    mixed = rng.choice(np.array([nan, inf, -1.0, 0.0, 100.0, 0.05, 8.0, 0.7, 1.3, 2.9, 4.4], np.float32), (N, 60, 80, 1))
    ids = rng.integers(-2, 8, (N, 60, 80)).astype(np.int32)
    _window_both(vec, w, _dev(ids), depth=_dev(mixed))
    _map_both(vec, m, mirror, _dev(ids), depth=_dev(mixed), clear=np.ones(N, np.uint8))
    vec.engine.check()
    vec.close()


# ---------------------------------------------------------------------------------------------------------------- the geometry

@pytest.mark.parametrize("env_id", ["MiniWorld-Hallway-v0", "MiniWorld-OneRoom-v0", "MiniWorld-PickupObjects-v0"])
def test_a_sensed_cell_lies_on_its_object_and_nowhere_the_privileged_plane_is_empty(env_id):
    vec = _vec(env_id)
    cell = 0.25
    bound = cell * math.sqrt(2) / 2 + 1e-6
    labels = vec.label_frame(meshes="bounds", depth=True)
    m = vec.object_map(cell=cell)
    sensed = vec.object_window(size=41, cell=cell)
    privileged = vec.ego_window(size=41, cell=cell, planes=("entity",), entity_pad=cell * math.sqrt(2) / 2 + 0.05)
    slots = _face_an_object(vec, 1.5)
    objects = _objects(vec)
    vec.label_update(labels)
    _map_both(vec, m, _mirror(m), labels)           # the label's own depth
    _window_both(vec, sensed, labels)
    vec.ego_update(privileged)
    maps, cells, pos = m.map.cpu().numpy(), m.cells.cpu().numpy(), m.pos.cpu().numpy()
    for i, (_, _, ext) in enumerate(_state(vec)):
        by_slot = {o[0]: o for o in objects[i]}
        for byte in sorted(set(np.unique(maps[i]).tolist()) - {0}):
            s, (_, ex, ez, radius, _) = byte - 1, by_slot[byte - 1]
            jj, ii = np.nonzero(maps[i] == byte)
            far = np.hypot(ext[0] + (ii + 0.5) * cell - ex, ext[2] + (jj + 0.5) * cell - ez)
            assert (far <= radius + bound).all(), (env_id, i, s, float(far.max()), radius + bound)
            assert math.hypot(pos[i, s, 0] - ex, pos[i, s, 2] - ez) <= radius + bound and cells[i, s] == len(ii), (env_id, i, s, pos[i, s])
        # the condition that keeps the statement from passing empty: the object each agent faces is on its map
        assert cells[i, slots[i]] >= 1, (env_id, i, slots[i], cells[i])
    stray = (sensed.plane.cpu().numpy() != 0) & (privileged.entity.cpu().numpy() == 0)
    assert not stray.any(), (env_id, np.argwhere(stray)[:8].tolist())
    assert (sensed.plane != 0).any()
    vec.engine.check()
    vec.close()


# ---------------------------------------------------------------------------------------------------------------- refusals, the adapter

def test_an_uncovered_extent_is_reported_once():
    from miniworld_amd import engine
    vec = _vec("MiniWorld-Hallway-v0")
    labels = vec.label_frame()
    vec.label_update(labels)
    short = _hand_built(vec, 3, 3, 0.25, 4)
    short.map.fill_(7)
    short.cells.fill_(5)
    vec.object_map_update(short, labels)
    assert not short.map.any() and not short.cells.any() and short.pos.isnan().all()
    with pytest.raises(engine.EngineError, match="mw_label_project refused an env"):
        vec.engine.check()
    vec.engine.check()          # once
    vec.close()


def test_the_library_refuses_what_the_header_says():
    import torch
    from miniworld_amd import engine
    vec = _vec("MiniWorld-Hallway-v0")
    e = vec.engine
    code = torch.zeros((N, 60, 80), dtype=torch.int32, device="cuda")
    plane = torch.full((N, 9, 9), 0xAB, dtype=torch.uint8, device="cuda")
    good = dict(base=0, min_range=0.05, max_range=8.0, floor_tol=0.1, top=1.6, size=9, cell=0.25, back=0.0, flags=0, plane=plane)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(min_range=0.0), dict(min_range=nan), dict(max_range=inf), dict(max_range=-1.0), dict(min_range=3.0, max_range=2.0), dict(floor_tol=-0.1),
               dict(floor_tol=nan), dict(top=0.05), dict(top=inf), dict(cell=0.0), dict(cell=inf), dict(back=nan), dict(flags=1), dict(flags=4), dict(base=-1),
               dict(ids=1), dict(ids=-1), dict(ids=256)):
        with pytest.raises(engine.EngineError, match="mw_label_project"):
            e.label_project(vec.depth, code, **dict(good, **kw))
    big = torch.zeros((N, 129, 129), dtype=torch.uint8, device="cuda")
    with pytest.raises(engine.EngineError, match="size 129"):
        e.label_project(vec.depth, code, **dict(good, size=129, plane=big))
    m = vec.object_map()
    m.map.fill_(0xAB)
    grid = dict(base=0, min_range=0.05, max_range=8.0, floor_tol=0.1, top=1.6, params=m.params, map=m.map, ids=m.ids, cells=m.cells, pos=m.pos)
    for kw in (dict(flags=2), dict(base=-5), dict(cells=None, pos=None), dict(ids=256, cells=None, pos=None), dict(ids=-1, cells=None, pos=None)):
        with pytest.raises(engine.EngineError, match="mw_label_project"):
            e.label_project(vec.depth, code, **dict(grid, **kw))
    e.label_project(vec.depth, code, **dict(grid, ids=0, cells=None, pos=None, mask=torch.zeros(N, dtype=torch.uint8, device="cuda")))     # ids = 0 needs neither
    wide = engine.MwNavParams(0.25, 0.0, 0.0, 129, 128, 0, 0)
    with pytest.raises(engine.EngineError, match="use a larger cell"):
        e.label_project(vec.depth, code, **dict(grid, params=wide, map=torch.zeros((N, 128, 129), dtype=torch.uint8, device="cuda")))
    # a null d_code and a null d_depth, past the binding
    host = (engine.C.c_double * 6)(0.05, 8.0, 0.1, 1.6, 0.25, 0.0)
    for depth_ptr, code_ptr in ((vec.depth.data_ptr(), None), (None, code.data_ptr())):
        rc = e.lib.mw_label_project(e.h, host, depth_ptr, code_ptr, 0, None, 9, 0, plane.data_ptr(), None, None, None, 0, None, None, None)
        assert rc == -1 and b"mw_label_project" in e.lib.mw_last_error(e.h)
    assert (plane == 0xAB).all() and (m.map == 0xAB).all() and not m.cells.any()          # nothing was written
    vec.engine.check()
    vec.close()


def test_the_adapters_key_is_a_direct_update_at_the_same_state():
    import torch
    from miniworld_amd.vector import MiniWorldVectorEnv
    plain = MiniWorldVectorEnv("MiniWorld-Hallway-v0", N, label_frame={}, seed=0)
    assert "object_map" not in plain.reset(seed=3)[1] and plain.object_win is None
    plain.close()
    envs = MiniWorldVectorEnv("MiniWorld-Hallway-v0", N, object_map=dict(size=17, max_range=5.0), label_frame=dict(meshes="bounds"), seed=0)
    _, info = envs.reset(seed=3)
    rng = np.random.default_rng(3705)
    cells = 0
    for k in range(4):
        if k:
            _, _, _, _, info = envs.step(torch.as_tensor(rng.integers(0, 3, N), dtype=torch.int32, device="cuda"))
        mine = envs.vec.object_window(size=17, max_range=5.0)
        want = _window_both(envs.vec, mine, info["label"])
        assert info["object_map"].dtype == torch.uint8 and tuple(info["object_map"].shape) == (N, 17, 17)
        assert torch.equal(info["object_map"], mine.plane) and info["object_map"] is not envs.object_win.plane
        cells += sum(int((x != 0).sum()) for x in want)
        if k == 0:
            _face_an_object(envs.vec, 2.5)
    assert cells > 0
    envs.close()
