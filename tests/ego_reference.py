"""The yardstick of the egocentric-window tests (tests/test_ego_cpu.py, tests/test_gpu_ego.py): an independent restatement of
include/mwengine.h's rules for mw_ego_map — numpy in float64, every operation of the documented order its own numpy call (nothing can be
contracted), every point of the window at once, the wall distance through tests/ray_reference.py's closest-point restatement, the line
of sight through its `cast` with max_t = 1 and radius 0, the heading through its `fan_directions` at offset 0 — that shares no code with
miniworld_amd/csrc/mw_ego.h.  Worlds are the dicts of tests/nav_reference.py.  Comparisons against it are exact."""
import numpy as np

import ray_reference as ray

WALL, ENTITY, VISIBLE = 1, 2, 4
NAMES = {"wall": WALL, "entity": ENTITY, "visible": VISIBLE}


def heading(direction):
    """(hx, hz) = (cos, -sin) of the agent's direction as the engine forms it"""
    hx, hz = ray.fan_directions(direction, [0.0])[0]
    return np.float64(hx), np.float64(hz)


def points(pose, size, cell, back, north, origin=None):
    """px, pz float64[S, S] of the window of the agent at pose = (x, z, dir); origin = (x, z) replaces the agent's position"""
    S = int(size)
    ox, oz = (np.float64(pose[0]), np.float64(pose[1])) if origin is None else (np.float64(origin[0]), np.float64(origin[1]))
    cell, back = np.float64(cell), np.float64(back)
    half = np.multiply(np.float64(S), np.float64(0.5))
    c = np.add(np.arange(S, dtype=np.float64), np.float64(0.5))
    r = np.add(np.arange(S, dtype=np.float64), np.float64(0.5))
    lat = np.multiply(np.subtract(c, half), cell)
    fwd = np.multiply(np.add(np.subtract(half, r), back), cell)
    if north:
        fx, fz, rx, rz = np.float64(0.0), np.float64(-1.0), np.float64(1.0), np.float64(0.0)
    else:
        hx, hz = heading(pose[2])
        fx, fz, rx, rz = hx, hz, np.negative(hz), hx
    F = fwd[:, None].repeat(S, 1)
    L = lat[None, :].repeat(S, 0)
    with np.errstate(all="ignore"):
        px = np.add(ox, np.add(np.multiply(F, fx), np.multiply(L, rx)))
        pz = np.add(oz, np.add(np.multiply(F, fz), np.multiply(L, rz)))
    return px, pz


def wall_plane(w, px, pz, wall_radius):
    ext = np.asarray(w["extent"], np.float64)
    with np.errstate(all="ignore"):
        inside = (px >= ext[0]) & (px <= ext[1]) & (pz >= ext[2]) & (pz <= ext[3])
        near = np.zeros(px.shape, bool)
        for ax, az, bx, bz in np.asarray(w["segs"], np.float64).reshape(-1, 4):
            near |= ray._closest(ax, az, bx, bz, px, pz) < np.float64(wall_radius)
    return np.where(inside & ~near, 0, 1).astype(np.uint8)


def entity_plane(w, px, pz, entity_pad):
    out = np.zeros(px.shape, np.uint8)
    with np.errstate(all="ignore"):
        for s in reversed(ray.listed_slots(w)):         # (the lowest slot is written last)
            R = np.add(np.float64(w["radius"][s]), np.float64(entity_pad))
            dx, dz = np.subtract(px, np.float64(w["pos"][s][0])), np.subtract(pz, np.float64(w["pos"][s][2]))
            inside = np.add(np.multiply(dx, dx), np.multiply(dz, dz)) < np.multiply(R, R)
            out[inside] = 1 + s
    return out


def visible_plane(w, px, pz, pose, origin, max_range, cos_half, entities):
    ox, oz = (np.float64(pose[0]), np.float64(pose[1])) if origin is None else (np.float64(origin[0]), np.float64(origin[1]))
    hx, hz = heading(pose[2])
    with np.errstate(all="ignore"):
        vx, vz = np.subtract(px, ox), np.subtract(pz, oz)
        dist = np.sqrt(np.add(np.multiply(vx, vx), np.multiply(vz, vz)))
        near = dist <= np.float64(max_range)
        cone = (dist == 0.0) | (np.add(np.multiply(vx, hx), np.multiply(vz, hz)) >= np.multiply(np.float64(cos_half), dist))
        if cos_half == -1.0:
            cone = np.ones_like(cone)
        cand = near & cone
    out = np.zeros(px.shape, np.uint8)
    if cand.any():
        d = np.stack([vx[cand], vz[cand]], axis=1)
        o = np.tile(np.array([[ox, oz]]), (len(d), 1))
        t, hit = ray.cast(w, o, d, 1.0, 0.0, entities)
        out[cand] = ((t == 1.0) & (hit == -1)).astype(np.uint8)
    return out


def sample(w, px, pz, src, src_cell, fill):
    """src: uint8 / uint16 [gz, gx] on the grid of src_cell metres from the extent's min_x, min_z"""
    ext = np.asarray(w["extent"], np.float64)
    gz, gx = src.shape
    with np.errstate(all="ignore"):
        fi = np.floor(np.divide(np.subtract(px, ext[0]), np.float64(src_cell)))
        fj = np.floor(np.divide(np.subtract(pz, ext[2]), np.float64(src_cell)))
        inside = (fi >= 0.0) & (fi < np.float64(gx)) & (fj >= 0.0) & (fj < np.float64(gz))
    out = np.full(px.shape, int(fill) & (0xFFFF if src.dtype == np.uint16 else 0xFF), src.dtype)
    out[inside] = src[fj[inside].astype(np.int64), fi[inside].astype(np.int64)]
    return out


def window(w, pose, size, cell, back, north, planes, wall_radius, entity_pad, max_range, cos_half, entities, origin=None, src=None, src_cell=None,
           fill=0):
    """one call for one env: (uint8[P, S, S] in bit order — P may be 0 —, the sample [S, S] or None).  planes: names or bits."""
    bits = planes if isinstance(planes, int) else sum(NAMES[n] for n in planes)
    px, pz = points(pose, size, cell, back, north, origin)
    out = []
    if bits & WALL:
        out.append(wall_plane(w, px, pz, wall_radius))
    if bits & ENTITY:
        out.append(entity_plane(w, px, pz, entity_pad))
    if bits & VISIBLE:
        out.append(visible_plane(w, px, pz, pose, origin, max_range, cos_half, entities))
    stack = np.stack(out) if out else np.zeros((0, size, size), np.uint8)
    return stack, (None if src is None else sample(w, px, pz, src, src_cell, fill))
