"""The yardstick of the ray-cast tests (tests/test_ray_cpu.py, tests/test_gpu_ray.py): an independent restatement of
include/mwengine.h's rules for mw_ray_cast — numpy in float64 in the documented order of operations, vectorised over the rays of an
env, one obstacle at a time in index order — that shares no code with miniworld_amd/csrc/mw_ray.h.  Worlds are the dicts of
tests/nav_reference.py (world_of_scene, world_of_engine).  The fan's sines and cosines come from pyoracle.sincos, bit-identical to the
engine's.  Comparisons against `cast` are exact.

`check_property` ties a result to the reference's own predicate instead of to a second copy of the formulas: just before a reported
hit the swept disc is clear of every obstacle by the closest-point distance of intersect_circle_segs (math.py:30-62), just behind it
it is not."""
import numpy as np

ENT_NONE = 0
RAY_ENT = 0x10000
NONE = -1.0


def _ray_seg(ox, oz, dx, dz, ax, az, bx, bz):
    ex, ez = bx - ax, bz - az
    den = dx * ez - dz * ex
    wx, wz = ax - ox, az - oz
    t = (wx * ez - wz * ex) / den
    s = (wx * dz - wz * dx) / den
    return np.where(~(den == 0.0) & (t >= 0.0) & (s >= 0.0) & (s <= 1.0), t, NONE)


def _ray_circle(ox, oz, dx, dz, cx, cz, R):
    wx, wz = ox - cx, oz - cz
    A = dx * dx + dz * dz
    B = wx * dx + wz * dz
    C = (wx * wx + wz * wz) - R * R
    disc = B * B - A * C
    t = (-B - np.sqrt(disc)) / A
    out = np.where(t >= 0.0, t, NONE)
    out = np.where(disc < 0.0, NONE, out)
    return np.where(C < 0.0, 0.0, out)


def _closest(ax, az, bx, bz, x, z):
    """the closest-point distance from (x, z) to the segment a-b: intersect_circle_segs' lines"""
    abx, abz = bx - ax, bz - az
    apx, apz = x - ax, z - az
    dap = apx * abx + apz * abz
    dab = abx * abx + abz * abz
    t = dap / dab
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    cx, cz = ax + t * abx, az + t * abz
    ddx, ddz = cx - x, cz - z
    return np.sqrt(ddx * ddx + ddz * ddz)


def _lower(best, t):
    return np.where((t >= 0.0) & (~(best >= 0.0) | (t < best)), t, best)


def _ray_wall(ox, oz, dx, dz, seg, r):
    ax, az, bx, bz = (float(v) for v in seg)
    if not r > 0.0:
        return _ray_seg(ox, oz, dx, dz, ax, az, bx, bz)
    ex, ez = bx - ax, bz - az
    ln = np.sqrt(np.float64(ex * ex + ez * ez))
    nx, nz = float((np.float64(ez) / ln) * r), float((np.float64(-ex) / ln) * r)
    t = _ray_circle(ox, oz, dx, dz, ax, az, r)
    t = _lower(t, _ray_circle(ox, oz, dx, dz, bx, bz, r))
    t = _lower(t, _ray_seg(ox, oz, dx, dz, ax + nx, az + nz, bx + nx, bz + nz))
    t = _lower(t, _ray_seg(ox, oz, dx, dz, ax - nx, az - nz, bx - nx, bz - nz))
    return np.where(_closest(ax, az, bx, bz, ox, oz) < r, 0.0, t)


def listed_slots(w):
    return [s for s in range(len(w["kind"])) if int(w["kind"][s]) != ENT_NONE and s != int(w["carry"])]


def cast(w, origin, direction, max_t, radius, entities):
    """origin float64[R, 2] (x, z), direction float64[R, 2] (dx, dz) -> t float64[R], hit int32[R]"""
    o, d = np.asarray(origin, np.float64).reshape(-1, 2), np.asarray(direction, np.float64).reshape(-1, 2)
    ox, oz, dx, dz = o[:, 0], o[:, 1], d[:, 0], d[:, 1]
    r = float(radius)
    best = np.full(len(o), float(max_t), np.float64)
    hit = np.full(len(o), -1, np.int32)

    def take(t, code):
        nonlocal best, hit
        ok = (t >= 0.0) & (t < best)
        best = np.where(ok, t + 0.0, best)
        hit = np.where(ok, np.int32(code), hit)
    with np.errstate(all="ignore"):
        for i, seg in enumerate(np.asarray(w["segs"], np.float64).reshape(-1, 4)):
            take(_ray_wall(ox, oz, dx, dz, seg, r), i)
        if entities:
            for s in listed_slots(w):
                take(_ray_circle(ox, oz, dx, dz, float(w["pos"][s][0]), float(w["pos"][s][2]), float(w["radius"][s]) + r), RAY_ENT + s)
    bad = np.isnan(ox) | np.isnan(oz) | np.isnan(dx) | np.isnan(dz)
    return np.where(bad, float(max_t), best), np.where(bad, np.int32(-1), hit).astype(np.int32)


def fan_directions(agent_dir, offsets):
    """float64[R, 2]: (cos, -sin) of agent_dir + offset through the engine's deterministic sin / cos; NaN beyond its domain"""
    import pyoracle
    out = np.full((len(offsets), 2), np.nan, np.float64)
    for k, off in enumerate(offsets):
        ang = float(agent_dir) + float(off)
        if -1e6 < ang < 1e6:
            s, c = pyoracle.sincos(ang)
            out[k] = (c, -s)
    return out


def lidar_offsets(rays, fov):
    import math
    if fov < 2 * math.pi:
        return [0.0] if rays == 1 else [-fov / 2 + k * fov / (rays - 1) for k in range(rays)]
    return [k * 2 * math.pi / rays for k in range(rays)]


# ---------------------------------------------------------------------------------------------------------------- the property

DELTA, GRAZE_BACK, GRAZE_SPEED, EXCUSED_SHARE, ON_WALL = 1e-6, 1e-3, 1e-2, 0.02, 1e-9


def clearance(w, x, z, entities):
    """the smallest closest-point distance from each point to a wall and, where entities count, to an entity's circle"""
    x, z = np.asarray(x, np.float64), np.asarray(z, np.float64)
    out = np.full(x.shape, np.inf)
    with np.errstate(all="ignore"):
        for ax, az, bx, bz in np.asarray(w["segs"], np.float64).reshape(-1, 4):
            out = np.fmin(out, _closest(ax, az, bx, bz, x, z))
        if entities:
            for s in listed_slots(w):
                out = np.fmin(out, np.hypot(x - float(w["pos"][s][0]), z - float(w["pos"][s][2])) - float(w["radius"][s]))
    return out


def check_property(w, origin, direction, t, hit, radius, entities):
    """asserts the property of every hit with t > 0 (radius > 0) and that a plain ray's hit point lies on the reported wall; returns
    (rays checked, rays excused as grazing)"""
    o, d = np.asarray(origin, np.float64).reshape(-1, 2), np.asarray(direction, np.float64).reshape(-1, 2)
    r = float(radius)
    ln = np.hypot(d[:, 0], d[:, 1])
    idx = np.nonzero((hit >= 0) & (t > 0.0) & (ln > 0.0))[0]
    if len(idx) == 0:
        return 0, 0
    o, d, t, ln, code = o[idx], d[idx], t[idx], ln[idx], hit[idx]
    if not r > 0.0:
        segs = np.asarray(w["segs"], np.float64).reshape(-1, 4)
        px, pz = o[:, 0] + t * d[:, 0], o[:, 1] + t * d[:, 1]
        for k in range(len(idx)):
            if code[k] < RAY_ENT:
                ax, az, bx, bz = segs[code[k]]
                off = float(_closest(ax, az, bx, bz, px[k], pz[k]))
                assert off <= ON_WALL, ("the hit point lies off the reported wall", int(idx[k]), off)
        return len(idx), 0

    def at(tt):
        return clearance(w, o[:, 0] + tt * d[:, 0], o[:, 1] + tt * d[:, 1], entities)
    before, after = at(t - DELTA / ln), at(t + DELTA / ln)
    good = (before >= r) & (after < r)
    speed = (at(t - GRAZE_BACK / ln) - r) / GRAZE_BACK
    grazing = ~good & (speed < GRAZE_SPEED)
    failed = ~good & ~grazing
    assert not failed.any(), ("rays whose hit is not where the swept disc first touches", idx[failed][:8].tolist(), before[failed][:8], after[failed][:8])
    return len(idx), int(grazing.sum())
