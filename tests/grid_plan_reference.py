"""Grid rollouts restated (include/mwengine.h, "grid rollouts"), the rule and nothing else: numpy float64 over the plans of one env, a
Python loop over the steps, every cell of every box looked at — no bits, no ring, no cached sine — with sines and cosines from
pyoracle.sincos as ray_reference.py takes them; and the cases the CPU and GPU tests share."""
import math

import numpy as np

BOUND, NO_FIELD, MAX_RADIUS = 2.0 ** 30, 0xFFFF, 8
_K = np.arange(2 * MAX_RADIUS + 3, dtype=np.float64)        # offsets into a box: floor(u + rc) - floor(u - rc) <= 2 * rc + 1


def cells_of(x, z, lo, cell, gx, gz):
    """the flat index of each pose's cell, -1 outside the grid (or for a pose that is no number)"""
    with np.errstate(all="ignore"):
        fu, fw = np.floor((x - lo[0]) / cell), np.floor((z - lo[1]) / cell)
        inside = (fu >= 0) & (fu < gx) & (fw >= 0) & (fw < gz)
    return np.where(inside, np.where(inside, fw, 0) * gx + np.where(inside, fu, 0), -1).astype(np.int64)


def blocked(px, pz, lo, cell, rc, opaque, outside):
    """bool[M]: blocked(px, pz) of the rule, over every cell of the box"""
    gz, gx = opaque.shape
    with np.errstate(all="ignore"):
        u, w = (px - lo[0]) / cell, (pz - lo[1]) / cell
        ok = np.isfinite(u) & np.isfinite(w) & (np.abs(u) < BOUND) & (np.abs(w) < BOUND)
        u, w = np.where(ok, u, 0.0)[:, None, None], np.where(ok, w, 0.0)[:, None, None]
        c, j = np.floor(u - rc) + _K[None, None, :], np.floor(w - rc) + _K[None, :, None]
        in_box = (c <= np.floor(u + rc)) & (j <= np.floor(w + rc))
        inside = (c >= 0) & (c < gx) & (j >= 0) & (j < gz)
        opq = np.where(inside, opaque.ravel()[np.where(inside, j * gx + c, 0).astype(np.int64)] != 0, bool(outside))
        dx, dz = np.maximum(np.maximum(c - u, u - (c + 1.0)), 0.0), np.maximum(np.maximum(j - w, w - (j + 1.0)), 0.0)
        own = (c == np.floor(u)) & (j == np.floor(w))
        hit = (in_box & opq & ((dx * dx + dz * dz < rc * rc) | own)).any((1, 2))
    return ~ok | hit


def rollout(plans, pose, step, radius, outside, stop_at, lo, cell, opaque, field=None, extra=None):
    """(pose float64[P, 3], stats int64[P, 5], trace float64[T, P, 3]) of one env: plans [T, P]; pose (x, z, dir); step (fwd, drift, turn);
    stop_at -1: never; lo (min_x, min_z); opaque uint8[gz, gx]; field uint16[gz, gx] or None; extra uint8[gz, gx] or None"""
    import pyoracle
    (T, P), (gz, gx) = plans.shape, opaque.shape
    cell, rc = np.float64(cell), np.float64(radius) / np.float64(cell)
    fwd, drift, dturn = np.float64(step[0]), np.float64(step[1]), np.float64(step[2]) * (math.pi / 180.0)
    x, z, d = (np.full(P, v, np.float64) for v in pose)

    def look():
        at = cells_of(x, z, lo, cell, gx, gz)
        v = np.where(at >= 0, field.ravel()[np.maximum(at, 0)], NO_FIELD).astype(np.int64) if field is not None else np.full(P, NO_FIELD, np.int64)
        return v, np.where(at >= 0, extra.ravel()[np.maximum(at, 0)], 0).astype(np.int64) if extra is not None else np.zeros(P, np.int64)

    reach = look()[0]
    reach_step, steps, bumps, cost = (np.zeros(P, np.int64) for _ in range(4))
    active, trace = ~((stop_at >= 0) & (reach <= stop_at)), np.zeros((T, P, 3))
    with np.errstate(all="ignore"):
        for k in range(T):
            a = plans[k].astype(np.int64)
            d = np.where(active & (a == 0), d + dturn, np.where(active & (a == 1), d + -dturn, d))
            mv = np.flatnonzero(active & ((a == 2) | (a == 3)))
            if len(mv):
                sc = np.array([pyoracle.sincos(float(t)) if -1e6 < t < 1e6 else (np.nan, np.nan) for t in d[mv]]).reshape(-1, 2)
                f = np.where(a[mv] == 2, fwd, -fwd)
                nx, nz = x[mv] + sc[:, 1] * f + sc[:, 0] * drift, z[mv] + (-sc[:, 0]) * f + sc[:, 1] * drift
                no = blocked(nx, nz, lo, cell, rc, opaque, outside)
                bumps[mv[no]] += 1
                x[mv[~no]], z[mv[~no]] = nx[~no], nz[~no]
            v, xv = look()
            cost += np.where(active, xv, 0)
            better = active & (v < reach)
            reach, reach_step, steps = np.where(better, v, reach), np.where(better, k + 1, reach_step), np.where(active, k + 1, steps)
            active = active & ~((stop_at >= 0) & (reach <= stop_at))
            trace[k] = np.stack([x, z, d], 1)
    return np.stack([x, z, d], 1), np.stack([reach, reach_step, steps, bumps, cost], 1), trace


# ---- the cases both test files run
POSES = ("inside", "on_line", "corner", "outside", "nan", "far")
DENSITIES = (0.0, 0.03, 0.30, 1.0)
RADII = (0.0, 1.6, 1.0, 8.0)            # in cells


def pose_of(name, rng, gx, gz, lo, cell):
    """a start pose (x, z, dir): inside the grid, on a grid line, in a corner of a cell, outside the grid (one cell, heading in), with
    a NaN, and 2^30 cells away"""
    i, j, d = gx // 3, gz // 3, float(rng.uniform(-math.pi, math.pi))
    u, w = {"inside": (rng.uniform(0.2, 0.8) * gx, rng.uniform(0.2, 0.8) * gz), "on_line": (float(i), j + 0.375), "corner": (float(i), float(j)),
            "outside": (-0.6, 0.5 * gz), "nan": (math.nan, 0.5 * gz), "far": (2.0 ** 30, 0.5 * gz)}[name]
    return (lo[0] + u * cell, lo[1] + w * cell, 0.05 if name == "outside" else d)


def plans_of(rng, T, P):
    """actions 0 .. 7 [T, P]: half of them moves, mostly forward, three in ten turns, the rest what moves no pose"""
    return rng.choice(8, (T, P), p=[0.15, 0.15, 0.4, 0.1, 0.05, 0.05, 0.05, 0.05]).astype(np.int32)


def planes_of(rng, gz, gx, density):
    """(opaque, field, extra): `density` of the cells hold a random byte 1 .. 255; a field of which one cell in 50 is a source (0), one in
    10 holds a low cost; random extra costs"""
    opaque = (rng.integers(1, 256, (gz, gx)) * (rng.random((gz, gx)) < density)).astype(np.uint8)
    pick = rng.random((gz, gx))
    field = np.where(pick < 0.02, 0, np.where(pick < 0.12, rng.integers(1, 40, (gz, gx)), rng.integers(40, 0x10000, (gz, gx)))).astype(np.uint16)
    return opaque, field, rng.integers(0, 256, (gz, gx)).astype(np.uint8)
