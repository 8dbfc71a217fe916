"""Scan weighing and resampling restated (include/mwengine.h, "scan weighing and resampling"), the rules and nothing else: numpy float64
broadcast over [P, R] and numpy uint64.  No lists, no keys, no prefix scan by parts, no bisection of its own."""
import numpy as np

BOUND = 2.0 ** 30


def weigh(pose, t, d, max_range, min_x, min_z, cell, plane):
    """(score int64[P], inside int64[P], best (p, score)) of one env: pose float64[P, 4] (x, z, c, s); t float64[R]; d float64[R, 2]; plane uint8[gz, gx]"""
    pose, t, d = np.asarray(pose, np.float64), np.asarray(t, np.float64), np.asarray(d, np.float64)
    gz, gx = plane.shape
    with np.errstate(all="ignore"):
        gu, gw = d[:, 0] / cell, d[:, 1] / cell
        u0, w0 = ((pose[:, 0] - min_x) / cell)[:, None], ((pose[:, 1] - min_z) / cell)[:, None]
        c, s = pose[:, 2, None], pose[:, 3, None]
        ru, rw = c * gu + s * gw, c * gw - s * gu
        u1, w1 = u0 + t * ru, w0 + t * rw
        fits = lambda v: np.isfinite(v) & (np.abs(v) < BOUND)
        counts = (t >= 0.0) & (t < max_range) & fits(u0) & fits(w0) & fits(u1) & fits(w1)
        row, col = np.floor(w1), np.floor(u1)
        inside = counts & (row >= 0) & (row < gz) & (col >= 0) & (col < gx)
    bytes_ = plane.astype(np.int64)[np.where(inside, row, 0).astype(np.int64), np.where(inside, col, 0).astype(np.int64)]
    score = np.where(inside, bytes_, 0).sum(1)
    first = int(np.argmax(score))          # (the first of the highest)
    return score, inside.sum(1), (first, int(score[first]))


def resample(weight, offset):
    """ancestor int64[P] of one env: weight, P non-negative integers below 2^32; offset, an unsigned 64-bit integer"""
    C = np.cumsum(np.asarray(weight).astype(np.uint64))        # (at most 2^12 * 2^32: exact)
    P, S = len(C), int(C[-1])
    if S == 0:
        return np.arange(P)
    T = (np.arange(P, dtype=np.uint64) * np.uint64(S) + np.uint64(int(offset) % S)) // np.uint64(P)      # (below 2^56: exact)
    return np.searchsorted(C, T, side="right")         # (the least p with C_p > T_j)


# ---- the poses both test files weigh: P rows (x, z, c, s) on a grid of `cell` metres per cell from `lo` = (min_x, min_z)
def poses_of(rng, P, origin, gx, gz, lo, cell):
    """row 0 the scan's own origin unturned, the others anywhere from a fifth of the grid before it to a fifth behind it under any turn;
    row 3 with a (c, s) of no unit length, 5 at 2^30 cells, 7 and 9 with a NaN, 11 far outside float64's integers"""
    ang = rng.uniform(0, 2 * np.pi, P)
    pose = np.stack([lo[0] + rng.uniform(-0.2, 1.2, P) * gx * cell, lo[1] + rng.uniform(-0.2, 1.2, P) * gz * cell, np.cos(ang), np.sin(ang)], 1)
    pose[0] = (origin[0], origin[1], 1.0, 0.0)
    for k, cols, values in ((3, (2, 3), (0.9, 0.3)), (5, (0,), (lo[0] + 2.0 ** 30 * cell,)), (7, (0,), (np.nan,)), (9, (2,), (np.nan,)), (11, (0, 1), (-1e300, 1e300))):
        if k < P:
            pose[k, list(cols)] = values
    return pose
