"""Scan matching restated (include/mwengine.h, "scan matching"), the rule and nothing else: numpy float64, the end cells broadcast over
[K, R], a zero-padded plane indexed over [K, 2W+1, 2W+1, R], the best candidate by a lexicographic sort.  No lists, no packed key."""
import numpy as np

BOUND = 2.0 ** 30
ROT5 = [(1.0, 0.0), (np.cos(0.05), np.sin(0.05)), (np.cos(0.05), -np.sin(0.05)), (0.9, 0.3), (np.cos(0.4), np.sin(0.4))]       # (0.9, 0.3): no unit pair


def match(origin, t, d, rot, W, max_range, min_x, min_z, cell, plane):
    """(best (r, a, b), score, volume int64[K, 2W+1, 2W+1]) of one env: origin (x, z); t float64[R]; d float64[R, 2]; rot [K][2]; plane uint8[gz, gx]"""
    t, d, rot = np.asarray(t, np.float64), np.asarray(d, np.float64), np.asarray(rot, np.float64)
    gz, gx = plane.shape
    with np.errstate(all="ignore"):
        u0, w0 = np.float64(origin[0] - min_x) / cell, np.float64(origin[1] - min_z) / cell
        gu, gw = d[:, 0] / cell, d[:, 1] / cell
        c, s = rot[:, 0, None], rot[:, 1, None]
        ru, rw = c * gu + s * gw, c * gw - s * gu
        u1, w1 = u0 + t * ru, w0 + t * rw
        fits = lambda v: np.isfinite(v) & (np.abs(v) < BOUND)
        counts = (t >= 0.0) & (t < max_range) & fits(u0) & fits(w0) & fits(u1) & fits(w1)
        # a beam that does not count, or ends farther out than any shift reaches, lands on the padding: row -W - 1
        row = np.where(counts, np.clip(np.floor(w1), -W - 1, gz + W), -W - 1).astype(np.int64)
        col = np.where(counts, np.clip(np.floor(u1), -W - 1, gx + W), -W - 1).astype(np.int64)
    P = 2 * W + 1
    pad = np.zeros((gz + 2 * P, gx + 2 * P), np.int64)
    pad[P:P + gz, P:P + gx] = plane
    k = np.arange(-W, W + 1)
    volume = pad[row[:, None, None, :] + k[None, :, None, None] + P, col[:, None, None, :] + k[None, None, :, None] + P].sum(-1)
    r, b, a = (v.ravel() for v in np.meshgrid(np.arange(len(rot)), k, k, indexing="ij"))
    first = np.lexsort((a, b, r, a * a + b * b, -volume.ravel()))[0]
    return (int(r[first]), int(a[first]), int(b[first])), int(volume.ravel()[first]), volume


def plane_of(rng, gz, gx):
    """a likelihood plane: two thirds of the cells hold a random byte 1 .. 255"""
    return (rng.integers(1, 256, (gz, gx)) * (rng.random((gz, gx)) < 0.67)).astype(np.uint8)
