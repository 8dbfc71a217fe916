"""Grid clearance restated (include/mwengine.h), the definition and nothing else: per cell the minimum over ALL marked cells of the squared
distance, int64, chunked numpy broadcasting, the lowest index among the minimisers, then limit and bands.  No column / row decomposition."""
import numpy as np

NONE, FAR = 0x7FFFFFFF, 0x7FFFFFFE

def transform(marked):
    """(dist2, nearest) int64[gz * gx] of one env's `marked` [gz, gx], no limit"""
    gz, gx = marked.shape
    dist2, nearest = np.full(gz * gx, NONE, np.int64), np.full(gz * gx, -1, np.int64)
    m = np.flatnonzero(np.asarray(marked).ravel())          # ascending: argmin's first minimiser is the lowest index
    if m.size:
        mj, mi = m // gx, m % gx
        for a in range(0, gz * gx, 1024):
            c = np.arange(a, min(a + 1024, gz * gx))
            d = (c[:, None] // gx - mj[None, :]) ** 2 + (c[:, None] % gx - mi[None, :]) ** 2
            k = d.argmin(axis=1)
            dist2[c], nearest[c] = d[np.arange(c.size), k], m[k]
    return dist2, nearest

def clearance(marked, limit=0, bands=(), exact=None):
    """(dist2 int32[gz, gx], nearest int32[gz, gx], cost uint8[gz, gx]) of one env's `marked` [gz, gx]; bands: (thr, cost) pairs;
    exact: transform(marked), where the caller has it"""
    dist2, nearest = (a.copy() for a in (exact or transform(marked)))
    if limit > 0 and marked.any():
        far = dist2 > limit * limit
        dist2[far], nearest[far] = FAR, -1
    cost = np.zeros(dist2.size, np.uint8)
    for thr, value in reversed(list(bands)):
        cost[dist2 <= thr] = value
    return dist2.astype(np.int32).reshape(marked.shape), nearest.astype(np.int32).reshape(marked.shape), cost.reshape(marked.shape)
