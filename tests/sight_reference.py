"""The yardstick of the grid-sight tests (tests/test_sight_cpu.py, tests/test_gpu_sight.py): an independent restatement of
include/mwengine.h's rule for mw_grid_sight that shares no code with miniworld_amd/csrc/mw_sight.h.  There is no walk in it: for a
viewpoint A the occlusion predicate is evaluated, in numpy, for every opaque cell Q against every target B at once — a cell that is
not opaque hides nothing, so these are all the Q of every bounding box —, and the heading is ray_reference.fan_directions'.  Range
and cone are the header's float64 expressions in its order; numpy does not contract them.

Every comparison against it is exact: both sides evaluate the same IEEE operations on the same operands."""
import math

import numpy as np


def heading(ang):
    """(hx, hz) of an angle: the fan of mw_ray_cast at offset 0; NaN for a NaN or an angle beyond the deterministic sin / cos"""
    from ray_reference import fan_directions
    h = fan_directions(ang, [0.0])[0]
    return float(h[0]), float(h[1])


def cell_of(x, org, cell, n):
    """mw_nav_query's clamp of a coordinate to a cell index: floor((x - org) / cell) in 0 .. n - 1, a NaN is cell 0"""
    c = math.floor((x - org) / cell) if not math.isnan(x) else 0
    return int(min(max(c, 0), n - 1))


def visible(opaque, cell, ja, ia, max_range, cos_half=-1.0, h=(math.nan, math.nan), closed=True):
    """bool[gz, gx]: the cells B seen from A = (ja, ia).  closed=False: the open form of the occlusion test (the header says why not)"""
    opaque = np.asarray(opaque) != 0
    gz, gx = opaque.shape
    # the targets: every cell whose offset can be in range, two cells to spare
    r = int(min(max(gx, gz), math.floor(max_range / cell) + 2))
    j0, j1, i0, i1 = max(0, ja - r), min(gz - 1, ja + r), max(0, ia - r), min(gx - 1, ia + r)
    dz, dx = np.meshgrid(np.arange(j0, j1 + 1) - ja, np.arange(i0, i1 + 1) - ia, indexing="ij")
    vx, vz = dx.astype(np.float64) * cell, dz.astype(np.float64) * cell
    dist = np.sqrt(vx * vx + vz * vz)
    with np.errstate(invalid="ignore"):
        ok = dist <= max_range
        if cos_half != -1.0:
            ok &= (dist == 0.0) | (vx * h[0] + vz * h[1] >= cos_half * dist)
    s = np.abs(dx) + np.abs(dz)
    lo_j, hi_j, lo_i, hi_i = np.minimum(dz, 0), np.maximum(dz, 0), np.minimum(dx, 0), np.maximum(dx, 0)
    hidden = np.zeros(dx.shape, bool)
    for j, i in zip(*np.nonzero(opaque[j0:j1 + 1, i0:i1 + 1])):       # (a Q outside the targets' box is in no bounding box)
        qj, qi = int(j) + j0 - ja, int(i) + i0 - ia
        if (qj, qi) == (0, 0):
            continue
        d = 2 * np.abs(dx * qj - dz * qi)
        meets = d <= s if closed else d < s
        hidden |= meets & (lo_j <= qj) & (qj <= hi_j) & (lo_i <= qi) & (qi <= hi_i) & ~((dz == qj) & (dx == qi))
    out = np.zeros((gz, gx), bool)
    out[j0:j1 + 1, i0:i1 + 1] = ok & ~hidden
    # nothing beyond the box is in range
    assert (r + 1) * cell > max_range or r == max(gx, gz)
    return out


def sight(opaque, cell, cells, dirs, max_range, cos_half, weight=None, seen=None):
    """(gain int32[V], seen uint8[gz, gx]) of one env: `cells` flat indices (outside the grid: no viewpoint), `dirs` angles or None"""
    opaque = np.asarray(opaque)
    gz, gx = opaque.shape
    seen = np.zeros((gz, gx), np.uint8) if seen is None else np.array(seen, np.uint8)
    gain = np.zeros(len(cells), np.int32)
    for v, c in enumerate(cells):
        c = int(c)
        if not 0 <= c < gx * gz:
            continue
        h = heading(float(dirs[v])) if dirs is not None else (math.nan, math.nan)
        vis = visible(opaque, cell, c // gx, c % gx, max_range, cos_half, h)
        gain[v] = int(np.asarray(weight, np.int64)[vis].sum()) if weight is not None else int(vis.sum())
        seen[vis] = 1
    return gain, seen


def agent_cell(pose, extent, cell, gx, gz):
    """the flat cell of an agent at pose (x, z, dir) on the env's grid, or -1 for a NaN position"""
    x, z = float(pose[0]), float(pose[1])
    if math.isnan(x) or math.isnan(z):
        return -1
    return cell_of(z, float(extent[2]), cell, gz) * gx + cell_of(x, float(extent[0]), cell, gx)
