"""The yardstick of the explored-area tests (tests/test_seen_cpu.py, tests/test_gpu_seen.py): an independent restatement of
include/mwengine.h's rules for mw_seen_update — numpy in float64 in the documented order of operations, every cell of the grid at once
(no box around the agent), the line of sight through tests/ray_reference.py's `cast` with max_t = 1 and radius 0, the heading through
its `fan_directions` at offset 0 — that shares no code with miniworld_amd/csrc/mw_seen.h.  Worlds are the dicts of
tests/nav_reference.py.  Comparisons against it are exact."""
import math

import numpy as np

import ray_reference as ray


def grid_shape(extent, cell):
    return max(1, math.ceil((float(extent[1]) - float(extent[0])) / cell)), max(1, math.ceil((float(extent[3]) - float(extent[2])) / cell))


def cos_half_of(fov):
    return -1.0 if fov == 2 * math.pi else math.cos(fov / 2)


def covers(extent, cell, gx, gz):
    return bool(extent[0] + (float(gx) + 0.5) * cell > extent[1] and extent[2] + (float(gz) + 0.5) * cell > extent[3])


def visible(w, cell, gx, gz, pose, max_range, cos_half, entities):
    """pose = (x, z, dir) of the agent -> (bool[gz, gx]: the cells visible from it, the number of cells that passed tests 1 - 3)"""
    ext = np.asarray(w["extent"], np.float64)
    ox, oz = np.float64(pose[0]), np.float64(pose[1])
    cx = (ext[0] + (np.arange(gx, dtype=np.float64) + 0.5) * cell)[None, :].repeat(gz, 0)
    cz = (ext[2] + (np.arange(gz, dtype=np.float64) + 0.5) * cell)[:, None].repeat(gx, 1)
    with np.errstate(all="ignore"):
        inside = ~((cx > ext[1]) | (cz > ext[3]))
        vx, vz = cx - ox, cz - oz
        dist = np.sqrt(vx * vx + vz * vz)
        near = dist <= max_range
        hx, hz = ray.fan_directions(pose[2], [0.0])[0]
        cone = (dist == 0.0) | (vx * hx + vz * hz >= cos_half * dist)
        if cos_half == -1.0:
            cone = np.ones_like(cone)
        cand = inside & near & cone
    out = np.zeros((gz, gx), bool)
    if cand.any():
        d = np.stack([vx[cand], vz[cand]], axis=1)
        o = np.tile(np.array([[ox, oz]]), (len(d), 1))
        t, hit = ray.cast(w, o, d, 1.0, 0.0, entities)
        out[cand] = (t == 1.0) & (hit == -1)
    return out, int(cand.sum())


class Map:
    """one env's map: seen uint8[gz, gx], count, new"""

    def __init__(self, gx, gz, fill=0, count=0, new=0):
        self.seen = np.full((gz, gx), fill, np.uint8)
        self.count, self.new = int(count), int(new)


def update(m, w, cell, pose, max_range, cos_half, entities, clear=False, mask=True):
    """one call for one env; returns the number of candidates (cells that passed tests 1 - 3), or -1 for an env that was skipped or refused"""
    if not mask:
        return -1
    gz, gx = m.seen.shape
    if not covers(np.asarray(w["extent"], np.float64), cell, gx, gz):
        m.seen[:] = 0
        m.count = m.new = 0
        return -1
    if clear:
        m.seen[:] = 0
        m.count = 0
    vis, cands = visible(w, cell, gx, gz, pose, max_range, cos_half, entities)
    fresh = vis & (m.seen == 0)
    m.seen[fresh] = 1
    m.new = int(fresh.sum())
    m.count += m.new
    return cands
