"""The yardstick of the grid-navigation-field tests (tests/test_nav_grid_cpu.py, tests/test_gpu_nav_grid.py): an independent restatement
of include/mwengine.h's rules for mw_nav_build_grid — numpy inflation by the documented stencil, a heapq Dijkstra with the corner rule
and an extra cost per cell — that shares no code with miniworld_amd/csrc/mw_nav.h or mw_nav_grid.h.  The constants and the query are
nav_reference's.

Every comparison against it is exact.  To keep that honest `field` asserts that no stencil distance of the case lies within EPS of
`inflate`, no cell centre within EPS of a point source's reach, and that no cost reaches 0xFFFE."""
import heapq
import math

import numpy as np

from nav_reference import BLOCKED, EPS, NEIGHBOURS, UNREACHED
from nav_reference import query as _query


def radius(cell, inflate):
    """R: the smallest integer with R * cell >= inflate"""
    r = 0
    while r * cell < inflate:
        r += 1
    return r


def stencil(cell, inflate):
    """the offsets (dj, di) != (0, 0) a raw obstacle cell blocks, and the smallest |distance - inflate| over |di|, |dj| <= R + 1"""
    r = radius(cell, inflate)
    offsets, slack = [], math.inf
    for dj in range(-r - 1, r + 2):
        for di in range(-r - 1, r + 2):
            if (dj, di) == (0, 0):
                continue
            d = math.sqrt(float(di * di + dj * dj)) * cell
            slack = min(slack, abs(d - inflate))
            if d < inflate:
                assert abs(dj) <= r and abs(di) <= r
                offsets.append((dj, di))
    return offsets, slack


def inflated(raw, offsets):
    """bool[gz, gx]: the raw cells and every cell at one of `offsets` from one; cells outside the grid hold no obstacle"""
    raw = np.asarray(raw) != 0
    gz, gx = raw.shape
    out = raw.copy()
    for j, i in zip(*np.nonzero(raw)):
        for dj, di in offsets:
            nj, ni = j + dj, i + di
            if 0 <= nj < gz and 0 <= ni < gx:
                out[nj, ni] = True
    return out


def dijkstra(blocked, sources, extra):
    """int64[gz, gx]: a source 0; any other cell its extra plus the cheapest admissible neighbour's cost + 5 / + 7; int64 max: unreached"""
    gz, gx = blocked.shape
    far = np.iinfo(np.int64).max
    cost = np.full((gz, gx), far, np.int64)
    heap = []
    for j, i in zip(*np.nonzero(sources)):
        cost[j, i] = 0
        heap.append((0, int(j), int(i)))
    heapq.heapify(heap)
    while heap:
        c, j, i = heapq.heappop(heap)
        if c > cost[j, i]:
            continue
        for dj, di in NEIGHBOURS:
            nj, ni = j + dj, i + di
            if not (0 <= nj < gz and 0 <= ni < gx) or blocked[nj, ni]:
                continue
            if dj and di and (blocked[j + dj, i] or blocked[j, i + di]):
                continue
            nc = c + (7 if dj and di else 5) + int(extra[nj, ni])
            if nc < cost[nj, ni]:
                cost[nj, ni] = nc
                heapq.heappush(heap, (nc, nj, ni))
    return cost


def point_sources(shape, cell, origin, point, reach):
    """bool[gz, gx]: the cells whose centre is closer than reach to point = (x, y, z), and the smallest |distance - reach|"""
    gz, gx = shape
    x = origin[0] + (np.arange(gx, dtype=np.float64) + 0.5) * cell
    z = origin[1] + (np.arange(gz, dtype=np.float64) + 0.5) * cell
    X, Z = np.meshgrid(x, z)
    dx, dz = float(point[0]) - X, float(point[2]) - Z
    d = np.sqrt(dx * dx + dz * dz)
    return d < reach, float(np.abs(d - reach).min())


def costs(blocked, sources, extra=None):
    """(uint16[gz, gx] or None where a cost reaches 0xFFFE, the largest cost): the field over a final occupancy"""
    extra = np.zeros(blocked.shape, np.int64) if extra is None else np.asarray(extra, np.int64)
    cost = dijkstra(blocked, (np.asarray(sources) != 0) & ~blocked, extra)
    reached = cost != np.iinfo(np.int64).max
    top = int(cost[reached].max()) if reached.any() else 0
    if top >= UNREACHED:
        return None, top
    out = np.where(reached, cost, UNREACHED)
    out[blocked] = BLOCKED
    return out.astype(np.uint16), top


def field(raw, cell, inflate, sources=None, extra=None, point=None, reach=None, origin=(0.0, 0.0)):
    """uint16[gz, gx] by the header's rules, with the assertions that keep an exact comparison honest"""
    offsets, slack = stencil(cell, inflate)
    assert slack > EPS, f"a stencil distance lies {slack:g} m from inflate: the exact comparison would hang on the last bits"
    blocked = inflated(raw, offsets)
    src = np.zeros(blocked.shape, bool) if sources is None else np.asarray(sources) != 0
    if point is not None:
        near, slack = point_sources(blocked.shape, cell, origin, point, reach)
        assert slack > EPS, f"a cell centre lies {slack:g} m from the reach"
        src = src | near
    out, top = costs(blocked, src, extra)
    assert out is not None, f"a cost reaches 0xFFFE: {top}"
    return out


def query(f, origin, cell, x, z):
    """(cost, next, wx, wz) on a grid field: nav_reference's query, the centre of the cell itself at cost 0"""
    gz, gx = f.shape
    ext = (origin[0], None, origin[1], None)
    c, n, wx, wz = _query(f, ext, cell, (None, None), x, z)
    if c == 0:
        wx, wz = float(origin[0] + (n % gx + 0.5) * cell), float(origin[1] + (n // gx + 0.5) * cell)
    return c, n, wx, wz
