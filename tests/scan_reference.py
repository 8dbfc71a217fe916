"""Scan maps restated (include/mwengine.h, "scan maps"), the rule and nothing else: numpy float64, the closed form broadcast over
[beams, lines] and scattered through boolean masks.  No walk, no prefix, no bit planes; and the same cases for the CPU and GPU tests."""
import numpy as np

BOUND = 2.0 ** 30


def sets(origin, t, d, max_range, min_x, min_z, cell, gx, gz):
    """(free, obstacle) bool[gz, gx] of one env's call: origin (x, z); t float64[R]; d float64[R, 2]"""
    t, d = np.asarray(t, np.float64), np.asarray(d, np.float64)
    with np.errstate(all="ignore"):
        u0, w0 = np.float64(origin[0] - min_x) / cell, np.float64(origin[1] - min_z) / cell
        gu, gw = d[:, 0] / cell, d[:, 1] / cell
        hit = t < max_range
        e = np.where(hit, t, max_range)
        u1, w1 = u0 + e * gu, w0 + e * gw
        fits = lambda v: np.isfinite(v) & (np.abs(v) < BOUND)
        keep = (t >= 0.0) & fits(u0) & fits(w0) & fits(u1) & fits(w1)
        free, obstacle = np.zeros((gz, gx), bool), np.zeros((gz, gx), bool)

        def mark(plane, row, col, ok):
            ok = ok & (row >= 0.0) & (row < gz) & (col >= 0.0) & (col < gx)
            plane[row[ok].astype(np.int64), col[ok].astype(np.int64)] = True

        mark(free, np.full(t.shape, np.floor(w0)), np.full(t.shape, np.floor(u0)), keep)
        mark(obstacle, np.floor(w1), np.floor(u1), keep & hit)
        for a0, a1, g, b0, h, n, x_lines in ((u0, u1, gu, w0, gw, gx, True), (w0, w1, gw, u0, gu, gz, False)):
            L = np.arange(n + 1, dtype=np.float64)[None, :]
            g_, a1_ = g[:, None], a1[:, None]
            crossed = np.where(g_ > 0.0, (L >= np.floor(a0) + 1.0) & (L <= np.floor(a1_)), (g_ < 0.0) & (L >= np.floor(a1_) + 1.0) & (L <= np.floor(a0)))
            other = np.floor(b0 + (L - a0) / g_ * h[:, None])
            own = np.where(g_ > 0.0, L, L - 1.0)
            mark(free, *((other, own) if x_lines else (own, other)), crossed & keep[:, None])
    return free & ~obstacle, obstacle


def update(planes, count, free, obstacle, clear=False):
    """the map target: planes uint8[2, gz, gx] and count int64[2] in place; returns new int64[2]"""
    new = np.zeros(2, np.int64)
    if clear:
        planes[:], count[:] = 0, 0
    for k, s in enumerate((free, obstacle)):
        add = s & (planes[k] == 0)
        planes[k][add] = 1
        new[k] = add.sum()
    count += new
    return new


# ---- the cases both test files run: case(name, rng, R, gx, gz) -> (origin (x, z), t[R], d[R, 2], max_range) on a grid of `cell` metres per cell
# from `lo` = (min_x, min_z); lengths scale with the cell, so that a beam crosses as many cells on any grid
MIN, CELL = (-1.5, 2.25), 0.25
CASES = ("random", "axes", "diagonal_centre", "diagonal_corner", "on_line", "outside", "nonfinite")
GRIDS = [(103, 103), (128, 256), (4, 12), (1, 40), (40, 1)]        # (gz, gx)
BAD_T = [np.nan, np.inf, -np.inf, -1.0, -0.0]
BAD_D = [(np.nan, 1.0), (1.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (1e300, 1e300), (1e-320, 1.0), (0.0, 0.0)]


def case(name, rng, R, gx, gz, lo=MIN, cell=CELL):
    origin, t, d, max_range = _case(name, rng, R, gx * CELL, gz * CELL, gx // 3, gz // 3, np.arange(R))
    return (lo[0] + origin[0] * (cell / CELL), lo[1] + origin[1] * (cell / CELL)), t, d * (cell / CELL), max_range


def _case(name, rng, R, wx, wz, i, j, k):
    def fan(span, origin):      # all four quadrants, any length of direction; a third of the longer fans' beams pass max_range or leave the grid
        ang = rng.uniform(0, 2 * np.pi, R)
        return origin, rng.uniform(0, span, R), np.stack([np.cos(ang), -np.sin(ang)], 1) * rng.uniform(0.5, 2.0, R)[:, None], 6.0
    inside = (rng.uniform(0.2, 0.8) * wx, rng.uniform(0.2, 0.8) * wz)
    if name == "random":
        return fan(9.0, inside)
    if name == "axes":              # gu == 0 or gw == 0, either sign; by fours t = 0, t = max_range, t > max_range, then any
        t = np.where(k % 16 < 4, 0.0, np.where(k % 16 < 8, 3.0, np.where(k % 16 < 12, 3.5, rng.uniform(0, 3.0, R))))
        return inside, t, np.array([(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0)])[k % 4], 3.0
    if name == "on_line":           # the origin on a grid line
        return fan(5.0, (i * CELL, (j + 0.375) * CELL))
    if name.startswith("diagonal"):  # exact diagonals from a cell's centre / corner, whole and half steps
        off = 0.5 if name == "diagonal_centre" else 0.0
        d = np.array([(1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0)])[k % 4] * CELL
        return ((i + off) * CELL, (j + off) * CELL), np.floor(rng.uniform(0, 12, R)) * np.where(k % 8 < 4, 1.0, 0.5), d, 20.0
    if name == "outside":           # origins outside the grid, beams that cross it or miss it
        return fan(9.0, (-0.6, 0.5 * wz) if R % 2 else (0.3 * wx, wz + 1.1))
    origin, t, d, max_range = fan(5.0, inside)      # "nonfinite": NaN, inf, negative t; NaN, inf, huge, tiny, zero directions; plain beams between
    for b in range(0, R, 2):
        if (b // 2) % 2:
            t[b] = BAD_T[(b // 4) % len(BAD_T)]
        else:
            d[b] = BAD_D[(b // 4) % len(BAD_D)]
    return origin, t, d, max_range
