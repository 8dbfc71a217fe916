"""Grid ray casts restated (include/mwengine.h, "grid ray casts"), the rule and nothing else: numpy float64, every candidate of every
ray as arrays over [rays, 1 + (gx + 1) + (gz + 1)], masked, and the least (s, flat index) by a lexicographic sort.  No walk, no key."""
import numpy as np

BOUND = 2.0 ** 30


def cast(origin, d, max_t, min_x, min_z, cell, opaque):
    """(t float64[R], hit int64[R]) of one env: origin float64[R, 2] (x, z); d float64[R, 2]; opaque uint8[gz, gx]"""
    origin, d = np.asarray(origin, np.float64).reshape(-1, 2), np.asarray(d, np.float64).reshape(-1, 2)
    gz, gx = opaque.shape
    with np.errstate(all="ignore"):
        u0, w0 = (origin[:, 0] - min_x) / cell, (origin[:, 1] - min_z) / cell
        gu, gw = d[:, 0] / cell, d[:, 1] / cell
        u1, w1 = u0 + max_t * gu, w0 + max_t * gw
        fits = lambda v: np.isfinite(v) & (np.abs(v) < BOUND)
        keep = fits(u0) & fits(w0) & fits(u1) & fits(w1)
        s, row, col, ok = [np.zeros((len(d), 1))], [np.floor(w0)[:, None]], [np.floor(u0)[:, None]], [keep[:, None]]
        for a0, a1, g, b0, h, n, x_lines in ((u0, u1, gu, w0, gw, gx, True), (w0, w1, gw, u0, gu, gz, False)):
            L = np.arange(n + 1, dtype=np.float64)[None, :]
            a0_, a1_, g_ = a0[:, None], a1[:, None], g[:, None]
            crossed = np.where(g_ > 0.0, (L >= np.floor(a0_) + 1.0) & (L <= np.floor(a1_)), (g_ < 0.0) & (L >= np.floor(a1_) + 1.0) & (L <= np.floor(a0_)))
            s_ = (L - a0_) / g_ + 0.0
            other, own = np.floor(b0[:, None] + s_ * h[:, None]), np.broadcast_to(np.where(g_ > 0.0, L, L - 1.0), s_.shape)
            s.append(s_), row.append(other if x_lines else own), col.append(own if x_lines else other), ok.append(crossed & keep[:, None])
        s, row, col, ok = (np.concatenate(v, 1) for v in (s, row, col, ok))
        ok = ok & (row >= 0.0) & (row < gz) & (col >= 0.0) & (col < gx)
        flat = np.where(ok, row * gx + col, 0).astype(np.int64)
        ok = ok & (opaque.ravel()[flat] != 0)
    t, hit = np.full(len(d), float(max_t)), np.full(len(d), -1, np.int64)
    for k in np.flatnonzero(ok.any(1)):
        c = np.flatnonzero(ok[k])
        c = c[np.lexsort((flat[k, c], s[k, c]))[0]]
        t[k], hit[k] = (s[k, c] if s[k, c] < max_t else max_t), flat[k, c]
    return t, hit


MAX_T, DENSITIES = 4.0, (0.03, 0.30, 0.0, 1.0)
CASES = ("random", "axes", "diagonal_centre", "diagonal_corner", "on_line", "outside", "nonfinite", "zero", "short")


def case(name, rng, R, gx, gz, lo, cell):
    """(origin[R, 2], d[R, 2]) for max_t = MAX_T: scan_reference's fans, stretched so that MAX_T spans the fan's own range, the random
    one from an origin per ray; "zero": zero directions, in opaque and in free cells; "short": rays that end inside their first cell"""
    import scan_reference as scan
    if name in scan.CASES:
        origin, _, d, span = scan.case(name, rng, R, gx, gz, lo, cell)
        origin = np.tile(np.array(origin), (R, 1)) + (name == "random") * rng.uniform(-1.0, 1.0, (R, 2)) * cell
        return origin, d * (span / MAX_T)
    origin, ang = np.array(lo) + rng.uniform(0.0, 1.0, (R, 2)) * (gx * cell, gz * cell), rng.uniform(0, 2 * np.pi, R)
    length = 0.0 if name == "zero" else rng.uniform(0.01, 0.6, R)[:, None] * cell / MAX_T
    return origin, np.stack([np.cos(ang), -np.sin(ang)], 1) * length


def opaque_of(rng, gz, gx, density):
    """an opaque plane: `density` of the cells hold a random byte 1 .. 255"""
    return (rng.integers(1, 256, (gz, gx)) * (rng.random((gz, gx)) < density)).astype(np.uint8)
