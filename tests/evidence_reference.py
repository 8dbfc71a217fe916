"""Scan evidence restated (include/mwengine.h, "scan evidence"), the rule and nothing else: numpy float64 for the beams, int64 for the
counts.  The (beam, cell) pairs come from the closed form broadcast over [beams, lines], as scan_reference.sets marks them; np.unique
drops a beam's second naming of a cell, np.bincount counts.  No walk, no prefix, no packed words, no look-up of the other axis' task."""
import numpy as np

BOUND = 2.0 ** 30


def counts(origin, t, d, max_range, min_x, min_z, cell, gx, gz):
    """(hits, passes) int64[gz * gx] of one env's call: origin (x, z); t float64[R]; d float64[R, 2]"""
    t, d = np.asarray(t, np.float64), np.asarray(d, np.float64)
    beams, cells = np.arange(len(t)), gx * gz
    with np.errstate(all="ignore"):
        u0, w0 = np.float64(origin[0] - min_x) / cell, np.float64(origin[1] - min_z) / cell
        gu, gw = d[:, 0] / cell, d[:, 1] / cell
        hit = t < max_range
        e = np.where(hit, t, max_range)
        u1, w1 = u0 + e * gu, w0 + e * gw
        fits = lambda v: np.isfinite(v) & (np.abs(v) < BOUND)       # noqa: E731
        keep = (t >= 0.0) & fits(u0) & fits(w0) & fits(u1) & fits(w1)

        def flat(row, col, ok):
            """(beam, cell) of the entries under `ok` that lie inside the grid: int64[k] each"""
            ok = ok & (row >= 0.0) & (row < gz) & (col >= 0.0) & (col < gx)
            b = np.broadcast_to(beams.reshape((-1,) + (1,) * (ok.ndim - 1)), ok.shape)
            return b[ok], (row[ok] * gx + col[ok]).astype(np.int64)

        found = [flat(np.full(t.shape, np.floor(w0)), np.full(t.shape, np.floor(u0)), keep)]
        for a0, a1, g, b0, h, n, x_lines in ((u0, u1, gu, w0, gw, gx, True), (w0, w1, gw, u0, gu, gz, False)):
            L = np.arange(n + 1, dtype=np.float64)[None, :]
            g_, a1_ = g[:, None], a1[:, None]
            crossed = np.where(g_ > 0.0, (L >= np.floor(a0) + 1.0) & (L <= np.floor(a1_)), (g_ < 0.0) & (L >= np.floor(a1_) + 1.0) & (L <= np.floor(a0)))
            other = np.floor(b0 + (L - a0) / g_ * h[:, None])
            own = np.broadcast_to(np.where(g_ > 0.0, L, L - 1.0), other.shape)
            found.append(flat(*((other, own) if x_lines else (own, other)), crossed & keep[:, None]))
        once = np.unique(np.concatenate([b * cells + c for b, c in found]))
        _, ends = flat(np.floor(w1), np.floor(u1), keep & hit)
    return np.bincount(ends, minlength=cells), np.bincount(once % cells, minlength=cells)


def update(ev, hits, passes, rule, clear=False):
    """the target: ev int8[gz, gx] in place; returns (map uint8[2, gz, gx], score uint8[gz, gx], count int64[2], changed int64[2])"""
    hit, miss, cap, lo, hi, free_at, occ_at = rule
    before = np.zeros(ev.shape, np.int64) if clear else ev.astype(np.int64)
    hits, passes = hits.reshape(ev.shape), passes.reshape(ev.shape)
    delta = np.where(hits > 0, hit * np.minimum(hits, cap), -miss * np.minimum(passes, cap))
    after = np.clip(before + delta, lo, hi)
    ev[:] = after
    planes = np.stack([after <= free_at, after >= occ_at])
    was = np.stack([before <= free_at, before >= occ_at])
    return planes.astype(np.uint8), np.maximum(after, 0).astype(np.uint8), planes.sum((1, 2)), (planes != was).sum((1, 2))
