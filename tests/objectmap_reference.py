"""The yardstick of the object-map tests (tests/test_labelmap_cpu.py, tests/test_gpu_labelmap.py): an independent restatement of
include/mwengine.h's rules for mw_label_project — numpy in float64 over every pixel of a frame, every operation of the documented order
its own numpy call (nothing can be contracted), sines and cosines from pyoracle.sincos — that shares no code with
miniworld_amd/csrc/mw_labelmap.h or mw_depth.h, nor with the other restatements.  Comparisons against it are exact; a position is
compared through its bits, so that a NaN equals a NaN."""
import numpy as np

import pyoracle

F = np.float64
RAY_ENT = 0x10000
UNSEEN, NONE = 0xFFFF, 0xFFFE
# sample 0 of the multisample pattern in 1/16 pixel, GL space (y up), by sample count — the header's table
SAMPLE0 = {8: (9, 5), 4: (6, 2), 1: (8, 8)}
SENSOR = dict(min_range=0.05, max_range=8.0, floor_tol=0.1, top=1.6)


def _sincos(x):
    s, c = pyoracle.sincos(float(x))
    return F(s), F(c)


def points(depth, pose, cam, msaa, min_range, max_range, floor_tol, top):
    """depth float32[H, W(, 1)], pose (x, z, dir), cam (height, fwd_disp, pitch_deg, fov_deg) -> dict of float64[H, W] lat, fwd, px, pz,
    the origin ox, oz, and counts bool[H, W]: the pixels mw_depth_project classes as floor or as obstacle"""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape[0], depth.shape[1]
    depth = depth.reshape(H, W)
    ox, oz = F(pose[0]), F(pose[1])
    hx = hz = F(np.nan)
    if -1e6 < float(pose[2]) < 1e6:
        s, c = _sincos(pose[2])
        hx, hz = c, np.negative(s)
    rtx, rtz = np.negative(hz), hx
    height, fwd_disp, pitch_deg, fov_deg = (F(v) for v in cam)
    sp, cp = _sincos(np.divide(np.multiply(pitch_deg, F(np.pi)), F(180.0)))
    sh, ch = _sincos(np.divide(np.multiply(np.multiply(fov_deg, F(0.5)), F(np.pi)), F(180.0)))
    th = np.divide(sh, ch)
    tx = np.multiply(th, np.divide(F(W), F(H)))
    sx, sy = SAMPLE0[int(msaa)]
    sub_x, sub_y = np.divide(F(sx), F(16.0)), np.subtract(F(1.0), np.divide(F(sy), F(16.0)))
    with np.errstate(all="ignore"):
        d = depth.astype(F)
        in_range = (d >= F(min_range)) & (d <= F(max_range))
        u, v = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
        xn = np.subtract(np.divide(np.multiply(np.add(u, sub_x), F(2.0)), F(W)), F(1.0))
        yn = np.subtract(F(1.0), np.divide(np.multiply(np.add(v, sub_y), F(2.0)), F(H)))
        lat = np.multiply(np.multiply(xn, tx), d)
        yc = np.multiply(np.multiply(yn, th), d)
        fwd = np.add(fwd_disp, np.subtract(np.multiply(d, cp), np.multiply(yc, sp)))
        up = np.add(height, np.add(np.multiply(d, sp), np.multiply(yc, cp)))
        px = np.add(ox, np.add(np.multiply(fwd, hx), np.multiply(lat, rtx)))
        pz = np.add(oz, np.add(np.multiply(fwd, hz), np.multiply(lat, rtz)))
        floor = (up >= np.negative(F(floor_tol))) & (up <= F(floor_tol))
        obstacle = (up > F(floor_tol)) & (up <= F(top))
    return dict(lat=lat, fwd=fwd, px=px, pz=pz, ox=ox, oz=oz, counts=in_range & (floor | obstacle))


def keys_of(code, base):
    """uint32[...]: the id where code >= base and code - base <= 254 (in 64 bits: nothing overflows), else NONE"""
    c = np.asarray(code, np.int64)
    ident = c - int(base)
    return np.where((c >= int(base)) & (ident <= 254), ident, NONE).astype(np.uint32)


def _lowest(rows, cols, kept, keys, n_rows, n_cols):
    out = np.full((n_rows, n_cols), UNSEEN, np.uint32)
    np.minimum.at(out, (rows[kept].astype(np.int64), cols[kept].astype(np.int64)), keys[kept])
    return out


def _bytes(keys):
    return np.where(keys <= 254, keys + 1, 0).astype(np.uint8)


def window_keys(p, keys, size, cell, back, north):
    S = F(size)
    half = np.multiply(S, F(0.5))
    with np.errstate(all="ignore"):
        a = np.subtract(p["px"], p["ox"]) if north else p["lat"]
        b = np.negative(np.subtract(p["pz"], p["oz"])) if north else p["fwd"]
        c = np.floor(np.add(np.divide(a, F(cell)), half))
        r = np.floor(np.subtract(np.add(half, F(back)), np.divide(b, F(cell))))
        kept = p["counts"] & (c >= 0.0) & (c < S) & (r >= 0.0) & (r < S)
    return _lowest(r, c, kept, keys, int(size), int(size))


def window(depth, code, base, pose, cam, msaa, size, cell, back, north, min_range, max_range, floor_tol, top):
    """one window call for one env: uint8[S, S], 1 + the lowest id of the cell's pixels, 0 for none"""
    p = points(depth, pose, cam, msaa, min_range, max_range, floor_tol, top)
    return _bytes(window_keys(p, keys_of(code, base), size, cell, back, north))


def map_keys(p, keys, extent, cell, gx, gz):
    with np.errstate(all="ignore"):
        fi = np.floor(np.divide(np.subtract(p["px"], F(extent[0])), F(cell)))
        fj = np.floor(np.divide(np.subtract(p["pz"], F(extent[2])), F(cell)))
        kept = p["counts"] & (fi >= 0.0) & (fi < F(gx)) & (fj >= 0.0) & (fj < F(gz))
    return _lowest(fj, fi, kept, keys, int(gz), int(gx))


def covers(extent, cell, gx, gz):
    cx = np.add(F(extent[0]), np.multiply(np.add(F(gx), F(0.5)), F(cell)))
    cz = np.add(F(extent[2]), np.multiply(np.add(F(gz), F(0.5)), F(cell)))
    return bool(cx > F(extent[1]) and cz > F(extent[3]))


class Map:
    """one env's object map: map uint8[gz, gx], cells int32[K], pos float64[K, 3]; every byte `garbage` before the first call"""

    def __init__(self, gx, gz, ids, garbage=0):
        self.map = np.full((gz, gx), garbage, np.uint8)
        self.cells = np.frombuffer(bytes([garbage]) * (4 * ids), np.int32).copy()
        self.pos = np.frombuffer(bytes([garbage]) * (24 * ids), np.float64).copy().reshape(ids, 3)

    def copy(self):
        m = Map(1, 1, 0)
        m.map, m.cells, m.pos = self.map.copy(), self.cells.copy(), self.pos.copy()
        return m


def objects(m, extent, cell):
    """cells and pos of every id below K over the whole map"""
    for q in range(len(m.cells)):
        jj, ii = np.nonzero(m.map == q + 1)
        n = len(ii)
        m.cells[q] = n
        if n == 0:
            m.pos[q] = np.nan
            continue
        si, sj = int(ii.astype(np.int64).sum()), int(jj.astype(np.int64).sum())
        m.pos[q, 0] = np.add(F(extent[0]), np.multiply(np.add(np.divide(F(si), F(n)), F(0.5)), F(cell)))
        m.pos[q, 1] = 0.0
        m.pos[q, 2] = np.add(F(extent[2]), np.multiply(np.add(np.divide(F(sj), F(n)), F(0.5)), F(cell)))


def map_update(m, depth, code, base, pose, cam, msaa, extent, cell, clear, min_range, max_range, floor_tol, top):
    """one map call for one env; False for an extent the grid does not cover"""
    gz, gx = m.map.shape
    if not covers(extent, cell, gx, gz):
        m.map[:] = 0
        m.cells[:] = 0
        m.pos[:] = np.nan
        return False
    keys = map_keys(points(depth, pose, cam, msaa, min_range, max_range, floor_tol, top), keys_of(code, base), extent, cell, gx, gz)
    rewrite = np.ones(keys.shape, bool) if clear else keys != UNSEEN
    m.map[rewrite] = _bytes(keys)[rewrite]
    objects(m, extent, cell)
    return True


def same_bits(a, b):
    """float64 arrays equal bit for bit"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
