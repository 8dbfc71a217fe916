"""The yardstick of the depth-projection tests (tests/test_depth_cpu.py, tests/test_gpu_depth.py): an independent restatement of
include/mwengine.h's rules for mw_depth_project — numpy in float64 over every pixel of a frame, every operation of the documented order
its own numpy call (nothing can be contracted), sines and cosines from pyoracle.sincos, the heading through tests/ray_reference.py's
`fan_directions` at offset 0 — that shares no code with miniworld_amd/csrc/mw_depth.h.  Comparisons against it are exact."""
import numpy as np

import pyoracle
import ray_reference as ray

F = np.float64
# sample 0 of the multisample pattern in 1/16 pixel, GL space (y up), by sample count — the header's table
SAMPLE0 = {8: (9, 5), 4: (6, 2), 1: (8, 8)}
SENSOR = dict(min_range=0.05, max_range=8.0, floor_tol=0.1, top=1.6)
DROPPED, FLOOR, OBSTACLE = 0, 1, 2


def subpixel(msaa):
    sx, sy = SAMPLE0[int(msaa)]
    return np.divide(F(sx), F(16.0)), np.subtract(F(1.0), np.divide(F(sy), F(16.0)))


def heading(direction):
    hx, hz = ray.fan_directions(direction, [0.0])[0]
    return F(hx), F(hz)


def unproject(depth, pose, cam, msaa, min_range, max_range, floor_tol, top):
    """depth float32[H, W(, 1)], pose (x, z, dir), cam (height, fwd_disp, pitch_deg, fov_deg) -> dict of float64[H, W] d, lat, yc, fwd, up,
    px, pz and cls uint8[H, W] (DROPPED, FLOOR, OBSTACLE)"""
    depth = np.asarray(depth, np.float32)
    depth = depth.reshape(depth.shape[0], depth.shape[1])
    H, W = depth.shape
    ox, oz = F(pose[0]), F(pose[1])
    hx, hz = heading(pose[2])
    rtx, rtz = np.negative(hz), hx
    height, fwd_disp, pitch_deg, fov_deg = (F(v) for v in cam)
    sp, cp = (F(v) for v in pyoracle.sincos(float(np.divide(np.multiply(pitch_deg, F(np.pi)), F(180.0)))))
    sh, ch = (F(v) for v in pyoracle.sincos(float(np.divide(np.multiply(np.multiply(fov_deg, F(0.5)), F(np.pi)), F(180.0)))))
    th = np.divide(sh, ch)
    aspect = np.divide(F(W), F(H))
    tx = np.multiply(th, aspect)
    sub_x, sub_y = subpixel(msaa)
    with np.errstate(all="ignore"):
        d = depth.astype(F)
        inside = (d >= F(min_range)) & (d <= F(max_range))
        u = np.arange(W, dtype=F)[None, :].repeat(H, 0)
        v = np.arange(H, dtype=F)[:, None].repeat(W, 1)
        xn = np.subtract(np.divide(np.multiply(np.add(u, sub_x), F(2.0)), F(W)), F(1.0))
        yn = np.subtract(F(1.0), np.divide(np.multiply(np.add(v, sub_y), F(2.0)), F(H)))
        lat = np.multiply(np.multiply(xn, tx), d)
        yc = np.multiply(np.multiply(yn, th), d)
        fwd = np.add(fwd_disp, np.subtract(np.multiply(d, cp), np.multiply(yc, sp)))
        up = np.add(height, np.add(np.multiply(d, sp), np.multiply(yc, cp)))
        px = np.add(ox, np.add(np.multiply(fwd, hx), np.multiply(lat, rtx)))
        pz = np.add(oz, np.add(np.multiply(fwd, hz), np.multiply(lat, rtz)))
        is_floor = inside & (up >= np.negative(F(floor_tol))) & (up <= F(floor_tol))
        is_obst = inside & (up > F(floor_tol)) & (up <= F(top))
    cls = np.where(is_floor, FLOOR, np.where(is_obst, OBSTACLE, DROPPED)).astype(np.uint8)
    return dict(d=d, lat=lat, yc=yc, fwd=fwd, up=up, px=px, pz=pz, cls=cls, ox=ox, oz=oz)


def _counts(rows, cols, kept, cls, n_rows, n_cols):
    """int64[2, n_rows, n_cols]: the floor and the obstacle points per cell"""
    out = np.zeros((2, n_rows, n_cols), np.int64)
    for k, which in enumerate((FLOOR, OBSTACLE)):
        m = kept & (cls == which)
        np.add.at(out[k], (rows[m].astype(np.int64), cols[m].astype(np.int64)), 1)
    return out


def window_counts(p, size, cell, back, north):
    S = F(size)
    half = np.multiply(S, F(0.5))
    with np.errstate(all="ignore"):
        a = np.subtract(p["px"], p["ox"]) if north else p["lat"]
        b = np.negative(np.subtract(p["pz"], p["oz"])) if north else p["fwd"]
        c = np.floor(np.add(np.divide(a, F(cell)), half))
        r = np.floor(np.subtract(np.add(half, F(back)), np.divide(b, F(cell))))
        kept = (c >= 0.0) & (c < S) & (r >= 0.0) & (r < S)
    return _counts(r, c, kept, p["cls"], int(size), int(size))


def window(depth, pose, cam, msaa, size, cell, back, north, min_range, max_range, floor_tol, top):
    """one window call for one env: uint8[2, S, S], floor points then obstacle points, clamped to 255"""
    p = unproject(depth, pose, cam, msaa, min_range, max_range, floor_tol, top)
    return np.minimum(window_counts(p, size, cell, back, north), 255).astype(np.uint8)


def map_counts(p, extent, cell, gx, gz):
    with np.errstate(all="ignore"):
        fi = np.floor(np.divide(np.subtract(p["px"], F(extent[0])), F(cell)))
        fj = np.floor(np.divide(np.subtract(p["pz"], F(extent[2])), F(cell)))
        kept = (fi >= 0.0) & (fi < F(gx)) & (fj >= 0.0) & (fj < F(gz))
    return _counts(fj, fi, kept, p["cls"], int(gz), int(gx))


def covers(extent, cell, gx, gz):
    cx = np.add(F(extent[0]), np.multiply(np.add(F(gx), F(0.5)), F(cell)))
    cz = np.add(F(extent[2]), np.multiply(np.add(F(gz), F(0.5)), F(cell)))
    return bool(cx > F(extent[1]) and cz > F(extent[3]))


class Map:
    """one env's accumulated map: map uint8[2, gz, gx], count and new int32[2]"""

    def __init__(self, gx, gz, garbage=0):
        self.map = np.full((2, gz, gx), garbage, np.uint8)
        self.count = np.frombuffer(bytes([garbage]) * 8, np.int32).copy()
        self.new = self.count.copy()


def map_update(m, depth, pose, cam, msaa, extent, cell, min_points, clear, min_range, max_range, floor_tol, top):
    """one map call for one env; False for an extent the grid does not cover"""
    _, gz, gx = m.map.shape
    if not covers(extent, cell, gx, gz):
        m.map[:] = 0
        m.count[:] = 0
        m.new[:] = 0
        return False
    if clear:
        m.map[:] = 0
        m.count[:] = 0
    hit = map_counts(unproject(depth, pose, cam, msaa, min_range, max_range, floor_tol, top), extent, cell, gx, gz) >= int(min_points)
    fresh = hit & (m.map == 0)
    m.map[fresh] = 1
    m.new[:] = fresh.reshape(2, -1).sum(1)
    with np.errstate(over="ignore"):
        m.count[:] = m.count + m.new
    return True


# ---- the geometry check: does an unprojected frame lie on the world the renderer drew? -------------------------------------------------
NEAR, FAR = 0.04, 100.0


def world_z(z16):
    """get_depth_map's conversion of a 16-bit depth value (opengl.py:426-431), in float64"""
    clip = (np.asarray(z16, np.float64) / 65535.0 - 0.5) * 2.0
    return -2.0 * FAR * NEAR / (clip * (FAR - NEAR) - (FAR + NEAR))


def solids_of_scene(scene):
    """what a neutral scene's frame can show: {"segs": [n, 4], "wall_h", "boxes": [(x, z, radius, height)]}"""
    return {"segs": np.asarray(scene["wall_segs"], np.float64).reshape(-1, 4),
            "wall_h": float(np.asarray(scene["polys_v"], np.float64).reshape(-1, 3)[:, 1].max()),
            "boxes": [(float(scene["ents_pos"][k][0]), float(scene["ents_pos"][k][2]), float(scene["ents_radius"][k]), float(scene["ents_height"][k]))
                      for k in range(len(scene["ents_kind"]))]}


def unclassified(depth, z16, pose, cam, msaa, solids, max_range=5.0):
    """The pixels within max_range that lie on nothing of the world: (their count, the pixels within range).  A pixel's point must lie
    on the floor, on the ceiling, on a collision segment or on a Box's padded circle, within its own tolerance: the true eye depth lies
    between the depths of z16 - 2 and z16 + 2 (one step of quantisation, one of the rasteriser's interpolation rounding); that interval,
    scaled along the pixel's ray, plus 1e-6."""
    H, W = depth.shape
    p = unproject(depth, pose, cam, msaa, NEAR, max_range, 0.0, 0.0)
    z = z16.astype(np.int64)
    lo, hi = world_z(np.maximum(z - 2, 0)), world_z(np.minimum(z + 2, 65535))
    d = p["d"]
    inside = (d >= NEAR) & (d <= max_range)
    assert ((d >= lo - 1e-6) & (d <= hi + 1e-6))[inside].all()          # the frame is the conversion of its own depth values
    with np.errstate(all="ignore"):
        ray_len = np.sqrt(1.0 + (p["lat"] / d) ** 2 + (p["yc"] / d) ** 2)
    tol = np.maximum(hi - d, d - lo) * ray_len + 1e-6
    up = p["up"]
    wall_h = solids["wall_h"]
    on_floor = np.abs(up) <= tol
    on_ceiling = np.abs(up - wall_h) <= tol
    dist = np.full(d.shape, np.inf)
    with np.errstate(all="ignore"):
        for s in solids["segs"]:
            dist = np.minimum(dist, ray._closest(s[0], s[1], s[2], s[3], p["px"], p["pz"]))
        on_wall = (dist <= tol) & (up >= -tol) & (up <= wall_h + tol)
        on_box = np.zeros(d.shape, bool)
        for ex, ez, radius, height in solids["boxes"]:
            r = np.sqrt((p["px"] - ex) ** 2 + (p["pz"] - ez) ** 2)
            on_box |= (r <= radius + tol) & (up >= -tol) & (up <= height + tol)
    return int((inside & ~(on_floor | on_ceiling | on_wall | on_box)).sum()), int(inside.sum())


def z16_of(depth):
    """the 16-bit depth value a depth map's element was converted from (the inverse of world_z, rounded: a step of z16 is far above
    float32's resolution within the ranges the tests use)"""
    d = np.asarray(depth, np.float64)
    clip = ((FAR + NEAR) - 2.0 * FAR * NEAR / d) / (FAR - NEAR)
    return np.clip(np.rint((clip / 2.0 + 0.5) * 65535.0), 0, 65535).astype(np.uint16)
