"""The yardstick of the label-frame tests (tests/test_label_cpu.py, tests/test_gpu_label.py): an independent restatement of
include/mwengine.h's rules for mw_label_frame — numpy in float64, every operation of the documented order its own numpy call (nothing can
be contracted), sines and cosines from pyoracle.sincos, the heading through tests/ray_reference.py's `fan_directions` — that shares no code
with miniworld_amd/csrc/mw_label.h.  It is brute force: every polygon, every slot and every triangle of a mesh slot against every pixel,
with no projection and no rectangle.  (`select="sphere"` skips, per mesh slot, the pixels whose ray passes the slot's own bounding sphere
— centre and radius from its transformed vertices, grown by a hundredth — at more than its radius: such a ray meets none of its
triangles.  `select="all"` skips nothing; tests/test_label_cpu.py compares the two.)  Comparisons against it are exact."""
import numpy as np

import pyoracle
import ray_reference as ray
from depth_reference import subpixel

F = np.float64
NOTHING, FLOOR, CEILING, WALL, FRAME, BOX, MESH = range(7)
POLY_ENTITY, POLY_XF, POLY_QUAD = 0x100, 0x200, 0x400
ENT_BOX, ENT_MESH = 1, 2
RAY_ENT = 0x10000
NEAR, FAR = 0.04, 100.0
mul, add, sub, div = np.multiply, np.add, np.subtract, np.divide


def _sincos(x):
    x = float(x)
    if not -1e6 < x < 1e6:
        return F(np.nan), F(np.nan)
    s, c = pyoracle.sincos(x)
    return F(s), F(c)


def camera(pose, cam, msaa, W, H):
    """pose (x, y, z, dir), cam (height, fwd_disp, pitch_deg, fov_deg) -> the eye and the axes"""
    ox, oy, oz = F(pose[0]), F(pose[1]), F(pose[2])
    hx, hz = (F(v) for v in ray.fan_directions(pose[3], [0.0])[0])
    height, fwd_disp, pitch_deg, fov_deg = (F(v) for v in cam)
    sp, cp = _sincos(div(mul(pitch_deg, F(np.pi)), F(180.0)))
    sh, ch = _sincos(div(mul(mul(fov_deg, F(0.5)), F(np.pi)), F(180.0)))
    th = div(sh, ch)
    tx = mul(th, div(F(W), F(H)))
    sub_x, sub_y = subpixel(msaa)
    return dict(ex=add(ox, mul(fwd_disp, hx)), ey=add(oy, height), ez=add(oz, mul(fwd_disp, hz)), fx=hx, fz=hz, rx=np.negative(hz), rz=hx, sp=sp, cp=cp, th=th,
                tx=tx, sub_x=sub_x, sub_y=sub_y, W=W, H=H)


def rays(c):
    """dx, dy, dz float64[H, W] and the pixels whose ray is no ray"""
    W, H = c["W"], c["H"]
    u = np.arange(W, dtype=F)[None, :].repeat(H, 0)
    v = np.arange(H, dtype=F)[:, None].repeat(W, 1)
    xn = sub(div(mul(add(u, c["sub_x"]), F(2.0)), F(W)), F(1.0))
    yn = sub(F(1.0), div(mul(add(v, c["sub_y"]), F(2.0)), F(H)))
    lat, yt = mul(xn, c["tx"]), mul(yn, c["th"])
    up = add(c["sp"], mul(yt, c["cp"]))
    fwd = sub(c["cp"], mul(yt, c["sp"]))
    dx = add(mul(fwd, c["fx"]), mul(lat, c["rx"]))
    dz = add(mul(fwd, c["fz"]), mul(lat, c["rz"]))
    bad = np.isnan(dx) | np.isnan(up) | np.isnan(dz) | np.isnan(c["ex"]) | np.isnan(c["ey"]) | np.isnan(c["ez"])
    return dx, up, dz, bad


def planes(V, c):
    """V float64[..., nv, 3] -> n [..., 3], k [...], m [..., nv, 3], mc [..., nv]"""
    nv = V.shape[-2]
    a, b = sub(V[..., 1, :], V[..., 0, :]), sub(V[..., 2, :], V[..., 0, :])
    nx = sub(mul(a[..., 1], b[..., 2]), mul(a[..., 2], b[..., 1]))
    ny = sub(mul(a[..., 2], b[..., 0]), mul(a[..., 0], b[..., 2]))
    nz = sub(mul(a[..., 0], b[..., 1]), mul(a[..., 1], b[..., 0]))
    k = add(add(mul(nx, sub(V[..., 0, 0], c["ex"])), mul(ny, sub(V[..., 0, 1], c["ey"]))), mul(nz, sub(V[..., 0, 2], c["ez"])))
    m, mc = [], []
    for i in range(nv):
        j = (i + 1) % nv
        e = sub(V[..., j, :], V[..., i, :])
        mx = sub(mul(ny, e[..., 2]), mul(nz, e[..., 1]))
        my = sub(mul(nz, e[..., 0]), mul(nx, e[..., 2]))
        mz = sub(mul(nx, e[..., 1]), mul(ny, e[..., 0]))
        m.append((mx, my, mz))
        mc.append(add(add(mul(mx, V[..., i, 0]), mul(my, V[..., i, 1])), mul(mz, V[..., i, 2])))
    return (nx, ny, nz), k, m, mc


def plane_hits(pl, c, d, cull, near, far):
    """the t of the plane hits that lie inside and within near .. far, +inf elsewhere; pl's arrays broadcast against d's"""
    (nx, ny, nz), k, m, mc = pl
    dx, dy, dz = d
    with np.errstate(all="ignore"):
        den = add(add(mul(nx, dx), mul(ny, dy)), mul(nz, dz))
        ok = (den < 0.0) if cull else ((den < 0.0) | (den > 0.0))
        t = div(k, den)
        ok = ok & (t >= F(near)) & (t <= F(far))
        px, py, pz = add(c["ex"], mul(t, dx)), add(c["ey"], mul(t, dy)), add(c["ez"], mul(t, dz))
        for (mx, my, mz), c0 in zip(m, mc):
            ok = ok & (sub(add(add(mul(mx, px), mul(my, py)), mul(mz, pz)), c0) >= 0.0)
        return np.where(ok, add(t, F(0.0)), np.inf)


def poly_vertices(scene, i):
    nv = int(scene["polys_nv"][i])
    n = 3 if (nv & 0xFF) == 3 else 4
    V = np.asarray(scene["polys_v"][i], np.float32)[:n].astype(F)
    if nv & POLY_XF:
        xf = np.asarray(scene["polys_xf"][i], np.float32).astype(F)
        s, co = _sincos(div(mul(xf[3], F(np.pi)), F(180.0)))
        x, y, z = V[:, 0].copy(), V[:, 1].copy(), V[:, 2].copy()
        V = np.stack([add(add(mul(co, x), mul(s, z)), xf[0]), add(y, xf[1]), add(sub(mul(co, z), mul(s, x)), xf[2])], -1)
    return V


def poly_class(scene, i):
    nv = int(scene["polys_nv"][i])
    if nv & POLY_ENTITY:
        return FRAME
    if nv & POLY_QUAD:
        return WALL
    V = np.asarray(scene["polys_v"][i], np.float32).astype(F)
    a, b = sub(V[1], V[0]), sub(V[2], V[0])
    return FLOOR if sub(mul(a[2], b[0]), mul(a[0], b[2])) > 0.0 else CEILING


def _axis(o, l, lo, hi, enter, leave, ok):
    with np.errstate(all="ignore"):
        zero = l == 0.0
        t1, t2 = div(sub(lo, o), l), div(sub(hi, o), l)
        first = t1 < t2
        tn, tf = np.where(first, t1, t2), np.where(first, t2, t1)
        good = np.where(zero, (o >= lo) & (o <= hi), tn <= tf)
        live = ok & good & ~zero
        enter = np.where(live & (tn > enter), tn, enter)
        leave = np.where(live & (tf < leave), tf, leave)
    return enter, leave, ok & good


def box_hits(c, d, pos, direction, size):
    dx, dy, dz = d
    s, co = _sincos(direction)
    qx, qy, qz = sub(c["ex"], F(pos[0])), sub(c["ey"], F(pos[1])), sub(c["ez"], F(pos[2]))
    ox, oz = sub(mul(co, qx), mul(s, qz)), add(mul(s, qx), mul(co, qz))
    lx, lz = sub(mul(co, dx), mul(s, dz)), add(mul(s, dx), mul(co, dz))
    hx, hy, hz = div(F(size[0]), F(2.0)), F(size[1]), div(F(size[2]), F(2.0))
    enter, leave, ok = np.full(dx.shape, -np.inf), np.full(dx.shape, np.inf), np.ones(dx.shape, bool)
    enter, leave, ok = _axis(np.broadcast_to(ox, dx.shape), lx, np.negative(hx), hx, enter, leave, ok)
    enter, leave, ok = _axis(np.broadcast_to(qy, dx.shape), dy, F(0.0), hy, enter, leave, ok)
    enter, leave, ok = _axis(np.broadcast_to(oz, dx.shape), lz, np.negative(hz), hz, enter, leave, ok)
    return np.where(ok & (enter <= leave), enter, -1.0)


def cylinder_hits(c, d, pos, radius, height):
    dx, dy, dz = d
    wx, wy, wz = sub(c["ex"], F(pos[0])), sub(c["ey"], F(pos[1])), sub(c["ez"], F(pos[2]))
    with np.errstate(all="ignore"):
        A = add(mul(dx, dx), mul(dz, dz))
        B = add(mul(wx, dx), mul(wz, dz))
        C = sub(add(mul(wx, wx), mul(wz, wz)), mul(F(radius), F(radius)))
        disc = sub(mul(B, B), mul(A, C))
        q = np.sqrt(disc)
        tn, tf = div(sub(np.negative(B), q), A), div(add(np.negative(B), q), A)
        zero = A == 0.0
        ok = np.where(zero, np.broadcast_to(C <= 0.0, dx.shape), (disc >= 0.0) & (tn <= tf))
        enter, leave = np.where(zero | ~ok, -np.inf, tn), np.where(zero | ~ok, np.inf, tf)
    enter, leave, ok = _axis(np.broadcast_to(wy, dx.shape), dy, F(0.0), F(height), enter, leave, ok)
    return np.where(ok & (enter <= leave), enter, -1.0)


def mesh_world(verts, pos, direction, scale):
    """verts float32[T, 3, 3] -> float64[T, 3, 3] in the world"""
    s, co = _sincos(direction)
    v = np.asarray(verts, np.float32).astype(F)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    rx, rz = add(mul(co, x), mul(s, z)), sub(mul(co, z), mul(s, x))
    sc = F(scale)
    return np.stack([add(F(pos[0]), mul(sc, rx)), add(F(pos[1]), mul(sc, y)), add(F(pos[2]), mul(sc, rz))], -1)


def mesh_hits(c, d, bad, Vw, near, far, select):
    """float64[H, W]: the smallest t of the slot's triangles per pixel, +inf for none"""
    dx, dy, dz = d
    out = np.full(dx.shape, np.inf)
    pick = ~bad
    if select == "sphere" and np.isfinite(Vw).all():
        pts = Vw.reshape(-1, 3)
        centre = (pts.min(0) + pts.max(0)) / 2
        r = np.sqrt(((pts - centre) ** 2).sum(1).max()) * 1.01 + 1e-6
        w = centre - np.array([c["ex"], c["ey"], c["ez"]])
        dd = dx * dx + dy * dy + dz * dz
        along = (w[0] * dx + w[1] * dy + w[2] * dz) / dd
        off2 = (w[0] - along * dx) ** 2 + (w[1] - along * dy) ** 2 + (w[2] - along * dz) ** 2
        pick = pick & ~(off2 > r * r)
    idx = np.argwhere(pick)
    if not len(idx) or not len(Vw):
        return out
    pl = planes(Vw, c)
    col = lambda a: a[:, None]
    pl = (tuple(col(a) for a in pl[0]), col(pl[1]), [tuple(col(a) for a in m) for m in pl[2]], [col(a) for a in pl[3]])
    for j in range(0, len(idx), 512):
        rows, cols = idx[j:j + 512, 0], idx[j:j + 512, 1]
        dj = (dx[rows, cols][None, :], dy[rows, cols][None, :], dz[rows, cols][None, :])
        out[rows, cols] = plane_hits(pl, c, dj, True, near, far).min(0)
    return out


def label_frame(scene, W, H, msaa, meshes=None, mode="exact", near=NEAR, far=FAR, select="sphere", pose=None, cam=None):
    """The label frame of a neutral scene (miniworld_amd.scene.scene_from_env's keys): dict(cls uint8[H, W], code int32[H, W], depth
    float32[H, W], t float64[H, W] (+inf for nothing), ent_pixels int32[E], ent_box int32[E, 4]).  meshes: name -> {"verts": float32[T, 3,
    3]} for scene["mesh_names"]; pose (x, y, z, dir) and cam (height, fwd_disp, pitch_deg, fov_deg) replace the scene's own."""
    if pose is None:
        p = np.asarray(scene["agent_pos"], F)
        pose = (p[0], p[1], p[2], float(scene["agent_dir"]))
    if cam is None:
        cam = tuple(float(scene[k]) for k in ("cam_height", "cam_fwd_disp", "cam_pitch", "cam_fov_y"))
    c = camera(pose, cam, msaa, W, H)
    dx, dy, dz, bad = rays(c)
    d = (dx, dy, dz)
    best = np.full((H, W), np.inf)
    code = np.full((H, W), -1, np.int32)
    cls = np.zeros((H, W), np.uint8)

    def take(t, this_code, this_cls):
        nonlocal best, code, cls
        with np.errstate(all="ignore"):
            m = ~bad & (F(near) <= t) & (t <= F(far)) & (t < best)
        best = np.where(m, add(t, F(0.0)), best)
        code = np.where(m, np.int32(this_code), code)
        cls = np.where(m, np.uint8(this_cls), cls)

    for i in range(len(scene["polys_nv"])):
        take(plane_hits(planes(poly_vertices(scene, i), c), c, d, False, near, far), i, poly_class(scene, i))
    kinds = [int(k) for k in scene["ents_kind"]]
    for s, kind in enumerate(kinds):
        if kind == ENT_BOX:
            take(box_hits(c, d, scene["ents_pos"][s], scene["ents_dir"][s], scene["ents_size"][s]), RAY_ENT + s, BOX)
    names = [str(n) for n in scene.get("mesh_names", [])]
    for s, kind in enumerate(kinds):
        if kind != ENT_MESH:
            continue
        if mode == "bounds":
            take(cylinder_hits(c, d, scene["ents_pos"][s], scene["ents_radius"][s], scene["ents_height"][s]), RAY_ENT + s, MESH)
            continue
        mid = int(scene["ents_mesh"][s])
        if meshes is None or not 0 <= mid < len(names) or names[mid] not in meshes:
            continue
        Vw = mesh_world(meshes[names[mid]]["verts"], scene["ents_pos"][s], scene["ents_dir"][s], scene["ents_scale"][s])
        take(mesh_hits(c, d, bad, Vw, near, far, select), RAY_ENT + s, MESH)
    E = len(kinds)
    ent_pixels, ent_box = np.zeros(E, np.int32), np.tile(np.array([W, H, -1, -1], np.int32), (E, 1))
    for s in range(E):
        vs, us = np.nonzero(code == RAY_ENT + s)
        ent_pixels[s] = len(vs)
        if len(vs):
            ent_box[s] = (us.min(), vs.min(), us.max(), vs.max())
    depth = np.where(code < 0, np.float32(F(far)), best.astype(np.float32)).astype(np.float32)
    return dict(cls=cls, code=code, depth=depth, t=best, ent_pixels=ent_pixels, ent_box=ent_box)


# ---- the renderer's own depth as the check of the labels ---------------------------------------------------------------------------

def interior(code):
    """the pixels whose four neighbours carry their code (a frame's border pixels have fewer neighbours: those they have)"""
    m = np.ones(code.shape, bool)
    m[1:, :] &= code[1:, :] == code[:-1, :]
    m[:-1, :] &= code[:-1, :] == code[1:, :]
    m[:, 1:] &= code[:, 1:] == code[:, :-1]
    m[:, :-1] &= code[:, :-1] == code[:, 1:]
    return m


def against_frame(label, z16):
    """(interior pixels that miss the frame's depth, interior pixels): at an interior pixel t lies inside the eye depths of z16 - 2 ..
    z16 + 2 widened by 1e-6, and a pixel that shows nothing has z16 = 65535"""
    from depth_reference import world_z
    z = np.asarray(z16).astype(np.int64).reshape(label["code"].shape)
    lo, hi = world_z(np.maximum(z - 2, 0)), world_z(np.minimum(z + 2, 65535))
    t = label["t"]
    good = np.where(label["code"] < 0, z >= 65535, (t >= lo - 1e-6) & (t <= hi + 1e-6))
    inner = interior(label["code"])
    return int((inner & ~good).sum()), int(inner.sum())
