"""What a label frame costs (mw_label_frame; MiniWorldVecEnv.label_update) for Hallway x 4096, FourRooms x 4096, Maze x 1024 and
PickupObjects with domain randomisation x 2048, each after 30 random steps:
    class      the class plane alone, mesh objects as their triangles
    all        every output (class, code, depth, per-slot pixels and boxes), mesh objects as their triangles
    bounds     every output, mesh objects as their bounding cylinders
    unpruned   as `all`, the mesh phase without its pruning rectangle (engine.LABEL_UNPRUNED): every triangle against every pixel
    route      the route the call replaces, written here with nothing this call added: the same ray / plane / box arithmetic as torch
               tensor operations in float64 over [N, H * W], one polygon and one Box slot at a time, no meshes — for the configs with one
               shared geometry set (Hallway, FourRooms); it also counts the pixels whose class differs from the kernel's (the route takes
               sin and cos from torch)

    python tools/perf/label_cost.py              # per config: five alternating windows, a process per window; one JSON line each

A window measures, each between two device synchronisations: wall us per call, and the device time per call between two events around the
window's back-to-back calls (launch gaps included: an upper bound of the kernel's duration)."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {
    "hallway": ("MiniWorld-Hallway-v0", 4096, {}),
    "fourrooms": ("MiniWorld-FourRooms-v0", 4096, {}),
    "maze": ("MiniWorld-Maze-v0", 1024, {}),
    "pickup_dr": ("MiniWorld-PickupObjects-v0", 2048, dict(domain_rand=True)),
}
KINDS = ("class", "all", "bounds", "unpruned", "route")
SAMPLE0 = {8: (9, 5), 4: (6, 2), 1: (8, 8)}


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(1e6 * (time.perf_counter() - t0) / reps, 2), round(1e3 * a.elapsed_time(b) / reps, 2)


def route(vec, n):
    """the class plane without mw_label_frame: uint8[N, H * W]"""
    import torch
    from miniworld_amd import engine
    H, W = int(vec.engine.cfg.obs_height), int(vec.engine.cfg.obs_width)
    sx, sy = SAMPLE0[int(vec.engine.cfg.msaa)]
    u = torch.arange(W, dtype=torch.float64, device="cuda")[None, :].expand(H, W).reshape(1, -1)
    v = torch.arange(H, dtype=torch.float64, device="cuda")[:, None].expand(H, W).reshape(1, -1)
    xn, yn = ((u + sx / 16.0) * 2.0) / W - 1.0, 1.0 - ((v + (1.0 - sy / 16.0)) * 2.0) / H
    polys, _ = vec.engine.get_geometry(-1)
    zero = torch.zeros(1, dtype=torch.float64, device="cuda")

    def run():
        st = vec.state(("agent_pos", "cam", "ent_kind", "ent_pos", "ent_dir", "ent_geom"))
        cam, pos = st["cam"], st["agent_pos"]
        h = vec.raycast(offsets=zero)["dir"][:, 0]
        hx, hz = h[:, 0:1], h[:, 1:2]
        pitch, half = cam[:, 2:3] * math.pi / 180.0, cam[:, 3:4] * 0.5 * math.pi / 180.0
        sp, cp, th = torch.sin(pitch), torch.cos(pitch), torch.sin(half) / torch.cos(half)
        lat, yt = xn * (th * (W / H)), yn * th
        up, fwd = sp + yt * cp, cp - yt * sp
        dx, dy, dz = fwd * hx + lat * -hz, up, fwd * hz + lat * hx
        ex, ey, ez = pos[:, 0:1] + cam[:, 1:2] * hx, pos[:, 1:2] + cam[:, 0:1], pos[:, 2:3] + cam[:, 1:2] * hz
        best = torch.full((n, H * W), math.inf, dtype=torch.float64, device="cuda")
        cls = torch.zeros((n, H * W), dtype=torch.uint8, device="cuda")
        for q in polys:
            nv = 3 if (int(q["nv"]) & 0xFF) == 3 else 4
            V = [[float(c) for c in q["v"][i]] for i in range(nv)]
            if int(q["nv"]) & engine.POLY_XF:
                s, c = math.sin(math.radians(float(q["xf"][3]))), math.cos(math.radians(float(q["xf"][3])))
                V = [[c * x + s * z + float(q["xf"][0]), y + float(q["xf"][1]), c * z - s * x + float(q["xf"][2])] for x, y, z in V]
            a, b = [V[1][k] - V[0][k] for k in range(3)], [V[2][k] - V[0][k] for k in range(3)]
            nrm = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
            den = nrm[0] * dx + nrm[1] * dy + nrm[2] * dz
            t = (nrm[0] * (V[0][0] - ex) + nrm[1] * (V[0][1] - ey) + nrm[2] * (V[0][2] - ez)) / den
            ok = (den != 0.0) & (t >= 0.04) & (t <= 100.0) & (t < best)
            px, py, pz = ex + t * dx, ey + t * dy, ez + t * dz
            for i in range(nv):
                j = (i + 1) % nv
                e = [V[j][k] - V[i][k] for k in range(3)]
                m = (nrm[1] * e[2] - nrm[2] * e[1], nrm[2] * e[0] - nrm[0] * e[2], nrm[0] * e[1] - nrm[1] * e[0])
                ok &= m[0] * px + m[1] * py + m[2] * pz - (m[0] * V[i][0] + m[1] * V[i][1] + m[2] * V[i][2]) >= 0.0
            kind = 4 if int(q["nv"]) & engine.POLY_ENTITY else 3 if int(q["nv"]) & engine.POLY_QUAD else 1 if nrm[1] > 0 else 2
            best = torch.where(ok, t, best)
            cls = torch.where(ok, torch.full_like(cls, kind), cls)
        for s in range(int(vec.engine.E)):
            isbox = st["ent_kind"][:, s:s + 1] == engine.ENT_BOX
            sn, cs = torch.sin(st["ent_dir"][:, s:s + 1]), torch.cos(st["ent_dir"][:, s:s + 1])
            qx, qy, qz = ex - st["ent_pos"][:, s, 0:1], ey - st["ent_pos"][:, s, 1:2], ez - st["ent_pos"][:, s, 2:3]
            o = (cs * qx - sn * qz, qy.expand(n, 1), sn * qx + cs * qz)
            l = (cs * dx - sn * dz, dy, sn * dx + cs * dz)
            g = st["ent_geom"][:, s]
            lo, hi = (-g[:, 0:1] / 2, torch.zeros_like(qx), -g[:, 2:3] / 2), (g[:, 0:1] / 2, g[:, 1:2], g[:, 2:3] / 2)
            enter = torch.full_like(best, -math.inf)
            leave = torch.full_like(best, math.inf)
            for k in range(3):
                t1, t2 = (lo[k] - o[k]) / l[k], (hi[k] - o[k]) / l[k]
                enter, leave = torch.maximum(enter, torch.minimum(t1, t2)), torch.minimum(leave, torch.maximum(t1, t2))
            ok = isbox & (enter <= leave) & (enter >= 0.04) & (enter <= 100.0) & (enter < best)
            best = torch.where(ok, enter, best)
            cls = torch.where(ok, torch.full_like(cls, 5), cls)
        return cls
    return run


def window(name, kind, reps):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n, kw = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0, **kw)
    vec.reset()
    g = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(30):
        vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
    out = {}
    if kind == "route":
        if not vec.engine.cfg.shared_geometry:
            out["route.skipped"] = "per-env geometry"
        else:
            run = route(vec, n)
            f = vec.label_frame(meshes="bounds", code=False)
            vec.label_update(f)
            out["route.pixels_that_differ"] = int((run() != f.cls.reshape(n, -1)).sum())
            out["route.wall"], out["route.device"] = timed(run, max(2, reps // 10))
    else:
        full = kind != "class"
        f = vec.label_frame(meshes="bounds" if kind == "bounds" else "exact", code=full, depth=full, stats=full)
        if kind == "unpruned":
            p = engine.MwLabelParams(f.near, f.far, engine.LABEL_MESH_EXACT | engine.LABEL_UNPRUNED, 0)
            run = lambda: vec.engine.label_frame(p, f.cls, f.code, f.depth, f.ent_pixels, f.ent_box)
            reps = max(2, reps // 10)
        else:
            run = lambda: vec.label_update(f)
        out[f"{kind}.wall"], out[f"{kind}.device"] = timed(run, reps)
        shares = torch.bincount(f.cls.reshape(-1).long(), minlength=7).double() / f.cls.numel()
        out[f"{kind}.class_shares"] = [round(float(x), 4) for x in shares]
    vec.engine.check()
    vec.close()
    print(json.dumps(out), flush=True)


def child(extra, timeout=600):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        print(json.dumps({"args": extra, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
        raise SystemExit(1)
    return json.loads(line[-1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default=",".join(CONFIGS))
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--kinds", default=",".join(KINDS))
    p.add_argument("--window", choices=KINDS, help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window:
        return window(args.config, args.window, args.reps)
    for name in [c for c in args.configs.split(",") if c in CONFIGS]:
        us = {}
        for w in range(args.windows):
            for kind in [k for k in KINDS if k in args.kinds.split(",")]:
                print(f"{name} window {w}: {kind}", file=sys.stderr, flush=True)
                for k, v in child(["--window", kind, "--config", name, "--reps", str(args.reps)]).items():
                    us.setdefault(k, []).append(v)
        print(json.dumps({"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "windows": us}), flush=True)


if __name__ == "__main__":
    main()
