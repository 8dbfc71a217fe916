"""What a ray cast costs (mw_ray_cast; MiniWorldVecEnv.raycast / lidar) for Hallway x 4096, FourRooms x 4096 and Maze x 1024, against
the two routes a user has without it — neither is the code under test:
    (a) torch   the same casts against the walls written in torch on the device as batched tensor operations over [N, R, S] (S the
                padded segment count), in the same formulas; t compared with the kernel's to 1e-9
    (b) host    engine.get_geometry(env) + engine.get_state() and numpy per env (tests/ray_reference.py, the tests' restatement),
                measured over the first --host-envs envs and reported per env

    python tools/perf/ray_cost.py               # per config: five alternating windows, a process per window; one JSON line each
    python tools/perf/ray_cost.py --forms       # both launch forms at R = 1, 4, 16, 64, 256 (Maze x 1024, Hallway x 4096): the threshold
    python tools/perf/ray_cost.py --loop        # Hallway x 4096: a vec.step loop with a lidar(64) per step against the plain loop

A window measures, each between two device synchronisations: wall us per call, and the device time per call between two events around
the window's back-to-back calls (launch gaps included: an upper bound of the kernel's duration).  Keys: <call>.<radius>.<obstacles>,
call = lidar64 | lidar256 | cast1 | cast8, radius = ray (0) | disc (the agent's radius), obstacles = w (walls) | we (+ entities)."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {
    "hallway": ("MiniWorld-Hallway-v0", 4096),
    "fourrooms": ("MiniWorld-FourRooms-v0", 4096),
    "maze": ("MiniWorld-Maze-v0", 1024),
}
FORM_RAYS = (1, 4, 16, 64, 256)


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


def make(name):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0)
    vec.reset()
    return vec, n


def directions(n, rays):
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    ang = torch.rand((n, rays), generator=g, device="cuda", dtype=torch.float64) * (2 * math.pi)
    return torch.stack([torch.cos(ang), torch.sin(ang)], dim=2).contiguous()


def torch_cast(segs, o, d, max_t, radius):
    """baseline (a): segs [N, S, 4] (NaN rows pad), o [N, 2], d [N, R, 2] -> t [N, R]; walls only"""
    import torch
    inf = float("inf")
    ox, oz = o[:, None, None, 0], o[:, None, None, 1]
    dx, dz = d[:, :, None, 0], d[:, :, None, 1]
    ax, az, bx, bz = (segs[:, None, :, k] for k in range(4))

    def ray_seg(ax, az, bx, bz):
        ex, ez = bx - ax, bz - az
        den = dx * ez - dz * ex
        wx, wz = ax - ox, az - oz
        t = (wx * ez - wz * ex) / den
        s = (wx * dz - wz * dx) / den
        return torch.where((den != 0) & (t >= 0) & (s >= 0) & (s <= 1), t, inf)

    def ray_circle(cx, cz, R):
        wx, wz = ox - cx, oz - cz
        A, B, C = dx * dx + dz * dz, wx * dx + wz * dz, (wx * wx + wz * wz) - R * R
        disc = B * B - A * C
        t = (-B - torch.sqrt(disc)) / A
        t = torch.where((disc >= 0) & (t >= 0), t, inf)
        return torch.where(C < 0, 0.0, t)
    if radius > 0:
        ex, ez = bx - ax, bz - az
        ln = torch.sqrt(ex * ex + ez * ez)
        nx, nz = ez / ln * radius, -ex / ln * radius
        u = ((ox - ax) * ex + (oz - az) * ez) / (ex * ex + ez * ez)
        u = u.clamp(0.0, 1.0)
        inside = torch.sqrt((ax + u * ex - ox) ** 2 + (az + u * ez - oz) ** 2) < radius
        t = torch.minimum(torch.minimum(ray_circle(ax, az, radius), ray_circle(bx, bz, radius)),
                          torch.minimum(ray_seg(ax + nx, az + nz, bx + nx, bz + nz), ray_seg(ax - nx, az - nz, bx - nx, bz - nz)))
        t = torch.where(inside.expand_as(t), 0.0, t)
    else:
        t = ray_seg(ax, az, bx, bz)
    t = torch.nan_to_num(t, nan=inf)
    return t.amin(dim=2).clamp(max=max_t)


def device_segments(vec, n):
    import numpy as np
    import torch
    e = vec.engine
    rows = [np.asarray(e.get_geometry(i)[1], np.float64).reshape(-1, 4) for i in range(n)]
    s = max(len(r) for r in rows)
    out = np.full((n, s, 4), np.nan)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return torch.from_numpy(out).cuda()


def window(name, kind, reps, host_envs):
    import numpy as np
    import torch
    vec, n = make(name)
    e = vec.engine
    ar = float(e.cfg.agent_radius)
    out = {"max_segs": int(e.cfg.max_segs)}
    if kind == "kernel":
        dirs = {r: directions(n, r) for r in (1, 8)}
        res = {}
        for rname, radius in (("ray", 0.0), ("disc", ar)):
            for oname, obstacles in (("w", "walls"), ("we", "walls+entities")):
                calls = {"lidar64": lambda: vec.lidar(64, radius=radius, obstacles=obstacles), "lidar256": lambda: vec.lidar(256, radius=radius, obstacles=obstacles)}
                for r in (1, 8):
                    key = (r, rname, oname)
                    res[key] = vec.raycast(direction=dirs[r], max_t=10.0, radius=radius, obstacles=obstacles)
                    calls[f"cast{r}"] = (lambda r=r, key=key: vec.raycast(direction=dirs[r], max_t=10.0, radius=radius, obstacles=obstacles, into=res[key]))
                for cname, fn in calls.items():
                    out[f"{cname}.{rname}.{oname}.wall"], out[f"{cname}.{rname}.{oname}.device"] = timed(fn, reps)
    elif kind == "forms":
        for form in (1, 2):
            e.debug_set_ray_form(form)
            for r in FORM_RAYS:
                d = directions(n, r)
                for rname, radius in (("ray", 0.0), ("disc", ar)):
                    res = vec.raycast(direction=d, max_t=10.0, radius=radius, obstacles="walls+entities")
                    _, out[f"form{form}.R{r}.{rname}.device"] = timed(lambda: vec.raycast(direction=d, max_t=10.0, radius=radius, obstacles="walls+entities", into=res), reps)
        e.debug_set_ray_form(0)
    elif kind == "torch":
        segs = device_segments(vec, n)
        o = vec.state(("agent_pos",))["agent_pos"][:, [0, 2]].contiguous()
        for r in (1, 8, 64, 256):
            d = directions(n, r)
            for rname, radius in (("ray", 0.0), ("disc", ar)):
                want = vec.raycast(direction=d, max_t=10.0, radius=radius)["t"]
                got = torch_cast(segs, o, d, 10.0, radius)
                assert float((got - want).abs().max()) < 1e-9, "the baseline's ranges are others"
                out[f"torch{r}.{rname}.w.wall"], out[f"torch{r}.{rname}.w.device"] = timed(lambda: torch_cast(segs, o, d, 10.0, radius), max(2, reps // 10))
    else:
        sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
        import nav_reference as nav
        import ray_reference as ref
        offs = ref.lidar_offsets(64, 2 * math.pi)
        want = vec.lidar(64, radius=ar)["t"][:host_envs].cpu().numpy()
        t0 = time.perf_counter()
        st = e.get_state()
        for i in range(host_envs):
            w = nav.world_of_engine(e, st, i)
            o = np.tile(st["agent_pos"][i][[0, 2]][None], (64, 1))
            t, _ = ref.cast(w, o, ref.fan_directions(st["agent_dir"][i], offs), 10.0, ar, True)
            assert np.array_equal(t, want[i]), i
        out["host_envs"] = host_envs
        out["host_lidar64_us_per_env"] = round(1e6 * (time.perf_counter() - t0) / host_envs, 1)
    e.check()
    vec.close()
    print(json.dumps(out), flush=True)


def loop_window(kind, steps, warmup):
    """Hallway x 4096: us per step of a random-action loop, with a lidar(64) per step or without"""
    import torch
    vec, n = make("hallway")
    g = torch.Generator(device="cuda").manual_seed(3)

    def step():
        if kind == "lidar":
            vec.lidar(64)
        vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    us = 1e6 * (time.perf_counter() - t0) / steps
    vec.engine.check()
    print(json.dumps({"us_per_step": round(us, 1)}), flush=True)
    vec.close()


def child(extra, timeout=600):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        print(json.dumps({"args": extra, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
        raise SystemExit(1)
    return json.loads(line[-1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="hallway,fourrooms,maze")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--host-envs", type=int, default=4)
    p.add_argument("--forms", action="store_true")
    p.add_argument("--loop", action="store_true")
    p.add_argument("--steps", type=int, default=600)
    p.add_argument("--warmup", type=int, default=100)
    p.add_argument("--window", choices=["kernel", "forms", "torch", "host", "lidar", "plain"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window in ("lidar", "plain"):
        return loop_window(args.window, args.steps, args.warmup)
    if args.window:
        return window(args.config, args.window, args.reps, args.host_envs)
    if args.loop:
        us = {}
        for _ in range(args.windows):
            for kind in ("lidar", "plain"):
                print(f"loop window: {kind}", file=sys.stderr, flush=True)
                for k, v in child(["--window", kind, "--steps", str(args.steps), "--warmup", str(args.warmup)]).items():
                    us.setdefault(kind + "." + k, []).append(v)
        print(json.dumps({"config": "hallway", "loop": us}), flush=True)
        return
    for name in [c for c in args.configs.split(",") if c in CONFIGS]:
        us = {}
        for w in range(args.windows):
            kinds = ("forms",) if args.forms else ("kernel", "torch") + (("host",) if w == 0 else ())
            for kind in kinds:
                print(f"{name} window {w}: {kind}", file=sys.stderr, flush=True)
                for k, v in child(["--window", kind, "--config", name, "--reps", str(args.reps), "--host-envs", str(args.host_envs)]).items():
                    us.setdefault(k, []).append(v)
        print(json.dumps({"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "forms": bool(args.forms), "windows": us}), flush=True)


if __name__ == "__main__":
    main()
