"""What grid ray casts cost (mw_grid_ray_cast; MiniWorldVecEnv.grid_lidar, grid_raycast) for Hallway x 4096, FourRooms x 4096 and Maze x
1024: grid_lidar at 64 / 256 / 1024 rays and 1 and 8 explicit casts from the agents, beside the route they replace — the same rule as
torch tensor operations: every candidate of every ray over [N, R, 1 + (gx + 1) + (gz + 1)], a gather, the least s and then the least
index among its equals — and beside the privileged lidar() of the same ray counts.

    python tools/perf/grid_ray_cost.py                  # per config: five alternating windows, a process per window; one JSON line each
    python tools/perf/grid_ray_cost.py --forms          # per config: either launch form forced at R = 1 .. 256, device us per call
    python tools/perf/grid_ray_cost.py --ab A.so B.so   # per config: kernel windows alternating between two libraries (MW_ENGINE_LIB)

The state: a DepthMap after --map-steps random steps; opaque its obstacle plane.  A window measures, each between two device
synchronisations: wall us per call, and the device time per call between two events around the window's back-to-back calls (launch
gaps included: an upper bound of the kernel's duration).  A torch window first counts the elements of t and hit in which the route
differs from the kernel: 0 is asserted.
The record: whether every kernel window lies below every torch window; nothing here is a threshold."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nav_cost import CONFIGS, timed  # noqa: E402

FANS, CASTS, RANGE, SWEEP = (64, 256, 1024), (1, 8), 10.0, (1, 2, 4, 8, 16, 32, 64, 128, 256)


def _run(extra, timeout=900, lib=None):
    """this file again as a process of its own, under its own time limit: the JSON line it prints"""
    import subprocess
    env = dict(os.environ, **({"MW_ENGINE_LIB": os.path.abspath(lib)} if lib else {}))
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        print(json.dumps({"args": extra, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
        raise SystemExit(1)
    return json.loads(line[-1])


def torch_cast(opaque, origin, d, max_t, lo, cell, budget=1 << 24):
    """the route: (t float64[N, R], hit int32[N, R]); origin [N, 2] (x, z), d [N, R, 2], lo [N, 2] the envs' min_x, min_z"""
    import torch
    n, gz, gx = opaque.shape
    R, dev, bound = d.shape[1], opaque.device, 2.0 ** 30
    t, hit = torch.empty((n, R), dtype=torch.float64, device=dev), torch.empty((n, R), dtype=torch.int32, device=dev)
    chunk = max(1, budget // (R * (gx + gz + 3)))
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        u0, w0 = ((origin[a:b, 0] - lo[a:b, 0]) / cell)[:, None, None], ((origin[a:b, 1] - lo[a:b, 1]) / cell)[:, None, None]
        gu, gw = (d[a:b, :, 0] / cell)[..., None], (d[a:b, :, 1] / cell)[..., None]
        u1, w1 = u0 + max_t * gu, w0 + max_t * gw
        keep = torch.ones_like(gu, dtype=torch.bool)
        for v in (u0, w0, u1, w1):
            keep = keep & torch.isfinite(v) & (v.abs() < bound)
        s, row, col, ok = [torch.zeros_like(gu)], [torch.floor(w0).expand_as(gu)], [torch.floor(u0).expand_as(gu)], [keep]
        for a0, a1, g, b0, h, lines, x_lines in ((u0, u1, gu, w0, gw, gx, True), (w0, w1, gw, u0, gu, gz, False)):
            L = torch.arange(lines + 1, dtype=torch.float64, device=dev)
            crossed = torch.where(g > 0.0, (L >= torch.floor(a0) + 1.0) & (L <= torch.floor(a1)), (g < 0.0) & (L >= torch.floor(a1) + 1.0) & (L <= torch.floor(a0)))
            s_ = (L - a0) / g + 0.0
            other, own = torch.floor(b0 + s_ * h), torch.where(g > 0.0, L, L - 1.0).expand_as(s_)
            s.append(s_), row.append(other if x_lines else own), col.append(own if x_lines else other), ok.append(crossed & keep)
        s, row, col, ok = (torch.cat(v, -1) for v in (s, row, col, ok))
        ok = ok & (row >= 0.0) & (row < gz) & (col >= 0.0) & (col < gx)
        flat = torch.where(ok, row * gx + col, torch.zeros_like(row)).to(torch.int64)
        ok = ok & (opaque[a:b].reshape(b - a, 1, -1).expand(-1, R, -1).gather(2, flat) != 0)       # the gather
        least = torch.where(ok, s, torch.full_like(s, float("inf"))).amin(-1, keepdim=True)
        index = torch.where(ok & (s == least), flat, torch.full_like(flat, 1 << 30)).amin(-1)
        any_ = ok.any(-1)
        t[a:b] = torch.where(any_, least[..., 0].clamp(max=max_t), torch.full_like(least[..., 0], max_t))
        hit[a:b] = torch.where(any_, index, torch.full_like(index, -1)).to(torch.int32)
    return t, hit


def window(name, kind, reps, map_steps):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0, want_depth=True)
    vec.reset()
    g = torch.Generator(device="cuda").manual_seed(5)
    m = vec.depth_map(max_range=8.0)
    vec.depth_map_update(m)
    for _ in range(map_steps):
        vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
        vec.depth_map_update(m)
    opaque = (m.obstacle != 0).contiguous()
    out = {"cells": m.gx * m.gz, "opaque_share": round(float(opaque.float().mean()), 4)}
    ang = {R: torch.rand((n, R), generator=g, device="cuda", dtype=torch.float64) * 6.283185307179586 for R in CASTS}
    dirs = {R: torch.stack([torch.cos(a), -torch.sin(a)], -1).contiguous() for R, a in ang.items()}
    calls = [(f"lidar_{R}", lambda R=R: vec.grid_lidar(opaque, rays=R, max_range=RANGE, like=m)) for R in FANS]
    calls += [(f"cast_{R}", lambda R=R: vec.grid_raycast(opaque, dirs[R], max_t=RANGE, like=m)) for R in CASTS]
    if kind == "forms":
        for form in (1, 2):
            vec.engine.debug_set_ray_form(form)
            for R in SWEEP:
                out[f"form{form}_device_{R}"] = timed(lambda: vec.grid_lidar(opaque, rays=R, max_range=RANGE, like=m), reps)[1]
    elif kind == "kernel":
        for key, call in calls:
            out[f"hits_{key}"] = round(float((call()["hit"] >= 0).float().mean()), 3)
            out[f"kernel_wall_{key}"], out[f"kernel_device_{key}"] = timed(call, reps)
        for R in FANS:
            out[f"privileged_wall_lidar_{R}"], out[f"privileged_device_lidar_{R}"] = timed(lambda: vec.lidar(R, max_range=RANGE), reps)
    else:
        origin = vec.state(("agent_pos",))["agent_pos"][:, [0, 2]].contiguous()
        lo = torch.as_tensor(vec.engine.get_state()["extent"], dtype=torch.float64, device="cuda")[:, [0, 2]].contiguous()
        for key, call in calls:
            r = call()
            t, hit = torch_cast(opaque, origin, r["dir"], RANGE, lo, m.cell)
            differ = int((t.view(torch.int64) != r["t"].view(torch.int64)).sum()) + int((hit != r["hit"]).sum())
            assert differ == 0, ("the route's t or hit are others", key, differ)
            out[f"differ_{key}"] = differ
            d = r["dir"].clone()
            out[f"torch_wall_{key}"], out[f"torch_device_{key}"] = timed(lambda: torch_cast(opaque, origin, d, RANGE, lo, m.cell), max(2, reps // 50))
    vec.engine.check()
    vec.close()
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="hallway,fourrooms,maze")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--map-steps", type=int, default=40, help="random steps the DepthMap accumulates over")
    p.add_argument("--no-torch", action="store_true", help="kernel windows only")
    p.add_argument("--forms", action="store_true", help="either launch form forced at every ray count of the sweep, in place of the windows")
    p.add_argument("--ab", nargs=2, metavar="LIB", help="kernel windows alternating between two libraries, in place of the torch route")
    p.add_argument("--window", choices=["kernel", "torch", "forms"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window:
        return window(args.config, args.window, args.reps, args.map_steps)
    keys = [f"lidar_{R}" for R in FANS] + [f"cast_{R}" for R in CASTS]
    for name in [c for c in args.configs.split(",") if c in CONFIGS]:
        us, tail = {}, ["--config", name, "--reps", str(args.reps), "--map-steps", str(args.map_steps)]
        for w in range(args.windows):
            for kind, lib in ((("forms", None),) if args.forms else tuple(("kernel", lib) for lib in args.ab) if args.ab
                              else (("kernel", None),) if args.no_torch else (("kernel", None), ("torch", None))):
                print(f"{name} window {w}: {kind} {lib or ''}", file=sys.stderr, flush=True)
                for k, v in _run(["--window", kind] + tail, lib=lib).items():
                    us.setdefault(k if not lib else f"{k}@{os.path.basename(lib)}", []).append(v)
        rec = {"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "range": RANGE, "windows": us}
        if not (args.no_torch or args.forms or args.ab):
            rec["every_kernel_window_below_every_torch_window"] = all(
                max(us[f"kernel_device_{k}"]) < min(us[f"torch_device_{k}"]) and max(us[f"kernel_wall_{k}"]) < min(us[f"torch_wall_{k}"]) for k in keys)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
