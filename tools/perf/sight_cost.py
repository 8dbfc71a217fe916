"""What grid sight costs (mw_grid_sight; MiniWorldVecEnv.grid_sight) for Hallway x 4096, FourRooms x 4096 and Maze x 1024 at V = 1 (the
agent's own cell and cone), 16 and 64 candidate cells, range 3 m, beside the route it replaces: the same predicate as torch tensor
operations over [N, V, targets of the range box], a gather per candidate cell of every step along the major axis.

    python tools/perf/sight_cost.py                 # per config: five alternating windows, a process per window; one JSON line each

The state: a DepthMap after --map-steps random steps; opaque its obstacle plane, the weight its unknown cells, the candidates frontier
cells sampled as examples/view_explore.py samples them (the same seed in every window).  A window measures, each between two device
synchronisations: wall us per call, and the device time per call between two events around the window's back-to-back calls (launch
gaps included: an upper bound of the kernel's duration).  A torch window first counts the gains and the cells of the seen plane in
which the route differs from the kernel: 0 is asserted.
The record: whether every kernel window lies below every torch window; nothing here is a threshold."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nav_cost import CONFIGS, timed  # noqa: E402

VIEWS = (1, 16, 64)
RANGE = 3.0


def _run(extra, timeout=900):
    """this file again as a process of its own, under its own time limit: the JSON line it prints"""
    import subprocess
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        print(json.dumps({"args": extra, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
        raise SystemExit(1)
    return json.loads(line[-1])


def torch_sight(opaque, weight, cells, heading, cell, max_range, cos_half, seen, chunk=512):
    """the route: gain int32[N, V]; `seen` (uint8[N, gz, gx]) gets a 1 in every seen cell.  heading: float64[N, V, 2] or None"""
    import torch
    n, gz, gx = opaque.shape
    dev = opaque.device
    r = int(min(max(gx, gz), math.floor(max_range / cell) + 1))
    off = torch.arange(-r, r + 1, device=dev)
    dz, dx = (t.reshape(-1) for t in torch.meshgrid(off, off, indexing="ij"))
    vx, vz = dx.double() * cell, dz.double() * cell
    dist = torch.sqrt(vx * vx + vz * vz)
    xmajor = dx.abs() >= dz.abs()
    big, m = torch.where(xmajor, dx.abs(), dz.abs()), torch.where(xmajor, dz, dx)
    sgn = torch.where(torch.where(xmajor, dx, dz) < 0, -1, 1)
    s, lo, hi, den = big + m.abs(), m.clamp(max=0), m.clamp(min=0), big.clamp(min=1)
    gain = torch.zeros(cells.shape, dtype=torch.int32, device=dev)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        c = cells[a:b].to(torch.int64)
        valid = (c >= 0) & (c < gx * gz)
        c = c.clamp(0, gx * gz - 1)
        ja, ia = (c // gx)[..., None], (c % gx)[..., None]
        jb, ib = ja + dz, ia + dx
        inside = valid[..., None] & (jb >= 0) & (jb < gz) & (ib >= 0) & (ib < gx)
        ok = (dist <= max_range).expand_as(inside)
        if cos_half != -1.0:
            h = heading[a:b]
            ok = ok & ((dist == 0.0) | (vx * h[..., 0:1] + vz * h[..., 1:2] >= cos_half * dist))
        base = (torch.arange(b - a, device=dev) * (gx * gz))[:, None, None]
        flat = opaque[a:b].reshape(-1)
        hidden = torch.zeros_like(inside)
        for k in range(r + 1):
            f = torch.div(m * k, den, rounding_mode="floor")
            for du in (-1, 0, 1):
                u = f + du
                cand = (k <= big) & (u >= lo) & (u <= hi) & (2 * (big * u - m * k).abs() <= s) & ~((u == 0) & (k == 0)) & ~((u == m) & (big == k))
                qj, qi = torch.where(xmajor, u, sgn * k), torch.where(xmajor, sgn * k, u)
                at = ((ja + qj) * gx + (ia + qi)).clamp(0, gx * gz - 1) + base
                hidden |= cand & inside & (flat[at] != 0)          # the gather
        vis = ok & inside & ~hidden
        tb = (jb * gx + ib).clamp(0, gx * gz - 1)
        w = weight[a:b].reshape(-1)[tb + base].to(torch.int32) if weight is not None else 1
        gain[a:b] = (vis.to(torch.int32) * w).sum(-1).to(torch.int32)
        seen[a:b].reshape(b - a, -1).scatter_reduce_(1, tb.reshape(b - a, -1), vis.reshape(b - a, -1).to(torch.uint8), "amax")
    return gain


def window(name, kind, reps, map_steps):
    import torch
    from depth_plan_explore import frontier_of
    from miniworld_amd.vec_env import MiniWorldVecEnv
    from view_explore import sample_cells
    env_id, n = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0, want_depth=True)
    vec.reset()
    g = torch.Generator(device="cuda").manual_seed(5)
    m = vec.depth_map(max_range=8.0)
    vec.depth_map_update(m)
    for _ in range(map_steps):
        vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
        vec.depth_map_update(m)
    frontier, unknown = frontier_of(m)
    opaque, weight = (m.obstacle != 0).contiguous(), unknown.contiguous()
    gz, gx, cell = m.gz, m.gx, m.cell
    out = {"cells": gx * gz, "opaque_share": round(float(opaque.float().mean()), 4), "unknown_share": round(float(unknown.float().mean()), 4)}
    cos_fov = math.cos(vec.default_fov() / 2)
    for views in VIEWS:
        cells = sample_cells(frontier, views, g) if views > 1 else None
        if kind == "kernel":
            gain = vec.grid_sight(opaque, cells, weight=weight, max_range=RANGE, like=m)
            out[f"gain_mean_{views}"] = round(float(gain.float().mean()), 1)
            out[f"kernel_wall_{views}"], out[f"kernel_device_{views}"] = timed(lambda: vec.grid_sight(opaque, cells, weight=weight, max_range=RANGE, like=m), reps)
            seen = torch.zeros((n, gz, gx), dtype=torch.uint8, device="cuda")
            out[f"kernel_seen_wall_{views}"], out[f"kernel_seen_device_{views}"] = timed(
                lambda: vec.grid_sight(opaque, cells, weight=weight, max_range=RANGE, like=m, seen=seen), reps)
            continue
        seen = torch.zeros((n, gz, gx), dtype=torch.uint8, device="cuda")
        gain = vec.grid_sight(opaque, cells, weight=weight, max_range=RANGE, like=m, seen=seen)
        if cells is None:       # the agents' own cells, clamped as the engine clamps them, and the fan's heading at offset 0
            st = vec.state(("agent_pos",))["agent_pos"]
            ext = torch.as_tensor(vec.engine.get_state()["extent"], dtype=torch.float64, device="cuda")
            i = torch.floor((st[:, 0] - ext[:, 0]) / cell).clamp(0, gx - 1).to(torch.int64)
            j = torch.floor((st[:, 2] - ext[:, 2]) / cell).clamp(0, gz - 1).to(torch.int64)
            route_cells = (j * gx + i).to(torch.int32)[:, None].contiguous()
            heading = vec.raycast(offsets=torch.zeros(1, dtype=torch.float64, device="cuda"))["dir"]
            cos_half = cos_fov
        else:
            route_cells, heading, cos_half = cells, None, -1.0
        seen_r = torch.zeros_like(seen)
        gain_r = torch_sight(opaque, weight, route_cells, heading, cell, RANGE, cos_half, seen_r)
        differ = int((gain_r != gain).sum()) + int((seen_r != seen).sum())
        assert differ == 0, ("the route's gains or seen cells are others", views, differ)
        out[f"differ_{views}"] = differ

        def route():
            torch_sight(opaque, weight, route_cells, heading, cell, RANGE, cos_half, seen_r)
        out[f"torch_wall_{views}"], out[f"torch_device_{views}"] = timed(route, max(2, reps // 50))
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
    p.add_argument("--window", choices=["kernel", "torch"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window:
        return window(args.config, args.window, args.reps, args.map_steps)
    for name in [c for c in args.configs.split(",") if c in CONFIGS]:
        us = {}
        for w in range(args.windows):
            for kind in ("kernel",) if args.no_torch else ("kernel", "torch"):
                print(f"{name} window {w}: {kind}", file=sys.stderr, flush=True)
                for k, v in _run(["--window", kind, "--config", name, "--reps", str(args.reps), "--map-steps", str(args.map_steps)]).items():
                    us.setdefault(k, []).append(v)
        rec = {"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "range": RANGE, "windows": us}
        if not args.no_torch:
            rec["every_kernel_window_below_every_torch_window"] = all(
                max(us[f"kernel_device_{v}"]) < min(us[f"torch_device_{v}"]) and max(us[f"kernel_wall_{v}"]) < min(us[f"torch_wall_{v}"]) for v in VIEWS)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
