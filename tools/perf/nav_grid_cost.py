"""What a grid navigation field costs (mw_nav_build_grid; MiniWorldVecEnv.grid_field) for Hallway x 4096, FourRooms x 4096 and Maze x 1024,
beside the privileged build on the same grid and the torch route it replaces (tools/perf/nav_cost.py: torch_relax, a min-plus
relaxation over such grids).

    python tools/perf/nav_grid_cost.py                 # per config: five alternating windows, a process per window; one JSON line each

A window measures, each between two device synchronisations: wall us per call, and the device time per call between two events around
the window's back-to-back calls (launch gaps included: an upper bound of the kernel's duration).
    build           nav_field(into=field) of the whole batch: the privileged build, the same relaxation (parity is the expectation)
    grid            grid_field(blocked, sources, inflate=0, into=) with occupancy and sources taken from the privileged field: the
                    same field (asserted)
    grid_extra      the same with extra costs 0 .. 20
    grid_depth      grid_field over a DepthMap after --map-steps random steps: blocked its obstacle plane, sources its frontier, the
                    default inflation (agent_radius + cell / 2)
    rounds_*        the relaxation's rounds per env (max, mean) of each
    torch           torch_relax on the privileged field's blocked and sources
The record: whether every `grid` window lies below every torch window; nothing here is a threshold."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nav_cost import BLOCKED, CONFIGS, INF, UNREACHED, timed, torch_relax  # noqa: E402


def _run(extra, timeout=900):
    """this file again as a process of its own: the JSON line it prints"""
    import subprocess
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        print(json.dumps({"args": extra, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
        raise SystemExit(1)
    return json.loads(line[-1])


def window(name, kind, reps, map_steps):
    import torch
    from depth_plan_explore import frontier_of
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0, want_depth=kind == "kernel")
    vec.reset()
    e = vec.engine
    fld = vec.nav_field()
    bits = fld.field.view(torch.int16)
    f = bits.to(torch.int32) & 0xFFFF
    blocked, sources = f == BLOCKED, f == 0
    out = {"cells": fld.gx * fld.gz}
    if kind == "kernel":
        passes = torch.zeros(n, dtype=torch.int32, device="cuda")
        e.debug_set_nav_passes(passes)

        def rounds(key):
            out[f"rounds_{key}_max"], out[f"rounds_{key}_mean"] = int(passes.max()), round(float(passes.float().mean()), 1)
        g = torch.Generator(device="cuda").manual_seed(5)
        extra = torch.randint(0, 21, f.shape, generator=g, device="cuda", dtype=torch.uint8)
        vec.nav_field(into=fld)
        rounds("build")
        grid = vec.grid_field(blocked, sources, inflate=0, like=fld)
        rounds("grid")
        assert torch.equal(grid.field.view(torch.int16), bits), "the grid build's field is another"
        weighted = vec.grid_field(blocked, sources, extra=extra, inflate=0, like=fld)
        rounds("grid_extra")
        m = vec.depth_map(like=fld, max_range=8.0)
        vec.depth_map_update(m)
        for _ in range(map_steps):
            vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
            vec.depth_map_update(m)
        frontier, _ = frontier_of(m)
        obstacle = m.obstacle != 0
        sensed = vec.grid_field(obstacle, frontier, like=m)
        rounds("grid_depth")
        e.debug_set_nav_passes(None)
        out["depth_obstacle_share"] = round(float(obstacle.float().mean()), 4)
        out["depth_blocked_share"] = round(float((sensed.field.view(torch.int16) == -1).float().mean()), 4)
        out["depth_frontier_cells_mean"] = round(float(frontier.sum((1, 2)).float().mean()), 1)
        out["build_wall"], out["build_device"] = timed(lambda: vec.nav_field(into=fld), reps)
        out["grid_wall"], out["grid_device"] = timed(lambda: vec.grid_field(blocked, sources, into=grid), reps)
        out["grid_extra_wall"], out["grid_extra_device"] = timed(lambda: vec.grid_field(blocked, sources, extra=extra, into=weighted), reps)
        out["grid_depth_wall"], out["grid_depth_device"] = timed(lambda: vec.grid_field(obstacle, frontier, into=sensed), reps)
    else:
        cost, passes = torch_relax(blocked, sources)
        same = torch.where(blocked, BLOCKED, torch.where(cost >= INF, UNREACHED, cost))
        assert torch.equal(same, f), "the baseline's field is another"
        out["torch_passes"] = passes
        out["torch_wall"], out["torch_device"] = timed(lambda: torch_relax(blocked, sources), max(2, reps // 20))
    e.check()
    vec.close()
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="hallway,fourrooms,maze")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--map-steps", type=int, default=40, help="random steps the DepthMap of grid_depth accumulates over")
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
        rec = {"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "windows": us}
        if not args.no_torch:
            rec["every_grid_window_below_every_torch_window"] = max(us["grid_device"]) < min(us["torch_device"]) and max(us["grid_wall"]) < min(us["torch_wall"])
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
