#!/usr/bin/env python3
"""examples/depth_plan_explore.py with the DepthMap replaced by a ScanMap: what each agent knows of its floor plan is what its range
scanner traced — `vec.scan_map_update(m)` casts a lidar from the agent and marks the cells the beams pass through free and the cells
they end in obstacles —, the planner is `vec.grid_field()` over that map towards the frontier (the free cells beside cells that are
neither free nor obstacle), the follower the turn-or-forward rule of examples/expert_nav.py.  No frame is needed for any of it:

    python examples/scan_explore.py --env MiniWorld-MazeS3-v0 --envs 256 --horizon 120 --steps 600 --frameless

`--frameless` steps with `vec.rollout(act[None], render=False)`: nothing is drawn at all, the env is made without depth maps.  Without
it the loop steps with `vec.step()` like its siblings.  `--compare` runs depth_plan_explore.py's explorer on the same settings too.

The coverage is scored exactly as depth_plan_explore.py scores it, on a SeenMap and the walls' own unblocked cells, neither of which
the policy reads.  Results, not thresholds: see README.md, "Scan maps".
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from depth_plan_explore import frontier_of  # noqa: E402
from expert_nav import TURN_LEFT, expert  # noqa: E402
from explore_frontier import unblocked_of  # noqa: E402


def run(args):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n = args.envs
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed, want_depth=False)
    turn_step = math.radians(float(vec.engine.cfg.turn_step.default))
    dev = vec.engine.device
    vec.reset()
    score = vec.seen_map(cell=args.cell, max_range=args.range)          # the yardstick: never read by the policy
    vec.seen_update(score)
    yard = vec.nav_field(target=vec.state(("agent_pos",))["agent_pos"].clone(), reach=2 * args.cell, cell=args.cell)
    m = vec.scan_map(like=score, rays=args.rays, max_range=args.range)
    vec.scan_map_update(m)
    plan = None
    taken, covered = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
    age = torch.zeros(n, dtype=torch.int32, device=dev)
    counted = torch.zeros(n, dtype=torch.bool, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        st = vec.state(("agent_pos", "agent_dir"))
        frontier, unknown = frontier_of(m)
        plan = vec.grid_field(m.obstacle != 0, frontier, like=m) if plan is None else vec.grid_field(m.obstacle != 0, frontier, into=plan)
        q = vec.nav_query(plan)
        act = expert(st["agent_pos"], st["agent_dir"], q["waypoint"], turn_step)
        act = torch.where(q["cost"] > 0, act, TURN_LEFT).to(torch.int32)
        _, _, term, trunc = vec.rollout(act[None], render=False) if args.frameless else vec.step(act)
        done = (term | trunc) != 0
        free = unblocked_of(yard)
        share = ((score.seen == 1) & free).sum((1, 2)).to(torch.float64) / free.sum((1, 2)).clamp(min=1).to(torch.float64)
        early = done & ~counted
        vec.seen_update(score, clear=done)
        vec.scan_map_update(m, clear=done)
        age = torch.where(done, 0, age + 1)
        due = ~done & ~counted & (age == args.horizon)
        now = ((score.seen == 1) & free).sum((1, 2)).to(torch.float64) / free.sum((1, 2)).clamp(min=1).to(torch.float64)
        taken += early.sum() + due.sum()
        covered += torch.where(early, share, 0.0).sum() + torch.where(due, now, 0.0).sum()
        counted = (counted | due) & ~done
        vec.nav_field(into=yard, mask=done)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    vec.engine.check()
    vec.close()
    return float(covered / taken.clamp(min=1)), int(taken), dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-MazeS3-v0")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--horizon", type=int, default=120, help="steps of an episode after which its coverage is taken")
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--rays", type=int, default=256, help="beams of the scanner, all round")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frameless", action="store_true", help="step with rollout(render=False): no frame is drawn")
    ap.add_argument("--compare", action="store_true", help="run depth_plan_explore.py's explorer (depth map) and depth_explore.py's (privileged planner) too")
    args = ap.parse_args()
    results = [(f"scan map of {args.rays} beams, grid planner{', frameless' if args.frameless else ''}", run(args))]
    if args.compare:
        from depth_explore import run as privileged_plan_run
        from depth_plan_explore import run as depth_run
        args.unknown = 0
        results.append(("depth map, grid planner", depth_run(args)))
        results.append(("depth map, privileged planner", privileged_plan_run(args)))
    for name, (cov, ended, dt) in results:
        print(f"{args.env} x {args.envs}, {args.steps} steps: {name}: mean coverage {cov:.3f} after {args.horizon} steps of an episode "
              f"(or at its end), over {ended} episodes ({dt:.2f} s, {dt / args.steps * 1e6:.0f} us per step)")


if __name__ == "__main__":
    main()
