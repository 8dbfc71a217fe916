#!/usr/bin/env python3
"""examples/plan_to_goal.py with no privileged state and no env per candidate: random shooting on the map the agent built itself.
What each agent knows of its floor plan is a ScanMap accumulated from its lidar; per control step ONE `vec.grid_field()` gives the way
to the nearest frontier cell of that map, ONE `vec.grid_clearance()` a cost for hugging obstacles, and ONE `vec.grid_rollout()` runs
`--candidates` random plans of `--horizon` actions per env through the agent's own kinematics against the map's obstacle plane —
stopping a plan where it reaches the frontier —, scored by (the least field value met, steps + clearance cost).  The best plan's first
action is executed.  Where examples/depth_plan_explore.py follows one greedy waypoint, this policy has a model of what its moves do.

    python examples/grid_shooting.py --env MiniWorld-MazeS3-v0 --envs 256 --steps 600

The coverage is scored exactly as depth_plan_explore.py scores it, on a SeenMap and the walls' own unblocked cells, neither of which
the policy reads.  Results, not thresholds: see README.md, "Grid rollouts".
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from depth_plan_explore import frontier_of  # noqa: E402
from explore_frontier import unblocked_of  # noqa: E402


def run(args):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n, P, T = args.envs, args.candidates, args.plan
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed)
    dev = vec.engine.device
    vec.reset()
    score = vec.seen_map(cell=args.cell, max_range=args.range)          # the yardstick: never read by the policy
    vec.seen_update(score)
    yard = vec.nav_field(target=vec.state(("agent_pos",))["agent_pos"].clone(), reach=2 * args.cell, cell=args.cell)
    m = vec.scan_map(like=score, max_range=args.range)
    vec.scan_map_update(m)
    plan = clear = shot = None
    g = torch.Generator(device=dev).manual_seed(args.seed)
    rows = torch.arange(n, device=dev)
    taken, covered = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
    age, counted = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.bool, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        frontier, _ = frontier_of(m)
        blocked = (m.obstacle != 0).contiguous()
        plan = vec.grid_field(blocked, frontier, like=m) if plan is None else vec.grid_field(blocked, frontier, into=plan)
        clear = vec.grid_clearance(blocked, radii=[0.5, 1.0], costs=[8, 2], like=m) if clear is None else vec.grid_clearance(blocked, into=clear)
        plans = torch.randint(0, 3, (T, n, P), generator=g, device=dev, dtype=torch.uint8)      # turn left, turn right, forward
        shot = vec.grid_rollout(blocked, plans, field=plan, extra=clear.cost, stop_at=0, into=shot)
        best = (shot.reach.long() * (1 << 20) + (shot.steps + shot.cost).long()).argmin(1)
        _, _, term, trunc = vec.step(plans[0, rows, best].to(torch.int32))
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
    ap.add_argument("--candidates", type=int, default=256, help="random plans per env and control step")
    ap.add_argument("--plan", type=int, default=24, help="actions per plan")
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    cov, ended, dt = run(args)
    print(f"{args.env} x {args.envs}, {args.steps} steps: scan map, {args.candidates} shots of {args.plan} actions: mean coverage {cov:.3f} after {args.horizon} "
          f"steps of an episode (or at its end), over {ended} episodes ({dt:.2f} s, {dt / args.steps * 1e6:.0f} us per step)")


if __name__ == "__main__":
    main()
