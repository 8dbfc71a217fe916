#!/usr/bin/env python3
"""examples/depth_plan_explore.py with examples/expert_smooth.py's string pulling, and still no privileged state in the policy: the
free-path test is `vec.grid_raycast()` on the planner's OWN inflated obstacle plane — the cells `vec.grid_field()` blocks on the
DepthMap — where expert_smooth.py casts the privileged `vec.raycast()` at the simulator's walls.

    python examples/depth_smooth_explore.py --env MiniWorld-MazeS3-v0 --envs 256 --horizon 120 --steps 600 --compare

Per step: one multi-source `grid_field` build gives the way to the nearest frontier cell; K chained `vec.nav_query(plan, pos=waypoint)`
calls follow its descent K cells ahead; `vec.grid_raycast(blocked, direction=waypoints - agent, max_t=1)` casts a ray from the agent
to each of them over the plan's blocked cells (K rays per env: the unstaged form; hit >= 0: something is in the way on the map) — the
inflation stands for the agent's disc —; the expert of expert_nav.py is aimed at the farthest waypoint whose cast is free.  A forward
move that left the agent where it was makes the next cell's centre the aim until one succeeds again, as in expert_smooth.py.

The coverage is scored exactly as depth_plan_explore.py scores it; --compare runs that explorer on the same settings.  Results, not
thresholds: see README.md, "Grid ray casts".
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from depth_plan_explore import frontier_of  # noqa: E402
from depth_plan_explore import run as plain_run  # noqa: E402
from expert_nav import FORWARD, TURN_LEFT, expert  # noqa: E402
from explore_frontier import unblocked_of  # noqa: E402

LOOKAHEAD = 6


def run(args):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n, k = args.envs, args.lookahead
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed, want_depth=True)
    turn_step = math.radians(float(vec.engine.cfg.turn_step.default))
    dev = vec.engine.device
    vec.reset()
    score = vec.seen_map(cell=args.cell, max_range=args.range)          # the yardstick: never read by the policy
    vec.seen_update(score)
    yard = vec.nav_field(target=vec.state(("agent_pos",))["agent_pos"].clone(), reach=2 * args.cell, cell=args.cell)
    m = vec.depth_map(like=score, max_range=min(args.range, 8.0))
    vec.depth_map_update(m)
    plan = cast = None
    way, dirs = torch.zeros((n, k, 3), dtype=torch.float64, device=dev), torch.zeros((n, k, 2), dtype=torch.float64, device=dev)
    rank, rows = torch.arange(1, k + 1, device=dev), torch.arange(n, device=dev)
    stuck, last_forward = torch.zeros(n, dtype=torch.bool, device=dev), torch.zeros(n, dtype=torch.bool, device=dev)
    last_pos = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    taken, covered = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
    age, counted = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.bool, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        st = vec.state(("agent_pos", "agent_dir"))
        pos = st["agent_pos"].clone()
        frontier, _ = frontier_of(m)
        plan = vec.grid_field(m.obstacle != 0, frontier, like=m) if plan is None else vec.grid_field(m.obstacle != 0, frontier, into=plan)
        stuck = torch.where(last_forward, (pos == last_pos).all(dim=1), stuck)
        cost = vec.nav_query(plan)["cost"].clone()
        for j in range(k):              # the plan's descent, k cells ahead
            w = vec.nav_query(plan, pos=way[:, j - 1].contiguous() if j else None)["waypoint"]
            way[:, j, 0], way[:, j, 2] = w[:, 0], w[:, 1]
        dirs[:, :, 0], dirs[:, :, 1] = way[:, :, 0] - pos[:, None, 0], way[:, :, 2] - pos[:, None, 2]
        cast = vec.grid_raycast(plan.field == 0xFFFF, dirs, max_t=1.0, like=m, into=cast)      # the planner's own inflated plane
        far = ((cast["hit"] < 0) * rank).amax(dim=1) - 1            # the farthest free waypoint's index, -1: none
        target = way[rows, torch.where(stuck | (far < 0), 0, far)][:, [0, 2]]
        act = expert(pos, st["agent_dir"], target, turn_step)
        act = torch.where(cost > 0, act, TURN_LEFT).to(torch.int32)
        _, _, term, trunc = vec.step(act)
        done = (term | trunc) != 0
        last_pos, last_forward, stuck = pos, (act == FORWARD) & ~done, stuck & ~done
        free = unblocked_of(yard)
        share = ((score.seen == 1) & free).sum((1, 2)).to(torch.float64) / free.sum((1, 2)).clamp(min=1).to(torch.float64)
        early = done & ~counted
        vec.seen_update(score, clear=done)
        vec.depth_map_update(m, clear=done)
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
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lookahead", type=int, default=LOOKAHEAD, help="cells down the plan that are tried as the aim")
    ap.add_argument("--compare", action="store_true", help="run depth_plan_explore.py's explorer (no string pulling) on the same settings too")
    args = ap.parse_args()
    args.unknown = 0
    results = [(f"depth map, grid planner, string pulling over {args.lookahead} cells with grid_raycast", run(args))]
    if args.compare:
        results.append(("depth map, grid planner (depth_plan_explore.py)", plain_run(args)))
    for name, (cov, ended, dt) in results:
        print(f"{args.env} x {args.envs}, {args.steps} steps: {name}: mean coverage {cov:.3f} after {args.horizon} steps of an episode "
              f"(or at its end), over {ended} episodes ({dt:.2f} s, {dt / args.steps * 1e6:.0f} us per step)")


if __name__ == "__main__":
    main()
