#!/usr/bin/env python3
"""examples/explore_frontier.py with the map a sensor gives in the place of the privileged one: what each agent knows of its floor plan
is a DepthMap (`vec.depth_map()`, `vec.depth_map_update()`), accumulated on the device from the depth maps the env draws — every pixel
unprojected with the env's own camera, floor points marking cells free, points up to the agent's height marking them obstacles.  The
frontier is the free cells beside cells that are neither free nor obstacle; the way there is still a privileged navigation field
(`vec.nav_field()`), and the follower is the turn-or-forward rule of examples/expert_nav.py.

    python examples/depth_explore.py --env MiniWorld-MazeS3-v0 --envs 256 --horizon 120 --steps 600

The coverage is scored exactly as explore_frontier.py scores it, on a SeenMap that the policy never reads, so the three figures —
this explorer, the privileged frontier explorer, a uniform-random policy — stand on one footing.  Results, not thresholds: see README.md,
"Depth projection".
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from expert_nav import TURN_LEFT, expert  # noqa: E402
from explore_frontier import run as privileged_run, unblocked_of  # noqa: E402


def depth_frontier_targets(m, from_agent, extent):
    """the cheapest frontier cell of every env under a DepthMap: (float64[N, 3] its centre, bool[N] whether there is one)"""
    import torch
    from miniworld_amd import engine
    cost = from_agent.field.view(torch.int16).to(torch.int32) & 0xFFFF
    free = m.free == 1
    unknown = (m.free == 0) & (m.obstacle == 0)
    beside = torch.zeros_like(unknown)
    beside[:, 1:, :] |= unknown[:, :-1, :]
    beside[:, :-1, :] |= unknown[:, 1:, :]
    beside[:, :, 1:] |= unknown[:, :, :-1]
    beside[:, :, :-1] |= unknown[:, :, 1:]
    frontier = free & beside & (cost < engine.NAV_UNREACHED)
    n = cost.shape[0]
    best, at = torch.where(frontier, cost, 1 << 20).reshape(n, -1).min(dim=1)
    j, i = at // m.gx, at % m.gx
    centre = torch.zeros((n, 3), dtype=torch.float64, device=cost.device)
    centre[:, 0] = extent[:, 0] + (i.to(torch.float64) + 0.5) * m.cell
    centre[:, 2] = extent[:, 2] + (j.to(torch.float64) + 0.5) * m.cell
    return centre, best < (1 << 20)


def run(args):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n = args.envs
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed, want_depth=True)
    turn_step = math.radians(float(vec.engine.cfg.turn_step.default))
    dev = vec.engine.device
    vec.reset()
    score = vec.seen_map(cell=args.cell, max_range=args.range)          # the yardstick: never read by the policy
    vec.seen_update(score)
    m = vec.depth_map(like=score, max_range=min(args.range, 8.0))
    vec.depth_map_update(m)
    taken, covered = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
    age = torch.zeros(n, dtype=torch.int32, device=dev)
    counted = torch.zeros(n, dtype=torch.bool, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        st = vec.state(("agent_pos", "agent_dir", "extent"))
        from_agent = vec.nav_field(target=st["agent_pos"].clone(), reach=2 * args.cell, cell=args.cell)
        free = unblocked_of(from_agent)
        target, has = depth_frontier_targets(m, from_agent, st["extent"])
        q = vec.nav_query(vec.nav_field(target=target, reach=args.cell, cell=args.cell))
        act = expert(st["agent_pos"], st["agent_dir"], q["waypoint"], turn_step)
        act = torch.where(has & (q["cost"] > 0), act, TURN_LEFT).to(torch.int32)
        _, _, term, trunc = vec.step(act)
        done = (term | trunc) != 0
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
    args = ap.parse_args()
    results = [("depth map", run(args))] + [(name, privileged_run(args, policy)) for name, policy in (("seen map (privileged)", "frontier"), ("random", "random"))]
    for name, (cov, ended, dt) in results:
        print(f"{args.env} x {args.envs}, {args.steps} steps: {name}: mean coverage {cov:.3f} after {args.horizon} steps of an episode "
              f"(or at its end), over {ended} episodes ({dt:.2f} s)")


if __name__ == "__main__":
    main()
