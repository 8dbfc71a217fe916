#!/usr/bin/env python3
"""examples/depth_explore.py with no privileged state left in the policy: sensor, map, planner on the sensed map, follower, all on the
device.  What each agent knows of its floor plan is a DepthMap accumulated from the depth frames the env draws; the planner is
`vec.grid_field()` over that map — `blocked` the map's obstacle plane, inflated by the agent's radius and half a cell, `sources` the
frontier mask (the free cells beside cells that are neither free nor obstacle) — so that ONE multi-source build gives the way to the
nearest frontier cell and ONE `vec.nav_query()` the waypoint, where depth_explore.py spends two privileged whole-batch builds and an
arg-min per step.  The follower is the turn-or-forward rule of examples/expert_nav.py.

    python examples/depth_plan_explore.py --env MiniWorld-MazeS3-v0 --envs 256 --horizon 120 --steps 600

Cells the map has not seen are either walked through at no extra cost (`--unknown 0`, optimistic: the default, and the one the README's
figure is for) or at `--unknown K` more per cell (cautious: paths prefer what has been seen).  Blocking them outright is no option
with one occupancy grid: a frontier cell lies beside unknown cells by definition and would fall inside their inflation.

The coverage is scored exactly as depth_explore.py scores it, on a SeenMap and the walls' own unblocked cells, neither of which the
policy reads.  Results, not thresholds: see README.md, "Grid navigation fields".
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from expert_nav import TURN_LEFT, expert  # noqa: E402
from explore_frontier import unblocked_of  # noqa: E402


def frontier_of(m):
    """(bool[N, gz, gx] the frontier of a DepthMap: its free cells beside unknown ones, bool[N, gz, gx] the unknown cells)"""
    import torch
    unknown = (m.free == 0) & (m.obstacle == 0)
    beside = torch.zeros_like(unknown)
    beside[:, 1:, :] |= unknown[:, :-1, :]
    beside[:, :-1, :] |= unknown[:, 1:, :]
    beside[:, :, 1:] |= unknown[:, :, :-1]
    beside[:, :, :-1] |= unknown[:, :, 1:]
    return (m.free == 1) & beside, unknown


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
    # ... and the cells no wall blocks, which the score is a share of: a privileged field kept current behind the resets, for the score alone
    yard = vec.nav_field(target=vec.state(("agent_pos",))["agent_pos"].clone(), reach=2 * args.cell, cell=args.cell)
    m = vec.depth_map(like=score, max_range=min(args.range, 8.0))
    vec.depth_map_update(m)
    plan = None
    taken, covered = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
    age = torch.zeros(n, dtype=torch.int32, device=dev)
    counted = torch.zeros(n, dtype=torch.bool, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        st = vec.state(("agent_pos", "agent_dir"))
        frontier, unknown = frontier_of(m)
        extra = unknown.to(torch.uint8) * args.unknown if args.unknown else None
        plan = vec.grid_field(m.obstacle != 0, frontier, extra=extra, like=m) if plan is None else vec.grid_field(m.obstacle != 0, frontier, extra=extra, into=plan)
        q = vec.nav_query(plan)
        act = expert(st["agent_pos"], st["agent_dir"], q["waypoint"], turn_step)
        act = torch.where(q["cost"] > 0, act, TURN_LEFT).to(torch.int32)
        _, _, term, trunc = vec.step(act)
        done = (term | trunc) != 0
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
    ap.add_argument("--unknown", type=int, default=0, help="extra cost 0 .. 255 of a cell the map has not seen (0: optimistic)")
    ap.add_argument("--compare", action="store_true", help="run depth_explore.py's explorer (privileged planner) on the same settings too")
    args = ap.parse_args()
    if not 0 <= args.unknown <= 255:
        ap.error("--unknown is a cost 0 .. 255")
    results = [(f"depth map, grid planner (unknown cells + {args.unknown})", run(args))]
    if args.compare:
        from depth_explore import run as privileged_plan_run
        results.append(("depth map, privileged planner", privileged_plan_run(args)))
    for name, (cov, ended, dt) in results:
        print(f"{args.env} x {args.envs}, {args.steps} steps: {name}: mean coverage {cov:.3f} after {args.horizon} steps of an episode "
              f"(or at its end), over {ended} episodes ({dt:.2f} s, {dt / args.steps * 1e6:.0f} us per step)")


if __name__ == "__main__":
    main()
