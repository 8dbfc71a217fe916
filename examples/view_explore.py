#!/usr/bin/env python3
"""examples/depth_plan_explore.py with the goal chosen by what the agent would SEE there, not by what is nearest: next-best-view
exploration with no privileged state in the policy and no host value in the loop.  Sensor, map, planner and follower are
depth_plan_explore.py's — a DepthMap accumulated from the depth frames, `vec.grid_field()` over it, the turn-or-forward rule —; what
is new is the choice of the frontier cell to walk to.  Per env, V frontier cells are sampled on the device;
`vec.grid_sight(m.obstacle != 0, cells, weight=unknown)` gives, for each, how many unknown cells lie in line of sight of it on the
agent's own map; a `grid_field` sourced at the agent gives the path cost to each; the goal is the candidate with the most gain per
metre of path (`--bias` metres added, so that a cell underfoot does not win with nothing to show), held for `--hold` steps or until
it is reached.  An env without a reachable candidate walks to the nearest frontier cell, as depth_plan_explore.py does.

    python examples/view_explore.py --env MiniWorld-MazeS3-v0 --envs 256 --horizon 120 --steps 600 --compare

The coverage is scored exactly as depth_plan_explore.py scores it, on a SeenMap and the walls' own unblocked cells, neither of which
the policy reads.  Results, not thresholds: see README.md, "Grid sight".
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


def sample_cells(mask, views, generator):
    """int32[N, views]: up to `views` distinct cells of each env's bool[N, gz, gx] mask, uniformly, as flat indices; -1 where the mask
    has fewer — on the device: a random key per cell, the mask's largest"""
    import torch
    n = mask.shape[0]
    flat = mask.reshape(n, -1)
    key = torch.rand(flat.shape, generator=generator, device=mask.device).masked_fill_(~flat, -1.0)
    top, idx = key.topk(min(views, flat.shape[1]), dim=1)
    return torch.where(top >= 0, idx, -1).to(torch.int32).contiguous()


def run(args, candidates=None):
    """`candidates(vec, m, frontier)`: int32[N, V] flat cells (-1: none) in place of the sampled ones (examples/cluster_explore.py)"""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n = args.envs
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed, want_depth=True)
    turn_step = math.radians(float(vec.engine.cfg.turn_step.default))
    dev = vec.engine.device
    vec.reset()
    score = vec.seen_map(cell=args.cell, max_range=args.range)          # the yardstick: never read by the policy
    vec.seen_update(score)
    yard = vec.nav_field(target=vec.state(("agent_pos",))["agent_pos"].clone(), reach=2 * args.cell, cell=args.cell)    # (for the score alone)
    m = vec.depth_map(like=score, max_range=min(args.range, 8.0))
    vec.depth_map_update(m)
    cells_per_env = m.gx * m.gz
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    goal = torch.full((n,), -1, dtype=torch.int64, device=dev)         # the held goal cell, -1: none (walk to the nearest frontier)
    held = torch.zeros(n, dtype=torch.int32, device=dev)
    rows = torch.arange(n, device=dev)
    here = plan = None
    taken, covered = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
    age = torch.zeros(n, dtype=torch.int32, device=dev)
    counted = torch.zeros(n, dtype=torch.bool, device=dev)
    chosen = torch.zeros((), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        st = vec.state(("agent_pos", "agent_dir"))
        frontier, unknown = frontier_of(m)
        opaque = m.obstacle != 0
        # the candidates, what each would see, and what the way there costs
        cells = candidates(vec, m, frontier) if candidates else sample_cells(frontier, args.views, gen)
        gain = vec.grid_sight(opaque, cells, weight=unknown, max_range=args.sight, like=m)
        pos = st["agent_pos"].clone()
        if here is None:
            here = vec.grid_field(opaque, target=pos, reach=2 * args.cell, like=m)
        else:
            here.target.copy_(pos)
            vec.grid_field(opaque, into=here)
        at = cells.clamp(min=0).to(torch.int64)
        cost = (here.field.view(torch.int16).reshape(n, -1).gather(1, at).to(torch.int32) & 0xFFFF)
        ok = (cells >= 0) & (cost < 0xFFFE)
        metres = cost.to(torch.float32) * (args.cell / 5.0)
        value = torch.where(ok, gain.to(torch.float32) / (metres + args.bias), -1.0)
        best = value.argmax(dim=1)
        pick = torch.where(value[rows, best] > 0, at[rows, best], -1)
        # a goal is held until it is reached, stops being a frontier cell's neighbourhood of unknowns (its gain is spent), or --hold steps pass
        spent = (goal < 0) | (held >= args.hold) | ~frontier.reshape(n, -1).gather(1, goal.clamp(min=0)[:, None])[:, 0]
        goal = torch.where(spent, pick, goal)
        held = torch.where(spent, 0, held + 1)
        chosen += (goal >= 0).sum()
        sources = torch.zeros((n, cells_per_env), dtype=torch.bool, device=dev)
        sources[rows, goal.clamp(min=0)] = goal >= 0
        sources = torch.where((goal >= 0)[:, None], sources, frontier.reshape(n, -1)).reshape(frontier.shape)
        plan = vec.grid_field(opaque, sources, like=m) if plan is None else vec.grid_field(opaque, sources, into=plan)
        q = vec.nav_query(plan)
        goal = torch.where(q["cost"] > 0, goal, -1)         # reached, or no way: choose again
        act = expert(st["agent_pos"], st["agent_dir"], q["waypoint"], turn_step)
        act = torch.where(q["cost"] > 0, act, TURN_LEFT).to(torch.int32)
        _, _, term, trunc = vec.step(act)
        done = (term | trunc) != 0
        free = unblocked_of(yard)
        share = ((score.seen == 1) & free).sum((1, 2)).to(torch.float64) / free.sum((1, 2)).clamp(min=1).to(torch.float64)
        early = done & ~counted
        vec.seen_update(score, clear=done)
        vec.depth_map_update(m, clear=done)
        goal = torch.where(done, -1, goal)
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
    return float(covered / taken.clamp(min=1)), int(taken), dt, float(chosen) / (n * args.steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-MazeS3-v0")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--horizon", type=int, default=120, help="steps of an episode after which its coverage is taken")
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--views", type=int, default=32, help="frontier cells sampled per env and step, 1 .. engine.SIGHT_MAX_VIEWS")
    ap.add_argument("--sight", type=float, default=3.0, help="how far a candidate is taken to see, in metres")
    ap.add_argument("--bias", type=float, default=1.0, help="metres added to a candidate's path length before the gain is divided by it")
    ap.add_argument("--hold", type=int, default=12, help="steps a goal is kept at the most")
    ap.add_argument("--unknown", type=int, default=0, help=argparse.SUPPRESS)       # (depth_plan_explore.run reads it under --compare)
    ap.add_argument("--compare", action="store_true", help="run depth_plan_explore.py (nearest frontier) and explore_frontier.py (privileged) on the same settings too")
    args = ap.parse_args()
    cov, ended, dt, share = run(args)
    print(f"{args.env} x {args.envs}, {args.steps} steps: depth map, goal by gain per metre ({args.views} candidates, sight {args.sight} m): mean coverage "
          f"{cov:.3f} after {args.horizon} steps of an episode (or at its end), over {ended} episodes ({dt:.2f} s, {dt / args.steps * 1e6:.0f} us per step; "
          f"a goal by gain was held in {share:.2f} of the env-steps)")
    if args.compare:
        from depth_plan_explore import run as nearest_run
        for name, (cov, ended, dt) in (("depth map, nearest frontier", nearest_run(args)),):
            print(f"{args.env} x {args.envs}, {args.steps} steps: {name}: mean coverage {cov:.3f} over {ended} episodes ({dt / args.steps * 1e6:.0f} us per step)")


if __name__ == "__main__":
    main()
