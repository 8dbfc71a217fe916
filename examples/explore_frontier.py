#!/usr/bin/env python3
"""A frontier explorer for any GOTO env id — MazeS3, FourRooms, the T- and Y-mazes — without a host value in the loop: what each agent
has seen so far is a map on the device (`vec.seen_map()`, `vec.seen_update()`), the frontier a few tensor operations on it, the way
there a navigation field (`vec.nav_field()`, `vec.nav_query()`) and the follower the turn-or-forward rule of examples/expert_nav.py.

    python examples/explore_frontier.py --env MiniWorld-MazeS3-v0 --envs 256 --horizon 120 --steps 600

Per step: a field built from each agent's own position gives the cost to every cell; the frontier is the cells that are seen, not
blocked (MW_NAV_BLOCKED in that field) and have an unseen unblocked 4-neighbour; the cheapest of them is the env's target, a second
field leads to its centre, one `nav_query` gives the waypoint, the follower the action; then the step and `seen_update(m, clear=done)`.
An env without a reachable frontier turns on the spot.  The coverage of an episode — seen unblocked cells over unblocked cells — is
taken after `--horizon` of its steps, or when it ends if that comes first (reaching the box ends one; the map then is the one from
before its last step), summed in torch and read once at the end, for the explorer and for a uniform-random policy under the same rule.

Printed on an MI355X (seed 0, 256 envs, horizon 120, 600 steps; results, not thresholds): see README.md, "Explored-area maps".
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from expert_nav import TURN_LEFT, expert  # noqa: E402


def unblocked_of(field):
    """bool[N, gz, gx]: the cells of a NavField that no wall blocks"""
    import torch
    from miniworld_amd import engine
    return (field.field.view(torch.int16).to(torch.int32) & 0xFFFF) != engine.NAV_BLOCKED


def frontier_targets(seen, from_agent, extent):
    """the cheapest frontier cell of every env: (float64[N, 3] its centre, bool[N] whether there is one).  `from_agent` is a NavField
    whose target is the agent's own position: its costs are the agent's way to every cell."""
    import torch
    from miniworld_amd import engine
    cost = from_agent.field.view(torch.int16).to(torch.int32) & 0xFFFF
    free = cost != engine.NAV_BLOCKED
    known = (seen.seen == 1) & free
    unknown = (seen.seen == 0) & free
    beside = torch.zeros_like(unknown)
    beside[:, 1:, :] |= unknown[:, :-1, :]
    beside[:, :-1, :] |= unknown[:, 1:, :]
    beside[:, :, 1:] |= unknown[:, :, :-1]
    beside[:, :, :-1] |= unknown[:, :, 1:]
    frontier = known & beside & (cost < engine.NAV_UNREACHED)
    n = cost.shape[0]
    best, at = torch.where(frontier, cost, 1 << 20).reshape(n, -1).min(dim=1)
    j, i = at // seen.gx, at % seen.gx
    centre = torch.zeros((n, 3), dtype=torch.float64, device=cost.device)
    centre[:, 0] = extent[:, 0] + (i.to(torch.float64) + 0.5) * seen.cell
    centre[:, 2] = extent[:, 2] + (j.to(torch.float64) + 0.5) * seen.cell
    return centre, best < (1 << 20)


def run(args, policy):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n = args.envs
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed)
    turn_step = math.radians(float(vec.engine.cfg.turn_step.default))
    dev = vec.engine.device
    vec.reset()
    m = vec.seen_map(cell=args.cell, max_range=args.range)
    vec.seen_update(m)
    g = torch.Generator(device=dev).manual_seed(args.seed)
    taken, covered = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
    age = torch.zeros(n, dtype=torch.int32, device=dev)             # steps of the env's episode so far
    counted = torch.zeros(n, dtype=torch.bool, device=dev)          # the episode's coverage has been taken
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        st = vec.state(("agent_pos", "agent_dir", "extent"))
        from_agent = vec.nav_field(target=st["agent_pos"].clone(), reach=2 * args.cell, cell=args.cell)
        free = unblocked_of(from_agent)
        if policy == "frontier":
            target, has = frontier_targets(m, from_agent, st["extent"])
            q = vec.nav_query(vec.nav_field(target=target, reach=args.cell, cell=args.cell))
            act = expert(st["agent_pos"], st["agent_dir"], q["waypoint"], turn_step)
            act = torch.where(has & (q["cost"] > 0), act, TURN_LEFT).to(torch.int32)
        else:
            act = torch.randint(0, 3, (n,), generator=g, device=dev, dtype=torch.int32)
        _, _, term, trunc = vec.step(act)
        done = (term | trunc) != 0
        # an episode that just ended is counted on the floor plan it was played on: `free` and the map are from before the step (a
        # finished env holds its next world already); one that reaches the horizon with this step is counted behind the update
        share = ((m.seen == 1) & free).sum((1, 2)).to(torch.float64) / free.sum((1, 2)).clamp(min=1).to(torch.float64)
        early = done & ~counted
        vec.seen_update(m, clear=done)
        age = torch.where(done, 0, age + 1)
        due = ~done & ~counted & (age == args.horizon)
        now = ((m.seen == 1) & free).sum((1, 2)).to(torch.float64) / free.sum((1, 2)).clamp(min=1).to(torch.float64)
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
    for policy in ("frontier", "random"):
        cov, ended, dt = run(args, policy)
        print(f"{args.env} x {args.envs}, {args.steps} steps: {policy}: mean coverage {cov:.3f} after {args.horizon} steps of an episode "
              f"(or at its end), over {ended} episodes ({dt:.2f} s)")


if __name__ == "__main__":
    main()
