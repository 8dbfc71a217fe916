#!/usr/bin/env python3
"""An explorer that looks at nothing but its egocentric map window, without a host value in the loop: per step one
`vec.ego_update(w, source=seen_map)` gives the wall plane and the crop of the explored-area map around each agent, turned with its
heading; the agent turns towards the sector of the window — left, ahead, right — that holds the most unseen, unwalled points, and walks
when that is the one ahead and no wall stands right in front of it.  No navigation field, no ray cast, no global map in the policy.

    python examples/ego_explore.py --env MiniWorld-MazeS3-v0 --envs 256 --horizon 120 --steps 240

Coverage is measured as in examples/explore_frontier.py — seen unblocked cells over unblocked cells after `--horizon` steps of an
episode, or when it ends if that comes first — and printed beside a uniform-random policy and that frontier explorer under the same
rule (the navigation field the measurement takes its unblocked cells from is no input of the policy).

Printed on an MI355X (seed 0, 256 envs, horizon 120; results, not thresholds): see README.md, "Egocentric map windows".
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import explore_frontier as frontier  # noqa: E402
from expert_nav import TURN_LEFT  # noqa: E402

TURN_RIGHT, FORWARD = 1, 2


def ego_policy(wall, sample, last):
    """int32[N] actions from the wall plane and the seen map's crop, both uint8[N, S, S] in the heading frame, the agent at the centre;
    `last`: the actions of the step before — an agent that is turning keeps its direction until it walks again, so that it cannot
    dither between left and right"""
    import torch
    S = wall.shape[1]
    mid, third = S // 2, S // 3
    unknown = ((sample == 0) & (wall == 0))[:, :mid + 1]          # the rows from the farthest ahead to the agent's own
    left = unknown[:, :, :third].sum((1, 2))
    ahead = unknown[:, :, third:S - third].sum((1, 2))
    right = unknown[:, :, S - third:].sum((1, 2))
    blocked = (wall[:, mid - 3:mid, mid - 1:mid + 2] != 0).any(2).any(1)          # a wall within three points straight ahead
    side = torch.where(last == FORWARD, torch.where(left >= right, TURN_LEFT, TURN_RIGHT), last)
    go = (ahead >= left) & (ahead >= right) & (ahead > 0) & ~blocked
    nothing = (left + ahead + right) == 0           # all seen in front: walk on unless a wall is there, else turn round
    act = torch.where(go | (nothing & ~blocked), FORWARD, side)
    return act.to(torch.int32)


def run(args, policy):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n = args.envs
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed)
    dev = vec.engine.device
    vec.reset()
    m = vec.seen_map(cell=args.cell, max_range=args.range)
    vec.seen_update(m)
    w = vec.ego_window(size=args.size, cell=args.cell, planes=("wall",))
    g = torch.Generator(device=dev).manual_seed(args.seed)
    taken, covered = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
    age = torch.zeros(n, dtype=torch.int32, device=dev)
    counted = torch.zeros(n, dtype=torch.bool, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    act = torch.full((n,), FORWARD, dtype=torch.int32, device=dev)
    for t in range(args.steps):
        if policy == "ego":
            planes, sample = vec.ego_update(w, source=m, fill=1)          # (outside the map nothing is left to see)
            act = ego_policy(planes[:, 0], sample, act)
        else:
            act = torch.randint(0, 3, (n,), generator=g, device=dev, dtype=torch.int32)
        # the measurement, not the policy: the floor plan's unblocked cells, as examples/explore_frontier.py counts them
        pos = vec.state(("agent_pos",))["agent_pos"].clone()
        free = frontier.unblocked_of(vec.nav_field(target=pos, reach=2 * args.cell, cell=args.cell))
        _, _, term, trunc = vec.step(act)
        done = (term | trunc) != 0
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
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--horizon", type=int, default=120, help="steps of an episode after which its coverage is taken")
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--size", type=int, default=33, help="points along a side of the window")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    for policy in ("ego", "random", "frontier"):
        cov, ended, dt = frontier.run(args, policy) if policy == "frontier" else run(args, policy)
        print(f"{args.env} x {args.envs}, {args.steps} steps: {policy}: mean coverage {cov:.3f} after {args.horizon} steps of an episode "
              f"(or at its end), over {ended} episodes ({dt:.2f} s)", flush=True)


if __name__ == "__main__":
    main()
