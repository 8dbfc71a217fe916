#!/usr/bin/env python3
"""A wall-aware go-to-the-box expert for any GOTO env id — Maze, FourRooms, TMaze, YMaze, WallGap, Sidewalk, Hallway, OneRoom —
without a host value in the loop: the shortest-path cost to the box is a field on the device (`vec.nav_field()`), the agent's next
waypoint a query into it (`vec.nav_query()`), and the expert the turn-or-forward rule of examples/expert_demos.py aimed at the
waypoint instead of at the box.

    python examples/expert_nav.py --env MiniWorld-MazeS3-v0 --envs 256 --steps 600

Per step: `vec.nav_field(into=field, mask=done)` rebuilds the field of the envs whose episode just ended (the Maze draws a new floor
plan every episode; a fixed floor plan still gets a new box), `vec.nav_query(field)` returns cost and waypoint for every agent, and a
dozen tensor operations turn the waypoint into an action.  Success rate and SPL (success weighted by shortest length over path
length; the shortest length is the field's distance at each episode's first step, the path length is summed from `vec.state()`) are
accumulated in torch and read once at the end.

Printed on an MI355X (seed 0, no domain randomisation):
    MiniWorld-MazeS3-v0 x 256, 600 steps: episodes ended 1928, reached the box 1922: success rate 0.997, SPL 0.956
    MiniWorld-FourRooms-v0 x 256, 600 steps: episodes ended 1651, reached the box 1651: success rate 1.000, SPL 0.963
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

TURN_LEFT, TURN_RIGHT, FORWARD = 0, 1, 2


def expert(agent_pos, agent_dir, waypoint, turn_step):
    """int32[N] actions: turn towards the waypoint (float64[N, 2]: x, z) while it is more than half a turn step off, else move forward
    (the agent looks along (cos dir, 0, -sin dir), entity.py:70-79)"""
    import torch
    want = torch.atan2(-(waypoint[:, 1] - agent_pos[:, 2]), waypoint[:, 0] - agent_pos[:, 0])
    off = torch.remainder(want - agent_dir + math.pi, 2 * math.pi) - math.pi       # in -pi .. pi, positive = to the left
    act = torch.where(off > 0, TURN_LEFT, TURN_RIGHT)
    return torch.where(off.abs() <= turn_step / 2, FORWARD, act).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-MazeS3-v0")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--obstacles", default="walls", choices=["walls", "walls+entities"])
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv

    n = args.envs
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed)
    turn_step = math.radians(float(vec.engine.cfg.turn_step.default))
    vec.reset()
    field = vec.nav_field(cell=args.cell, obstacles=args.obstacles)
    dev = vec.engine.device
    start = torch.ones(n, dtype=torch.bool, device=dev)             # the env's episode begins with this step
    shortest = torch.zeros(n, dtype=torch.float32, device=dev)
    walked = torch.zeros(n, dtype=torch.float64, device=dev)
    ended, reached, spl = (torch.zeros((), dtype=torch.float64, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        st = vec.state(("agent_pos", "agent_dir"))
        q = vec.nav_query(field)
        shortest = torch.where(start, q["distance"], shortest)
        walked = torch.where(start, 0.0, walked)
        before = st["agent_pos"].clone()
        act = expert(st["agent_pos"], st["agent_dir"], q["waypoint"], turn_step)
        _, _, term, trunc = vec.step(act)
        done = (term | trunc) != 0
        # (an env that finished holds its next episode's state already: its last move is at most one forward step, counted as one)
        moved = (vec.state(("agent_pos",))["agent_pos"] - before)[:, [0, 2]].norm(dim=1)
        walked = walked + torch.where(done, (act == FORWARD).to(torch.float64) * float(vec.engine.cfg.forward_step.default), moved)
        ok = done & (term != 0)
        ended += done.sum()
        reached += ok.sum()
        spl += torch.where(ok, shortest.to(torch.float64) / torch.maximum(walked, shortest.to(torch.float64)).clamp(min=1e-9), 0.0).sum()
        vec.nav_field(into=field, mask=done)
        start = done
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    vec.engine.check()
    print(f"{args.env} x {n}, {args.steps} steps in {dt:.2f} s ({n * args.steps / dt / 1e6:.3f} M env-steps/s)")
    print(f"episodes ended {int(ended)}, reached the box {int(reached)}: success rate {float(reached / ended.clamp(min=1)):.3f}, "
          f"SPL {float(spl / ended.clamp(min=1)):.3f}")
    vec.close()


if __name__ == "__main__":
    main()
