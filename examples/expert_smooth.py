#!/usr/bin/env python3
"""examples/expert_nav.py's go-to-the-box expert with string pulling: instead of steering at the centre of the next cell of the
navigation field — an 8-connected staircase — the agent steers at the farthest of the next K cells down the field that it can walk
to in a straight line, and "can walk to" is one swept-disc ray cast (`vec.raycast`).  No host value in the loop.

    python examples/expert_smooth.py --env MiniWorld-MazeS3-v0 --envs 256 --steps 600

Per step: K chained `vec.nav_query(field, pos=waypoint)` calls follow the field's descent K cells ahead; `vec.raycast(direction=
waypoints - agent, max_t=1, radius=agent_radius + margin)` casts a disc from the agent to each of them (K rays per env, t < 1: something
is in the way); the expert of expert_nav.py is aimed at the farthest waypoint whose cast is free.  If a forward move left the agent
where it was (the heading is a multiple of the turn step, so the walked line is not quite the cast one), the next cell's centre is
the aim until a forward move succeeds again.  With --casts 0 the loop is expert_nav.py's; the script prints success rate and SPL
both ways.

Printed on an MI355X (seed 0, no domain randomisation, K = 6, margin 0.05):
    MiniWorld-MazeS3-v0 x 256, 600 steps, without casts: episodes ended 1928, reached the box 1922: success rate 0.997, SPL 0.956
    MiniWorld-MazeS3-v0 x 256, 600 steps, with casts: episodes ended 1924, reached the box 1919: success rate 0.997, SPL 0.958
    MiniWorld-FourRooms-v0 x 256, 600 steps, without casts: episodes ended 1651, reached the box 1651: success rate 1.000, SPL 0.963
    MiniWorld-FourRooms-v0 x 256, 600 steps, with casts: episodes ended 1648, reached the box 1648: success rate 1.000, SPL 0.964
(SPL divides by the field's own grid-metric distance and is capped at 1, and the heading moves in steps of 15 degrees: the straighter
aim shows as a thousandth or two, profiles/r24/README.md.)
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from expert_nav import FORWARD, expert  # noqa: E402

LOOKAHEAD, MARGIN = 6, 0.05


class Smoother:
    """the aim of every env's agent: the farthest free waypoint of the next `lookahead` cells down `field`"""

    def __init__(self, vec, field, lookahead=LOOKAHEAD, margin=MARGIN):
        import torch
        self.vec, self.field, self.k = vec, field, int(lookahead)
        self.radius = float(vec.engine.cfg.agent_radius) + float(margin)
        n, dev = vec.num_envs, vec.engine.device
        self.way = torch.zeros((n, self.k, 3), dtype=torch.float64, device=dev)       # (x, 0, z) of the k-th cell ahead
        self.dirs = torch.zeros((n, self.k, 2), dtype=torch.float64, device=dev)
        self.cast = None
        self.stuck = torch.zeros(n, dtype=torch.bool, device=dev)
        self.last_pos = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.last_forward = torch.zeros(n, dtype=torch.bool, device=dev)
        self.rank = torch.arange(1, self.k + 1, device=dev)

    def aim(self, agent_pos):
        """float64[N, 2]: where to steer, and the query of the agent's own cell"""
        import torch
        vec, field = self.vec, self.field
        # a forward move that went nowhere: the next cell's centre until one succeeds
        self.stuck = torch.where(self.last_forward, (agent_pos == self.last_pos).all(dim=1), self.stuck)
        first = vec.nav_query(field)
        first = {k: v.clone() for k, v in first.items()}        # (nav_query's tensors are reused by the next call)
        self.way[:, 0, 0], self.way[:, 0, 2] = first["waypoint"][:, 0], first["waypoint"][:, 1]
        for j in range(1, self.k):
            w = vec.nav_query(field, pos=self.way[:, j - 1].contiguous())["waypoint"]
            self.way[:, j, 0], self.way[:, j, 2] = w[:, 0], w[:, 1]
        self.dirs[:, :, 0] = self.way[:, :, 0] - agent_pos[:, None, 0]
        self.dirs[:, :, 1] = self.way[:, :, 2] - agent_pos[:, None, 2]
        self.cast = vec.raycast(direction=self.dirs, max_t=1.0, radius=self.radius, into=self.cast)
        free = self.cast["hit"] < 0
        far = (free * self.rank).amax(dim=1) - 1                # the farthest free waypoint's index, -1: none
        pick = torch.where(self.stuck | (far < 0), 0, far)
        target = self.way[torch.arange(vec.num_envs, device=pick.device), pick][:, [0, 2]]
        return target, first

    def moved(self, agent_pos, act, done):
        """after the step: what the next aim() compares with (an env that finished starts afresh)"""
        self.last_pos = agent_pos.clone()
        self.last_forward = (act == FORWARD) & ~done
        self.stuck = self.stuck & ~done


def run(env_id, n, steps, cell, casts, lookahead, margin, seed):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    vec = MiniWorldVecEnv(env_id, n, seed=seed)
    turn_step = math.radians(float(vec.engine.cfg.turn_step.default))
    vec.reset()
    field = vec.nav_field(cell=cell)
    sm = Smoother(vec, field, lookahead, margin) if casts else None
    dev = vec.engine.device
    start = torch.ones(n, dtype=torch.bool, device=dev)
    shortest = torch.zeros(n, dtype=torch.float32, device=dev)
    walked = torch.zeros(n, dtype=torch.float64, device=dev)
    ended, reached, spl = (torch.zeros((), dtype=torch.float64, device=dev) for _ in range(3))
    for _ in range(steps):
        st = vec.state(("agent_pos", "agent_dir"))
        pos, heading = st["agent_pos"].clone(), st["agent_dir"].clone()
        if sm:
            target, q = sm.aim(pos)
        else:
            q = vec.nav_query(field)
            target = q["waypoint"]
        shortest = torch.where(start, q["distance"], shortest)
        walked = torch.where(start, 0.0, walked)
        act = expert(pos, heading, target, turn_step)
        _, _, term, trunc = vec.step(act)
        done = (term | trunc) != 0
        after = vec.state(("agent_pos",))["agent_pos"]
        if sm:
            sm.moved(after, act, done)
        step_len = (after - pos)[:, [0, 2]].norm(dim=1)
        walked = walked + torch.where(done, (act == FORWARD).to(torch.float64) * float(vec.engine.cfg.forward_step.default), step_len)
        ok = done & (term != 0)
        ended += done.sum()
        reached += ok.sum()
        spl += torch.where(ok, shortest.to(torch.float64) / torch.maximum(walked, shortest.to(torch.float64)).clamp(min=1e-9), 0.0).sum()
        vec.nav_field(into=field, mask=done)
        start = done
    torch.cuda.synchronize()
    vec.engine.check()
    out = (int(ended), int(reached), float(reached / ended.clamp(min=1)), float(spl / ended.clamp(min=1)))
    vec.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default=None, help="default: MazeS3 and FourRooms")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--lookahead", type=int, default=LOOKAHEAD)
    ap.add_argument("--margin", type=float, default=MARGIN)
    ap.add_argument("--casts", type=int, default=None, help="1: with the casts only, 0: without only; default both")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    for env_id in [args.env] if args.env else ["MiniWorld-MazeS3-v0", "MiniWorld-FourRooms-v0"]:
        for casts in [bool(args.casts)] if args.casts is not None else [False, True]:
            ended, reached, rate, spl = run(env_id, args.envs, args.steps, args.cell, casts, args.lookahead, args.margin, args.seed)
            print(f"{env_id} x {args.envs}, {args.steps} steps, {'with' if casts else 'without'} casts: episodes ended {ended}, "
                  f"reached the box {reached}: success rate {rate:.3f}, SPL {spl:.3f}")


if __name__ == "__main__":
    main()
