#!/usr/bin/env python3
"""A go-to-the-box agent with no privileged state in the policy: examples/depth_plan_explore.py's explorer until the goal has been SEEN,
then a planner to where it was seen.  Everything the policy reads is a sensor image or a map built from sensor images, on the device:

    per step   vec.label_update(labels)                     which entity slot each pixel shows (meshes="bounds")
               vec.depth_map_update(depth_map)              free and obstacle cells from the depth frame
               vec.object_map_update(object_map, labels)    the slot sensed in each cell; cells[:, goal] and pos[:, goal]
    exploring  while object_map.cells[:, goal] == 0: one vec.grid_field() to the nearest frontier of the depth map, as depth_plan_explore.py
    going      afterwards: vec.grid_field(blocked=depth_map.obstacle, target=object_map.pos[:, goal], reach=...) and vec.nav_query()

The goal SLOT is the task (cfg.goal_ent: "go to the red box" names it), not state; where that slot is comes from the object map alone.

How `reach` is chosen.  The goal is an obstacle on the depth map, and grid_field() inflates it by agent_radius + cell / 2 like every
obstacle: the goal's sensed position lies inside blocked cells, and point sources are only marked on unblocked ones.  Every sensed cell of
the goal has its centre within r + d of the goal's own centre (r the goal's radius, d = cell * sqrt(2) / 2: the object-map tests'
statement), and so has their centroid `pos`; the goal's obstacle cells therefore lie within 2 (r + d) of `pos` and the cells they block
within 2 (r + d) + inflate.  reach = 2 (r + d) + inflate + cell reaches one cell past that, so at least the ring of free cells around the
blocked blob holds sources (--goal-radius: the task's box, 0.8 m a side, has r = 0.566).  The planner brings the agent to the nearest
source cell; from there (cost 0) the follower aims at `pos` itself, and the episode ends when the env's own near() test holds.  What
this costs: a goal sensed through a doorway may have its sources on the far side of the wall, where the final approach runs into it.

    python examples/label_goto.py --env MiniWorld-FourRooms-v0 --envs 256 --steps 600
    python examples/label_goto.py --env MiniWorld-FourRooms-v0 --policy random          # the floor: uniform-random actions

Success rate and SPL are scored as examples/expert_nav.py scores them (the ceiling: the same follower on the privileged field), on a
privileged nav field that the policy never reads.  Results, not thresholds: see README.md, "Object maps".
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from depth_plan_explore import frontier_of  # noqa: E402
from expert_nav import FORWARD, TURN_LEFT, expert  # noqa: E402


def run(args):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n = args.envs
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed, want_depth=True)
    cfg = vec.engine.cfg
    goal = int(cfg.goal_ent)
    if goal < 0:
        raise SystemExit(f"{args.env} has no goal entity")
    turn_step = math.radians(float(cfg.turn_step.default))
    dev = vec.engine.device
    vec.reset()
    inflate = float(cfg.agent_radius) + args.cell / 2
    reach = args.reach if args.reach is not None else 2 * (args.goal_radius + args.cell * math.sqrt(2) / 2) + inflate + args.cell
    yard = vec.nav_field(cell=args.cell)             # the yardstick of the score: never read by the policy
    labels = vec.label_frame(meshes="bounds")
    depth_map = vec.depth_map(cell=args.cell)
    object_map = vec.object_map(like=depth_map)
    goal_pos = torch.zeros((n, 3), dtype=torch.float64, device=dev)      # where the goal was sensed; the agent's own place before that
    explore = go = None
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    start = torch.ones(n, dtype=torch.bool, device=dev)
    done = None
    shortest = torch.zeros(n, dtype=torch.float32, device=dev)
    walked = torch.zeros(n, dtype=torch.float64, device=dev)
    ended, reached, spl, found_steps = (torch.zeros((), dtype=torch.float64, device=dev) for _ in range(4))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        st = vec.state(("agent_pos", "agent_dir"))
        pos, direction = st["agent_pos"].clone(), st["agent_dir"].clone()
        shortest = torch.where(start, vec.nav_query(yard)["distance"], shortest)
        walked = torch.where(start, 0.0, walked)
        if args.policy == "random":
            act = torch.randint(0, 3, (n,), generator=gen, device=dev, dtype=torch.int32)
        else:
            vec.label_update(labels)
            vec.depth_map_update(depth_map, clear=done)
            vec.object_map_update(object_map, labels, clear=done)
            found = object_map.cells[:, goal] > 0
            found_steps += found.sum()
            goal_pos.copy_(torch.where(found[:, None], object_map.pos[:, goal], pos))
            blocked = depth_map.obstacle != 0
            frontier, _ = frontier_of(depth_map)
            explore = vec.grid_field(blocked, frontier, like=depth_map) if explore is None else vec.grid_field(blocked, frontier, into=explore)
            q = vec.nav_query(explore)
            e_cost, e_way = q["cost"].clone(), q["waypoint"].clone()
            go = vec.grid_field(blocked, target=goal_pos, reach=reach, like=depth_map) if go is None else vec.grid_field(blocked, into=go)
            q = vec.nav_query(go)
            going = found & (q["cost"] >= 0)
            # in a source cell the planner has done its part: the last stretch aims at the sensed position itself
            g_way = torch.where((q["cost"] == 0)[:, None], goal_pos[:, [0, 2]], q["waypoint"])
            act = expert(pos, direction, torch.where(going[:, None], g_way, e_way), turn_step)
            act = torch.where(going | (e_cost > 0), act, TURN_LEFT).to(torch.int32)        # nothing to go to: look around
        _, _, term, trunc = vec.step(act)
        done = (term | trunc) != 0
        moved = (vec.state(("agent_pos",))["agent_pos"] - pos)[:, [0, 2]].norm(dim=1)
        walked = walked + torch.where(done, (act == FORWARD).to(torch.float64) * float(cfg.forward_step.default), moved)
        ok = done & (term != 0)
        ended += done.sum()
        reached += ok.sum()
        spl += torch.where(ok, shortest.to(torch.float64) / torch.maximum(walked, shortest.to(torch.float64)).clamp(min=1e-9), 0.0).sum()
        vec.nav_field(into=yard, mask=done)
        start = done
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    vec.engine.check()
    vec.close()
    return dict(ended=int(ended), reached=int(reached), success=float(reached / ended.clamp(min=1)), spl=float(spl / ended.clamp(min=1)),
                goal_known=float(found_steps) / (n * args.steps), reach=reach, seconds=dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-FourRooms-v0")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--policy", default="sensed", choices=["sensed", "random"])
    ap.add_argument("--goal-radius", type=float, default=0.566, help="the radius of the task's goal object: the 0.8 m box")
    ap.add_argument("--reach", type=float, default=None, help="metres around the sensed goal that count as arrived (default: see the module's docstring)")
    args = ap.parse_args()
    r = run(args)
    print(f"{args.env} x {args.envs}, {args.steps} steps, policy {args.policy} (reach {r['reach']:.3f} m): episodes ended {r['ended']}, reached the box "
          f"{r['reached']}: success rate {r['success']:.3f}, SPL {r['spl']:.3f}; the goal was on the map in {r['goal_known']:.3f} of the env-steps "
          f"({r['seconds']:.2f} s, {r['seconds'] / args.steps * 1e6:.0f} us per step)")


if __name__ == "__main__":
    main()
