#!/usr/bin/env python3
"""examples/depth_plan_explore.py with a cost ramp about what the map holds for an obstacle: per env and step
`vec.grid_clearance(obstacle_plane, radii, costs)` turns the sensed obstacle plane into a cost per cell that falls with the distance to
the nearest obstacle cell, and `.cost`, as it stands, is the `extra` of the planner's `vec.grid_field()` — the inflation layer of a
costmap, so that a path keeps off the walls where there is room and still passes a door.  Everything else — sensor, map, frontier,
follower, the score — is depth_plan_explore.py's own loop, which also counts the forward moves that moved nothing.

    python examples/clear_plan_explore.py --env MiniWorld-MazeS3-v0 --envs 256 --horizon 120 --steps 600

Results, not thresholds: see README.md, "Grid clearance".
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from depth_plan_explore import run as plan_run  # noqa: E402


def cost_ramp(radii, costs):
    """depth_plan_explore.run's `ramp`: the cost bands about the map's obstacle cells, the record reused from step to step"""
    held = []

    def plane(vec, m):
        if held:
            vec.grid_clearance(m.obstacle != 0, into=held[0])
        else:
            held.append(vec.grid_clearance(m.obstacle != 0, radii=radii, costs=costs, limit=radii[-1], like=m))
        return held[0].cost
    return plane


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-MazeS3-v0")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--horizon", type=int, default=120, help="steps of an episode after which its coverage is taken")
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--radii", type=float, nargs="+", default=[0.75, 1.0, 1.25], help="metres from an obstacle cell, ascending")
    ap.add_argument("--costs", type=int, nargs="+", default=[20, 10, 5], help="the cost 0 .. 255 of a cell closer than each radius")
    args = ap.parse_args()
    args.unknown = 0
    for name, ramp in ((f"cost ramp {args.costs} within {args.radii} m of an obstacle cell", cost_ramp(args.radii, args.costs)), ("no cost ramp", None)):
        moves = {}
        cov, ended, dt = plan_run(args, ramp, moves)
        print(f"{args.env} x {args.envs}, {args.steps} steps: depth map, grid planner, {name}: mean coverage {cov:.3f} after {args.horizon} steps of an "
              f"episode (or at its end), over {ended} episodes; {int(moves['blocked'])} of {int(moves['forward'])} forward moves moved nothing "
              f"({float(moves['blocked']) / max(1, int(moves['forward'])):.4f}) ({dt:.2f} s, {dt / args.steps * 1e6:.0f} us per step)")


if __name__ == "__main__":
    main()
