#!/usr/bin/env python3
"""examples/view_explore.py with its candidates taken from the frontier's CLUSTERS, not drawn cell by cell: per env and step
`vec.grid_regions(frontier, connectivity=8, min_cells=--min-cells, max_regions=--views)` turns the mask of frontier cells into
frontiers — connected regions, each with a size and one cell of its own nearest its centroid — and `.cell`, as it stands, is the row
of viewpoints that `vec.grid_sight()` scores.  A speck of fewer than --min-cells cells is no candidate, an opening of forty cells is
one and not ten, and every doorway gets its own.  Everything else — sensor, map, planner, follower, the gain per metre, the held
goal, the score — is view_explore.py's own loop.

    python examples/cluster_explore.py --env MiniWorld-MazeS3-v0 --envs 256 --horizon 120 --steps 600 --compare

Results, not thresholds: see README.md, "Grid regions".
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from view_explore import run as view_run  # noqa: E402


def cluster_cells(min_cells, views):
    """view_explore.run's `candidates`: the representatives of the frontier's regions, the record reused from step to step"""
    held = []

    def pick(vec, m, frontier):
        if held:
            vec.grid_regions(frontier, into=held[0])
        else:
            held.append(vec.grid_regions(frontier, connectivity=8, min_cells=min_cells, max_regions=views, like=m, sums=False))
        return held[0].cell
    return pick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-MazeS3-v0")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--horizon", type=int, default=120, help="steps of an episode after which its coverage is taken")
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--views", type=int, default=32, help="frontier clusters listed per env and step, 1 .. engine.REGION_MAX")
    ap.add_argument("--min-cells", type=int, default=2, help="frontier clusters of fewer cells are no candidates")
    ap.add_argument("--sight", type=float, default=3.0, help="how far a candidate is taken to see, in metres")
    ap.add_argument("--bias", type=float, default=1.0, help="metres added to a candidate's path length before the gain is divided by it")
    ap.add_argument("--hold", type=int, default=12, help="steps a goal is kept at the most")
    ap.add_argument("--compare", action="store_true", help="run view_explore.py (sampled frontier cells) on the same settings too")
    args = ap.parse_args()
    runs = [(f"frontier clusters of {args.min_cells} cells and more, at most {args.views}", cluster_cells(args.min_cells, args.views))]
    if args.compare:
        runs.append((f"{args.views} sampled frontier cells", None))
    for name, candidates in runs:
        cov, ended, dt, share = view_run(args, candidates)
        print(f"{args.env} x {args.envs}, {args.steps} steps: depth map, goal by gain per metre among {name} (sight {args.sight} m): mean coverage "
              f"{cov:.3f} after {args.horizon} steps of an episode (or at its end), over {ended} episodes ({dt:.2f} s, {dt / args.steps * 1e6:.0f} us per step; "
              f"a goal by gain was held in {share:.2f} of the env-steps)")


if __name__ == "__main__":
    main()
