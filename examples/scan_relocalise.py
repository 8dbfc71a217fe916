#!/usr/bin/env python3
"""Relocalisation after a lost track, all on the device.  The agents of `scan_slam.py` map from their true poses for a while; then each
pose ESTIMATE is thrown off — up to `--lost` metres along each axis and any heading — as after a teleport the odometry did not see.
One wide-window search over the full turn recovers it against the map so far:

    cost = vec.grid_clearance(m.obstacle != 0, radii, costs, like=m).cost
    r = vec.scan_search(cost, scan, origin=estimate, window=W, turn=pi, turns=63, like=m)       # W cells either way, up to 128
    scan, estimate = r.apply(scan, estimate); heading += r.offset()[:, 2]

    python examples/scan_relocalise.py --env MiniWorld-FourRooms-v0 --envs 256 --steps 80

reports the position and heading error of the estimate before and after the search, the share of envs recovered to within a cell and
one rotation step, and the share of the blocks of translations the kernel had to score.  Results, not thresholds: a room that looks
alike from two places is matched to either.
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from scan_slam import COSTS, RADII, turned  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-FourRooms-v0")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=80, help="steps of mapping from the true poses before the track is lost")
    ap.add_argument("--rays", type=int, default=256, help="beams of the scanner, all round")
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--lost", type=float, default=7.0, help="metres: the estimate is thrown off by up to this along x and along z")
    ap.add_argument("--turns", type=int, default=63, help="rotations over the full turn, odd")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n = args.envs
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed, want_depth=False)
    dev = vec.engine.device
    vec.reset()
    g = torch.Generator(device=dev).manual_seed(args.seed + 1)
    m = vec.scan_map(rays=args.rays, max_range=args.range)
    vec.scan_map_update(m)
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    for _ in range(args.steps):
        act = torch.multinomial(torch.tensor([0.25, 0.25, 0.5], device=dev), n, replacement=True, generator=g).to(torch.int32)
        _, _, term, trunc = vec.rollout(act[None], render=False)
        alive &= ~((term | trunc).reshape(-1) != 0)
        vec.scan_map_update(m)
    st = vec.state(("agent_pos", "agent_dir"))
    pos, heading = st["agent_pos"], st["agent_dir"]
    est, est_dir = pos.clone(), heading + (torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 2 - 1) * math.pi
    est[:, 0] += (torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 2 - 1) * args.lost
    est[:, 2] += (torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 2 - 1) * args.lost
    scan = vec.lidar(args.rays, m.fov, args.range)
    mine = dict(scan, dir=turned(scan["dir"], est_dir - heading))              # the same beams along the estimated heading
    cost = vec.grid_clearance(m.obstacle != 0, radii=RADII, costs=COSTS, like=m).cost
    window = min(128, int(math.ceil(args.lost / m.cell)) + 2)
    r = vec.scan_search(cost, mine, origin=est, window=window, turn=math.pi, turns=args.turns, max_range=args.range, like=m, stats=True)
    _, found = r.apply(mine, est)
    found_dir = est_dir + r.offset()[:, 2]
    k = alive.sum().clamp(min=1)

    def errors(p, d):
        err = ((p[:, 0] - pos[:, 0]) ** 2 + (p[:, 2] - pos[:, 2]) ** 2).sqrt()
        return err, torch.rad2deg(torch.remainder(d - heading + math.pi, 2 * math.pi) - math.pi).abs()

    (e0, t0), (e1, t1) = errors(est, est_dir), errors(found, found_dir)
    close = (e1 <= 1.5 * m.cell) & (t1 <= 360.0 / args.turns) & alive
    share = float(r.stats[:, 0].double().sum() / r.stats[:, 1].double().sum())
    vec.engine.check()
    print(f"{args.env} x {n}, {args.steps} steps of mapping, lost by up to {args.lost} m and any heading; one scan_search, window {window} cells, "
          f"{args.turns} rotations: position error {float((e0 * alive).sum() / k):.3f} -> {float((e1 * alive).sum() / k):.3f} m, heading error "
          f"{float((t0 * alive).sum() / k):.2f} -> {float((t1 * alive).sum() / k):.2f} deg, {float(close.sum() / k):.3f} of {int(alive.sum())} envs within 1.5 cells "
          f"and a rotation step; {share:.3f} of the blocks scored")
    vec.close()


if __name__ == "__main__":
    main()
