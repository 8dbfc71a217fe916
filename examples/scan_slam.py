#!/usr/bin/env python3
"""Mapping under noisy odometry, with and without scan matching, all on the device.  Each agent dead-reckons: its pose estimate is the
last one plus the step's true pose increment in its own frame with Gaussian noise on it.  Its scan — `vec.lidar()`, known to the agent
in its own frame, so expressed along the ESTIMATED heading — goes into a scan map from the estimated position,
`vec.scan_map_update(m, scan, origin=estimate)`.  With `--match` the estimate is first corrected against the map so far:

    cost = vec.grid_clearance(m.obstacle != 0, radii, costs, like=m).cost       # a banded likelihood field around the obstacle cells
    r = vec.scan_match(cost, scan, origin=estimate, window=W, turn=a, turns=K, like=m)
    scan, estimate = r.apply(scan, estimate); heading += r.offset()[:, 2]

    python examples/scan_slam.py --env MiniWorld-FourRooms-v0 --envs 256 --steps 120

runs both and reports, over the envs whose episode did not end: the final position and heading error of the estimate, and the share of
the obstacle cells of the estimate-built map that the map built from the true poses also holds.  Results, not thresholds: see README.md,
"Scan matching".  With `--evidence` each is run a second time on an evidence map, which takes back what a later scan contradicts:

    m = vec.scan_evidence(rays=R, max_range=E)              # hit 3, miss 1, a vote per scan and cell, clamped to -20 .. 20
    r = vec.scan_match(m.score, scan, origin=estimate, ...) # its own likelihood plane, no clearance call
    vec.scan_evidence_update(m, scan, origin=estimate)
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

RADII, COSTS = (0.2, 0.45, 0.8), (255, 160, 60)


def turned(d, delta):
    """directions [N, R, 2] (dx, dz) turned by delta [N] radians in the sense agent_dir grows: dir_vec = (cos, -sin)"""
    import torch
    c, s = torch.cos(delta)[:, None], torch.sin(delta)[:, None]
    return torch.stack([c * d[..., 0] + s * d[..., 1], c * d[..., 1] - s * d[..., 0]], -1).contiguous()


def run(args, match, evidence=False):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n = args.envs
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed, want_depth=False)
    dev = vec.engine.device
    vec.reset()
    g = torch.Generator(device=dev).manual_seed(args.seed + 1)
    truth = vec.scan_map(rays=args.rays, max_range=args.range)
    m = vec.scan_evidence(rays=args.rays, max_range=args.range) if evidence else vec.scan_map(rays=args.rays, max_range=args.range)
    update = vec.scan_evidence_update if evidence else vec.scan_map_update
    st = vec.state(("agent_pos", "agent_dir"))
    pos, heading = st["agent_pos"].clone(), st["agent_dir"].clone()
    est, est_dir = pos.clone(), heading.clone()
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    scan = vec.lidar(args.rays, truth.fov, args.range)
    vec.scan_map_update(truth, scan)
    update(m, scan, origin=est)
    field = r = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        act = torch.multinomial(torch.tensor([0.25, 0.25, 0.5], device=dev), n, replacement=True, generator=g).to(torch.int32)
        _, _, term, trunc = vec.rollout(act[None], render=False)
        alive &= ~((term | trunc).reshape(-1) != 0)
        st = vec.state(("agent_pos", "agent_dir"))
        # the step's increment in the agent's own frame (forward, sideways, turn), with noise where it moved or turned
        dx, dz, dth = st["agent_pos"][:, 0] - pos[:, 0], st["agent_pos"][:, 2] - pos[:, 2], st["agent_dir"] - heading
        fwd, side = dx * torch.cos(heading) - dz * torch.sin(heading), dx * torch.sin(heading) + dz * torch.cos(heading)
        moved, spun = (fwd.abs() + side.abs()) > 0, dth != 0
        fwd = fwd + moved * args.pos_noise * torch.randn(n, generator=g, device=dev, dtype=torch.float64)
        side = side + moved * args.pos_noise * torch.randn(n, generator=g, device=dev, dtype=torch.float64)
        dth = dth + (moved | spun) * math.radians(args.turn_noise) * torch.randn(n, generator=g, device=dev, dtype=torch.float64)
        est[:, 0] += fwd * torch.cos(est_dir) + side * torch.sin(est_dir)
        est[:, 2] += -fwd * torch.sin(est_dir) + side * torch.cos(est_dir)
        est_dir += dth
        pos, heading = st["agent_pos"].clone(), st["agent_dir"].clone()
        scan = vec.lidar(args.rays, truth.fov, args.range)
        vec.scan_map_update(truth, scan)
        mine = dict(scan, dir=turned(scan["dir"], est_dir - heading))          # the same beams along the estimated heading
        if match:
            if not evidence:
                marked = m.obstacle != 0
                field = vec.grid_clearance(marked, radii=RADII, costs=COSTS, like=m) if field is None else vec.grid_clearance(marked, into=field)
            kw = dict(window=args.window, turn=math.radians(args.turn), turns=args.turns, max_range=args.range, like=m) if r is None else dict(into=r)
            r = vec.scan_match(m.score if evidence else field.cost, mine, origin=est, **kw)
            mine, est = r.apply(mine, est)
            est_dir += r.offset()[:, 2]
        update(m, mine, origin=est)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    k = alive.sum().clamp(min=1)
    err = ((est[:, 0] - pos[:, 0]) ** 2 + (est[:, 2] - pos[:, 2]) ** 2).sqrt()
    turn_err = torch.rad2deg(torch.remainder(est_dir - heading + math.pi, 2 * math.pi) - math.pi).abs()
    mine, true = (m.obstacle != 0) & alive[:, None, None], (truth.obstacle != 0) & alive[:, None, None]
    out = (float((err * alive).sum() / k), float((turn_err * alive).sum() / k), float((mine & true).sum() / mine.sum().clamp(min=1)), int(alive.sum()), dt)
    vec.engine.check()
    vec.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-FourRooms-v0")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--rays", type=int, default=256, help="beams of the scanner, all round")
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--pos-noise", type=float, default=0.03, help="metres, the standard deviation per step that moved, forward and sideways")
    ap.add_argument("--turn-noise", type=float, default=1.5, help="degrees, the standard deviation per step that moved or turned")
    ap.add_argument("--window", type=int, default=3, help="cells either way")
    ap.add_argument("--turn", type=float, default=6.0, help="degrees either way")
    ap.add_argument("--turns", type=int, default=13)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--evidence", action="store_true", help="run each once more on a ScanEvidence, matched on its own score plane")
    args = ap.parse_args()
    runs = [("dead reckoning", False, False), ("dead reckoning + scan_match", True, False)]
    if args.evidence:
        runs += [("dead reckoning, evidence map", False, True), ("dead reckoning + scan_match on the evidence map", True, True)]
    for name, match, evidence in runs:
        err, turn_err, share, alive, dt = run(args, match, evidence)
        print(f"{args.env} x {args.envs}, {args.steps} steps: {name}: position error {err:.3f} m, heading error {turn_err:.2f} deg, "
              f"{share:.3f} of the map's obstacle cells are the true-pose map's, over {alive} envs ({dt / args.steps * 1e6:.0f} us per step)")


if __name__ == "__main__":
    main()
