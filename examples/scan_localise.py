#!/usr/bin/env python3
"""Global localisation on a map the agents built themselves, all on the device: a particle filter whose loop never visits the host.
First each agent maps its world for --map-steps steps from its true poses (`vec.scan_map_update`).  Then it forgets where it is: P
particles per env are spread over the map's free cells under any heading, and every step

    particles move by the step's own increment, with noise                    # the caller's torch code
    w = vec.scan_weigh(field.cost, scan, particles, like=m)                   # a score per particle
    weights = ((w.score - w.score.amax(1, keepdim=True)).double() / T).exp().mul(2 ** 20).long()
    particles = vec.resample(weights, poses=particles)["pose"]                # the next generation

    python examples/scan_localise.py --env MiniWorld-FourRooms-v0 --envs 256 --particles 1024

reports in how many envs the best particle of the last weighing lies within a cell of the true pose.  Results, not thresholds.
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

RADII, COSTS = (0.2, 0.45, 0.8), (255, 160, 60)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-FourRooms-v0")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--particles", type=int, default=1024)
    ap.add_argument("--map-steps", type=int, default=150)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rays", type=int, default=128, help="beams of the scanner, all round")
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--temperature", type=float, default=400.0, help="score units per e-fold of weight")
    ap.add_argument("--pos-noise", type=float, default=0.05, help="metres per step, on every particle")
    ap.add_argument("--turn-noise", type=float, default=2.0, help="degrees per step, on every particle")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n, P = args.envs, args.particles
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed, want_depth=False)
    dev = vec.engine.device
    vec.reset()
    g = torch.Generator(device=dev).manual_seed(args.seed + 1)
    policy = torch.tensor([0.25, 0.25, 0.5], device=dev)
    step = lambda: vec.rollout(torch.multinomial(policy, n, replacement=True, generator=g).to(torch.int32)[None], render=False)      # noqa: E731
    m = vec.scan_map(rays=args.rays, max_range=args.range)
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    for _ in range(args.map_steps):
        vec.scan_map_update(m)
        _, _, term, trunc = step()
        alive &= ~((term | trunc).reshape(-1) != 0)
    field = vec.grid_clearance(m.obstacle != 0, radii=RADII, costs=COSTS, like=m)
    # the particles: (x, z, turn, spare) at the centres of free cells drawn per env, under any heading
    ext = vec.state(("extent",))["extent"]
    free = (m.free != 0).reshape(n, -1).double() + 1e-9
    cells = torch.multinomial(free, P, replacement=True, generator=g)
    u = torch.rand((n, P, 3), generator=g, device=dev, dtype=torch.float64)
    particles = torch.stack([ext[:, None, 0] + ((cells % m.gx).double() + u[..., 0]) * m.cell, ext[:, None, 2] + ((cells // m.gx).double() + u[..., 1]) * m.cell,
                             u[..., 2] * 2 * math.pi, torch.zeros_like(u[..., 0])], -1).contiguous()
    st = vec.state(("agent_pos", "agent_dir"))
    pos, heading = st["agent_pos"].clone(), st["agent_dir"].clone()
    w = drawn = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        _, _, term, trunc = step()
        alive &= ~((term | trunc).reshape(-1) != 0)
        st = vec.state(("agent_pos", "agent_dir"))
        dx, dz, dth = st["agent_pos"][:, 0] - pos[:, 0], st["agent_pos"][:, 2] - pos[:, 2], st["agent_dir"] - heading
        fwd, side = (dx * torch.cos(heading) - dz * torch.sin(heading))[:, None], (dx * torch.sin(heading) + dz * torch.cos(heading))[:, None]
        pos, heading = st["agent_pos"].clone(), st["agent_dir"].clone()
        noise = torch.randn((n, P, 3), generator=g, device=dev, dtype=torch.float64)
        th = particles[..., 2]
        particles[..., 0] += fwd * torch.cos(th) + side * torch.sin(th) + args.pos_noise * noise[..., 0]
        particles[..., 1] += -fwd * torch.sin(th) + side * torch.cos(th) + args.pos_noise * noise[..., 1]
        particles[..., 2] += dth[:, None] + math.radians(args.turn_noise) * noise[..., 2]
        # the scan as the agent knows it: in its own frame, so a particle's turn is its heading
        scan = vec.lidar(args.rays, m.fov, args.range)
        c, s, d = torch.cos(-heading)[:, None], torch.sin(-heading)[:, None], scan["dir"]
        own = dict(scan, dir=torch.stack([c * d[..., 0] + s * d[..., 1], c * d[..., 1] - s * d[..., 0]], -1).contiguous())
        w = vec.scan_weigh(field.cost, own, particles, max_range=args.range, like=m) if w is None else vec.scan_weigh(field.cost, own, particles, into=w)
        weights = ((w.score - w.score.amax(1, keepdim=True)).double() / args.temperature).exp().mul(2 ** 20).long()
        drawn = vec.resample(weights, poses=particles) if drawn is None else vec.resample(weights, poses=particles, into=drawn)
        particles, drawn["pose"] = drawn["pose"], particles
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    best = w.pose[torch.arange(n, device=dev), w.best[:, 0].long()]
    near = ((best[:, 0] - pos[:, 0]).abs() < m.cell) & ((best[:, 1] - pos[:, 2]).abs() < m.cell) & alive
    print(f"{args.env} x {n}, {P} particles, {args.rays} beams, {args.steps} steps on a map of {args.map_steps}: the best particle lies within a cell of the "
          f"true pose in {int(near.sum())} of {int(alive.sum())} envs ({dt / args.steps * 1e6:.0f} us per step)")
    vec.engine.check()
    vec.close()


if __name__ == "__main__":
    main()
