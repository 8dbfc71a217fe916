#!/usr/bin/env python3
"""Random-shooting MPC on the device: R real environments, each planned for with P candidate action sequences of T steps.

    python examples/plan_shooting.py --env MiniWorld-Hallway-v0 --real 64 --candidates 32 --horizon 16 --steps 50

The batch holds R x P envs; the first R are the real ones.  Every control step: save the batch with its frames, make env j a copy
of real env j % R, roll P random plans per real env out WITHOUT drawing a frame (`vec.rollout(plans, render=False)`: one kernel
launch for T steps), score them from the per-step rewards with a discount, put the batch back — frames included, nothing is
redrawn — and step the real envs with the first action of their best plan.  No state or frame leaves the GPU.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-Hallway-v0")
    ap.add_argument("--real", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=32)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--gamma", type=float, default=0.95)
    args = ap.parse_args()

    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv

    R, P, T = args.real, args.candidates, args.horizon
    n = R * P
    vec = MiniWorldVecEnv(args.env, n, seed=0)
    vec.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    owner = torch.arange(n, device="cuda", dtype=torch.int32) % R       # env j plans for real env j % R
    discount = args.gamma ** torch.arange(T, device="cuda", dtype=torch.float32)
    ret = torch.zeros(R, device="cuda")
    for _ in range(args.steps):
        snap = vec.save_state(frames=True)
        vec.load_state(snap, records=owner)
        plans = torch.randint(0, vec.n_actions, (T, n), generator=g, device="cuda", dtype=torch.int32)
        vec.rollout(plans, render=False)
        score = (vec.step_rewards * discount[:, None]).sum(0).view(P, R)        # [candidate, real env]
        best = score.argmax(0) * R + torch.arange(R, device="cuda")             # the env that ran real env r's best plan
        vec.load_state(snap)
        actions = torch.zeros(n, dtype=torch.int32, device="cuda")
        actions[:R] = plans[0, best]
        _, reward, _, _ = vec.step(actions)
        ret += reward[:R]
    vec.engine.check()
    print(f"{args.env}: {R} real envs x {P} plans x {T} steps, {args.steps} control steps, mean return {ret.mean().item():.3f}")
    vec.close()


if __name__ == "__main__":
    main()
