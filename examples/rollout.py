#!/usr/bin/env python3
"""A minimal rollout loop on the batched engine: a (random-weight) CNN policy picks actions from the
observation tensor the raster kernel has just written — observations, rewards and flags never leave the GPU.

    python examples/rollout.py --env MiniWorld-Hallway-v0 --envs 4096 --steps 200
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-Hallway-v0")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=1, help="action repeat: env steps per policy decision and frame (1 .. 256)")
    ap.add_argument("--frame-stack", type=int, default=None, metavar="K",
                    help="stack the last K frames on the device (2 .. 16): the policy sees uint8[N, 3K, W, H]")
    args = ap.parse_args()

    import torch
    from miniworld_amd.vector import MiniWorldVectorEnv

    # obs_layout="cwh": the kernel stores uint8[N, 3, W, H] (the reference's PyTorchObsWrapper layout) directly
    envs = MiniWorldVectorEnv(args.env, args.envs, seed=args.seed, obs_layout="cwh", action_repeat=args.repeat,
                              frame_stack=args.frame_stack)
    n_act = envs.single_action_space.n
    channels = 3 * (args.frame_stack or 1)
    # with a frame stack the observation is the engine's view [N, K, 3, W, H] of its ring; merging K and 3 is a view again
    flat = (lambda o: o.reshape(o.shape[0], channels, *o.shape[-2:])) if args.frame_stack else (lambda o: o)
    policy = torch.nn.Sequential(
        torch.nn.Conv2d(channels, 16, 5, stride=2), torch.nn.ReLU(),
        torch.nn.Conv2d(16, 32, 5, stride=2), torch.nn.ReLU(),
        torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), torch.nn.Linear(32, n_act),
    ).cuda().half()

    obs, _ = envs.reset(seed=args.seed)
    with torch.no_grad():           # warm-up: MIOpen picks its convolution kernels on the first calls
        for _ in range(5):
            policy(flat(obs).half() / 255.0)
    episodes, returns = 0, torch.zeros(args.envs, device="cuda")
    sim_steps = torch.zeros((), dtype=torch.int64, device="cuda")       # env steps simulated: the sum of info["substeps"]
    finished_returns = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for _ in range(args.steps):
            logits = policy(flat(obs).half() / 255.0)
            actions = torch.distributions.Categorical(logits=logits.float()).sample().to(torch.int32)
            obs, rew, term, trunc, info = envs.step(actions)
            sim_steps += info["substeps"].sum() if args.repeat > 1 else args.envs
            returns += rew
            done = term | trunc
            if done.any():
                finished_returns.append(returns[done].clone())
                episodes += int(done.sum())
                returns[done] = 0.0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    mean_ret = torch.cat(finished_returns).mean().item() if finished_returns else float("nan")
    decisions = f" ({args.envs * args.steps / dt:,.0f} decisions/s at repeat {args.repeat})" if args.repeat > 1 else ""
    print(f"{args.env}: {sim_steps.item() / dt:,.0f} env-steps/s with the policy in the loop{decisions}, "
          f"{episodes} episodes finished, mean return {mean_ret:.3f}")
    envs.close()


if __name__ == "__main__":
    main()
