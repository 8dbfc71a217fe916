#!/usr/bin/env python3
"""Random-shooting MPC with a dense cost from a rollout trace: the loop of examples/plan_shooting.py, scored by where the plans go.

    python examples/plan_to_goal.py --env MiniWorld-Hallway-v0 --real 64 --candidates 32 --horizon 16 --steps 60

Miniworld pays once, at the goal: a plan that does not reach the box inside the horizon scores exactly 0 by reward, whether it halves
the distance or walks into a wall.  `vec.rollout(plans, render=False, trace=("agent_pos",))` returns, from the same one kernel launch,
where every candidate's agent was after each of its T steps; the cost here is the smallest distance to the box over the horizon (the
box's position is read once per control step with `vec.state()`), with the discounted reward on top of it.  The script runs the same
budget twice, scored by reward alone and scored with the trace, and prints how many of the real envs reached their box in each.
No state, trace or frame leaves the GPU.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def run(args, use_trace):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv

    R, P, T = args.real, args.candidates, args.horizon
    n = R * P
    vec = MiniWorldVecEnv(args.env, n, seed=0)
    vec.reset()
    slot = int(vec.engine.cfg.goal_ent)
    g = torch.Generator(device="cuda").manual_seed(0)
    owner = torch.arange(n, device="cuda", dtype=torch.int32) % R       # env j plans for real env j % R
    discount = args.gamma ** torch.arange(T, device="cuda", dtype=torch.float32)
    reached = torch.zeros(R, dtype=torch.bool, device="cuda")
    episodes = torch.zeros(R, dtype=torch.int64, device="cuda")
    wins = torch.zeros(R, dtype=torch.int64, device="cuda")
    for _ in range(args.steps):
        snap = vec.save_state(frames=True)
        vec.load_state(snap, records=owner)
        plans = torch.randint(0, vec.n_actions, (T, n), generator=g, device="cuda", dtype=torch.int32)
        score = None
        if use_trace:
            goal = vec.state(("ent_pos",))["ent_pos"][:, slot].clone()          # [n, 3], before the plans run
            vec.rollout(plans, render=False, trace=("agent_pos",))
            d = vec.trace["agent_pos"] - goal[None]                             # [T, n, 3]
            dist = torch.sqrt(d[..., 0] ** 2 + d[..., 2] ** 2).amin(0)          # the closest the plan comes to the box
            score = -dist.to(torch.float32)
        else:
            vec.rollout(plans, render=False)
        ret = (vec.step_rewards * discount[:, None]).sum(0)
        score = (ret if score is None else score + args.reward_weight * ret).view(P, R)     # [candidate, real env]
        best = score.argmax(0) * R + torch.arange(R, device="cuda")             # the env that ran real env r's best plan
        vec.load_state(snap)
        actions = torch.zeros(n, dtype=torch.int32, device="cuda")
        actions[:R] = plans[0, best]
        _, reward, term, trunc = vec.step(actions)
        won = (reward[:R] > 0) & (term[:R] != 0)
        reached |= won
        wins += won
        episodes += ((term[:R] | trunc[:R]) != 0)
    vec.engine.check()
    vec.close()
    return reached.float().mean().item(), int(wins.sum().item()), int(episodes.sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-Hallway-v0")
    ap.add_argument("--real", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=32)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--gamma", type=float, default=0.95)
    ap.add_argument("--reward-weight", type=float, default=10.0, help="weight of the discounted reward beside the distance (trace scoring)")
    args = ap.parse_args()
    head = f"{args.env}: {args.real} real envs x {args.candidates} plans x {args.horizon} steps, {args.steps} control steps"
    for name, use_trace in (("reward only", False), ("trace: closest approach to the box", True)):
        rate, wins, episodes = run(args, use_trace)
        print(f"{head}, scored by {name}: {100 * rate:.1f} % of the real envs reached their box, {wins} boxes reached, {episodes} episodes ended")


if __name__ == "__main__":
    main()
