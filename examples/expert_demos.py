#!/usr/bin/env python3
"""Demonstrations from a scripted expert, without a host value in the loop: a go-to-the-box policy for Hallway or OneRoom written in
torch on the device, fed by the envs' own state.

    python examples/expert_demos.py --env MiniWorld-Hallway-v0 --envs 256 --steps 300

Code around the reference reads `env.agent.pos`, `env.agent.dir` and `env.box.pos` as Python attributes to script such an expert.  Here
`vec.state()` gathers them for every env into device tensors with one small kernel behind the step (mw_get_state_device), and the
expert is a dozen tensor operations on them: the heading towards the box (the agent looks along (cos dir, 0, -sin dir),
entity.py:70-79), a turn towards it while it is more than half a turn step off, else a step forward.  The (observation, action) pairs
go into a ring of the last `--keep` steps on the device — the batch an imitation learner would sample from.  There is no `.item()`
and no other synchronisation inside the loop; the success rate is read once at the end.
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

TURN_LEFT, TURN_RIGHT, FORWARD = 0, 1, 2


def expert(state, goal_ent, turn_step):
    """int32[N] actions from state()'s agent_pos, agent_dir and ent_pos: turn towards the box, else move forward"""
    import torch
    to_box = state["ent_pos"][:, goal_ent] - state["agent_pos"]
    want = torch.atan2(-to_box[:, 2], to_box[:, 0])
    off = torch.remainder(want - state["agent_dir"] + math.pi, 2 * math.pi) - math.pi       # in -pi .. pi, positive = to the left
    act = torch.where(off > 0, TURN_LEFT, TURN_RIGHT)
    return torch.where(off.abs() <= turn_step / 2, FORWARD, act).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-Hallway-v0", choices=["MiniWorld-Hallway-v0", "MiniWorld-OneRoom-v0", "MiniWorld-OneRoomS6-v0"])
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--keep", type=int, default=64, help="steps of (observation, action) pairs the demonstration ring holds")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv

    n = args.envs
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed)
    goal_ent = int(vec.engine.cfg.goal_ent)
    turn_step = math.radians(float(vec.engine.cfg.turn_step.default))
    obs = vec.reset()
    demo_obs = torch.zeros((args.keep,) + tuple(obs.shape), dtype=obs.dtype, device="cuda")
    demo_act = torch.zeros((args.keep, n), dtype=torch.int32, device="cuda")
    reached, ended = torch.zeros((), device="cuda"), torch.zeros((), device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        act = expert(vec.state(("agent_pos", "agent_dir", "ent_pos")), goal_ent, turn_step)
        demo_obs[t % args.keep].copy_(obs)          # the pair: what the expert saw, what it did
        demo_act[t % args.keep].copy_(act)
        obs, _, term, trunc = vec.step(act)
        reached += term.sum()
        ended += (term | trunc).sum()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    vec.engine.check()
    kept = min(args.keep, args.steps) * n
    print(f"{args.env} x {n}: {args.steps} steps in {dt:.2f} s ({n * args.steps / dt / 1e6:.3f} M env-steps/s), {kept} (obs, action) pairs kept")
    print(f"episodes ended {int(ended)}, reached the box {int(reached)}: success rate {float(reached / ended.clamp(min=1)):.3f}")
    vec.close()


if __name__ == "__main__":
    main()
