#!/usr/bin/env python3
"""Level replay without a learner: a finite set of levels, a random policy, and a sampler that sends envs back to the levels they do
worst on — every part of it on the device.

    python examples/level_replay.py --env MiniWorld-Hallway-v0 --envs 1024 --levels 64 --steps 400

`vec.make_levels(seeds)` builds the bank: level l is the reference's `env.reset(seed=seeds[l])` with its first observation.  With
`autoreset="levels"` every `vec.step()` restarts the envs whose episode it ended from record `vec.next_level[i]` of the bank — two
masked copy kernels behind the step, no frame drawn, and the host never learns which envs finished.  The loop below keeps a per-level
mean return with `index_add_` and writes `vec.next_level` from a softmax over the negative mean, a stand-in for the score of
Prioritized Level Replay; there is no `.item()` and no other synchronisation inside it.  Nothing is trained.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MiniWorld-Hallway-v0")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--levels", type=int, default=64)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--temperature", type=float, default=0.2)
    args = ap.parse_args()

    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv

    n, L = args.envs, args.levels
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed, autoreset="levels")
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    bank = vec.make_levels(torch.arange(L) + 1000 * (args.seed + 1))
    vec.set_levels(bank, generator=g)
    vec.reset()
    ret = torch.zeros(n, device="cuda")                  # the running episode's return, per env
    ret_sum, visits = torch.zeros(L, device="cuda"), torch.zeros(L, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        act = torch.randint(0, vec.n_actions, (n,), generator=g, device="cuda", dtype=torch.int32)
        _, reward, term, trunc = vec.step(act)
        done = (term | trunc).float()
        ret += reward
        played = vec.played_level.long()                 # the level each env played in this step (vec.level: the one it plays now)
        ret_sum.index_add_(0, played, ret * done)
        visits.index_add_(0, played, done)
        ret *= 1 - done
        # the sampler: levels with a low mean return so far are replayed more often (unvisited levels count as return 0)
        mean = ret_sum / visits.clamp(min=1)
        choice = torch.multinomial(torch.softmax(-mean / args.temperature, 0), n, replacement=True, generator=g)
        vec.next_level.copy_(choice)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    vec.engine.check()
    counts = visits.long().tolist()
    print(f"{args.env} x {n}, {L} levels: {args.steps} steps in {dt:.2f} s ({n * args.steps / dt / 1e6:.2f} M env-steps/s), "
          f"{sum(counts)} episodes finished")
    print("visits per level:", " ".join(str(c) for c in counts))
    vec.close()


if __name__ == "__main__":
    main()
