#!/usr/bin/env python3
"""Level replay over seeds, without a learner: a range of training seeds, a random policy, a sampler that sends envs back to the seeds
they do worst on, and an evaluation on held-out seeds — every part of it on the device.  The seed twin of examples/level_replay.py.

    python examples/seed_replay.py --env MiniWorld-Hallway-v0 --envs 1024 --levels 64 --steps 400 --eval-seeds 256

With `autoreset="seeds"` a level is eight bytes: an env whose episode ends in a `vec.step()` starts, in that step, the reference's
`env.reset(seed=vec.next_seed[i])`, generated on the device, and the host never learns which envs finished.  There is no bank to
build, so the training range may be as large as the seeds (Procgen's `start_level` / `num_levels`), and a held-out evaluation is the same
env with other numbers in `next_seed`.  The loop below keeps a per-seed mean return with `index_add_` (`vec.episode_seed` tells which
seed each env is playing) and writes `vec.next_seed` from a softmax over the negative mean, a stand-in for the score of Prioritized Level
Replay; there is no `.item()` and no other synchronisation inside it.  Nothing is trained.
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
    ap.add_argument("--start-level", type=int, default=1000)
    ap.add_argument("--levels", type=int, default=64, help="training seeds: start-level .. start-level + levels - 1")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--eval-seeds", type=int, default=256, help="held-out seeds, right behind the training range; one episode each")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--temperature", type=float, default=0.2)
    args = ap.parse_args()

    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv

    n, L, first = args.envs, args.levels, args.start_level
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed, autoreset="seeds")
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    ones = torch.ones(n, dtype=torch.uint8, device="cuda")

    def sample(probs):
        return first + torch.multinomial(probs, n, replacement=True, generator=g)

    # every env starts on a training seed (a masked seeded reset of the whole batch, on the device), and so does its next episode
    uniform = torch.full((L,), 1.0 / L, device="cuda")
    vec.reset_where(ones, sample(uniform))
    vec.next_seed.copy_(sample(uniform))
    ret = torch.zeros(n, device="cuda")                  # the running episode's return, per env
    ret_sum, visits = torch.zeros(L, device="cuda"), torch.zeros(L, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        played = vec.episode_seed - first                # the seed each env plays in this step (afterwards: the one it plays now)
        act = torch.randint(0, vec.n_actions, (n,), generator=g, device="cuda", dtype=torch.int32)
        _, reward, term, trunc = vec.step(act)
        done = (term | trunc).float()
        ret += reward
        ret_sum.index_add_(0, played, ret * done)
        visits.index_add_(0, played, done)
        ret *= 1 - done
        # the sampler: seeds with a low mean return so far are replayed more often (unvisited seeds count as return 0); the engine
        # reads next_seed[i] only when env i finishes, so writing all of it every step is the whole protocol
        mean = ret_sum / visits.clamp(min=1)
        vec.next_seed.copy_(sample(torch.softmax(-mean / args.temperature, 0)))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    vec.engine.check()
    counts = visits.long().tolist()
    print(f"{args.env} x {n}, {L} training seeds from {first}: {args.steps} steps in {dt:.2f} s "
          f"({n * args.steps / dt / 1e6:.2f} M env-steps/s), {sum(counts)} episodes finished")
    print("visits per seed:", " ".join(str(c) for c in counts))

    # Held-out evaluation: the seeds right behind the training range, one episode each, n at a time.  An env that finishes its
    # episode is parked on its own seed again (next_seed = the seed it just played) and counted once.
    held = torch.arange(first + L, first + L + args.eval_seeds, device="cuda")
    total, finished = torch.zeros((), device="cuda"), torch.zeros((), device="cuda")
    for base in range(0, args.eval_seeds, n):
        chunk = held[base:base + n]
        m = chunk.numel()
        seeds = torch.cat([chunk, chunk[:1].expand(n - m)])         # (the envs beyond the chunk play along and are not counted)
        vec.reset_where(ones, seeds)
        vec.next_seed.copy_(seeds)
        counted = torch.arange(n, device="cuda") < m
        open_ = counted.clone()
        ret.zero_()
        for _ in range(vec.template.max_episode_steps):
            act = torch.randint(0, vec.n_actions, (n,), generator=g, device="cuda", dtype=torch.int32)
            _, reward, term, trunc = vec.step(act)
            vec.next_seed.copy_(seeds)
            done = (term | trunc).bool() & open_
            ret += reward * open_
            total += (ret * done).sum()
            finished += done.sum()
            open_ &= ~done
    vec.engine.check()
    print(f"held-out seeds {first + L} .. {first + L + args.eval_seeds - 1}: {int(finished)} episodes, mean return {float(total / finished.clamp(min=1)):.3f}")
    vec.close()


if __name__ == "__main__":
    main()
