#!/usr/bin/env python3
"""Fork the best of N: a population of environments explores with random actions; every `--every` steps the members in the upper
half by return since the last selection are cloned over the lower half — states, random streams and all — with one `vec.fork(src)`
on the device (a save kernel, a load kernel, a frame).  No state leaves the GPU and the copies continue exactly as their sources
would have; here they diverge again because each member draws its own actions.

    python examples/fork_best.py --env MiniWorld-Hallway-v0 --envs 1024 --steps 200 --every 20
    python examples/fork_best.py --frame-stack 4        # a policy input of the last 4 frames: the fork carries the frames too

With `--frame-stack K` the members keep a stack of their last K frames (`vec.stack`) and the fork is `vec.fork(src, frames=True)`: the
copy gets its source's observation and stack — what a policy that reads the stack saw in the source — through four copy kernels, and
no frame is drawn.  The default fork redraws and starts every copy's stack over from its one new frame.

`vec.save_state()` / `vec.load_state(snap)` are the other two calls: a checkpoint (`torch.save(snap.cpu().state_dict(), path)`) and
"go back to a state seen earlier".
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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--every", type=int, default=20, help="steps between two selections")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frame-stack", type=int, default=None, metavar="K", help="keep the last K frames per member; forks then carry the frames")
    args = ap.parse_args()

    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv

    n = args.envs
    vec = MiniWorldVecEnv(args.env, n, seed=args.seed, frame_stack=args.frame_stack)
    carry_frames = args.frame_stack is not None
    vec.reset()
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    score = torch.zeros(n, device="cuda")
    total, forks = 0.0, 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(1, args.steps + 1):
        act = torch.randint(0, vec.n_actions, (n,), generator=g, device="cuda", dtype=torch.int32)
        _, reward, _, _ = vec.step(act)
        score += reward
        if t % args.every == 0:
            # src[j]: the env that member j continues from — the better half keeps itself, the rest copy a member of it
            order = torch.argsort(score, descending=True)
            src = torch.arange(n, device="cuda")
            src[order[n // 2:]] = order[:n - n // 2]
            vec.fork(src, frames=carry_frames)
            total += float(score.sum())
            score.zero_()
            forks += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    vec.engine.check()
    print(f"{args.env} x {n}: {args.steps} steps, {forks} forks in {dt:.2f} s ({n * args.steps / dt / 1e6:.2f} M env-steps/s), "
          f"return collected {total:.1f}")
    vec.close()


if __name__ == "__main__":
    main()
