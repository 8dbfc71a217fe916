"""What frame stacking costs: env-steps/s of 4096 Hallway envs (a) without a stack, (b) with the engine's stack
(MiniWorldVecEnv(frame_stack=K): one push kernel per step, the stack is a view of the ring) and (c) without one plus the stack a
user writes in torch around `vec.obs` — a [N, K, H, W, 3] tensor shifted on every step, the envs that started an episode refilled
through torch.where on the done mask —, at K = 4 and K = 8.

    python tools/perf/frame_stack_cost.py                    # all five variants in one session, one JSON line
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o stack -- python tools/perf/frame_stack_cost.py --profile 4
                                                              # a run of its own: the push kernel's duration at K = 4

All engines run side by side on the same random actions; the timed windows alternate between the variants (a, b4, c4, b8, c8,
a, ...), each preceded by a device synchronisation.  Reports the medians, every window, each variant's cost per step against (a)
in microseconds, and the checks the comparison is read by: (b) >= (c) at both depths, and (b)'s cost at K = 8 against K = 4."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

ENV_ID, N, N_ACT = "MiniWorld-Hallway-v0", 4096, 3


class TorchShift:
    """(c): the stack in torch on an env without one."""

    def __init__(self, vec, K):
        import torch
        self.vec, self.torch = vec, torch
        self.stack = torch.zeros((vec.num_envs, K) + tuple(vec.obs.shape[1:]), dtype=vec.obs.dtype, device=vec.obs.device)

    def reset(self):
        obs = self.vec.reset()
        self.stack[:] = obs[:, None]

    def step(self, act):
        obs, _, te, tr = self.vec.step(act)
        self.stack[:, :-1] = self.stack[:, 1:].clone()
        self.stack[:, -1] = obs
        done = (te | tr).bool()[:, None, None, None, None]
        self.stack = self.torch.where(done, obs[:, None], self.stack)


class Plain:
    def __init__(self, vec):
        self.vec = vec

    def reset(self):
        self.vec.reset()

    def step(self, act):
        self.vec.step(act)


def main():
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=200, help="steps per timed window")
    p.add_argument("--windows", type=int, default=6, help="timed windows per variant")
    p.add_argument("--warmup", type=int, default=300, help="steps before timing (episodes spread over their length)")
    p.add_argument("--profile", type=int, default=0, metavar="K", help="only variant (b) at this depth, untimed: the run a profiler wraps")
    args = p.parse_args()
    g = torch.Generator(device="cuda").manual_seed(1)
    if args.profile:
        vec = MiniWorldVecEnv(ENV_ID, N, seed=0, frame_stack=args.profile)
        vec.reset()
        for _ in range(args.steps):
            vec.step(torch.randint(0, N_ACT, (N,), generator=g, device="cuda", dtype=torch.int32))
        torch.cuda.synchronize()
        vec.engine.check()
        vec.close()
        return
    runs = {"none": Plain(MiniWorldVecEnv(ENV_ID, N, seed=0))}
    for K in (4, 8):
        runs[f"engine_k{K}"] = Plain(MiniWorldVecEnv(ENV_ID, N, seed=0, frame_stack=K))
        runs[f"torch_k{K}"] = TorchShift(MiniWorldVecEnv(ENV_ID, N, seed=0), K)
    for r in runs.values():
        r.reset()
        for _ in range(args.warmup):
            r.step(torch.randint(0, N_ACT, (N,), generator=g, device="cuda", dtype=torch.int32))
    acts = torch.randint(0, N_ACT, (args.steps, N), generator=g, device="cuda", dtype=torch.int32)
    rates = {k: [] for k in runs}
    for w in range(args.windows):
        for k, r in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(args.steps):
                r.step(acts[t])
            torch.cuda.synchronize()
            rates[k].append(N * args.steps / (time.perf_counter() - t0))
    med = {k: sorted(r)[len(r) // 2] for k, r in rates.items()}
    us = {k: 1e6 * N / m for k, m in med.items()}            # microseconds per step of the whole batch
    cost = {k: round(us[k] - us["none"], 1) for k in runs if k != "none"}
    out = {"env_id": ENV_ID, "num_envs": N, "steps_per_window": args.steps,
           "env_steps_per_s": {k: round(m) for k, m in med.items()},
           "windows": {k: [round(x) for x in r] for k, r in rates.items()},
           "us_per_step": {k: round(v, 1) for k, v in us.items()},
           "cost_us_per_step_vs_none": cost,
           "engine_ge_torch": {f"k{K}": med[f"engine_k{K}"] >= med[f"torch_k{K}"] for K in (4, 8)},
           "engine_cost_k8_minus_k4_us": round(cost["engine_k8"] - cost["engine_k4"], 1),
           "window_scatter_us_none": round(1e6 * N / min(rates["none"]) - 1e6 * N / max(rates["none"]), 1)}
    for r in runs.values():
        r.vec.engine.check()
        r.vec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
