"""What final observations cost: env-steps/s of plain same-step auto-reset against same-step + final_obs (MiniWorldVecEnv(...,
final_obs=True): the finished envs' terminal frames drawn in a second pass of the step), with default episode lengths, and the
mean number of episode ends per step.

    python tools/perf/final_obs_cost.py --config hallway     # 4096 Hallway envs
    python tools/perf/final_obs_cost.py --config pickup_dr   # 2048 PickupObjects envs with domain randomisation
    python tools/perf/final_obs_cost.py --config maze        # 1024 Maze envs

One config per process (a GPU job runs each under its own time limit).  Both engines run side by side on the same random actions;
the timed windows alternate between them (plain, final, plain, final, ...), each preceded by a device synchronisation.  Prints one
JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

CONFIGS = {     # name -> env id, envs, depth, domain_rand, actions (BASELINE.json configs 1, 3, 4)
    "hallway": ("MiniWorld-Hallway-v0", 4096, False, False, 3),
    "pickup_dr": ("MiniWorld-PickupObjects-v0", 2048, False, True, 5),
    "maze": ("MiniWorld-Maze-v0", 1024, False, False, 3),
}


def main():
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    p = argparse.ArgumentParser()
    p.add_argument("--config", choices=sorted(CONFIGS), default="hallway")
    p.add_argument("--steps", type=int, default=200, help="steps per timed window")
    p.add_argument("--windows", type=int, default=6, help="timed windows per engine")
    p.add_argument("--warmup", type=int, default=600, help="steps before timing (episodes spread over their length)")
    args = p.parse_args()
    env_id, n, depth, dr, n_act = CONFIGS[args.config]
    vecs = {"plain": MiniWorldVecEnv(env_id, n, seed=0, want_depth=depth, domain_rand=dr),
            "final_obs": MiniWorldVecEnv(env_id, n, seed=0, want_depth=depth, domain_rand=dr, final_obs=True)}
    g = torch.Generator(device="cuda").manual_seed(1)
    ends = {k: torch.zeros((), dtype=torch.int64, device="cuda") for k in vecs}
    for v in vecs.values():
        v.reset()
        for _ in range(args.warmup):
            v.step(torch.randint(0, n_act, (n,), generator=g, device="cuda", dtype=torch.int32))
    rates = {k: [] for k in vecs}
    steps_timed = {k: 0 for k in vecs}
    acts = torch.randint(0, n_act, (args.steps, n), generator=g, device="cuda", dtype=torch.int32)
    for w in range(args.windows):
        for k, v in vecs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(args.steps):
                v.step(acts[t])
            torch.cuda.synchronize()
            rates[k].append(n * args.steps / (time.perf_counter() - t0))
            # (episode ends counted outside the timed loop: the same actions once more, then a device-side sum per step)
            for t in range(args.steps // 4):
                _, _, te, tr = v.step(acts[t])
                ends[k] += (te | tr).sum()
            steps_timed[k] += args.steps // 4
    med = {k: sorted(r)[len(r) // 2] for k, r in rates.items()}
    out = {"config": args.config, "env_id": env_id, "num_envs": n,
           "env_steps_per_s": {k: round(m) for k, m in med.items()},
           "ratio_final_obs_vs_plain": round(med["final_obs"] / med["plain"], 4),
           "windows": {k: [round(x) for x in r] for k, r in rates.items()},
           "mean_ends_per_step": round(ends["final_obs"].item() / max(steps_timed["final_obs"], 1), 2)}
    for v in vecs.values():
        v.engine.check()
        v.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
