"""What action repeat buys: calls/s and simulated env-steps/s of MiniWorldVecEnv.step(actions, repeat=K) for K in {1, 2, 4, 8}
(K = 1 is the plain mw_step), uniform-random actions, default episode lengths, same-step auto-reset.

    python tools/perf/action_repeat_cost.py --config hallway     # 4096 Hallway envs
    python tools/perf/action_repeat_cost.py --config pickup_dr   # 2048 PickupObjects envs with domain randomisation
    python tools/perf/action_repeat_cost.py --config maze        # 1024 Maze envs

One config per process (a GPU job runs each under its own time limit).  One engine per K, side by side on the same random actions;
the timed windows alternate between them (K = 1, 2, 4, 8, 1, 2, ...), each preceded by a device synchronisation; medians over the
windows.  The sub-steps per call and the share of clean envs (frame_clean: holding a random action changes it) are counted outside
the timed loops, on the same actions once more.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

CONFIGS = {     # name -> env id, envs, domain_rand, actions (BASELINE.json configs 1, 3, 4)
    "hallway": ("MiniWorld-Hallway-v0", 4096, False, 3),
    "pickup_dr": ("MiniWorld-PickupObjects-v0", 2048, True, 5),
    "maze": ("MiniWorld-Maze-v0", 1024, False, 3),
}
REPEATS = (1, 2, 4, 8)


def main():
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    p = argparse.ArgumentParser()
    p.add_argument("--config", choices=sorted(CONFIGS), default="hallway")
    p.add_argument("--calls", type=int, default=200, help="calls per timed window")
    p.add_argument("--windows", type=int, default=5, help="timed windows per K")
    p.add_argument("--warmup", type=int, default=400, help="calls before timing (episodes spread over their length)")
    p.add_argument("--repeats", default=",".join(map(str, REPEATS)),
                   help="the K values, 1 first (a kernel trace wants two: the repeat kernels of every K > 1 share their names)")
    args = p.parse_args()
    env_id, n, dr, n_act = CONFIGS[args.config]
    repeats = tuple(int(k) for k in args.repeats.split(","))
    assert repeats[0] == 1, "K = 1, the plain step, is the yardstick of the ratios"
    vecs = {K: MiniWorldVecEnv(env_id, n, seed=0, domain_rand=dr) for K in repeats}
    g = torch.Generator(device="cuda").manual_seed(1)
    for K, v in vecs.items():
        v.reset()
        for _ in range(args.warmup):
            v.step(torch.randint(0, n_act, (n,), generator=g, device="cuda", dtype=torch.int32), repeat=K)
    acts = torch.randint(0, n_act, (args.calls, n), generator=g, device="cuda", dtype=torch.int32)
    rates = {K: [] for K in vecs}
    subs = {K: torch.zeros((), dtype=torch.int64, device="cuda") for K in vecs}
    clean = {K: torch.zeros((), dtype=torch.int64, device="cuda") for K in vecs}
    counted = {K: 0 for K in vecs}
    for w in range(args.windows):
        for K, v in vecs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(args.calls):
                v.step(acts[t], repeat=K)
            torch.cuda.synchronize()
            rates[K].append(args.calls / (time.perf_counter() - t0))
            for t in range(args.calls // 4):
                v.step(acts[t], repeat=K)
                subs[K] += v.substeps.sum() if K > 1 else n
                clean[K] += v.frame_clean().sum()
            counted[K] += args.calls // 4
    med = {K: sorted(r)[len(r) // 2] for K, r in rates.items()}
    per_call = {K: subs[K].item() / max(counted[K], 1) for K in vecs}       # simulated steps per call, the whole batch
    out = {"config": args.config, "env_id": env_id, "num_envs": n, "frame_reuse": vecs[1].frame_reuse,
           "calls_per_s": {K: round(m, 1) for K, m in med.items()},
           "sim_steps_per_s": {K: round(med[K] * per_call[K]) for K in vecs},
           "sim_steps_ratio_to_K1": {K: round(med[K] * per_call[K] / (med[1] * per_call[1]), 3) for K in vecs},
           "mean_substeps_per_env_and_call": {K: round(per_call[K] / n, 3) for K in vecs},
           "clean_share": {K: round(clean[K].item() / max(counted[K], 1) / n, 4) for K in vecs},
           "windows_calls_per_s": {K: [round(x, 1) for x in r] for K, r in rates.items()}}
    # (a capacity report of mw_check — a rare pose's display list or mesh slow path over its per-env capacity, drawn in bounds —
    # goes into the line: the rates stand, the K that met it is named)
    from miniworld_amd.engine import EngineError
    status = {}
    for K, v in vecs.items():
        try:
            v.engine.check()
        except EngineError as e:
            status[K] = str(e)
        v.close()
    out["mw_check"] = status or "ok"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
