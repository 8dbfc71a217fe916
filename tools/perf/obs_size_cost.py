"""What an observation size costs: env-steps/s of 4096 Hallway envs at one size against the same batch at 80 x 60, and the raster
path each size takes (mw_raster_path; sizes off the 16 x 4 grid take the generic-resolution kernels).

    python tools/perf/obs_size_cost.py --size 84x84
    python tools/perf/obs_size_cost.py --size 64x64
    python tools/perf/obs_size_cost.py --size 100x75

One size per process (a GPU job runs each under its own time limit).  Both engines run side by side on the same random actions;
the timed windows alternate between them (80x60, size, 80x60, size, ...), each preceded by a device synchronisation.  Prints one
JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

PATH_NAMES = {0: "tile", 1: "quad", 2: "quad_mesh", 3: "generic"}


def main():
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    p = argparse.ArgumentParser()
    p.add_argument("--size", default="84x84", help="WxH of the measured observation")
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--steps", type=int, default=200, help="steps per timed window")
    p.add_argument("--windows", type=int, default=5, help="timed windows per engine")
    p.add_argument("--warmup", type=int, default=300, help="steps before timing (episodes spread over their length)")
    args = p.parse_args()
    w, h = (int(x) for x in args.size.split("x"))
    n = args.envs
    sizes = {"80x60": (80, 60), args.size: (w, h)}
    vecs = {k: MiniWorldVecEnv("MiniWorld-Hallway-v0", n, seed=0, obs_width=sw, obs_height=sh) for k, (sw, sh) in sizes.items()}
    g = torch.Generator(device="cuda").manual_seed(1)
    for v in vecs.values():
        v.reset()
        for _ in range(args.warmup):
            v.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
    acts = torch.randint(0, 3, (args.steps, n), generator=g, device="cuda", dtype=torch.int32)
    rates = {k: [] for k in vecs}
    for _ in range(args.windows):
        for k, v in vecs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(args.steps):
                v.step(acts[t])
            torch.cuda.synchronize()
            rates[k].append(n * args.steps / (time.perf_counter() - t0))
    med = {k: sorted(r)[len(r) // 2] for k, r in rates.items()}
    out = {"env_id": "MiniWorld-Hallway-v0", "num_envs": n, "size": args.size,
           "env_steps_per_s": {k: round(m) for k, m in med.items()},
           "ratio_vs_80x60": round(med[args.size] / med["80x60"], 4),
           "raster_path": {k: PATH_NAMES.get(v.engine.raster_path(), "?") for k, v in vecs.items()},
           "windows": {k: [round(x) for x in r] for k, r in rates.items()},
           "env": {k: os.environ[k] for k in ("MW_K2Q", "MW_GENERIC_RASTER") if k in os.environ}}
    for v in vecs.values():
        v.engine.check()
        v.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
