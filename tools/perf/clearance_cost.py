"""What grid clearance costs (mw_grid_clearance; MiniWorldVecEnv.grid_clearance) for Hallway x 4096, FourRooms x 4096 and Maze x 1024 on
two masks, beside the route it replaces: the exact transform as torch tensor operations — per chunk of envs a [gz, gz, gx] broadcast for
every column's nearest marked row, then a [gz, gx, gx] broadcast for the least d^2 + dj^2 of every cell's row, `bucketize` for the bands.

    python tools/perf/clearance_cost.py             # per config: five alternating windows, a process per window; one JSON line each

The masks: `obstacle`, the obstacle plane of a DepthMap after --map-steps random steps, and `blocked`, the blocked cells of a privileged
nav field.  A window measures, each between two device synchronisations: wall us per call, and the device time per call between two
events around the window's back-to-back calls (launch gaps included: an upper bound of the kernel's duration).  A kernel window times
the call with everything (nearest and three bands, no limit), bare (dist2 alone) and bare under a limit of --limit metres.  A torch
window first counts the elements of dist2 and cost in which the route differs from the kernel: 0 is asserted.
`--ab LIB` is an A/B of the design instead: per config --windows kernel windows alternately with the product library and with the
variant library LIB (csrc/Makefile: `make OBJ=... OUT=... EXTRA=-D...`), a JSON line per window behind a line that names its side.
The record: whether every kernel window lies below every torch window; nothing here is a threshold."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nav_cost import CONFIGS, timed  # noqa: E402

RADII, COSTS = (0.5, 0.75, 1.0), (200, 50, 10)
FORMS = {"full": dict(radii=RADII, costs=COSTS, nearest=True), "bare": {}, "limit": None}


def _run(extra, timeout=900, lib=None):
    """this file again as a process of its own, under its own time limit (lib: with that engine library): the JSON line it prints"""
    import subprocess
    env = dict(os.environ, MW_ENGINE_LIB=os.path.abspath(lib)) if lib else None
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        print(json.dumps({"args": extra, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
        raise SystemExit(1)
    return json.loads(line[-1])


def torch_clearance(marked, thresholds, costs, chunk_elems=1 << 27):
    """the route: (dist2 int32[N, gz, gx], cost uint8[N, gz, gx]); no nearest"""
    import torch
    n, gz, gx = marked.shape
    dev, far = marked.device, 1 << 15
    rows, cols = torch.arange(gz, device=dev), torch.arange(gx, device=dev)
    dj = (rows[:, None] - rows[None, :]).abs()[None, :, :, None]                # [1, j, j', 1]
    di2 = ((cols[:, None] - cols[None, :]) ** 2)[None, None]                      # [1, 1, i, i']
    step = max(1, chunk_elems // (gz * gx * max(gz, gx)))
    out = []
    for a in range(0, n, step):
        m = marked[a:a + step]
        g = torch.where(m[:, None, :, :], dj, far).amin(dim=2)                  # [n, j, i]: the column's nearest marked row, in rows
        d2 = (di2 + torch.where(g < far, g * g, 1 << 40)[:, :, None, :]).amin(dim=3)
        out.append(torch.where(d2 < (1 << 40), d2, 0x7FFFFFFF).to(torch.int32))
    dist2 = torch.cat(out)
    table = torch.tensor(list(costs) + [0], dtype=torch.uint8, device=dev)
    cost = table[torch.bucketize(dist2, torch.tensor(thresholds, dtype=torch.int32, device=dev))]
    return dist2, cost


def masks_of(vec, n, map_steps):
    """{"obstacle": bool[N, gz, gx], "blocked": bool[N, gz, gx]} and the map whose grid they share"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    m = vec.depth_map(max_range=8.0)
    vec.depth_map_update(m)
    for _ in range(map_steps):
        vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
        vec.depth_map_update(m)
    f = vec.nav_field()
    assert (f.gz, f.gx) == (m.gz, m.gx)
    return {"obstacle": (m.obstacle != 0).contiguous(), "blocked": (f.field.view(torch.int16) == -1).contiguous()}, m


def window(name, kind, reps, map_steps, limit):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0, want_depth=True)
    vec.reset()
    masks, m = masks_of(vec, n, map_steps)
    out = {"cells": m.gx * m.gz}
    for which, marked in masks.items():
        out[f"{which}_share"] = round(float(marked.float().mean()), 4)
        full = vec.grid_clearance(marked, like=m, **FORMS["full"])
        out[f"{which}_dist_mean"] = round(float(full.metres()[full.dist2 < 0x7FFFFFFE].mean()), 3)
        if kind == "kernel":
            for form, kw in FORMS.items():
                r = vec.grid_clearance(marked, like=m, **(dict(limit=limit) if kw is None else kw))
                out[f"kernel_{form}_wall_{which}"], out[f"kernel_{form}_device_{which}"] = timed(lambda: vec.grid_clearance(marked, into=r), reps)
            continue
        thresholds, costs = zip(*full.bands)
        dist2, cost = torch_clearance(marked, thresholds, costs)
        differ = int((dist2 != full.dist2).sum()) + int((cost != full.cost).sum())
        assert differ == 0, ("the route's transform is another", which, differ)
        out[f"differ_{which}"] = differ
        out[f"torch_wall_{which}"], out[f"torch_device_{which}"] = timed(lambda: torch_clearance(marked, thresholds, costs), max(2, reps // 20))
    vec.engine.check()
    vec.close()
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="hallway,fourrooms,maze")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--map-steps", type=int, default=40, help="random steps the DepthMap accumulates over")
    p.add_argument("--limit", type=float, default=1.0, help="metres, the limited form's")
    p.add_argument("--ab", metavar="LIB", help="a variant engine library: kernel windows alternately without and with it, nothing else")
    p.add_argument("--window", choices=["kernel", "torch"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window:
        return window(args.config, args.window, args.reps, args.map_steps, args.limit)
    if args.ab:
        for w in range(args.windows):
            for name in [c for c in args.configs.split(",") if c in CONFIGS]:
                for side, lib in (("product", None), ("variant", args.ab)):
                    print(json.dumps({"ab": side, "config": name}), flush=True)
                    print(json.dumps(_run(["--window", "kernel", "--config", name, "--reps", str(args.reps), "--map-steps", str(args.map_steps)], lib=lib)), flush=True)
        return
    for name in [c for c in args.configs.split(",") if c in CONFIGS]:
        us = {}
        for w in range(args.windows):
            for kind in ("kernel", "torch"):
                print(f"{name} window {w}: {kind}", file=sys.stderr, flush=True)
                extra = ["--window", kind, "--config", name, "--reps", str(args.reps), "--map-steps", str(args.map_steps), "--limit", str(args.limit)]
                for k, v in _run(extra).items():
                    us.setdefault(k, []).append(v)
        below = all(max(us[f"kernel_full_{t}_{w}"]) < min(us[f"torch_{t}_{w}"]) for w in ("obstacle", "blocked") for t in ("device", "wall"))
        print(json.dumps({"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "windows": us,
                          "every_kernel_window_below_every_torch_window": below}), flush=True)


if __name__ == "__main__":
    main()
