"""What scan search costs (mw_scan_search; MiniWorldVecEnv.scan_search) for Hallway x 4096, FourRooms x 4096 and Maze x 1024, beside
mw_scan_match where its window reaches, in match_cost.py's setting: the score is a three-band clearance cost of a scan map's obstacle
plane after 40 steps, the scan a held lidar(256).

    python tools/perf/search_cost.py                     # per config: five alternating windows, a process per window; one JSON line each

scan_match is this tree's build: the binding cannot load a library without mw_scan_search, and tools/perf/device_symbols.py against
the parent commit's build says whether its kernel is the parent's.

A window measures, each between two device synchronisations, the device us per call between two events around the window's
back-to-back calls (launch gaps included: an upper bound of the kernel's duration).  A search window times (W, K, R) = (10, 21, 256),
(32, 21, 256) over -0.2 .. 0.2 rad and (64, 21, 256), (128, 63, 256) over the full turn, each with pruning on and off, records the refined
share of the blocks from `stats`, asserts best and score equal with pruning on and off — and equal to scan_match's where W <= 32 —, and
times (32, 21, 256) on a constant plane, the worst case.  A match window times scan_match at the two sets it reaches and on the constant
plane.  Nothing here is a threshold."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from match_cost import MAX_RANGE, _setting  # noqa: E402
from nav_cost import CONFIGS, timed  # noqa: E402

SETS, R = ((10, 21, 0.2), (32, 21, 0.2), (64, 21, math.pi), (128, 63, math.pi)), 256
FLAT = (32, 21, 0.2)


def _run(extra, timeout=300):
    """this file again as a process of its own, under its own time limit: the JSON line it prints"""
    import subprocess
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        print(json.dumps({"args": extra, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
        raise SystemExit(1)
    return json.loads(line[-1])


def window(name, kind, reps):
    import torch
    from miniworld_amd import engine
    vec, m, cost, scans = _setting(name, (R,))
    scan, flat, out = scans[R], torch.full_like(cost, 160), {"cells": m.gx * m.gz}
    kw = lambda W, K, turn: dict(window=W, turn=turn, turns=K, max_range=MAX_RANGE, like=m)      # noqa: E731
    for k, (W, K, turn) in enumerate(SETS + (FLAT,)):
        plane, tag = (flat, "flat") if k == len(SETS) else (cost, f"{W}_{K}")
        few = max(2, reps // 8) if W > 32 else reps
        if kind == "match":
            if W <= engine.MATCH_MAX_WINDOW:
                r = vec.scan_match(plane, scan, **kw(W, K, turn))
                out[f"match_device_{tag}"] = timed(lambda: vec.scan_match(plane, scan, into=r), few)[1]
            continue
        r = vec.scan_search(plane, scan, stats=True, **kw(W, K, turn))
        out[f"search_device_{tag}"] = timed(lambda: vec.scan_search(plane, scan, into=r), few)[1]
        best, score = r.best.clone(), r.score.clone()
        out[f"refined_share_{tag}"] = round(float(r.stats[:, 0].double().sum() / r.stats[:, 1].double().sum()), 4)
        out[f"moved_share_{tag}"] = round(float((best != 0).any(1).float().mean()), 4)
        if W <= 32 or name == "maze":       # (every block of a wide window on 4096 envs: seconds per call, left out)
            vec.engine.debug_set_search_prune(False)
            out[f"unpruned_device_{tag}"] = timed(lambda: vec.scan_search(plane, scan, into=r), max(2, few // 4))[1]
            vec.engine.debug_set_search_prune(True)
            assert torch.equal(best, r.best) and torch.equal(score, r.score), ("pruning changed the answer", tag)
        if W <= engine.MATCH_MAX_WINDOW:
            a = vec.scan_match(plane, scan, **kw(W, K, turn))
            assert torch.equal(best, a.best) and torch.equal(score, a.score), ("scan_match's answer is another", tag)
    vec.engine.check()
    vec.close()
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="hallway,fourrooms,maze")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=40)
    p.add_argument("--window", choices=["search", "match"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window:
        return window(args.config, args.window, args.reps)
    for name in [c for c in args.configs.split(",") if c in CONFIGS]:
        us = {}
        for w in range(args.windows):
            for kind in ("search", "match"):
                print(f"{name} window {w}: {kind}", file=sys.stderr, flush=True)
                rec = _run(["--window", kind, "--config", name, "--reps", str(args.reps)])
                for k, v in rec.items():
                    us.setdefault(k, []).append(v)
        print(json.dumps({"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "windows": us}), flush=True)


if __name__ == "__main__":
    main()
