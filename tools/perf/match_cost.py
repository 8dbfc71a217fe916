"""What scan matching costs (mw_scan_match; MiniWorldVecEnv.scan_match) for Hallway x 4096, FourRooms x 4096 and Maze x 1024, beside the
most direct torch route for the same rule that fits in memory: per rotation the end cells, a gather from a zero-padded plane over
[envs, 2W+1, 2W+1, beams] in chunks of envs, a sum, and the arg-max through the packed tie key.

    python tools/perf/match_cost.py              # per config: five alternating windows, a process per window; one JSON line each
    python tools/perf/match_cost.py --loop       # a frameless step loop with lidar + match + map update per step against the loop without the match

The score is a three-band clearance cost of a scan map's obstacle plane after 40 steps; the scan is a held lidar().  A window measures,
each between two device synchronisations: wall us per call, and the device time per call between two events around the window's
back-to-back calls (launch gaps included: an upper bound of the kernel's duration).  A kernel window times (W, K, R) = (4, 1, 256),
(10, 21, 256), (10, 21, 1024) and the middle one with the volume; a torch window first counts the elements of volume, best and score in
which the route differs from the kernel at the middle set — 0 is asserted — and times the route there.  The record: whether every
kernel window lies below every torch window; nothing here is a threshold.  `--ab LIB1,LIB2` is an A/B of the design instead: kernel
windows alternately with each of the variant libraries (csrc/Makefile: `make OBJ=... OUT=... EXTRA=-DMW_MATCH_FORM=1` / `=2`: one form
of the correlation for every window), a JSON line per window behind a line that names its side."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nav_cost import CONFIGS, timed  # noqa: E402

SETS, MIDDLE, MAX_RANGE, TURN = ((4, 1, 256), (10, 21, 256), (10, 21, 1024)), (10, 21, 256), 10.0, 0.2
RADII, COSTS = (0.2, 0.45, 0.8), (255, 160, 60)


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


def torch_match(score, lo, pos, t, d, rot, W, cell, max_range, chunk_elems=1 << 25):
    """the route: (best int64[N, 3], best_score int64[N], volume int32[N, K, 2W+1, 2W+1]) by the rule of include/mwengine.h as tensor operations"""
    import torch
    n, R = t.shape
    gz, gx = score.shape[1:]
    side, P, bound, K = 2 * W + 1, 2 * W + 1, 2.0 ** 30, len(rot)
    pad = torch.zeros((n, gz + 2 * P, gx + 2 * P), dtype=torch.uint8, device=t.device)
    pad[:, P:P + gz, P:P + gx] = score
    pad, width = pad.reshape(n, -1), gx + 2 * P
    k = torch.arange(-W, W + 1, device=t.device)
    shift = (k[:, None] * width + k[None, :]).reshape(1, side * side, 1)                # [1, T, 1]: b rows, a columns
    volume = torch.empty((n, K, side * side), dtype=torch.int32, device=t.device)
    step = max(1, chunk_elems // (R * side * side))
    for a in range(0, n, step):
        s = slice(a, a + step)
        u0, w0 = ((pos[s, 0] - lo[s, 0]) / cell)[:, None], ((pos[s, 1] - lo[s, 1]) / cell)[:, None]
        gu, gw = d[s, :, 0] / cell, d[s, :, 1] / cell
        fits = lambda v: v.isfinite() & (v.abs() < bound)       # noqa: E731
        for r, (c, sn) in enumerate(rot):
            u1, w1 = u0 + t[s] * (c * gu + sn * gw), w0 + t[s] * (c * gw - sn * gu)
            counts = (t[s] >= 0) & (t[s] < max_range) & fits(u0) & fits(w0) & fits(u1) & fits(w1)
            row = torch.where(counts, w1.floor().clamp(-W - 1, gz + W), float(-W - 1)).long()
            col = torch.where(counts, u1.floor().clamp(-W - 1, gx + W), float(-W - 1)).long()
            flat = ((row + P) * width + col + P)[:, None, :] + shift                     # [n, T, R]
            volume[s, r] = torch.gather(pad[s], 1, flat.reshape(flat.shape[0], -1)).reshape(flat.shape).sum(-1, dtype=torch.int32)
    b, a_ = k[:, None].expand(side, side).reshape(-1), k[None, :].expand(side, side).reshape(-1)
    flat = (torch.arange(K, device=t.device)[:, None] * side * side + torch.arange(side * side, device=t.device)[None, :])
    rank = ((a_ * a_ + b * b)[None, :] << 19 | flat).reshape(-1)
    key = volume.reshape(n, -1).long() << 36 | (~rank & 0xFFFFFFFFF)[None, :]
    top = key.argmax(1)
    best = torch.stack([top // (side * side), top % side - W, top // side % side - W], 1)
    return best, volume.reshape(n, -1).gather(1, top[:, None])[:, 0].long(), volume.reshape(n, K, side, side)


def _setting(name, rays):
    """a reset batch stepped 40 times with a scan map kept: (vec, the cost plane, a held scan of `rays` beams)"""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0)
    vec.reset()
    m = vec.scan_map(max_range=MAX_RANGE)
    g = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(40):
        vec.rollout(torch.randint(0, 3, (1, n), generator=g, device="cuda", dtype=torch.int32), render=False)
        vec.scan_map_update(m)
    cost = vec.grid_clearance(m.obstacle != 0, radii=RADII, costs=COSTS, like=m).cost
    return vec, m, cost, {r: {k: v.clone() for k, v in vec.lidar(r, m.fov, MAX_RANGE, obstacles=m.obstacles).items()} for r in rays}


def window(name, kind, reps):
    import torch
    vec, m, cost, scans = _setting(name, sorted({s[2] for s in SETS}))
    out = {"cells": m.gx * m.gz}
    kw = lambda W, K: dict(window=W, turn=TURN if K > 1 else 0.0, turns=K, max_range=MAX_RANGE, like=m)      # noqa: E731
    if kind == "kernel":
        for W, K, R in SETS:
            r = vec.scan_match(cost, scans[R], **kw(W, K))
            out[f"match_wall_{W}_{K}_{R}"], out[f"match_device_{W}_{K}_{R}"] = timed(lambda: vec.scan_match(cost, scans[R], into=r), reps)
        W, K, R = MIDDLE
        r = vec.scan_match(cost, scans[R], volume=True, **kw(W, K))
        out["volume_wall"], out["volume_device"] = timed(lambda: vec.scan_match(cost, scans[R], into=r), reps)
        out["moved_share"] = round(float((r.best != 0).any(1).float().mean()), 4)
    else:
        W, K, R = MIDDLE
        r = vec.scan_match(cost, scans[R], volume=True, **kw(W, K))
        pos = vec.state(("agent_pos",))["agent_pos"][:, [0, 2]].contiguous()
        lo = torch.as_tensor(vec.engine.get_state()["extent"], device="cuda", dtype=torch.float64)[:, [0, 2]].contiguous()
        route = lambda: torch_match(cost, lo, pos, scans[R]["t"], scans[R]["dir"], r.pairs, W, m.cell, MAX_RANGE)      # noqa: E731
        best, score, volume = route()
        differ = int((volume != r.volume).sum()) + int((best != r.best).sum()) + int((score != r.score).sum())
        assert differ == 0, ("the route's answer is another", differ)
        out["differ"] = differ
        out["torch_wall"], out["torch_device"] = timed(route, max(2, reps // 20))
    vec.engine.check()
    vec.close()
    print(json.dumps(out), flush=True)


def loop_window(name, kind, steps, warmup):
    """us per step of a frameless step loop with one lidar(256) and one scan_map_update per step, with a match (10, 21) between them or without"""
    import time
    import torch
    vec, m, cost, _ = _setting(name, ())
    n = vec.num_envs
    W, K, R = MIDDLE
    r = vec.scan_match(cost, vec.lidar(R, m.fov, MAX_RANGE), window=W, turn=TURN, turns=K, max_range=MAX_RANGE, like=m)
    g = torch.Generator(device="cuda").manual_seed(3)
    plans = torch.randint(0, 3, (steps + warmup, 1, n), generator=g, device="cuda", dtype=torch.int32)
    for k in range(steps + warmup):
        if k == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        vec.rollout(plans[k], render=False)
        scan = vec.lidar(R, m.fov, MAX_RANGE)
        if kind == "match":
            vec.scan_match(cost, scan, into=r)
        vec.scan_map_update(m, scan)
    torch.cuda.synchronize()
    us = 1e6 * (time.perf_counter() - t0) / steps
    vec.close()
    print(json.dumps({f"{kind}_us_per_step": round(us, 2), f"{kind}_env_steps_per_s": round(n / us * 1e6)}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="hallway,fourrooms,maze")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=40)
    p.add_argument("--loop", action="store_true", help="the step loop with a match per step against the loop without it")
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--ab", metavar="LIBS", help="variant engine libraries, comma-separated: kernel windows alternately with each, nothing else")
    p.add_argument("--window", choices=["kernel", "torch", "match", "nomatch"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window in ("match", "nomatch"):
        return loop_window(args.config, args.window, args.steps, args.warmup)
    if args.window:
        return window(args.config, args.window, args.reps)
    if args.ab:
        for w in range(args.windows):
            for name in [c for c in args.configs.split(",") if c in CONFIGS]:
                for lib in args.ab.split(","):
                    print(json.dumps({"ab": os.path.basename(lib), "config": name}), flush=True)
                    print(json.dumps(_run(["--window", "kernel", "--config", name, "--reps", str(args.reps)], lib=lib)), flush=True)
        return
    for name in [c for c in args.configs.split(",") if c in CONFIGS]:
        us = {}
        for w in range(args.windows):
            for kind in ("match", "nomatch") if args.loop else ("kernel", "torch"):
                print(f"{name} window {w}: {kind}", file=sys.stderr, flush=True)
                extra = ["--window", kind, "--config", name, "--reps", str(args.reps), "--steps", str(args.steps), "--warmup", str(args.warmup)]
                for k, v in _run(extra).items():
                    us.setdefault(k, []).append(v)
        rec = {"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "windows": us}
        if not args.loop:
            W, K, R = MIDDLE
            rec["every_kernel_window_below_every_torch_window"] = all(max(us[f"match_{t}_{W}_{K}_{R}"]) < min(us[f"torch_{t}"]) and max(us[f"volume_{t}"]) < min(us[f"torch_{t}"])
                                                                      for t in ("device", "wall"))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
