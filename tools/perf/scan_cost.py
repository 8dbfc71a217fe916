"""What scan maps cost (mw_scan_project; MiniWorldVecEnv.scan_map_update) for Hallway x 4096, FourRooms x 4096 and Maze x 1024, beside
the route they replace: the same rule as torch tensor operations — the closed form broadcast over [envs, beams, lines] in chunks of envs,
a scatter of the flat cell indices, the 0 -> 1 bytes and their counts.

    python tools/perf/scan_cost.py              # per config: five alternating windows, a process per window; one JSON line each
    python tools/perf/scan_cost.py --loop       # a step loop with a scan per step against the plain loop, alternating windows

A window measures, each between two device synchronisations: wall us per call, and the device time per call between two events around
the window's back-to-back calls (launch gaps included: an upper bound of the kernel's duration).  A kernel window times the update
alone on a held lidar() scan at 64, 256 and 1024 beams, and lidar() plus update; a torch window first counts the cells of both planes
in which the route differs from the kernel — 0 is asserted — and times the route at 256 beams; a depth window times depth_map_update on
a want_depth batch.  `--ab LIB` is an A/B of the design instead: kernel windows alternately with the product library and with the
variant library LIB (csrc/Makefile: `make OBJ=... OUT=... EXTRA=-D...`), a JSON line per window behind a line that names its side.
The record: whether every kernel window lies below every torch window; nothing here is a threshold."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nav_cost import CONFIGS, timed  # noqa: E402

RAYS, MAX_RANGE = (64, 256, 1024), 10.0


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


def torch_scan(m, lo, pos, t, d, chunk_elems=1 << 25):
    """the route, into the ScanMap-like record `m` (map, count, new): the rule of include/mwengine.h as tensor operations"""
    import torch
    n, R = t.shape
    gx, gz, cell, bound = m.gx, m.gz, m.cell, 2.0 ** 30
    step = max(1, chunk_elems // (R * (max(gx, gz) + 1)))
    for a in range(0, n, step):
        s = slice(a, a + step)
        u0, w0 = ((pos[s, 0] - lo[s, 0]) / cell)[:, None], ((pos[s, 1] - lo[s, 1]) / cell)[:, None]
        gu, gw = d[s, :, 0] / cell, d[s, :, 1] / cell
        hit = t[s] < m.max_range
        e = torch.where(hit, t[s], m.max_range)
        u1, w1 = u0 + e * gu, w0 + e * gw
        fits = lambda v: v.isfinite() & (v.abs() < bound)       # noqa: E731
        keep = (t[s] >= 0) & fits(u0) & fits(w0) & fits(u1) & fits(w1)
        k = u0.shape[0]
        planes = torch.zeros((2, k, gz * gx + 1), dtype=torch.bool, device=t.device)         # (the last cell takes what does not count)

        def mark(plane, row, col, ok):
            ok = ok & (row >= 0) & (row < gz) & (col >= 0) & (col < gx)
            flat = torch.where(ok, row * gx + col, float(gz * gx)).long().reshape(k, -1)
            plane.scatter_(1, flat, True)

        mark(planes[0], w0.floor().expand_as(e), u0.floor().expand_as(e), keep)
        mark(planes[1], w1.floor(), u1.floor(), keep & hit)
        for a0, a1, g, b0, h, lines, x_lines in ((u0, u1, gu, w0, gw, gx, True), (w0, w1, gw, u0, gu, gz, False)):
            L = torch.arange(lines + 1, dtype=torch.float64, device=t.device)[None, None, :]
            g_, a0_, a1_, b0_ = g[:, :, None], a0[:, :, None], a1[:, :, None], b0[:, :, None]
            crossed = torch.where(g_ > 0, (L >= a0_.floor() + 1) & (L <= a1_.floor()), (g_ < 0) & (L >= a1_.floor() + 1) & (L <= a0_.floor()))
            other = (b0_ + (L - a0_) / g_ * h[:, :, None]).floor()
            own = torch.where(g_ > 0, L, L - 1).expand_as(other)
            mark(planes[0], *((other, own) if x_lines else (own, other)), crossed & keep[:, :, None])
        obstacle = planes[1, :, :-1].reshape(k, gz, gx)
        free = planes[0, :, :-1].reshape(k, gz, gx) & ~obstacle
        for p, want in enumerate((free, obstacle)):
            add = want & (m.map[s, p] == 0)
            m.map[s, p] |= add.to(torch.uint8)
            m.new[s, p] = add.sum(dim=(1, 2), dtype=torch.int32)
        m.count[s] += m.new[s]


def window(name, kind, reps):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0, want_depth=kind == "depth")
    vec.reset()
    g = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(10):
        vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
    out = {}
    if kind == "depth":
        dm = vec.depth_map(max_range=8.0)
        out["cells"] = dm.gx * dm.gz
        out["depth_wall"], out["depth_device"] = timed(lambda: vec.depth_map_update(dm), reps)
    for R in RAYS if kind == "kernel" else (256,) if kind == "torch" else ():
        m = vec.scan_map(rays=R, max_range=MAX_RANGE)
        out["cells"] = m.gx * m.gz
        scan = {k: v.clone() for k, v in vec.lidar(R, m.fov, MAX_RANGE, obstacles=m.obstacles).items()}
        if kind == "kernel":
            out[f"update_wall_{R}"], out[f"update_device_{R}"] = timed(lambda: vec.scan_map_update(m, scan), reps)
            out[f"lidar_update_wall_{R}"], out[f"lidar_update_device_{R}"] = timed(lambda: vec.scan_map_update(m), reps)
            out[f"lidar_wall_{R}"], out[f"lidar_device_{R}"] = timed(lambda: vec.lidar(R, m.fov, MAX_RANGE, obstacles=m.obstacles), reps)
            out[f"free_share_{R}"] = round(float((m.free != 0).float().mean()), 4)
            continue
        st = vec.state(("agent_pos",))["agent_pos"]
        pos = st[:, [0, 2]].contiguous()
        ext = torch.as_tensor(vec.engine.get_state()["extent"], device="cuda", dtype=torch.float64)
        lo = ext[:, [0, 2]].contiguous()
        mine, theirs = vec.scan_map(rays=R, max_range=MAX_RANGE), vec.scan_map(rays=R, max_range=MAX_RANGE)
        for _ in range(2):      # (the second call adds nothing: the bytes hold)
            vec.scan_map_update(mine, scan)
            torch_scan(theirs, lo, pos, scan["t"], scan["dir"])
        differ = int((mine.map != theirs.map).sum()) + int((mine.count != theirs.count).sum()) + int((mine.new != theirs.new).sum())
        assert differ == 0, ("the route's map is another", differ)
        out["differ"] = differ
        out[f"torch_wall_{R}"], out[f"torch_device_{R}"] = timed(lambda: torch_scan(theirs, lo, pos, scan["t"], scan["dir"]), max(2, reps // 20))
    vec.engine.check()
    vec.close()
    print(json.dumps(out), flush=True)


def loop_window(name, kind, steps, warmup):
    """us per step of a frameless step loop (rollout of one action, render=False), with a 256-beam scan per step or plain"""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0)
    vec.reset()
    m = vec.scan_map()
    g = torch.Generator(device="cuda").manual_seed(3)
    plans = torch.randint(0, 3, (steps + warmup, 1, n), generator=g, device="cuda", dtype=torch.int32)
    import time
    for k in range(steps + warmup):
        if k == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        vec.rollout(plans[k], render=False)
        if kind == "scan":
            vec.scan_map_update(m)
    torch.cuda.synchronize()
    us = 1e6 * (time.perf_counter() - t0) / steps
    vec.close()
    print(json.dumps({f"{kind}_us_per_step": round(us, 2), f"{kind}_env_steps_per_s": round(n / us * 1e6)}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="hallway,fourrooms,maze")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--loop", action="store_true", help="the step loop with a scan per step against the plain loop")
    p.add_argument("--steps", type=int, default=400)
    p.add_argument("--warmup", type=int, default=50)
    p.add_argument("--ab", metavar="LIB", help="a variant engine library: kernel windows alternately without and with it, nothing else")
    p.add_argument("--window", choices=["kernel", "torch", "depth", "scan", "plain"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window in ("scan", "plain"):
        return loop_window(args.config, args.window, args.steps, args.warmup)
    if args.window:
        return window(args.config, args.window, args.reps)
    names = [c for c in args.configs.split(",") if c in CONFIGS]
    if args.ab:
        for w in range(args.windows):
            for name in names:
                for side, lib in (("product", None), ("variant", args.ab)):
                    print(json.dumps({"ab": side, "config": name}), flush=True)
                    print(json.dumps(_run(["--window", "kernel", "--config", name, "--reps", str(args.reps)], lib=lib)), flush=True)
        return
    for name in names:
        us = {}
        kinds = ("scan", "plain") if args.loop else ("kernel", "torch", "depth")
        for w in range(args.windows):
            for kind in kinds:
                print(f"{name} window {w}: {kind}", file=sys.stderr, flush=True)
                extra = ["--window", kind, "--config", name, "--reps", str(args.reps), "--steps", str(args.steps), "--warmup", str(args.warmup)]
                for k, v in _run(extra).items():
                    us.setdefault(k, []).append(v)
        rec = {"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "windows": us}
        if not args.loop:
            rec["every_kernel_window_below_every_torch_window"] = all(max(us[f"update_{t}_256"]) < min(us[f"torch_{t}_256"]) for t in ("device", "wall"))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
