"""What a navigation field costs (mw_nav_build / mw_nav_query; MiniWorldVecEnv.nav_field / nav_query) for Maze x 1024, FourRooms x 4096
and Hallway x 4096, against the two routes a user has without it — neither is the code under test:
    (a) torch   the same field by a min-plus relaxation written in torch on the device, from the same occupancy and sources (taken
                from the kernel's field: cells of 0xFFFF and of 0): 8 shifted minima per pass with the corner rule, a convergence
                test (one host read) every 8 passes — what can be written today without a host round trip per env
    (b) host    engine.get_geometry(env) + engine.get_state() and Dijkstra in Python (numpy occupancy, heapq), measured over the
                first --host-envs envs and reported per env

    python tools/perf/nav_cost.py                      # per config: five alternating windows, a process per window; one JSON line each
    python tools/perf/nav_cost.py --loop               # Maze x 1024: the expert loop (masked rebuild + query every step) against a
                                                       # plain vec.step loop with the same actions' distribution, alternating windows

A window measures, each between two device synchronisations: wall us per call, and the device time per call between two events around
the window's back-to-back calls (launch gaps included: an upper bound of the kernel's duration).
    build / build_jacobi   nav_field(into=field) of the whole batch: directional sweeps (the product) / whole-grid passes
    build_masked           nav_field(into=field, mask=2 % of the envs)
    query                  nav_query(field)
    passes                 the relaxation's rounds per env (max, mean), sweeps and whole-grid passes
The criterion: every window's build below every window of (a), at Maze x 1024 and FourRooms x 4096."""
import argparse
import heapq
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "examples"))

CONFIGS = {
    "maze": ("MiniWorld-Maze-v0", 1024),
    "fourrooms": ("MiniWorld-FourRooms-v0", 4096),
    "hallway": ("MiniWorld-Hallway-v0", 4096),
}
BLOCKED, UNREACHED, INF = 0xFFFF, 0xFFFE, 1 << 24


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(1e6 * (time.perf_counter() - t0) / reps, 2), round(1e3 * a.elapsed_time(b) / reps, 2)


def torch_relax(blocked, sources, check_every=8):
    """baseline (a): int32 costs [N, gz, gx]; returns (field, passes)"""
    import torch
    import torch.nn.functional as F
    free = ~blocked
    cost = torch.where(sources, 0, INF).to(torch.int32)
    fp = F.pad(free, (1, 1, 1, 1), value=False)
    gz, gx = blocked.shape[1:]
    sh = lambda t, dj, di: t[:, 1 + dj:1 + dj + gz, 1 + di:1 + di + gx]     # noqa: E731
    ok = {(dj, di): sh(fp, dj, 0) & sh(fp, 0, di) for dj in (-1, 1) for di in (-1, 1)}      # the corner rule: both cells between free
    passes = 0
    while True:
        for _ in range(check_every):
            cp = F.pad(cost, (1, 1, 1, 1), value=INF)
            new = cost
            for dj, di in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                new = torch.minimum(new, sh(cp, dj, di) + 5)
            for (dj, di), m in ok.items():
                new = torch.minimum(new, torch.where(m, sh(cp, dj, di) + 7, INF))
            new = torch.where(free, new, INF)
            same = torch.equal(new, cost) if _ == check_every - 1 else False
            cost = new
            passes += 1
        if same:
            break
    return cost, passes


def host_field(segs, extent, agent_radius, cell, margin, gx, gz, tx, tz, reach):
    """baseline (b) for one env: numpy occupancy, heapq Dijkstra"""
    import numpy as np
    x = extent[0] + (np.arange(gx) + 0.5) * cell
    z = extent[2] + (np.arange(gz) + 0.5) * cell
    X, Z = np.meshgrid(x, z)
    blocked = (X > extent[1]) | (Z > extent[3])
    r = agent_radius + margin
    for sax, saz, sbx, sbz in segs:
        abx, abz = sbx - sax, sbz - saz
        t = np.clip(((X - sax) * abx + (Z - saz) * abz) / (abx * abx + abz * abz), 0.0, 1.0)
        blocked |= np.hypot(sax + t * abx - X, saz + t * abz - Z) < r
    cost = np.full((gz, gx), INF, np.int64)
    heap = []
    for j, i in zip(*np.nonzero((np.hypot(tx - X, tz - Z) < reach) & ~blocked)):
        cost[j, i] = 0
        heap.append((0, int(j), int(i)))
    while heap:
        c, j, i = heapq.heappop(heap)
        if c > cost[j, i]:
            continue
        for dj, di in ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)):
            nj, ni = j + dj, i + di
            if not (0 <= nj < gz and 0 <= ni < gx) or blocked[nj, ni] or (dj and di and (blocked[nj, i] or blocked[j, ni])):
                continue
            nc = c + (7 if dj and di else 5)
            if nc < cost[nj, ni]:
                cost[nj, ni] = nc
                heapq.heappush(heap, (nc, nj, ni))
    return np.where(blocked, BLOCKED, np.where(cost == INF, UNREACHED, cost)).astype(np.uint16)


def make(name):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0)
    vec.reset()
    return vec, n


def window(name, kind, reps, host_envs):
    import numpy as np
    import torch
    vec, n = make(name)
    e = vec.engine
    fld = vec.nav_field()
    bits = fld.field.view(torch.int16)
    out = {"cells": fld.gx * fld.gz}
    if kind == "kernel":
        jac = vec.nav_field()
        jac.params.flags |= 2
        passes = torch.zeros(n, dtype=torch.int32, device="cuda")
        e.debug_set_nav_passes(passes)
        vec.nav_field(into=fld)
        out["rounds_sweeps_max"], out["rounds_sweeps_mean"] = int(passes.max()), round(float(passes.float().mean()), 1)
        vec.nav_field(into=jac)
        out["passes_jacobi_max"], out["passes_jacobi_mean"] = int(passes.max()), round(float(passes.float().mean()), 1)
        e.debug_set_nav_passes(None)
        assert torch.equal(jac.field.view(torch.int16), bits)
        mask = (torch.rand(n, generator=torch.Generator(device="cuda").manual_seed(1), device="cuda") < 0.02).to(torch.uint8)
        out["masked_envs"] = int(mask.sum())
        out["build_wall"], out["build_device"] = timed(lambda: vec.nav_field(into=fld), reps)
        out["build_jacobi_wall"], out["build_jacobi_device"] = timed(lambda: vec.nav_field(into=jac), reps)
        out["build_masked_wall"], out["build_masked_device"] = timed(lambda: vec.nav_field(into=fld, mask=mask), reps)
        out["query_wall"], out["query_device"] = timed(lambda: vec.nav_query(fld), reps)
    elif kind == "torch":
        f = bits.to(torch.int32) & 0xFFFF
        blocked, sources = f == BLOCKED, f == 0
        cost, passes = torch_relax(blocked, sources)
        same = torch.where(blocked, BLOCKED, torch.where(cost >= INF, UNREACHED, cost))
        assert torch.equal(same, f), "the baseline's field is another"
        out["torch_passes"] = passes
        out["torch_wall"], out["torch_device"] = timed(lambda: torch_relax(blocked, sources), max(2, reps // 20))
    else:
        t0 = time.perf_counter()
        st = e.get_state()
        got = bits[:host_envs].cpu().numpy().view(np.uint16)
        for i in range(host_envs):
            _, segs = e.get_geometry(i)
            s = int(e.cfg.goal_ent)
            reach = float(st["ent_geom"][i][s][7]) + float(e.cfg.agent_radius) + 1.1 * float(e.cfg.max_forward_step)
            f = host_field(np.asarray(segs, np.float64).reshape(-1, 4), st["extent"][i], float(e.cfg.agent_radius), fld.cell, fld.margin, fld.gx, fld.gz,
                           float(st["ent_pos"][i][s][0]), float(st["ent_pos"][i][s][2]), reach)
            assert np.array_equal(f, got[i]), i
        out["host_envs"] = host_envs
        out["host_us_per_env"] = round(1e6 * (time.perf_counter() - t0) / host_envs, 1)
    e.check()
    vec.close()
    print(json.dumps(out), flush=True)


def loop_window(kind, steps, warmup):
    """Maze x 1024: us per step of the expert loop, or of a plain step loop fed by the same kind of actions"""
    import torch
    from expert_nav import expert
    vec, n = make("maze")
    turn = math.radians(float(vec.engine.cfg.turn_step.default))
    fld = vec.nav_field()
    g = torch.Generator(device="cuda").manual_seed(3)
    ended = torch.zeros((), dtype=torch.int64, device="cuda")

    def nav_step():
        st = vec.state(("agent_pos", "agent_dir"))
        q = vec.nav_query(fld)
        _, _, term, trunc = vec.step(expert(st["agent_pos"], st["agent_dir"], q["waypoint"], turn))
        done = (term | trunc) != 0
        vec.nav_field(into=fld, mask=done)
        ended.add_(done.sum())

    def plain_step():
        _, _, term, trunc = vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
        ended.add_(((term | trunc) != 0).sum())
    fn = nav_step if kind == "nav" else plain_step
    for _ in range(warmup):
        fn()
    ended.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    us = 1e6 * (time.perf_counter() - t0) / steps
    vec.engine.check()
    print(json.dumps({"us_per_step": round(us, 1), "episodes_ended_per_step": round(int(ended) / steps, 2)}), flush=True)
    vec.close()


def child(extra, timeout=900):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        print(json.dumps({"args": extra, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
        raise SystemExit(1)
    return json.loads(line[-1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="maze,fourrooms,hallway")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--host-envs", type=int, default=4)
    p.add_argument("--loop", action="store_true")
    p.add_argument("--steps", type=int, default=600)
    p.add_argument("--warmup", type=int, default=100)
    p.add_argument("--window", choices=["kernel", "torch", "host", "nav", "plain"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window in ("nav", "plain"):
        return loop_window(args.window, args.steps, args.warmup)
    if args.window:
        return window(args.config, args.window, args.reps, args.host_envs)
    if args.loop:
        us = {}
        for _ in range(args.windows):
            for kind in ("nav", "plain"):
                print(f"loop window: {kind}", file=sys.stderr, flush=True)
                for k, v in child(["--window", kind, "--steps", str(args.steps), "--warmup", str(args.warmup)]).items():
                    us.setdefault(kind + "." + k, []).append(v)
        print(json.dumps({"config": "maze", "loop": us}), flush=True)
        return
    for name in [c for c in args.configs.split(",") if c in CONFIGS]:
        us = {}
        for w in range(args.windows):
            for kind in ("kernel", "torch") + (("host",) if w == 0 else ()):
                print(f"{name} window {w}: {kind}", file=sys.stderr, flush=True)
                for k, v in child(["--window", kind, "--config", name, "--reps", str(args.reps), "--host-envs", str(args.host_envs)]).items():
                    us.setdefault(k, []).append(v)
        below = max(us["build_device"]) < min(us["torch_device"]) and max(us["build_wall"]) < min(us["torch_wall"])
        print(json.dumps({"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "windows": us,
                          "every_build_window_below_every_torch_window": below}), flush=True)


if __name__ == "__main__":
    main()
