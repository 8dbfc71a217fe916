"""What an explored-area update costs (mw_seen_update; MiniWorldVecEnv.seen_update) for Hallway x 4096, FourRooms x 4096 and
Maze x 1024 at the default range and cone and at max_range = 3 and 10 all round, against the route a user has without it — which is
not the code under test and uses nothing this call added, so it runs on a checkout from before it as well:
    route   vec.raycast(direction=[N, R, 2]) to the centre of every cell of the window around each agent, in chunks of at most
            engine.RAY_MAX rays, tests 1 - 3 as torch tensor operations on the device, a scatter into the map and the compare that
            counts the new cells; its map is compared with the kernel's, exactly

    python tools/perf/seen_cost.py              # per config: five alternating windows, a process per window; one JSON line each
    python tools/perf/seen_cost.py --loop       # Hallway x 4096: a vec.step loop with a seen_update per step against the plain loop

A window measures, each between two device synchronisations: wall us per call, and the device time per call between two events around
the window's back-to-back calls (launch gaps included: an upper bound of the kernel's duration).  Keys: <what>.<sight>, what = seen |
route, sight = default | r3 | r10."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {
    "hallway": ("MiniWorld-Hallway-v0", 4096),
    "fourrooms": ("MiniWorld-FourRooms-v0", 4096),
    "maze": ("MiniWorld-Maze-v0", 1024),
}
SIGHTS = {"default": dict(), "r3": dict(max_range=3.0, fov=2 * math.pi), "r10": dict(max_range=10.0, fov=2 * math.pi)}
CELL = 0.25


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


def make(name):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0)
    vec.reset()
    return vec, n


class Route:
    """the update without mw_seen_update: ray casts to the window's cell centres, the cheap tests in torch, scatter and compare"""

    def __init__(self, vec, n, gx, gz, max_range, cos_half):
        import torch
        from miniworld_amd import engine
        self.vec, self.n, self.gx, self.gz, self.range, self.cos_half = vec, n, gx, gz, max_range, cos_half
        half = int(math.ceil(max_range / CELL)) + 1
        k = torch.arange(-half, half + 1, device="cuda")
        self.dj, self.di = [t.reshape(-1) for t in torch.meshgrid(k, k, indexing="ij")]
        self.rays = int(self.di.numel())
        self.chunks = [(a, min(a + engine.RAY_MAX, self.rays)) for a in range(0, self.rays, engine.RAY_MAX)]
        self.zero = torch.zeros(1, dtype=torch.float64, device="cuda")
        self.seen = torch.zeros((n, gz, gx), dtype=torch.uint8, device="cuda")
        self.count = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.env = torch.arange(n, device="cuda")[:, None].expand(n, self.rays)

    def __call__(self):
        import torch
        vec, n = self.vec, self.n
        st = vec.state(("agent_pos", "extent"))
        ox, oz, ext = st["agent_pos"][:, 0:1], st["agent_pos"][:, 2:3], st["extent"]
        i = torch.floor((ox - ext[:, 0:1]) / CELL).long() + self.di[None]
        j = torch.floor((oz - ext[:, 2:3]) / CELL).long() + self.dj[None]
        cx, cz = ext[:, 0:1] + (i.double() + 0.5) * CELL, ext[:, 2:3] + (j.double() + 0.5) * CELL
        vx, vz = cx - ox, cz - oz
        d = torch.stack([vx, vz], dim=2)
        free = torch.cat([vec.raycast(direction=d[:, a:b].contiguous(), max_t=1.0)["hit"] == -1 for a, b in self.chunks], dim=1)
        dist = torch.sqrt(vx * vx + vz * vz)
        ok = (i >= 0) & (i < self.gx) & (j >= 0) & (j < self.gz) & ~((cx > ext[:, 1:2]) | (cz > ext[:, 3:4])) & (dist <= self.range) & free
        if self.cos_half != -1.0:
            h = vec.raycast(offsets=self.zero)["dir"][:, 0]
            ok &= (dist == 0.0) | (vx * h[:, 0:1] + vz * h[:, 1:2] >= self.cos_half * dist)
        vis = torch.zeros_like(self.seen)
        vis[self.env[ok], j[ok], i[ok]] = 1
        new = ((vis == 1) & (self.seen == 0)).sum((1, 2)).to(torch.int32)
        self.seen |= vis
        self.count += new
        return new


def window(name, kind, reps):
    import torch
    vec, n = make(name)
    e = vec.engine
    out = {"max_segs": int(e.cfg.max_segs)}
    for sname, kw in SIGHTS.items():
        m = vec.seen_map(cell=CELL, **kw)
        if kind == "seen":
            out[f"seen.{sname}.wall"], out[f"seen.{sname}.device"] = timed(lambda: vec.seen_update(m), reps)
            out[f"seen.{sname}.cells"] = round(float(m.count.double().mean()), 1)
        else:
            route = Route(vec, n, m.gx, m.gz, m.max_range, m.cos_half)
            vec.seen_update(m)
            route()
            assert torch.equal(route.seen, m.seen) and torch.equal(route.count, m.count), "the route's map is another"
            out[f"route.{sname}.wall"], out[f"route.{sname}.device"] = timed(route, max(2, reps // 10))
            out[f"route.{sname}.rays"] = route.rays
    e.check()
    vec.close()
    print(json.dumps(out), flush=True)


def loop_window(kind, steps, warmup):
    """Hallway x 4096: us per step of a random-action loop, with a seen_update (cleared on done) per step or without"""
    import torch
    vec, n = make("hallway")
    g = torch.Generator(device="cuda").manual_seed(3)
    m = vec.seen_map()

    def step():
        _, _, term, trunc = vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
        if kind == "seen":
            vec.seen_update(m, clear=term | trunc)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    us = 1e6 * (time.perf_counter() - t0) / steps
    vec.engine.check()
    print(json.dumps({"us_per_step": round(us, 1)}), flush=True)
    vec.close()


def child(extra, timeout=600):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        print(json.dumps({"args": extra, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
        raise SystemExit(1)
    return json.loads(line[-1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="hallway,fourrooms,maze")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--kinds", default="seen,route", help="seen alone: a variant library (MW_ENGINE_LIB) against the product")
    p.add_argument("--loop", action="store_true")
    p.add_argument("--steps", type=int, default=600)
    p.add_argument("--warmup", type=int, default=100)
    p.add_argument("--window", choices=["seen", "route", "plain"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    p.add_argument("--looped", action="store_true", help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window and args.looped:
        return loop_window(args.window, args.steps, args.warmup)
    if args.window:
        return window(args.config, args.window, args.reps)
    if args.loop:
        us = {}
        for _ in range(args.windows):
            for kind in ("seen", "plain"):
                print(f"loop window: {kind}", file=sys.stderr, flush=True)
                for k, v in child(["--looped", "--window", kind, "--steps", str(args.steps), "--warmup", str(args.warmup)]).items():
                    us.setdefault(kind + "." + k, []).append(v)
        print(json.dumps({"config": "hallway", "loop": us}), flush=True)
        return
    for name in [c for c in args.configs.split(",") if c in CONFIGS]:
        us = {}
        for w in range(args.windows):
            for kind in [k for k in ("seen", "route") if k in args.kinds.split(",")]:
                print(f"{name} window {w}: {kind}", file=sys.stderr, flush=True)
                for k, v in child(["--window", kind, "--config", name, "--reps", str(args.reps)]).items():
                    us.setdefault(k, []).append(v)
        print(json.dumps({"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "windows": us}), flush=True)


if __name__ == "__main__":
    main()
