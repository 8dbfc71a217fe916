"""What a depth projection costs (mw_depth_project; MiniWorldVecEnv.depth_update / depth_map_update) for Hallway x 4096, FourRooms x 4096 and
Maze x 1024 — the window at 33 x 33 and 65 x 65 cells of 0.25 m, the map on the nav field's grid — against the route a user has without
it, written here with nothing this call added: the same unprojection as torch tensor operations in float64 over [N, H * W], the class by
height, an index computation and a `bincount` scatter per class (`index_put_(accumulate=True)` with --scatter index_put), a clamp or a
threshold and an OR.  Every window also counts the cells in which the route's result differs from the kernel's (cells_that_differ; the
route takes sin and cos from torch, the kernel from the engine's own, so a point on a cell's border may fall on the other side).
Two states per config: `typical` — the batch after 30 random steps — and `pileup` — every agent moved to half a metre in front of the
wall it faces (set_state_where), where thousands of points fall into a handful of cells: the kernel's LDS atomics at their worst.

    python tools/perf/depth_cost.py              # per config: five alternating windows, a process per window; one JSON line each
    python tools/perf/depth_cost.py --loop       # Hallway x 4096, want_depth: a vec.step loop with a depth_update per step against the plain loop

A window measures, each between two device synchronisations: wall us per call, and the device time per call between two events around
the window's back-to-back calls (launch gaps included: an upper bound of the kernel's duration).  Keys: <what>.<state>.<target>, what =
depth | route, target = window33 | window65 | map."""
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
SIZES = (33, 65)
CELL = 0.25
SAMPLE0 = {8: (9, 5), 4: (6, 2), 1: (8, 8)}


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
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0, want_depth=True)
    vec.reset()
    g = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(30):
        vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
    return vec, n


def pile_up(vec, n):
    """every agent to half a metre in front of the wall it faces; the frame and the depth map are redrawn by the state write"""
    import torch
    zero = torch.zeros(1, dtype=torch.float64, device="cuda")
    hit = vec.raycast(offsets=zero, max_t=1000.0)
    t, d = hit["t"][:, 0], hit["dir"][:, 0]
    pos = vec.state(("agent_pos",))["agent_pos"].clone()
    move = (t - 0.5).clamp(min=0.0)
    pos[:, 0] += move * d[:, 0]
    pos[:, 2] += move * d[:, 1]
    vec.set_state_where(torch.ones(n, dtype=torch.uint8, device="cuda"), agent_pos=pos)


class Route:
    """the projection without mw_depth_project: tensor operations and a scatter"""

    def __init__(self, vec, n, scatter):
        import torch
        self.vec, self.n, self.scatter = vec, n, scatter
        H, W = int(vec.engine.cfg.obs_height), int(vec.engine.cfg.obs_width)
        sx, sy = SAMPLE0[int(vec.engine.cfg.msaa)]
        u = torch.arange(W, dtype=torch.float64, device="cuda")[None, :].expand(H, W).reshape(1, -1)
        v = torch.arange(H, dtype=torch.float64, device="cuda")[:, None].expand(H, W).reshape(1, -1)
        self.xn = ((u + sx / 16.0) * 2.0) / W - 1.0
        self.yn = 1.0 - ((v + (1.0 - sy / 16.0)) * 2.0) / H
        self.aspect = W / H
        self.zero = torch.zeros(1, dtype=torch.float64, device="cuda")
        self.rows = torch.arange(n, device="cuda")[:, None]

    def points(self, o):
        import torch
        st = self.vec.state(("agent_pos", "cam", "extent"))
        cam, self.ext = st["cam"], st["extent"]
        self.ox, self.oz = st["agent_pos"][:, 0:1], st["agent_pos"][:, 2:3]
        h = self.vec.raycast(offsets=self.zero)["dir"][:, 0]
        hx, hz = h[:, 0:1], h[:, 1:2]
        pitch, half = cam[:, 2:3] * math.pi / 180.0, cam[:, 3:4] * 0.5 * math.pi / 180.0
        sp, cp, th = torch.sin(pitch), torch.cos(pitch), torch.sin(half) / torch.cos(half)
        d = self.vec.depth.reshape(self.n, -1).to(torch.float64)
        inside = (d >= o.min_range) & (d <= o.max_range)
        self.lat = (self.xn * (th * self.aspect)) * d
        yc = (self.yn * th) * d
        self.fwd = cam[:, 1:2] + (d * cp - yc * sp)
        up = cam[:, 0:1] + (d * sp + yc * cp)
        self.floor = inside & (up >= -o.floor_tol) & (up <= o.floor_tol)
        self.obst = inside & (up > o.floor_tol) & (up <= o.top)
        self.px = self.ox + (self.fwd * hx + self.lat * -hz)
        self.pz = self.oz + (self.fwd * hz + self.lat * hx)

    def counts(self, row, col, kept, n_rows, n_cols):
        """int64[N, 2, n_rows, n_cols]: the floor and the obstacle points per cell"""
        import torch
        cells = n_rows * n_cols
        at = (self.rows * 2) * cells + row.clamp(0, n_rows - 1).long() * n_cols + col.clamp(0, n_cols - 1).long()
        out = torch.zeros(self.n * 2 * cells, dtype=torch.int64, device="cuda")
        for k, which in enumerate((self.floor, self.obst)):
            m = kept & which
            idx = (at + k * cells)[m]
            if self.scatter == "bincount":
                out += torch.bincount(idx, minlength=out.numel())
            else:
                out.index_put_((idx,), torch.ones_like(idx), accumulate=True)
        return out.reshape(self.n, 2, n_rows, n_cols)

    def window(self, w):
        import torch
        self.points(w)
        S = w.size
        a, b = (self.px - self.ox, -(self.pz - self.oz)) if w.frame == "north" else (self.lat, self.fwd)
        c = torch.floor(a / w.cell + S * 0.5)
        r = torch.floor((S * 0.5 + w.back) - b / w.cell)
        kept = (c >= 0.0) & (c < S) & (r >= 0.0) & (r < S)
        return self.counts(r, c, kept, S, S).clamp(max=255).to(torch.uint8)

    def map(self, m, into):
        import torch
        self.points(m)
        fi = torch.floor((self.px - self.ext[:, 0:1]) / m.cell)
        fj = torch.floor((self.pz - self.ext[:, 2:3]) / m.cell)
        kept = (fi >= 0.0) & (fi < float(m.gx)) & (fj >= 0.0) & (fj < float(m.gz))
        hit = self.counts(fj, fi, kept, m.gz, m.gx) >= m.min_points
        fresh = hit & (into == 0)
        into[fresh] = 1
        return fresh.reshape(self.n, 2, -1).sum(2)


def window(name, kind, reps, scatter):
    import torch
    vec, n = make(name)
    out = {}
    route = Route(vec, n, scatter)
    for state in ("typical", "pileup"):
        if state == "pileup":
            pile_up(vec, n)
        for S in SIZES:
            w = vec.depth_window(size=S, cell=CELL)
            key = f"{state}.window{S}"
            if kind == "depth":
                out[f"depth.{key}.wall"], out[f"depth.{key}.device"] = timed(lambda: vec.depth_update(w), reps)
                out[f"depth.{key}.most_points_in_a_cell"] = int(route.counts(*_bins(route, w), S, S).max())
            else:
                vec.depth_update(w)
                out[f"route.{key}.cells_that_differ"] = int((route.window(w) != w.planes).sum())
                out[f"route.{key}.wall"], out[f"route.{key}.device"] = timed(lambda: route.window(w), max(2, reps // 10))
        m = vec.depth_map(cell=CELL)
        key = f"{state}.map"
        if kind == "depth":
            out[f"depth.{key}.wall"], out[f"depth.{key}.device"] = timed(lambda: vec.depth_map_update(m), reps)
        else:
            vec.depth_map_update(m)
            mine = torch.zeros_like(m.map)
            route.map(m, mine)
            out[f"route.{key}.cells_that_differ"] = int((mine != m.map).sum())
            out[f"route.{key}.wall"], out[f"route.{key}.device"] = timed(lambda: route.map(m, mine), max(2, reps // 10))
    vec.engine.check()
    vec.close()
    print(json.dumps(out), flush=True)


def _bins(route, w):
    import torch
    route.points(w)
    c = torch.floor(route.lat / w.cell + w.size * 0.5)
    r = torch.floor((w.size * 0.5 + w.back) - route.fwd / w.cell)
    return r, c, (c >= 0.0) & (c < w.size) & (r >= 0.0) & (r < w.size)


def loop_window(kind, steps, warmup):
    """Hallway x 4096 with depth maps: us per step of a random-action loop, with a depth_update (33 x 33) per step or without"""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n = CONFIGS["hallway"]
    vec = MiniWorldVecEnv(env_id, n, seed=0, want_depth=True)
    vec.reset()
    g = torch.Generator(device="cuda").manual_seed(3)
    w = vec.depth_window()

    def step():
        vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
        if kind == "depth":
            vec.depth_update(w)
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
    p.add_argument("--kinds", default="depth,route", help="depth alone: a variant library (MW_ENGINE_LIB) against the product")
    p.add_argument("--scatter", choices=["bincount", "index_put"], default="bincount")
    p.add_argument("--loop", action="store_true")
    p.add_argument("--steps", type=int, default=600)
    p.add_argument("--warmup", type=int, default=100)
    p.add_argument("--window", choices=["depth", "route", "plain"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    p.add_argument("--looped", action="store_true", help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window and args.looped:
        return loop_window(args.window, args.steps, args.warmup)
    if args.window:
        return window(args.config, args.window, args.reps, args.scatter)
    if args.loop:
        us = {}
        for _ in range(args.windows):
            for kind in ("depth", "plain"):
                print(f"loop window: {kind}", file=sys.stderr, flush=True)
                for k, v in child(["--looped", "--window", kind, "--steps", str(args.steps), "--warmup", str(args.warmup)]).items():
                    us.setdefault(kind + "." + k, []).append(v)
        print(json.dumps({"config": "hallway", "loop": us}), flush=True)
        return
    for name in [c for c in args.configs.split(",") if c in CONFIGS]:
        us = {}
        for w in range(args.windows):
            for kind in [k for k in ("depth", "route") if k in args.kinds.split(",")]:
                print(f"{name} window {w}: {kind}", file=sys.stderr, flush=True)
                for k, v in child(["--window", kind, "--config", name, "--reps", str(args.reps), "--scatter", args.scatter]).items():
                    us.setdefault(k, []).append(v)
        print(json.dumps({"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "scatter": args.scatter, "windows": us}), flush=True)


if __name__ == "__main__":
    main()
