"""What an egocentric map window costs (mw_ego_map; MiniWorldVecEnv.ego_update) for Hallway x 4096, FourRooms x 4096 and Maze x 1024 at
33 x 33 and 65 x 65 points of 0.25 m — all three planes, VISIBLE alone, the sample of a seen map alone — against the routes a user has
without it, which use nothing this call added:
    visible  vec.raycast(direction=[N, R, 2]) to every point of the window, in chunks of at most engine.RAY_MAX rays, range and cone as
             torch tensor operations on the device
    wall     the extent test and a broadcast closest-point distance [N, S * S, segments] in float64, in chunks of segments that keep a
             temporary below 512 MB
    sample   a float64 index computation and a gather from the seen map
Every window also counts the cells in which a route's result differs from the kernel's (cells_that_differ; the rounding is torch's).
The route for all three planes is visible + wall: the entity plane's broadcast is left out, so that figure is a lower bound.

    python tools/perf/ego_cost.py              # per config: five alternating windows, a process per window; one JSON line each
    python tools/perf/ego_cost.py --loop       # Hallway x 4096: a vec.step loop with an ego_update per step against the plain loop

A window measures, each between two device synchronisations: wall us per call, and the device time per call between two events around
the window's back-to-back calls (launch gaps included: an upper bound of the kernel's duration).  Keys: <what>.<planes>.<size>, what =
ego | route, planes = all | visible | sample."""
import argparse
import json
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
SETS = {"all": ("wall", "entity", "visible"), "visible": ("visible",), "sample": ()}
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
    """the window without mw_ego_map: the points in torch, ray casts, a broadcast wall distance, an index and a gather"""

    def __init__(self, vec, n, w, seen):
        import numpy as np
        import torch
        from miniworld_amd import engine
        self.vec, self.n, self.w, self.seen, self.S = vec, n, w, seen, w.size
        S = w.size
        idx = torch.arange(S, dtype=torch.float64, device="cuda") + 0.5
        lat, fwd = (idx - S * 0.5) * w.cell, ((S * 0.5 - idx) + w.back) * w.cell
        self.F, self.L = fwd[:, None].expand(S, S).reshape(1, -1), lat[None, :].expand(S, S).reshape(1, -1)
        self.rays = S * S
        self.chunks = [(a, min(a + engine.RAY_MAX, self.rays)) for a in range(0, self.rays, engine.RAY_MAX)]
        self.zero = torch.zeros(1, dtype=torch.float64, device="cuda")
        e = vec.engine
        sets = [0] if e.cfg.shared_geometry else range(n)
        segs = np.full((len(sets), int(e.cfg.max_segs), 4), np.nan)         # (a row of NaN is no wall: every comparison fails)
        for k, env in enumerate(sets):
            s = np.asarray(e.get_geometry(env)[1], np.float64).reshape(-1, 4)
            segs[k, :len(s)] = s
        self.segs = torch.from_numpy(segs).cuda()
        self.seg_chunk = max(1, (512 << 20) // (n * self.rays * 8))

    def points(self):
        st = self.vec.state(("agent_pos", "extent"))
        self.ox, self.oz, self.ext = st["agent_pos"][:, 0:1], st["agent_pos"][:, 2:3], st["extent"]
        self.h = self.vec.raycast(offsets=self.zero)["dir"][:, 0]
        hx, hz = self.h[:, 0:1], self.h[:, 1:2]
        self.px = self.ox + (self.F * hx + self.L * -hz)
        self.pz = self.oz + (self.F * hz + self.L * hx)

    def visible(self):
        import torch
        self.points()
        vx, vz = self.px - self.ox, self.pz - self.oz
        d = torch.stack([vx, vz], dim=2)
        free = torch.cat([self.vec.raycast(direction=d[:, a:b].contiguous(), max_t=1.0)["hit"] == -1 for a, b in self.chunks], dim=1)
        dist = torch.sqrt(vx * vx + vz * vz)
        ok = (dist <= self.w.max_range) & free
        if self.w.cos_half != -1.0:
            ok &= (dist == 0.0) | (vx * self.h[:, 0:1] + vz * self.h[:, 1:2] >= self.w.cos_half * dist)
        return ok.to(torch.uint8).reshape(self.n, self.S, self.S)

    def wall(self):
        import torch
        self.points()
        px, pz, ext = self.px, self.pz, self.ext
        inside = (px >= ext[:, 0:1]) & (px <= ext[:, 1:2]) & (pz >= ext[:, 2:3]) & (pz <= ext[:, 3:4])
        near = torch.zeros_like(inside)
        x, z = px[:, :, None], pz[:, :, None]
        for a in range(0, self.segs.shape[1], self.seg_chunk):
            s = self.segs[:, None, a:a + self.seg_chunk]
            sax, saz, abx, abz = s[..., 0], s[..., 1], s[..., 2] - s[..., 0], s[..., 3] - s[..., 1]
            t = ((x - sax) * abx + (z - saz) * abz) / (abx * abx + abz * abz)
            t = torch.where(t < 0.0, 0.0, torch.where(t > 1.0, 1.0, t))
            dx, dz = (sax + t * abx) - x, (saz + t * abz) - z
            near |= (torch.sqrt(dx * dx + dz * dz) < self.w.wall_radius).any(dim=2)
        return torch.where(inside & ~near, 0, 1).to(torch.uint8).reshape(self.n, self.S, self.S)

    def sample(self):
        import torch
        self.points()
        m = self.seen
        fi = torch.floor((self.px - self.ext[:, 0:1]) / m.cell)
        fj = torch.floor((self.pz - self.ext[:, 2:3]) / m.cell)
        inside = (fi >= 0.0) & (fi < float(m.gx)) & (fj >= 0.0) & (fj < float(m.gz))
        at = fj.clamp(0, m.gz - 1).long() * m.gx + fi.clamp(0, m.gx - 1).long()
        got = torch.gather(m.seen.reshape(self.n, -1), 1, at)
        return torch.where(inside, got, 0).to(torch.uint8).reshape(self.n, self.S, self.S)

    def all(self):
        return self.visible(), self.wall()


def window(name, kind, reps):
    import torch
    vec, n = make(name)
    e = vec.engine
    out = {"max_segs": int(e.cfg.max_segs)}
    seen = vec.seen_map(cell=CELL)
    vec.seen_update(seen)
    for S in SIZES:
        for sname, planes in SETS.items():
            w = vec.ego_window(size=S, cell=CELL, planes=planes)
            source = seen if sname == "sample" else None
            key = f"{sname}.{S}"
            if kind == "ego":
                out[f"ego.{key}.wall"], out[f"ego.{key}.device"] = timed(lambda: vec.ego_update(w, source=source), reps)
                continue
            route = Route(vec, n, w, seen)
            if sname == "sample":
                out[f"route.{key}.cells_that_differ"] = int((route.sample() != vec.ego_update(w, source=seen)[1]).sum())
            else:
                vec.ego_update(w)
                out[f"route.{key}.cells_that_differ"] = int((route.visible() != w.visible).sum())
                if sname == "all":
                    out[f"route.{key}.wall_cells_that_differ"] = int((route.wall() != w.wall).sum())
            out[f"route.{key}.wall"], out[f"route.{key}.device"] = timed(getattr(route, sname), max(2, reps // 10))
    e.check()
    vec.close()
    print(json.dumps(out), flush=True)


def loop_window(kind, steps, warmup):
    """Hallway x 4096: us per step of a random-action loop, with an ego_update (33 x 33, three planes) per step or without"""
    import torch
    vec, n = make("hallway")
    g = torch.Generator(device="cuda").manual_seed(3)
    w = vec.ego_window()

    def step():
        vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
        if kind == "ego":
            vec.ego_update(w)
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
    p.add_argument("--kinds", default="ego,route", help="ego alone: a variant library (MW_ENGINE_LIB) against the product")
    p.add_argument("--loop", action="store_true")
    p.add_argument("--steps", type=int, default=600)
    p.add_argument("--warmup", type=int, default=100)
    p.add_argument("--window", choices=["ego", "route", "plain"], help=argparse.SUPPRESS)
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
            for kind in ("ego", "plain"):
                print(f"loop window: {kind}", file=sys.stderr, flush=True)
                for k, v in child(["--looped", "--window", kind, "--steps", str(args.steps), "--warmup", str(args.warmup)]).items():
                    us.setdefault(kind + "." + k, []).append(v)
        print(json.dumps({"config": "hallway", "loop": us}), flush=True)
        return
    for name in [c for c in args.configs.split(",") if c in CONFIGS]:
        us = {}
        for w in range(args.windows):
            for kind in [k for k in ("ego", "route") if k in args.kinds.split(",")]:
                print(f"{name} window {w}: {kind}", file=sys.stderr, flush=True)
                for k, v in child(["--window", kind, "--config", name, "--reps", str(args.reps)]).items():
                    us.setdefault(k, []).append(v)
        print(json.dumps({"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "windows": us}), flush=True)


if __name__ == "__main__":
    main()
