"""What an object projection costs (mw_label_project; MiniWorldVecEnv.object_update / object_map_update) for Hallway x 4096, FourRooms x 4096
and PickupObjects x 2048 under domain randomisation — the window at 33 x 33 cells of 0.25 m, the map on the nav field's grid with `ids` at
its default — against the route a user has without it, written here with nothing this call added: the same unprojection as torch tensor
operations in float64 over [N, H * W], the class by height, an index computation, a `scatter_reduce_(amin)` of the keys, the merge into
the map and the per-id counts and centroids as `scatter_add_`s.  Every window of the route first counts the cells in which its result
differs from the kernel's (cells_that_differ: the plane, the map, the cell counts; the route takes sin and cos of the camera from torch,
the kernel from the engine's own, so a point on a cell's border could fall on the other side).  The state: the batch after 30 random
steps, labelled with meshes="bounds".

    python tools/perf/labelmap_cost.py              # per config: five alternating windows, a process per window; one JSON line each
    MW_ENGINE_LIB=<variant> python tools/perf/labelmap_cost.py --kinds kernel     # a variant library (make EXTRA=-DMW_LABELMAP_HOLD=0) alone

A window measures, each between two device synchronisations: wall us per call, and the device time per call between two events around
the window's back-to-back calls (launch gaps included: an upper bound of the kernel's duration).  Keys: <what>.<target>, what = kernel |
route, target = window33 | map."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {
    "hallway": ("MiniWorld-Hallway-v0", 4096, False),
    "fourrooms": ("MiniWorld-FourRooms-v0", 4096, False),
    "pickup_dr": ("MiniWorld-PickupObjects-v0", 2048, True),
}
SIZE = 33
CELL = 0.25
SAMPLE0 = {8: (9, 5), 4: (6, 2), 1: (8, 8)}
UNSEEN, NONE = 0xFFFF, 0xFFFE


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
    env_id, n, domain_rand = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0, want_depth=True, domain_rand=domain_rand)
    vec.reset()
    g = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(30):
        vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
    labels = vec.label_frame(meshes="bounds")
    vec.label_update(labels)
    return vec, n, labels


class Route:
    """the projection without mw_label_project: tensor operations and scatters"""

    def __init__(self, vec, n, labels):
        import torch
        self.vec, self.n, self.labels = vec, n, labels
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
        from miniworld_amd import engine
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
        self.counts = inside & (up >= -o.floor_tol) & (up <= o.top)
        self.px = self.ox + (self.fwd * hx + self.lat * -hz)
        self.pz = self.oz + (self.fwd * hz + self.lat * hx)
        code = self.labels.code.reshape(self.n, -1)
        ident = code - engine.RAY_ENT
        self.keys = torch.where((code >= engine.RAY_ENT) & (ident <= 254), ident, NONE)

    def lowest(self, row, col, kept, n_rows, n_cols):
        """int32[N, n_rows, n_cols]: the lowest key per cell, UNSEEN where no pixel fell"""
        import torch
        cells = n_rows * n_cols
        at = self.rows * cells + row.clamp(0, n_rows - 1).long() * n_cols + col.clamp(0, n_cols - 1).long()
        m = kept & self.counts
        out = torch.full((self.n * cells,), UNSEEN, dtype=torch.int32, device="cuda")
        out.scatter_reduce_(0, at[m], self.keys[m], "amin")
        return out.reshape(self.n, n_rows, n_cols)

    def window(self, w):
        import torch
        self.points(w)
        S = w.size
        a, b = (self.px - self.ox, -(self.pz - self.oz)) if w.frame == "north" else (self.lat, self.fwd)
        c = torch.floor(a / w.cell + S * 0.5)
        r = torch.floor((S * 0.5 + w.back) - b / w.cell)
        keys = self.lowest(r, c, (c >= 0.0) & (c < S) & (r >= 0.0) & (r < S), S, S)
        return torch.where(keys <= 254, keys + 1, 0).to(torch.uint8)

    def map(self, m, into):
        """the update of `into` (uint8[N, gz, gx]) and (cells int32[N, K], pos float64[N, K, 3])"""
        import torch
        self.points(m)
        fi = torch.floor((self.px - self.ext[:, 0:1]) / m.cell)
        fj = torch.floor((self.pz - self.ext[:, 2:3]) / m.cell)
        keys = self.lowest(fj, fi, (fi >= 0.0) & (fi < float(m.gx)) & (fj >= 0.0) & (fj < float(m.gz)), m.gz, m.gx)
        torch.where(keys != UNSEEN, torch.where(keys <= 254, keys + 1, 0).to(torch.uint8), into, out=into)
        K = m.ids
        byte = into.reshape(self.n, -1).long()
        held = (byte > 0) & (byte <= K)
        at = (self.rows * K + (byte - 1).clamp(0, max(K - 1, 0)))[held]
        cell_index = torch.arange(m.gz * m.gx, device="cuda")[None, :].expand(self.n, -1)[held]
        sums = torch.zeros((3, self.n * K), dtype=torch.int64, device="cuda")
        sums[0].scatter_add_(0, at, torch.ones_like(at))
        sums[1].scatter_add_(0, at, cell_index % m.gx)
        sums[2].scatter_add_(0, at, cell_index // m.gx)
        cnt = sums[0].reshape(self.n, K)
        nd = cnt.to(torch.float64)
        x = self.ext[:, 0:1] + (sums[1].reshape(self.n, K).to(torch.float64) / nd + 0.5) * m.cell
        z = self.ext[:, 2:3] + (sums[2].reshape(self.n, K).to(torch.float64) / nd + 0.5) * m.cell
        pos = torch.stack((x, torch.where(cnt > 0, 0.0, float("nan")).to(torch.float64), z), dim=2)
        return cnt.to(torch.int32), pos


def window(name, kind, reps):
    import torch
    vec, n, labels = make(name)
    out = {}
    route = Route(vec, n, labels)
    w = vec.object_window(size=SIZE, cell=CELL)
    m = vec.object_map(cell=CELL)
    out["map.cells"], out["map.ids"] = m.gx * m.gz, m.ids
    if kind == "kernel":
        out[f"kernel.window{SIZE}.wall"], out[f"kernel.window{SIZE}.device"] = timed(lambda: vec.object_update(w, labels), reps)
        out["kernel.map.wall"], out["kernel.map.device"] = timed(lambda: vec.object_map_update(m, labels), reps)
        out["object_cells_per_env"] = round(float((m.map != 0).sum()) / n, 2)
    else:
        vec.object_update(w, labels)
        out[f"route.window{SIZE}.cells_that_differ"] = int((route.window(w) != w.plane).sum())
        out[f"route.window{SIZE}.wall"], out[f"route.window{SIZE}.device"] = timed(lambda: route.window(w), max(2, reps // 10))
        vec.object_map_update(m, labels)
        mine = torch.zeros_like(m.map)
        cells, pos = route.map(m, mine)
        out["route.map.cells_that_differ"] = int((mine != m.map).sum()) + int((cells != m.cells).sum())
        both = ~(pos.isnan() & m.pos.isnan())
        out["route.map.largest_position_difference"] = float((pos - m.pos)[both].abs().max()) if both.any() else 0.0
        out["route.map.wall"], out["route.map.device"] = timed(lambda: route.map(m, mine), max(2, reps // 10))
    vec.engine.check()
    vec.close()
    print(json.dumps(out), flush=True)


def child(extra, timeout=600):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        print(json.dumps({"args": extra, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
        raise SystemExit(1)
    return json.loads(line[-1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="hallway,fourrooms,pickup_dr")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--kinds", default="kernel,route", help="kernel alone: a variant library (MW_ENGINE_LIB) against the product")
    p.add_argument("--window", choices=["kernel", "route"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window:
        return window(args.config, args.window, args.reps)
    for name in [c for c in args.configs.split(",") if c in CONFIGS]:
        us = {}
        for w in range(args.windows):
            for kind in [k for k in ("kernel", "route") if k in args.kinds.split(",")]:
                print(f"{name} window {w}: {kind}", file=sys.stderr, flush=True)
                for k, v in child(["--window", kind, "--config", name, "--reps", str(args.reps)]).items():
                    us.setdefault(k, []).append(v)
        print(json.dumps({"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "library": os.environ.get("MW_ENGINE_LIB", "product"),
                          "windows": us}), flush=True)


if __name__ == "__main__":
    main()
