"""What grid rollouts cost (mw_grid_plan; MiniWorldVecEnv.grid_rollout) for Hallway x 4096, FourRooms x 4096 and Maze x 1024 at (P, T) =
(32, 16), (256, 32), (4096, 32): with int32 and uint8 plans, with and without a field and a cost plane, beside the route they replace
— the same rule as torch tensor operations: T dependent steps over [N, P], the engine's sine and cosine written out in + - *, a
gather of every cell of every box, a scatter of the refusals — and, at (32, 16), beside the privileged rollout(render=False, trace=)
over 32 x the envs.

    python tools/perf/grid_plan_cost.py                 # per config: three alternating windows, a process per window; one JSON line each

The state: a ScanMap after --map-steps random steps; blocked its obstacle plane, the field grid_field's to the map's frontier, extra
grid_clearance's cost.  A window measures, each between two device synchronisations: wall us per call, and the device time per call
between two events around the window's back-to-back calls (launch gaps included: an upper bound of the kernel's duration).  A torch
window first counts the elements of pose and stats in which the route differs from the kernel: 0 is asserted.  The route runs the
two smaller shapes only: at 4096 plans its boxes do not fit the device.
The record: whether every kernel window lies below every torch window; nothing here is a threshold."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nav_cost import CONFIGS, timed  # noqa: E402

SHAPES, TORCH_SHAPES, RADIUS = ((32, 16), (256, 32), (4096, 32)), ((32, 16), (256, 32)), 0.4


def _run(extra, timeout=900):
    """this file again as a process of its own, under its own time limit: the JSON line it prints"""
    import subprocess
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        print(json.dumps({"args": extra, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
        raise SystemExit(1)
    return json.loads(line[-1])


def torch_sincos(x):
    """mw::sincos_det as tensor operations, each rounded on its own"""
    import torch
    t = x * 6.36619772367581382433e-01
    fn = torch.where(t >= 0.0, torch.trunc(t + 0.5), -torch.trunc(0.5 - t))
    q = fn.to(torch.int64) & 3
    head = x - fn * 1.57079632673412561417e+00
    w = fn * 6.07710050630396597660e-11
    r = head - w
    w = fn * 2.02226624879595063154e-21 - ((head - r) - w)
    y0 = r - w
    y1 = (r - y0) - w
    z = y0 * y0
    v = z * y0
    rs = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))
    sn = y0 - ((z * (0.5 * y1 - v * rs) - y1) - v * -1.66666666666666324348e-01)
    rc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 + z * (
        2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))))
    hz = 0.5 * z
    ww = 1.0 - hz
    cs = ww + (((1.0 - ww) - hz) + (z * rc - y0 * y1))
    s = torch.where(q == 0, sn, torch.where(q == 1, cs, torch.where(q == 2, -sn, -cs)))
    c = torch.where(q == 0, cs, torch.where(q == 1, -sn, torch.where(q == 2, -cs, sn)))
    return s, c


def torch_rollout(blocked, plans, pose, step, radius, lo, cell, field, extra, stop_at, budget=1 << 25):
    """the route: (pose float64[N, P, 3], stats int32[N, P, 5]); cells outside the grid are opaque"""
    import torch
    n, gz, gx = blocked.shape
    T, P, dev = plans.shape[0], plans.shape[2], blocked.device
    rc = radius / cell
    K = torch.arange(2 * math.ceil(rc) + 3, dtype=torch.float64, device=dev)
    pose_out, stats = torch.empty((n, P, 3), dtype=torch.float64, device=dev), torch.empty((n, P, 5), dtype=torch.int32, device=dev)
    chunk = max(1, budget // (P * len(K) * len(K)))
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        m, lx, lz = b - a, lo[a:b, 0:1], lo[a:b, 1:2]
        x, z, d = (pose[a:b, k:k + 1].expand(m, P).clone() for k in range(3))
        flat_b = blocked[a:b].reshape(m, -1)
        flat_f, flat_x = (None if t is None else t[a:b].reshape(m, -1) for t in (field, extra))

        def look():
            fu, fw = torch.floor((x - lx) / cell), torch.floor((z - lz) / cell)
            ok = (fu >= 0) & (fu < gx) & (fw >= 0) & (fw < gz)
            at = torch.where(ok, fw * gx + fu, torch.zeros_like(fu)).to(torch.int64)
            v = torch.where(ok, flat_f.view(torch.int16).gather(1, at).to(torch.int32) & 0xFFFF, 0xFFFF) if flat_f is not None else torch.full((m, P), 0xFFFF, dtype=torch.int32, device=dev)
            return v, torch.where(ok, flat_x.gather(1, at).to(torch.int32), 0) if flat_x is not None else torch.zeros((m, P), dtype=torch.int32, device=dev)

        reach = look()[0]
        reach_step, steps, bumps, cost = (torch.zeros((m, P), dtype=torch.int32, device=dev) for _ in range(4))
        active = ~(reach <= stop_at) if stop_at >= 0 else torch.ones((m, P), dtype=torch.bool, device=dev)
        fwd, drift, dturn = step[0], step[1], step[2] * (math.pi / 180.0)
        for k in range(T):
            act = plans[k, a:b].to(torch.int32)
            d = torch.where(active & (act == 0), d + dturn, torch.where(active & (act == 1), d + -dturn, d))
            move = active & ((act == 2) | (act == 3))
            s, c = torch_sincos(d)
            f = torch.where(act == 2, torch.full_like(x, fwd), torch.full_like(x, -fwd))
            nx, nz = x + c * f + s * drift, z + (-s) * f + c * drift
            u, w = ((nx - lx) / cell)[..., None, None], ((nz - lz) / cell)[..., None, None]
            col, row = torch.floor(u - rc) + K[None, None, None, :], torch.floor(w - rc) + K[None, None, :, None]
            in_box = (col <= torch.floor(u + rc)) & (row <= torch.floor(w + rc))
            inside = (col >= 0) & (col < gx) & (row >= 0) & (row < gz)
            at = torch.where(inside, row * gx + col, torch.zeros_like(row * col)).to(torch.int64)
            opq = torch.where(inside, flat_b.gather(1, at.reshape(m, -1)).reshape(at.shape) != 0, True)         # the gather
            dx, dz = torch.clamp(torch.maximum(col - u, u - (col + 1.0)), min=0.0), torch.clamp(torch.maximum(row - w, w - (row + 1.0)), min=0.0)
            own = (col == torch.floor(u)) & (row == torch.floor(w))
            no = (in_box & opq & ((dx * dx + dz * dz < rc * rc) | own)).any(-1).any(-1)
            bumps += (move & no).to(torch.int32)
            go = move & ~no
            x, z = torch.where(go, nx, x), torch.where(go, nz, z)
            v, xv = look()
            cost += torch.where(active, xv, 0)
            better = active & (v < reach)
            reach, reach_step, steps = torch.where(better, v, reach), torch.where(better, k + 1, reach_step), torch.where(active, k + 1, steps)
            if stop_at >= 0:
                active = active & ~(reach <= stop_at)
        pose_out[a:b], stats[a:b] = torch.stack([x, z, d], -1), torch.stack([reach, reach_step, steps, bumps, cost], -1)
    return pose_out, stats


def window(name, kind, reps, map_steps):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n = CONFIGS[name]
    out = {}
    if kind == "privileged":        # what the call replaces at (32, 16): an env per candidate
        vec = MiniWorldVecEnv(env_id, n * 32, seed=0)
        vec.reset()
        plans = torch.randint(0, 4, (16, n * 32), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda", dtype=torch.int32)
        snap = vec.save_state()

        def call():
            vec.load_state(snap)
            vec.rollout(plans, render=False, trace=("agent_pos", "agent_dir"))
        out["privileged_wall_32x16"], out["privileged_device_32x16"] = timed(call, max(2, reps // 10))
        out["restore_wall_32x16"], out["restore_device_32x16"] = timed(lambda: vec.load_state(snap), max(2, reps // 10))
    else:
        vec = MiniWorldVecEnv(env_id, n, seed=0)
        vec.reset()
        g = torch.Generator(device="cuda").manual_seed(5)
        m = vec.scan_map()
        vec.scan_map_update(m)
        for _ in range(map_steps):
            vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
            vec.scan_map_update(m)
        blocked, free = (m.obstacle != 0).contiguous(), (m.free != 0).contiguous()
        unknown = ~(blocked | free)
        frontier = free & (torch.roll(unknown, 1, 1) | torch.roll(unknown, -1, 1) | torch.roll(unknown, 1, 2) | torch.roll(unknown, -1, 2))
        field = vec.grid_field(blocked, sources=frontier.contiguous(), like=m)
        extra = vec.grid_clearance(blocked, radii=[0.5, 1.0], costs=[8, 2], like=m).cost
        out.update(cells=m.gx * m.gz, blocked_share=round(float(blocked.float().mean()), 4))
        lo = torch.as_tensor(vec.engine.get_state()["extent"], dtype=torch.float64, device="cuda")[:, [0, 2]].contiguous()
        st = vec.state(("agent_pos", "agent_dir"))
        pose = torch.cat([st["agent_pos"][:, [0, 2]], st["agent_dir"][:, None]], 1).contiguous()
        step = [float(getattr(vec.engine.cfg, k).default) for k in ("forward_step", "forward_drift", "turn_step")]
        for P, T in (SHAPES if kind == "kernel" else TORCH_SHAPES):
            plans = torch.randint(0, 4, (T, n, P), generator=g, device="cuda", dtype=torch.int32)
            bytes_, key = plans.to(torch.uint8), f"{P}x{T}"
            scored = dict(field=field.field, extra=extra, stop_at=0)
            if kind == "kernel":
                keep = {}
                for label, pl, kw in (("i32", plans, {}), ("u8", bytes_, {}), ("i32_scored", plans, scored), ("u8_scored", bytes_, scored)):
                    call = lambda: keep.__setitem__(label, vec.grid_rollout(blocked, pl, radius=RADIUS, like=m, into=keep.get(label), **kw))      # noqa: E731
                    out[f"kernel_wall_{label}_{key}"], out[f"kernel_device_{label}_{key}"] = timed(call, reps)
                out[f"bumps_{key}"], out[f"stopped_{key}"] = round(float(keep["i32"].bumps.float().mean()), 2), round(float((keep["i32_scored"].steps < T).float().mean()), 3)
            else:
                r = vec.grid_rollout(blocked, plans, radius=RADIUS, like=m, **scored)
                route = lambda: torch_rollout(blocked, plans, pose, step, RADIUS, lo, m.cell, field.field, extra, 0)       # noqa: E731
                p, s = route()
                differ = int((p.view(torch.int64) != r.pose.view(torch.int64)).sum()) + int((s != r.stats).sum())
                assert differ == 0, ("the route's pose or stats are others", key, differ)
                out[f"differ_{key}"] = differ
                out[f"torch_wall_{key}"], out[f"torch_device_{key}"] = timed(route, 2)
    vec.engine.check()
    vec.close()
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="hallway,fourrooms,maze")
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--map-steps", type=int, default=40, help="random steps the ScanMap accumulates over")
    p.add_argument("--kinds", default="kernel,torch,privileged")
    p.add_argument("--window", choices=["kernel", "torch", "privileged"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window:
        return window(args.config, args.window, args.reps, args.map_steps)
    for name in [c for c in args.configs.split(",") if c in CONFIGS]:
        us, tail = {}, ["--config", name, "--reps", str(args.reps), "--map-steps", str(args.map_steps)]
        for w in range(args.windows):
            for kind in args.kinds.split(","):
                print(f"{name} window {w}: {kind}", file=sys.stderr, flush=True)
                for k, v in _run(["--window", kind] + tail).items():
                    us.setdefault(k, []).append(v)
        rec = {"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "radius": RADIUS, "windows": us}
        if "torch_device_32x16" in us and "kernel_device_i32_scored_32x16" in us:
            rec["every_kernel_window_below_every_torch_window"] = all(
                max(us[f"kernel_device_i32_scored_{P}x{T}"]) < min(us[f"torch_device_{P}x{T}"]) for P, T in TORCH_SHAPES)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
