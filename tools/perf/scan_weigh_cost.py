"""What scan weighing and resampling cost (mw_scan_weigh, mw_resample; MiniWorldVecEnv.scan_weigh, resample) on the Maze's default
scan-map grid at (N, P, R) = (1024, 256, 256), (1024, 1024, 256) and (256, 4096, 1024), beside the route they replace — the same rules
as torch tensor operations: N * P * R float64 end points and a gather of as many bytes; a cumsum and a searchsorted.

    python tools/perf/scan_weigh_cost.py            # per shape: three alternating windows of each route; one JSON line each
    python tools/perf/scan_weigh_cost.py --forms    # Maze x 1024: either launch form forced at P = 16 .. 4096, R = 64, 256, 1024; one JSON line per R

The state: a ScanMap after one lidar scan; the score plane is its obstacle plane times 255; the particles are spread over each env's
extent under any turn.  A window measures the device time per call between two events around its back-to-back calls (launch gaps
included: an upper bound of the kernel's duration) and the wall time per call.  Before the windows the elements in which the torch
route differs from the kernels are counted: 0 is asserted.
The record: whether every kernel window lies below every torch window; nothing here is a threshold."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), ROOT]

from nav_cost import timed  # noqa: E402

SHAPES, SWEEP_P, SWEEP_R, RANGE = ((1024, 256, 256), (1024, 1024, 256), (256, 4096, 1024)), (16, 32, 64, 128, 256, 512, 1024, 2048, 4096), (64, 256, 1024), 10.0


def torch_weigh(score, t, d, pose, max_range, lo, cell, budget=1 << 25):
    """the route: (score int32[N, P], inside int32[N, P]); pose [N, P, 4], lo [N, 2] the envs' min_x, min_z"""
    import torch
    n, gz, gx = score.shape
    P, R, bound = pose.shape[1], t.shape[1], 2.0 ** 30
    out, inside = (torch.empty((n, P), dtype=torch.int32, device=score.device) for _ in range(2))
    chunk = max(1, budget // (P * R))
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        tt, gu, gw = t[a:b, None, :], (d[a:b, :, 0] / cell)[:, None, :], (d[a:b, :, 1] / cell)[:, None, :]
        u0, w0 = ((pose[a:b, :, 0] - lo[a:b, None, 0]) / cell)[..., None], ((pose[a:b, :, 1] - lo[a:b, None, 1]) / cell)[..., None]
        c, s = pose[a:b, :, 2, None], pose[a:b, :, 3, None]
        u1, w1 = u0 + tt * (c * gu + s * gw), w0 + tt * (c * gw - s * gu)
        ok = (tt >= 0.0) & (tt < max_range)
        for v in (u0, w0, u1, w1):
            ok = ok & (v.abs() < bound)
        row, col = torch.floor(w1), torch.floor(u1)
        ok = ok & (row >= 0.0) & (row < gz) & (col >= 0.0) & (col < gx)
        flat = torch.where(ok, row * gx + col, torch.zeros_like(row)).to(torch.int64).reshape(b - a, -1)
        seen = score[a:b].reshape(b - a, -1).gather(1, flat).reshape(b - a, P, R)       # the gather
        out[a:b], inside[a:b] = torch.where(ok, seen, torch.zeros_like(seen)).sum(-1, dtype=torch.int32), ok.sum(-1, dtype=torch.int32)
    return out, inside


def torch_resample(weight, offset):
    """the route: ancestor int32[N, P]; weight int64[N, P] in 0 .. 2^32 - 1, offset int64[N] >= 0"""
    import torch
    P = weight.shape[1]
    C = weight.cumsum(1)
    S = C[:, -1:]
    j = torch.arange(P, device=weight.device)[None]
    T = (j * S + offset[:, None] % S.clamp(min=1)) // P
    return torch.where(S > 0, torch.searchsorted(C, T, right=True), j).to(torch.int32)


def state(n, P, R, seed=11):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    vec = MiniWorldVecEnv("MiniWorld-Maze-v0", n, seed=0)
    vec.reset()
    m, scan = vec.scan_map(), vec.lidar(R, max_range=RANGE)
    vec.scan_map_update(m, scan)
    g = torch.Generator(device="cuda").manual_seed(seed)
    ext = vec.state(("extent",))["extent"]
    u = torch.rand((n, P, 4), generator=g, device="cuda", dtype=torch.float64)
    poses = torch.stack([ext[:, None, 0] + u[..., 0] * (ext[:, None, 1] - ext[:, None, 0]), ext[:, None, 2] + u[..., 1] * (ext[:, None, 3] - ext[:, None, 2]),
                         u[..., 2] * 6.283185307179586, u[..., 3]], -1).contiguous()
    return vec, m, scan, (m.obstacle * 255).contiguous(), poses, ext[:, [0, 2]].contiguous()


def cost(n, P, R, reps, windows):
    import torch
    vec, m, scan, score, poses, lo = state(n, P, R)
    r = vec.scan_weigh(score, scan, poses, max_range=RANGE, like=m)
    want = torch_weigh(score, scan["t"], scan["dir"], r.pose, RANGE, lo, m.cell)
    weights = r.score.long() + 1
    offset = torch.randint(0, 2 ** 62, (n,), device="cuda")
    drawn = vec.resample(weights, offset, poses)
    differing = int((want[0] != r.score).sum() + (want[1] != r.inside).sum() + (torch_resample(weights, offset) != drawn["ancestor"]).sum())
    assert differing == 0, differing
    routes = {"weigh_kernel": lambda: vec.scan_weigh(score, scan, poses, into=r), "weigh_torch": lambda: torch_weigh(score, scan["t"], scan["dir"], r.pose, RANGE, lo, m.cell),
              "resample_kernel": lambda: vec.resample(weights, offset, poses, into=drawn), "resample_torch": lambda: torch.gather(poses, 1, torch_resample(weights, offset).long()[..., None].expand(-1, -1, 4))}
    rec = {"envs": n, "particles": P, "beams": R, "grid": [m.gz, m.gx], "differing": differing, "device_us": {k: [] for k in routes}, "wall_us": {k: [] for k in routes}}
    for _ in range(windows):
        for k, fn in routes.items():
            wall, device = timed(fn, 2 if k == "weigh_torch" else reps)
            rec["device_us"][k].append(device), rec["wall_us"][k].append(wall)
    for k in ("weigh", "resample"):
        rec[k + "_kernel_below_torch"] = max(rec["device_us"][k + "_kernel"]) < min(rec["device_us"][k + "_torch"])
    vec.close()
    return rec


def forms(R, reps, windows, n=1024):
    vec, m, scan, score, poses, _ = state(n, max(SWEEP_P), R)
    rec = {"envs": n, "beams": R, "grid": [m.gz, m.gx], "device_us": {}}
    for P in SWEEP_P:
        part = poses[:, :P].contiguous()
        r = vec.scan_weigh(score, scan, part, max_range=RANGE, like=m)
        rec["device_us"][P] = {1: [], 2: []}
        for _ in range(windows):
            for form in (1, 2):
                vec.engine.debug_set_weigh_form(form)
                rec["device_us"][P][form].append(timed(lambda: vec.scan_weigh(score, scan, part, into=r), reps)[1])
        vec.engine.debug_set_weigh_form(0)
    vec.close()
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    a = ap.parse_args()
    for job in (SWEEP_R if a.forms else SHAPES):
        print(json.dumps(forms(job, a.reps, a.windows) if a.forms else cost(*job, a.reps, a.windows)), flush=True)
