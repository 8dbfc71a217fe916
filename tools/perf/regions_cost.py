"""What grid regions cost (mw_grid_regions; MiniWorldVecEnv.grid_regions) for Hallway x 4096, FourRooms x 4096 and Maze x 1024 on two
masks, beside the route it replaces: label propagation by a masked 3 x 3 max-pooling to a fixed point, `scatter_add_` for the sizes and
sums, a `scatter_reduce_(amin)` twice for the representative, a prefix sum for the scan order.

    python tools/perf/regions_cost.py               # per config: five alternating windows, a process per window; one JSON line each

The masks: `frontier`, the frontier cells of a DepthMap after --map-steps random steps (8-connected, regions of 2 cells and more, as
examples/cluster_explore.py asks for them), and `free`, the unblocked cells of a privileged nav field (4-connected, every region);
32 listed regions, with labels and sums.  A window measures, each between two device synchronisations: wall us per call, and the device
time per call between two events around the window's back-to-back calls (launch gaps included: an upper bound of the kernel's
duration).  A kernel window also times the call without the optional outputs.  A torch window first counts the elements of count, size, cell, sum and label in which the route differs from the
kernel: 0 is asserted.
The record: whether every kernel window lies below every torch window; nothing here is a threshold."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nav_cost import CONFIGS, timed  # noqa: E402

MASKS = {"frontier": (8, 2), "free": (4, 1)}        # connectivity, min_cells
K = 32


def _run(extra, timeout=900):
    """this file again as a process of its own, under its own time limit: the JSON line it prints"""
    import subprocess
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        print(json.dumps({"args": extra, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
        raise SystemExit(1)
    return json.loads(line[-1])


def torch_regions(member, connectivity, min_cells, k_max, check_every=8):
    """the route: (count int32[N], size int32[N, K], cell int32[N, K], sum int32[N, K, 2], label int16[N, gz, gx], rounds)"""
    import torch
    import torch.nn.functional as F
    n, gz, gx = member.shape
    cells, dev = gz * gx, member.device
    idx = torch.arange(cells, device=dev).view(1, gz, gx)
    # a label is cells - index, 0 off the mask: the largest label of a region is its lowest index (float32 holds 32768 exactly)
    lab = torch.where(member, cells - idx, 0).to(torch.float32)[:, None]
    inside = member[:, None]
    rounds = 0
    while True:
        for r in range(check_every):
            if connectivity == 8:
                pooled = F.max_pool2d(lab, 3, 1, 1)
            else:
                pooled = torch.maximum(F.max_pool2d(lab, (1, 3), 1, (0, 1)), F.max_pool2d(lab, (3, 1), 1, (1, 0)))
            new = torch.where(inside, pooled, 0.0)
            same = torch.equal(new, lab) if r == check_every - 1 else False         # (one host read per check_every rounds)
            lab = new
            rounds += 1
        if same:
            break
    flat = member.reshape(n, cells)
    root = torch.where(flat, cells - lab.reshape(n, cells).to(torch.int64), 0)
    one = flat.to(torch.int64)
    at = torch.arange(cells, device=dev)
    size_at = torch.zeros((n, cells), dtype=torch.int64, device=dev).scatter_add_(1, root, one)
    sj_at = torch.zeros_like(size_at).scatter_add_(1, root, one * (at // gx))
    si_at = torch.zeros_like(size_at).scatter_add_(1, root, one * (at % gx))
    qualified = size_at >= min_cells
    rank = qualified.cumsum(1) - 1
    count = qualified.sum(1).to(torch.int32)
    listed = qualified & (rank < k_max)
    # the representative: the least distance per root, then the lowest cell at it
    s, sj, si = (t.gather(1, root) for t in (size_at, sj_at, si_at))
    d = torch.where(flat, (s * (at // gx) - sj) ** 2 + (s * (at % gx) - si) ** 2, torch.iinfo(torch.int64).max)
    d_at = torch.full((n, cells), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev).scatter_reduce_(1, root, d, "amin")
    cand = torch.where(flat & (d == d_at.gather(1, root)), at, cells)
    cell_at = torch.full((n, cells), cells, dtype=torch.int64, device=dev).scatter_reduce_(1, root, cand, "amin")
    slot = torch.where(listed, rank, k_max)
    pick = lambda t, fill: torch.full((n, k_max + 1), fill, dtype=torch.int64, device=dev).scatter_(1, slot, torch.where(listed, t, fill))[:, :k_max]   # noqa: E731
    size, cell = pick(size_at, 0).to(torch.int32), pick(cell_at, -1).to(torch.int32)
    total = torch.stack([pick(sj_at, 0), pick(si_at, 0)], dim=2).to(torch.int32)
    code_at = torch.where(listed, rank + 1, -1)
    label = torch.where(flat, code_at.gather(1, root), 0).to(torch.int16).view(n, gz, gx)
    return count, size, cell, total, label, rounds


def masks_of(vec, n, map_steps):
    """{"frontier": bool[N, gz, gx], "free": bool[N, gz, gx]} and the grid they share"""
    import torch
    from depth_plan_explore import frontier_of
    g = torch.Generator(device="cuda").manual_seed(5)
    m = vec.depth_map(max_range=8.0)
    vec.depth_map_update(m)
    for _ in range(map_steps):
        vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
        vec.depth_map_update(m)
    frontier, _ = frontier_of(m)
    f = vec.nav_field()
    assert (f.gz, f.gx) == (m.gz, m.gx)
    return {"frontier": frontier.contiguous(), "free": (f.field.view(torch.int16) != -1).contiguous()}, m


def window(name, kind, reps, map_steps):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0, want_depth=True)
    vec.reset()
    masks, m = masks_of(vec, n, map_steps)
    out = {"cells": m.gx * m.gz}
    for which, member in masks.items():
        conn, min_cells = MASKS[which]
        r = vec.grid_regions(member, connectivity=conn, min_cells=min_cells, max_regions=K, like=m, labels=True)
        out[f"{which}_share"] = round(float(member.float().mean()), 4)
        out[f"{which}_count_mean"], out[f"{which}_count_max"] = round(float(r.count.float().mean()), 1), int(r.count.max())
        if kind == "kernel":
            bare = vec.grid_regions(member, connectivity=conn, min_cells=min_cells, max_regions=K, like=m, sums=False)
            out[f"kernel_wall_{which}"], out[f"kernel_device_{which}"] = timed(lambda: vec.grid_regions(member, into=r), reps)
            out[f"kernel_bare_wall_{which}"], out[f"kernel_bare_device_{which}"] = timed(lambda: vec.grid_regions(member, into=bare), reps)
            continue
        *route, rounds = torch_regions(member, conn, min_cells, K)
        differ = sum(int((a != b).sum()) for a, b in zip(route, (r.count, r.size, r.cell, r.sum, r.label)))
        assert differ == 0, ("the route's regions are others", which, differ)
        out[f"differ_{which}"], out[f"torch_rounds_{which}"] = differ, rounds
        out[f"torch_wall_{which}"], out[f"torch_device_{which}"] = timed(lambda: torch_regions(member, conn, min_cells, K), max(2, reps // 20))
    vec.engine.check()
    vec.close()
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="hallway,fourrooms,maze")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--map-steps", type=int, default=40, help="random steps the DepthMap accumulates over")
    p.add_argument("--window", choices=["kernel", "torch"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window:
        return window(args.config, args.window, args.reps, args.map_steps)
    for name in [c for c in args.configs.split(",") if c in CONFIGS]:
        us = {}
        for w in range(args.windows):
            for kind in ("kernel", "torch"):
                print(f"{name} window {w}: {kind}", file=sys.stderr, flush=True)
                for k, v in _run(["--window", kind, "--config", name, "--reps", str(args.reps), "--map-steps", str(args.map_steps)]).items():
                    us.setdefault(k, []).append(v)
        below = all(max(us[f"kernel_device_{w}"]) < min(us[f"torch_device_{w}"]) and max(us[f"kernel_wall_{w}"]) < min(us[f"torch_wall_{w}"]) for w in MASKS)
        print(json.dumps({"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "regions": K, "windows": us,
                          "every_kernel_window_below_every_torch_window": below}), flush=True)


if __name__ == "__main__":
    main()
