"""What scan evidence costs (mw_scan_evidence; MiniWorldVecEnv.scan_evidence_update) for Hallway x 4096, FourRooms x 4096 and Maze x 1024,
beside the parent's kernel (scan_map_update, the natural floor) and beside the same rule as torch tensor operations — the closed form
broadcast over [envs, beams, lines] in chunks of envs, the (env, beam, cell) keys made unique, a scatter_add_ of the passes and hits,
the clamp and the thresholds.

    python tools/perf/evidence_cost.py              # per config: five alternating windows, a process per window; one JSON line each
    python tools/perf/evidence_cost.py --ab LIB     # kernel windows alternately with the product library and the variant library LIB

A window measures device us per call between two events around back-to-back calls (tools/perf/nav_cost.py: timed; launch gaps included:
an upper bound of the kernel's duration).  A kernel window times, on a held lidar() scan at 64, 256 and 1024 beams: the update with all
outputs, the update without `map` and `score`, and scan_map_update.  A torch window first counts the elements of ev, map, score and
count in which the route differs from the kernel over two updates — 0 is asserted — and times the route at 256 beams.  The record:
whether every kernel window lies below every torch window; nothing here is a threshold."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nav_cost import CONFIGS, timed  # noqa: E402

RAYS, MAX_RANGE = (64, 256, 1024), 10.0


def _run(extra, timeout=900, lib=None):
    import subprocess
    env = dict(os.environ, MW_ENGINE_LIB=os.path.abspath(lib)) if lib else None
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        print(json.dumps({"args": extra, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
        raise SystemExit(1)
    return json.loads(line[-1])


def torch_evidence(m, lo, pos, t, d, chunk_elems=1 << 24):
    """the route, into the ScanEvidence-like record `m` (ev, map, score, count): the rule of include/mwengine.h as tensor operations"""
    import torch
    n, R = t.shape
    gx, gz, cell, bound, cells = m.gx, m.gz, m.cell, 2.0 ** 30, m.gx * m.gz
    hit_w, miss_w, cap, lo_c, hi_c, free_at, occ_at = m.rule
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
        beam = (torch.arange(k, device=t.device)[:, None] * R + torch.arange(R, device=t.device)[None, :]) * (cells + 1)      # [k, R]: the key's high part

        def keys(row, col, ok, b):
            """(env, beam, cell) keys of the entries that count, the others on their beam's spare cell"""
            ok = ok & (row >= 0) & (row < gz) & (col >= 0) & (col < gx)
            return (b + torch.where(ok, row * gx + col, float(cells)).long()).reshape(-1)

        found = [keys(w0.floor().expand_as(e), u0.floor().expand_as(e), keep, beam)]
        for a0, a1, g, b0, h, lines, x_lines in ((u0, u1, gu, w0, gw, gx, True), (w0, w1, gw, u0, gu, gz, False)):
            L = torch.arange(lines + 1, dtype=torch.float64, device=t.device)[None, None, :]
            g_, a0_, a1_, b0_ = g[:, :, None], a0[:, :, None], a1[:, :, None], b0[:, :, None]
            crossed = torch.where(g_ > 0, (L >= a0_.floor() + 1) & (L <= a1_.floor()), (g_ < 0) & (L >= a1_.floor() + 1) & (L <= a0_.floor()))
            other = (b0_ + (L - a0_) / g_ * h[:, :, None]).floor()
            own = torch.where(g_ > 0, L, L - 1).expand_as(other)
            found.append(keys(*((other, own) if x_lines else (own, other)), crossed & keep[:, :, None], beam[:, :, None]))
        once = torch.unique(torch.cat(found))
        env_of, cell_of = once // ((cells + 1) * R), once % (cells + 1)
        passes = torch.zeros((k, cells + 1), dtype=torch.int32, device=t.device)
        passes.view(-1).scatter_add_(0, env_of * (cells + 1) + cell_of, torch.ones_like(once, dtype=torch.int32))
        ends = keys(w1.floor(), u1.floor(), keep & hit, beam)
        hits = torch.zeros((k, cells + 1), dtype=torch.int32, device=t.device)
        hits.view(-1).scatter_add_(0, ends // ((cells + 1) * R) * (cells + 1) + ends % (cells + 1), torch.ones_like(ends, dtype=torch.int32))
        hits, passes = hits[:, :-1].reshape(k, gz, gx), passes[:, :-1].reshape(k, gz, gx)
        delta = torch.where(hits > 0, hit_w * hits.clamp(max=cap), -miss_w * passes.clamp(max=cap))
        after = (m.ev[s].to(torch.int32) + delta).clamp(lo_c, hi_c)
        m.ev[s] = after.to(torch.int8)
        m.map[s, 0], m.map[s, 1] = (after <= free_at).to(torch.uint8), (after >= occ_at).to(torch.uint8)
        m.score[s] = after.clamp(min=0).to(torch.uint8)
        m.count[s] = m.map[s].sum(dim=(2, 3), dtype=torch.int32)


def window(name, kind, reps):
    import torch
    from miniworld_amd.queries import ScanEvidence
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0, want_depth=False)
    vec.reset()
    g = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(10):
        vec.step(torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32))
    out = {}
    for R in RAYS if kind == "kernel" else (256,):
        m = vec.scan_evidence(rays=R, max_range=MAX_RANGE)
        out["cells"] = m.gx * m.gz
        scan = {k: v.clone() for k, v in vec.lidar(R, m.fov, MAX_RANGE, obstacles=m.obstacles).items()}
        if kind == "kernel":
            bare = ScanEvidence(m.ev.clone(), None, None, m.count.clone(), None, m.params, R, m.fov, MAX_RANGE, m.obstacles, m.rule)
            binary = vec.scan_map(like=m, rays=R, max_range=MAX_RANGE)
            out[f"evidence_device_{R}"] = timed(lambda: vec.scan_evidence_update(m, scan), reps)[1]
            out[f"evidence_bare_device_{R}"] = timed(lambda: vec.scan_evidence_update(bare, scan), reps)[1]
            out[f"scan_map_device_{R}"] = timed(lambda: vec.scan_map_update(binary, scan), reps)[1]
            continue
        pos = vec.state(("agent_pos",))["agent_pos"][:, [0, 2]].contiguous()
        lo = torch.as_tensor(vec.engine.get_state()["extent"], device="cuda", dtype=torch.float64)[:, [0, 2]].contiguous()
        theirs = vec.scan_evidence(like=m, rays=R, max_range=MAX_RANGE)
        for _ in range(2):
            vec.scan_evidence_update(m, scan)
            torch_evidence(theirs, lo, pos, scan["t"], scan["dir"])
        differ = sum(int((getattr(m, f) != getattr(theirs, f)).sum()) for f in ("ev", "map", "score", "count"))
        assert differ == 0, ("the route's evidence is another", differ)
        out["differ"] = differ
        out[f"torch_device_{R}"] = timed(lambda: torch_evidence(theirs, lo, pos, scan["t"], scan["dir"]), max(2, reps // 20))[1]
    vec.engine.check()
    vec.close()
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="hallway,fourrooms,maze")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--ab", metavar="LIB", help="a variant engine library: kernel windows alternately without and with it, nothing else")
    p.add_argument("--window", choices=["kernel", "torch"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    if args.window:
        return window(args.config, args.window, args.reps)
    names = [c for c in args.configs.split(",") if c in CONFIGS]
    for name in names:
        us = {}
        sides = (("product", "kernel", None), ("variant", "kernel", args.ab)) if args.ab else (("kernel", "kernel", None), ("torch", "torch", None))
        for w in range(args.windows):
            for side, kind, lib in sides:
                print(f"{name} window {w}: {side}", file=sys.stderr, flush=True)
                for k, v in _run(["--window", kind, "--config", name, "--reps", str(args.reps)], lib=lib).items():
                    us.setdefault(f"{side}_{k}" if args.ab else k, []).append(v)
        rec = {"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "windows": us}
        if args.ab:
            rec["ab"] = args.ab
        else:
            rec["every_kernel_window_below_every_torch_window"] = max(us["evidence_device_256"]) < min(us["torch_device_256"])
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
