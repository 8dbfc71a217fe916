"""What reading and writing env state on the device costs (mw_get_state_device / mw_set_state_where; MiniWorldVecEnv.state /
set_state_where), for Hallway x 4096, PickupObjects (domain randomisation) x 2048 and Maze x 1024, against the only route the parent
commit has: engine.get_state() and engine.set_state() + a render, through the host.

    python tools/perf/state_view_cost.py --parent <built checkout of the parent commit>
                                            # per config: alternating windows, a process per window — this tree's calls, then the
                                            # parent's host route run ON THE PARENT CHECKOUT; one JSON line per config
    python tools/perf/state_view_cost.py --bench <parent checkout>
                                            # `python bench.py --windows 5` alternately in the parent checkout and in this tree
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o sv -- python tools/perf/state_view_cost.py --profile hallway
                                            # a run of its own, no counters: the two kernels' durations (state() with the default
                                            # fields and with all fields, set_state_where of the pose under a 10 % mask, a step between)

A window of this tree measures, each between two device synchronisations:
    state_default / state_all        vec.state() with the default fields / with every field: wall us per call, and the device time
                                     per call between two events around the window's back-to-back calls (launch gaps included: an
                                     upper bound of the kernel's duration; the profiled run gives the kernel alone)
    set_where / set_where_render     engine.set_state_where of agent_pos + agent_dir under a 10 % mask alone / vec.set_state_where (the
                                     same plus its render); set_where_all_render: every field
    step / step_state                us per step of a step() loop with uniform-random actions, without and with one state() per step
A window of the parent measures engine.get_state() (all fields: the host route has no subset that saves its synchronisation),
engine.set_state(pose) + render and engine.set_state(every field) + render over the whole batch — the host route to "write 10 % of
the envs" is a read of the batch, a change of rows on the host and a write of the batch — and the same step loop."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {
    "hallway": ("MiniWorld-Hallway-v0", 4096, 3, {}),
    "pickup_dr": ("MiniWorld-PickupObjects-v0", 2048, 5, {"domain_rand": True}),
    "maze": ("MiniWorld-Maze-v0", 1024, 3, {}),
}
POSE = ("agent_pos", "agent_dir")


def make(name, warmup):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n, n_act, kw = CONFIGS[name]
    vec = MiniWorldVecEnv(env_id, n, seed=0, **kw)
    vec.reset()
    g = torch.Generator(device="cuda").manual_seed(1)
    step = lambda: vec.step(torch.randint(0, n_act, (n,), generator=g, device="cuda", dtype=torch.int32))     # noqa: E731
    for _ in range(warmup):
        step()
    return vec, n, g, step


def timed(fn, reps, events=False):
    """wall us per call between two synchronisations; with events also the device time per call between two events"""
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if events else (None, None)
    t0 = time.perf_counter()
    if events:
        a.record()
    for _ in range(reps):
        fn()
    if events:
        b.record()
    torch.cuda.synchronize()
    wall = 1e6 * (time.perf_counter() - t0) / reps
    return (round(wall, 2), round(1e3 * a.elapsed_time(b) / reps, 2)) if events else round(wall, 2)


def window(name, tree, reps, warmup):
    import torch
    from miniworld_amd import engine as eng
    vec, n, g, step = make(name, warmup)
    e = vec.engine
    out = {}
    if tree == "tree":
        every = tuple(eng.STATE_FIELDS)
        mask = (torch.rand(n, generator=g, device="cuda") < 0.1).to(torch.uint8)
        out["masked_envs"] = int(mask.sum())
        rows = {k: t.clone() for k, t in vec.state(every).items()}
        pose = {k: rows[k] for k in POSE}
        out["state_default_wall"], out["state_default_device"] = timed(lambda: vec.state(), reps, True)
        out["state_all_wall"], out["state_all_device"] = timed(lambda: vec.state(every), reps, True)
        out["set_where_wall"], out["set_where_device"] = timed(lambda: e.set_state_where(mask, pose), reps, True)
        out["set_where_render_wall"] = timed(lambda: vec.set_state_where(mask, **pose), reps)
        out["set_where_all_render_wall"] = timed(lambda: vec.set_state_where(mask, **rows), reps)
        out["step_wall"] = timed(step, reps)
        out["step_state_wall"] = timed(lambda: (step(), vec.state()), reps)
    else:
        host = max(3, reps // 20)
        st = e.get_state()
        pose = {k: st[k] for k in POSE}
        out["host_get_state_wall"] = timed(lambda: e.get_state(), host)
        out["host_set_pose_render_wall"] = timed(lambda: (e.set_state(pose), e.render(vec.obs, vec.depth)), host)
        out["host_set_all_render_wall"] = timed(lambda: (e.set_state(st), e.render(vec.obs, vec.depth)), host)
        out["step_wall"] = timed(step, reps)
        out["step_get_state_wall"] = timed(lambda: (step(), e.get_state()), host)
    e.check()
    vec.close()
    print(json.dumps(out), flush=True)


def child(root, extra, timeout=600):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root] + extra, cwd=root, capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        print(json.dumps({"root": root, "args": extra, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
        raise SystemExit(1)
    return json.loads(line[-1])


def compare(parent, names, windows, reps, warmup):
    for name in names:
        us = {}
        for _ in range(windows):
            for tag, root in (("tree", ROOT), ("parent", parent)):
                res = child(root, ["--window", tag, "--config", name, "--reps", str(reps), "--warmup", str(warmup)])
                for k, v in res.items():
                    us.setdefault(tag + "." + k, []).append(v)
        med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
        below = {"state_all_below_host_get_state_in_every_window": max(us["tree.state_all_wall"]) < min(us["parent.host_get_state_wall"]),
                 "set_where_all_render_below_host_set_all_render_in_every_window":
                     max(us["tree.set_where_all_render_wall"]) < min(us["parent.host_set_all_render_wall"])}
        print(json.dumps({"config": name, "env_id": CONFIGS[name][0], "num_envs": CONFIGS[name][1], "calls_per_window": reps, "median_us": med,
                          "windows_us": us, **below}), flush=True)


def bench_alternation(parent, rounds, windows):
    """bench.py in the parent checkout and in this tree, alternately; prints each run's JSON result line tagged with its tree"""
    for r in range(rounds):
        for tag, root in (("parent", parent), ("tree", ROOT)):
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--windows", str(windows), "--no-also", "--no-pmc", "--no-cpu-baseline", "--no-parity-check"],
                               cwd=root, capture_output=True, text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not line:
                print(json.dumps({"tree": tag, "round": r, "error": (p.stdout + p.stderr)[-2000:]}), flush=True)
                raise SystemExit(1)
            print(json.dumps({"tree": tag, "round": r, "result": json.loads(line[-1])}), flush=True)


def profile(name, reps, warmup):
    """the run a profiler wraps: untimed"""
    import torch
    from miniworld_amd import engine as eng
    vec, n, g, step = make(name, warmup)
    mask = (torch.rand(n, generator=g, device="cuda") < 0.1).to(torch.uint8)
    pose = {k: t.clone() for k, t in vec.state(POSE).items()}
    for _ in range(reps):
        vec.state()
        vec.state(tuple(eng.STATE_FIELDS))
        vec.engine.set_state_where(mask, pose)
        step()
    torch.cuda.synchronize()
    vec.engine.check()
    vec.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="hallway,pickup_dr,maze")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=200, help="calls per timed window (the host routes: a twentieth)")
    p.add_argument("--warmup", type=int, default=50, help="steps before anything is measured")
    p.add_argument("--parent", metavar="PARENT", help="a built checkout of the parent commit: the host route is measured there")
    p.add_argument("--bench", metavar="PARENT", help="a built checkout of the parent commit: alternate bench.py between it and this tree")
    p.add_argument("--rounds", type=int, default=1)
    p.add_argument("--profile", choices=sorted(CONFIGS), help="one config, untimed: the run a profiler wraps")
    p.add_argument("--window", choices=["tree", "parent"], help=argparse.SUPPRESS)
    p.add_argument("--config", choices=sorted(CONFIGS), help=argparse.SUPPRESS)
    p.add_argument("--root", help=argparse.SUPPRESS)
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else ROOT)      # (a window: the package of that tree)
    if args.window:
        return window(args.config, args.window, args.reps, args.warmup)
    if args.profile:
        return profile(args.profile, args.reps, args.warmup)
    if args.bench:
        return bench_alternation(os.path.abspath(args.bench), args.rounds, args.windows)
    if not args.parent:
        p.error("need --parent <built checkout of the parent commit> (the baseline is never this tree), --bench or --profile")
    compare(os.path.abspath(args.parent), [c for c in args.configs.split(",") if c in CONFIGS], args.windows, args.reps, args.warmup)


if __name__ == "__main__":
    main()
