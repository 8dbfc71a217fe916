"""What a frameless rollout buys: simulated env-steps/s of MiniWorldVecEnv.rollout(plans, render=False) for T in {4, 8, 32} against
T drawn step() calls and against step(actions, repeat=T), uniform-random actions, default episode lengths, same-step auto-reset.

    python tools/perf/rollout_cost.py --config hallway     # 4096 Hallway envs
    python tools/perf/rollout_cost.py --config pickup_dr   # 2048 PickupObjects envs with domain randomisation
    python tools/perf/rollout_cost.py --config maze        # 1024 Maze envs

One config per process (a GPU job runs each under its own time limit).  One engine; per T the timed windows alternate between the
three methods (frameless, steps, repeat, frameless, ...), each preceded by a device synchronisation; medians and ranges over the
windows.  A window is `calls` x CALLS[method] calls over `calls` different plans (a "call" of the steps method is T step() calls).  The sub-steps per call of the rollout and
repeat methods are counted outside the timed loops, on the same actions once more; a drawn step() executes one step per env.
Prints one JSON line.

    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python tools/perf/rollout_cost.py --config hallway --trace 4
    python tools/perf/rollout_cost.py --summarise DIR/NAME_kernel_trace.csv --windows 5

--trace T: the plan kernel against the repeat kernel, for a kernel trace.  Constant plans (every row the call's actions) through
rollout(render=True) and the same actions through step(repeat=T), alternating windows of `calls` calls on twin engines; nothing is
timed on the host.  --summarise reads the trace, cuts every step kernel's dispatches into the windows and prints per kernel the
median duration of each window, their range and the overall median.

    python tools/perf/rollout_cost.py --window traced [--root PARENT_CHECKOUT] >> cost.jsonl
    python tools/perf/rollout_cost.py --collect cost.jsonl

--window METHOD: what a rollout trace costs and buys, ONE timed window per process (a job alternates the processes: parent untraced,
tree untraced, traced, loop, parent untraced, ...).  Hallway x 4096 (or --config), frameless, uniform-random plans, per T one window of
`calls` x WINDOW_CALLS[method] calls behind a warm-up; prints one JSON line.  The methods:
    untraced  rollout(plans, render=False) — with --root, of the checkout given there (the parent commit's, built), else of this tree
    traced    rollout(plans, render=False, trace=True): the three default fields
    loop      what a trace replaces: T x (rollout(plans[k:k + 1], render=False) + state() of the same three fields)
--collect reads the lines of such a job and prints, per T and method, the median and the range of the windows (us per call and simulated
env-steps/s) and the three comparisons of profiles/r19/README.md."""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

CONFIGS = {     # name -> env id, envs, domain_rand, actions (BASELINE.json configs 1, 3, 4)
    "hallway": ("MiniWorld-Hallway-v0", 4096, False, 3),
    "pickup_dr": ("MiniWorld-PickupObjects-v0", 2048, True, 5),
    "maze": ("MiniWorld-Maze-v0", 1024, False, 3),
}
HORIZONS = (4, 8, 32)
METHODS = ("frameless", "steps", "repeat")
CALLS = {"frameless": 20, "steps": 1, "repeat": 4}      # a window is `calls` times this many calls: every window lasts a tenth of a second or more
COUNTED = 25                                            # calls per window whose sub-steps are counted, behind the timed loop
WINDOW_METHODS = ("untraced", "traced", "loop")
WINDOW_CALLS = {"untraced": 20, "traced": 20, "loop": 1}
TRACE_FIELDS = ("agent_pos", "agent_dir", "carrying")


def window(args, env_id, n, dr, n_act):
    """one timed window per horizon of one method, in this process"""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    m = args.window
    v = MiniWorldVecEnv(env_id, n, seed=0, domain_rand=dr)
    g = torch.Generator(device="cuda").manual_seed(1)
    v.reset()
    for _ in range(args.warmup):
        v.step(torch.randint(0, n_act, (n,), generator=g, device="cuda", dtype=torch.int32))

    def run(plans, t, T, count=None):
        if m == "untraced":
            v.rollout(plans[t], render=False)
        elif m == "traced":
            v.rollout(plans[t], render=False, trace=True)
        else:
            for k in range(T):
                v.rollout(plans[t, k:k + 1], render=False)
                v.state(TRACE_FIELDS)
                if count is not None:
                    count += v.substeps.sum()
            return
        if count is not None:
            count += v.substeps.sum()

    out = {"window": m, "root": args.root or "tree", "config": args.config, "num_envs": n, "calls": args.calls, "horizons": {}}
    for T in (int(x) for x in args.horizons.split(",")):
        plans = torch.randint(0, n_act, (args.calls, T, n), generator=g, device="cuda", dtype=torch.int32)
        reps = args.calls * WINDOW_CALLS[m]
        for t in range(min(args.calls, 50)):        # (the method's kernels and buffers exist, the clocks are up)
            run(plans, t, T)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(reps):
            run(plans, t % args.calls, T)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        subs = torch.zeros((), dtype=torch.int64, device="cuda")
        for t in range(COUNTED):
            run(plans, t, T, subs)
        per_call = subs.item() / COUNTED
        out["horizons"][T] = {"call_us": round(1e6 * sec / reps, 2), "sim_steps_per_s": round(per_call * reps / sec),
                              "mean_substeps_per_env_and_call": round(per_call / n, 3)}
    from miniworld_amd.engine import EngineError
    try:
        v.engine.check()
        out["mw_check"] = "ok"
    except EngineError as e:
        out["mw_check"] = str(e)
    v.close()
    print(json.dumps(out))


def collect(path):
    rows = [json.loads(line) for line in open(path) if line.startswith("{")]
    assert all(r["mw_check"] == "ok" for r in rows)
    keys = sorted({(("parent " if r["root"] != "tree" else "") + r["window"]) for r in rows})
    by = {}
    for r in rows:
        for T, h in r["horizons"].items():
            by.setdefault((int(T), ("parent " if r["root"] != "tree" else "") + r["window"]), []).append(h)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {}
    for T in sorted({k[0] for k in by}):
        o = out.setdefault(T, {})
        for name in keys:
            h = by.get((T, name), [])
            if h:
                us, rate = [x["call_us"] for x in h], [x["sim_steps_per_s"] for x in h]
                o[name] = {"windows": len(h), "call_us": [med(us), min(us), max(us)], "sim_steps_per_s": [med(rate), min(rate), max(rate)]}
        us = lambda name: o[name]["call_us"] if name in o else None
        if us("untraced") and us("parent untraced"):
            o["tree_slower_than_parent_in_every_window"] = us("untraced")[1] > us("parent untraced")[2]
        if us("traced") and us("untraced"):
            o["traced_over_untraced_median"] = round(us("traced")[0] / us("untraced")[0], 3)
        if us("traced") and us("loop"):
            o["every_traced_window_beats_every_loop_window"] = us("traced")[2] < us("loop")[1]
            o["loop_over_traced_median"] = round(us("loop")[0] / us("traced")[0], 1)
    print(json.dumps(out, indent=1))


def summarise(path, windows):
    durs = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            if name.startswith("mw_step_plan") or name.startswith("mw_step_repeat"):
                durs.setdefault(name, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    med = lambda v: sorted(v)[len(v) // 2]
    out = {}
    for name, d in durs.items():
        d = [x[1] / 1000.0 for x in sorted(d)]
        per = len(d) // (windows + 1)       # (--trace runs one more window first, the warm-up: dropped)
        w = [round(med(d[k * per:(k + 1) * per]), 2) for k in range(1, windows + 1)]
        out[name] = {"dispatches": len(d), "window_medians_us": w, "range_us": [min(w), max(w)], "median_us": round(med(d[per:]), 2)}
    print(json.dumps(out))


def trace(args, env_id, n, dr, n_act):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    T = args.trace
    P, R = (MiniWorldVecEnv(env_id, n, seed=0, domain_rand=dr) for _ in range(2))
    g = torch.Generator(device="cuda").manual_seed(1)
    acts = torch.randint(0, n_act, (args.calls, n), generator=g, device="cuda", dtype=torch.int32)
    plans = acts[:, None, :].repeat(1, T, 1).contiguous()
    for v in (P, R):
        v.reset()
    for _ in range(args.windows + 1):       # (the first window of each is the warm-up: --summarise drops it)
        for t in range(args.calls):
            P.rollout(plans[t])
        torch.cuda.synchronize()
        for t in range(args.calls):
            R.step(acts[t], repeat=T)
        torch.cuda.synchronize()
    same = bool(torch.equal(P.obs, R.obs) and torch.equal(P.reward, R.reward))
    print(json.dumps({"config": args.config, "trace": T, "calls": args.calls, "windows": args.windows + 1, "twins_equal": same}))
    for v in (P, R):
        v.engine.check()
        v.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", choices=sorted(CONFIGS), default="hallway")
    p.add_argument("--calls", type=int, default=200, help="plans per timed window (x CALLS[method] calls)")
    p.add_argument("--windows", type=int, default=5, help="timed windows per method")
    p.add_argument("--warmup", type=int, default=400, help="step() calls before timing (episodes spread over their length)")
    p.add_argument("--horizons", default=",".join(map(str, HORIZONS)))
    p.add_argument("--trace", type=int, default=0, metavar="T")
    p.add_argument("--summarise", metavar="KERNEL_TRACE_CSV")
    p.add_argument("--window", choices=WINDOW_METHODS)
    p.add_argument("--root", help="--window: the checkout whose package and library run (default: this tree)")
    p.add_argument("--collect", metavar="JSONL")
    args = p.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.windows)
    if args.collect:
        return collect(args.collect)
    if args.root:
        sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id, n, dr, n_act = CONFIGS[args.config]
    if args.window:
        return window(args, env_id, n, dr, n_act)
    if args.trace:
        return trace(args, env_id, n, dr, n_act)
    v = MiniWorldVecEnv(env_id, n, seed=0, domain_rand=dr)
    g = torch.Generator(device="cuda").manual_seed(1)
    v.reset()
    for _ in range(args.warmup):
        v.step(torch.randint(0, n_act, (n,), generator=g, device="cuda", dtype=torch.int32))
    out = {"config": args.config, "env_id": env_id, "num_envs": n, "calls": args.calls, "horizons": {}}

    def run(method, T, plans, t):
        if method == "frameless":
            v.rollout(plans[t], render=False)
        elif method == "repeat":
            v.step(plans[t, 0], repeat=T)
        else:
            for k in range(T):
                v.step(plans[t, k])

    for T in (int(x) for x in args.horizons.split(",")):
        plans = torch.randint(0, n_act, (args.calls, T, n), generator=g, device="cuda", dtype=torch.int32)
        secs = {m: [] for m in METHODS}
        subs = {m: torch.zeros((), dtype=torch.int64, device="cuda") for m in METHODS}
        counted = 0
        for m in METHODS:       # (every method's kernels and buffers exist before the first timed window)
            run(m, T, plans, 0)
        for w in range(args.windows):
            for m in METHODS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in range(args.calls * CALLS[m]):
                    run(m, T, plans, t % args.calls)
                torch.cuda.synchronize()
                secs[m].append((time.perf_counter() - t0) / CALLS[m])
                for t in range(COUNTED):
                    run(m, T, plans, t)
                    subs[m] += v.substeps.sum() if m != "steps" else T * n
            counted += COUNTED
        per_call = {m: subs[m].item() / max(counted, 1) for m in METHODS}       # simulated steps per call, the whole batch
        rate = {m: sorted(per_call[m] * args.calls / s for s in secs[m]) for m in METHODS}
        med = {m: r[len(r) // 2] for m, r in rate.items()}
        out["horizons"][T] = {
            "sim_steps_per_s": {m: round(med[m]) for m in METHODS},
            "sim_steps_per_s_range": {m: [round(rate[m][0]), round(rate[m][-1])] for m in METHODS},
            "call_us": {m: round(1e6 * sorted(secs[m])[len(secs[m]) // 2] / args.calls, 1) for m in METHODS},
            "mean_substeps_per_env_and_call": {m: round(per_call[m] / n, 3) for m in METHODS},
            "frameless_over_steps": round(med["frameless"] / med["steps"], 2),
            "frameless_over_repeat": round(med["frameless"] / med["repeat"], 2)}
    from miniworld_amd.engine import EngineError
    try:
        v.engine.check()
        out["mw_check"] = "ok"
    except EngineError as e:
        out["mw_check"] = str(e)
    v.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
