"""How often an env is back in a state it was in a few steps ago — what the frame cache (mw_set_frame_cache) can save.

    python tools/perf/revisit_share.py --cpu                      # the replay, no GPU: the table of the share of revisits
    python tools/perf/revisit_share.py --gpu                      # the device: mean of mw_get_frame_source, slots 2, 4, 8
    python tools/perf/revisit_share.py --gpu --windows 5          # ... and timed windows, the engines alternating
    python tools/perf/revisit_share.py --gpu --policy left --windows 5 --slots 0,4      # the worst case: no state ever returns

--cpu replays the benchmark's policy (uniform over turn left, turn right, forward) through the CPU oracle's dynamics
(pyoracle.Dynamics; tests/helpers.py: EpisodeMirror), `--seeds` envs of `--steps` steps each over whole episodes, and compares
agent position and direction byte for byte: per family the share of all steps whose new state equals the state one step earlier
(clean: skipped by frame reuse), equals the one two steps earlier and is not clean, and lies within the last 3, 4 and 8 — with the
seed-to-seed spread (standard deviation over the seeds).  The history still holds the duplicate states of clean steps, so a cache of
distinct drawn frames does at least as well per slot.

--gpu steps one engine per slot count side by side on the same actions (4096 envs, the benchmark's size) and reports, per engine,
the shares of envs left alone as clean, copied from the cache and drawn, over `--steps` steps after `--warmup`; with --windows W the
engines then take W timed windows of `--calls` steps each in turn (slots a, b, c, a, b, c, ...), env-steps/s per window.
One JSON line per family and mode."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

FAMILIES = {"hallway": ("MiniWorld-Hallway-v0", "Hallway"), "oneroom": ("MiniWorld-OneRoom-v0", "OneRoom")}
POLICIES = {"uniform": (0, 1, 2), "left": (0,)}


def cpu_replay(family, seeds, steps):
    import numpy as np
    import helpers
    from miniworld_amd import engine as eng
    from miniworld_amd import envs
    cls = getattr(envs, FAMILIES[family][1])
    cols = ("clean", "t2_not_clean", "within_3", "within_4", "within_8")
    per_seed = []
    for s in range(seeds):
        m = helpers.EpisodeMirror(cls, 1000 + s, False, eng.TASK_GOTO)
        rng = np.random.default_rng(s)
        hist, counts = [], dict.fromkeys(cols, 0)
        for a in rng.integers(0, 3, steps):
            if not hist:
                pos, d = m.state()[0:2]
                hist.append(pos.tobytes() + np.float64(d).tobytes())
            _, te, tr = m.step(int(a))
            pos, d = m.state()[0:2]
            key = pos.tobytes() + np.float64(d).tobytes()
            if te or tr:
                hist = [key]            # a new world: nothing of the old episode returns
                continue
            back = [len(hist) >= k and hist[-k] == key for k in range(1, 9)]        # back[k - 1]: equals the state k steps earlier
            clean = back[0]
            counts["clean"] += clean
            counts["t2_not_clean"] += (not clean) and back[1]
            for depth, name in ((3, "within_3"), (4, "within_4"), (8, "within_8")):
                counts[name] += (not clean) and any(back[1:depth])
            hist = (hist + [key])[-8:]
        per_seed.append([counts[c] / steps for c in cols])
    a = np.array(per_seed)
    return {"family": family, "mode": "cpu replay", "seeds": seeds, "steps_each": steps,
            "share": dict(zip(cols, a.mean(0).round(4).tolist())), "seed_to_seed_sd": dict(zip(cols, a.std(0).round(4).tolist()))}


def gpu_run(family, args):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    env_id = FAMILIES[family][0]
    slots = [int(s) for s in args.slots.split(",")]
    acts_of = POLICIES[args.policy]
    n = args.envs
    vecs = {s: MiniWorldVecEnv(env_id, n, seed=0, frame_cache=s, want_depth=args.depth) for s in slots}
    g = torch.Generator(device="cuda").manual_seed(1)
    table = torch.tensor(acts_of, dtype=torch.int32, device="cuda")
    draw = lambda k: table[torch.randint(0, len(acts_of), (k, n), generator=g, device="cuda")]
    for v in vecs.values():
        assert v.frame_cache == v.engine.frame_cache
        v.reset()
    warm = draw(args.warmup)
    for v in vecs.values():
        for t in range(args.warmup):
            v.step(warm[t])
    acts = draw(args.steps)
    out = {"family": family, "mode": "device", "policy": args.policy, "envs": n, "steps": args.steps, "depth": args.depth, "slots": {}}
    for s, v in vecs.items():
        hist = torch.zeros(16, dtype=torch.int64, device="cuda")
        for t in range(args.steps):
            v.step(acts[t])
            hist += torch.bincount(v.frame_source().long(), minlength=16)
        h = (hist.double() / (args.steps * n)).cpu().tolist()
        out["slots"][s] = {"in_effect": v.frame_cache, "drawn": round(h[0], 4), "clean": round(h[1], 4), "copied": round(sum(h[2:]), 4),
                           "copied_per_slot": [round(x, 4) for x in h[2:2 + max(s, 0)]]}
    if args.windows:
        rates = {s: [] for s in vecs}
        for w in range(args.windows):
            for s, v in vecs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in range(args.calls):
                    v.step(acts[t % args.steps])
                torch.cuda.synchronize()
                rates[s].append(round(args.calls * n / (time.perf_counter() - t0)))
        out["env_steps_per_s"] = rates
    for v in vecs.values():
        v.engine.check()
        v.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cpu", action="store_true")
    p.add_argument("--gpu", action="store_true")
    p.add_argument("--families", default="hallway,oneroom")
    p.add_argument("--seeds", type=int, default=60)
    p.add_argument("--steps", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=400)
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--slots", default="2,4,8")
    p.add_argument("--policy", choices=sorted(POLICIES), default="uniform")
    p.add_argument("--depth", action="store_true")
    p.add_argument("--windows", type=int, default=0)
    p.add_argument("--calls", type=int, default=500)
    args = p.parse_args()
    if args.cpu == args.gpu:
        p.error("one of --cpu, --gpu")
    for family in args.families.split(","):
        print(json.dumps(cpu_replay(family, args.seeds, args.steps) if args.cpu else gpu_run(family, args)), flush=True)


if __name__ == "__main__":
    main()
