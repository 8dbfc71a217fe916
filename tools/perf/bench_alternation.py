"""The plain step before and after a change: `bench.py` alternately in this tree and in a checkout of the parent commit that has been
built (`git worktree add DIR HEAD~1`, `DIR/miniworld_amd/csrc/build.sh`), a process per run; one JSON line per run, in r41's form.

    python tools/perf/bench_alternation.py PARENT_DIR [--rounds 2] [--windows 5]

Nothing here is a threshold: the record is the windows of both, read side by side (profiles/rNN/bench_alternation.jsonl)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LEAN = ["--gpus", "1", "--steps", "200", "--warmup", "20", "--no-cpu-baseline", "--no-parity-check", "--no-also", "--no-pmc"]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("parent")
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--windows", type=int, default=5)
    args = p.parse_args()
    for _ in range(args.rounds):
        for which, where in (("tree", ROOT), ("parent", os.path.abspath(args.parent))):
            out = subprocess.run([sys.executable, "bench.py"] + LEAN + ["--windows", str(args.windows)], cwd=where, capture_output=True, text=True, timeout=600)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
            if out.returncode != 0 or not line:
                print(json.dumps({"which": which, "error": (out.stdout + out.stderr)[-1500:]}), flush=True)
                return 1
            values = [round(v / 1e6, 3) for v in json.loads(line[-1])["windows"]["values"]]
            print(json.dumps({"which": which, "windows_M": values, "median_M": round(statistics.median(values), 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
