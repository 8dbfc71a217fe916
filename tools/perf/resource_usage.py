#!/usr/bin/env python3
"""Compares the kernels' resource usage of two builds of the library.

Each argument is the log of `make EXTRA=-Rpass-analysis=kernel-resource-usage` (a clean build, stderr included) in
miniworld_amd/csrc: the parent commit's first, this tree's second.  Prints one line per kernel — VGPRs, AGPRs, SGPRs, scratch bytes
per lane, occupancy (waves per SIMD), static LDS — for both builds, the kernels only this tree has, and the number of kernels
that differ; exit status 1 if any kernel of the parent differs or is missing.

    python tools/perf/resource_usage.py parent_build.log this_build.log > profiles/r08/resource_usage.txt
"""
import re
import sys

KEYS = (("VGPR", "VGPRs"), ("AGPR", "AGPRs"), ("SGPR", "TotalSGPRs"), ("scratch", r"ScratchSize \[bytes/lane\]"), ("occupancy", r"Occupancy \[waves/SIMD\]"),
        ("LDS", r"LDS Size \[bytes/block\]"))


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for short, pat in KEYS:
            m = re.search(r"remark:\s+" + pat + r": (\d+)", line)
            if m:
                cur[short] = int(m.group(1))
    return out


def fmt(d):
    return " ".join(f"{k} {d.get(k, '?')}" for k, _ in KEYS)


def main():
    parent, this = parse(sys.argv[1]), parse(sys.argv[2])
    differ = [k for k in parent if parent[k] != this.get(k)]
    new = [k for k in this if k not in parent]
    print(f"# -Rpass-analysis=kernel-resource-usage of the library's kernels, parent commit and this tree: {len(parent)} kernels in the")
    print(f"# parent, {len(this)} here; VGPRs, AGPRs, SGPRs, scratch bytes per lane, occupancy (waves per SIMD) and static LDS.")
    print("# kernel | parent | this tree")
    for k in parent:
        print(f"{k} | {fmt(parent[k])} | {fmt(this[k]) if k in this else 'missing'}")
    print(f"differing kernels: {len(differ)} of {len(parent)}" + ("".join("\n  " + k for k in differ)))
    print("# kernels only this tree has")
    for k in new:
        print(f"{k} | - | {fmt(this[k])}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
