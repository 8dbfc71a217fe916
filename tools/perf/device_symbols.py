"""Whether a change left the device code of another build alone: the gfx950 code object of every object file of two build trees
(csrc/_obj of each), disassembled and compared function symbol by function symbol.

    python tools/perf/device_symbols.py PARENT/miniworld_amd/csrc/_obj miniworld_amd/csrc/_obj      # one JSON line

A symbol's text is its instructions as llvm-objdump prints them, without the address and encoding comments, so that a function that
moved inside its unit still compares equal.  The line: the parent's device function symbols, how many of them differ or are missing
in the tree (with their names), and the symbols only the tree has.  Needs no GPU."""
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def functions(obj, tmp):
    """{symbol: instruction text} of the device code object bundled in `obj`"""
    fat, co = os.path.join(tmp, os.path.basename(obj) + ".fatbin"), os.path.join(tmp, os.path.basename(obj) + ".co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")], capture_output=True)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return {}           # (a unit without device code)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}", "--unbundle"],
                   check=True, capture_output=True)
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        head = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if head:
            name = head.group(1)
            out[name] = []
        elif name and line.strip():
            out[name].append(re.sub(r"\s*//.*$", "", line).strip())
    return {k: "\n".join(v) for k, v in out.items()}


def tree(obj_dir, tmp):
    out = {}
    for f in sorted(os.listdir(obj_dir)):
        if f.endswith(".o"):
            for k, v in functions(os.path.join(obj_dir, f), tmp).items():
                out[f"{f}:{k}"] = v
    return out


def main():
    parent_dir, tree_dir = sys.argv[1:3]
    with tempfile.TemporaryDirectory() as tmp:
        parent, mine = tree(parent_dir, os.path.join(tmp, "")), tree(tree_dir, os.path.join(tmp, ""))
    differ = sorted(k for k in parent if k in mine and parent[k] != mine[k])
    missing = sorted(k for k in parent if k not in mine)
    print(json.dumps({"parent_symbols": len(parent), "differ": len(differ), "missing": len(missing), "differing": differ, "gone": missing,
                      "new": sorted(k for k in mine if k not in parent)}))
    return 1 if differ or missing else 0


if __name__ == "__main__":
    sys.exit(main())
