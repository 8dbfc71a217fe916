"""The launch arithmetic of the depth projection (mwpolicy::depth_launch, miniworld_amd/csrc/mw_policy.h), without a GPU: compiled for the
host in tests/hostcheck/depth_project.cpp and compared with the rule written out here — a workgroup per env, four bytes of LDS per cell
of the target, never less than the map reduction's two words per wavefront, at most 64 KiB.  (Beside tests/test_launch_policy_cpu.py,
whose table was recorded before this call existed.)"""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "miniworld_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("depth_policy") / "depth_project")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(HERE, "hostcheck", "depth_project.cpp"), "-o", exe])
    return exe


def _policy(program, n, cells):
    out = subprocess.run([program, "--policy", str(n), str(cells)], capture_output=True, text=True, check=True).stdout.split()
    return dict(zip(("grid", "threads", "lds", "fits"), map(int, out)))


def test_depth_launch_is_a_workgroup_per_env_and_four_bytes_per_cell(program):
    src = open(os.path.join(CSRC, "mw_depth.h")).read()
    threads = int(re.search(r"#define MW_DEPTH_THREADS (\d+)", src).group(1))
    assert threads % 64 == 0 and int(re.search(r"#define MW_DEPTH_CELL_BYTES (\d+)", src).group(1)) == 4
    assert int(re.search(r"#define MW_DEPTH_MAX_CELLS (\d+)", src).group(1)) == 16384 == 64 * 1024 // 4
    least = 2 * (threads // 64)
    for n in (1, 3, 1024, 4096):
        for cells in (1, 2, 4, 9, 33 * 33, 65 * 65, 103 * 103, 128 * 128):
            want = -(-(max(cells, least) * 4) // 16) * 16
            assert _policy(program, n, cells) == {"grid": n, "threads": threads, "lds": want, "fits": 1}, (n, cells)
    # the boundary: a window of 128 x 128 and a map of 16384 cells fit exactly; one cell more does not
    assert _policy(program, 5, 16384)["lds"] == 64 * 1024 and _policy(program, 5, 16384)["fits"] == 1
    assert _policy(program, 5, 16385)["fits"] == 0 and _policy(program, 5, 16385)["lds"] > 64 * 1024
    assert _policy(program, 5, 32768)["fits"] == 0            # a nav grid's limit is twice this one
    # the Maze at 0.25 m: 103 x 103 cells
    assert _policy(program, 1024, 10609) == {"grid": 1024, "threads": threads, "lds": 42448, "fits": 1}


def test_the_binding_knows_the_same_limit():
    from miniworld_amd import engine
    assert engine.DEPTH_MAX_CELLS == 16384 and engine.EGO_MAX_SIZE ** 2 == engine.DEPTH_MAX_CELLS
    text = " ".join(open(os.path.join(CSRC, "mw_engine_depth.hip")).read().split())
    assert "mwpolicy::depth_launch(a.N, cells)" in text and "use a larger cell" in text
