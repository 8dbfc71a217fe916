"""bench.py's plain run on the GPU box: the headline line and the dump, none of --full's legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_is_the_headline_only(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                          "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 1 and line["steps"] == 4 and line["warmup"] == 1 and line["config"]["name"] == "hallway"
    assert line["value"] > 0 and np.isfinite(line["ms_per_step"]) and line["higher_is_better"] is True and line["dtype"] == "f32"
    # --full's legs stay out: no oracle comparison, no profiler child runs, no other configs, no CPU baseline
    assert line["parity_checked"] == 0 and line["roofline"]["valu"] is None and line["roofline"]["traffic_source"] != "live"
    assert "also" not in line and "cpu_baseline" not in line
    assert line["roofline"]["kernel_ms"] > 0
    rew = np.load(tmp_path / "dump" / "reward.npy")
    assert rew.shape == (line["config"]["envs_per_gpu"],) and rew.dtype == np.float32
