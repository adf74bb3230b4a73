"""A plain `bench.py --gpus 1 --steps N --warmup W` run on the GPU, at a small shape: it
times the steps and prints the headline line alone (what `--full` adds is absent), and
`--dump-outputs DIR` writes the verdicts of the contexts' last timed passes."""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--inflight", "2",
           "--calls-per-pass", "3", "--sets", "64", "--dump-outputs", str(tmp_path / "out")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(ROOT))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    assert r["unit"] == "sets/s" and r["higher_is_better"] is True and r["value"] > 0
    assert r["steps"] == 2 and r["warmup"] == 1 and r["ms_per_step"] > 0
    assert r["metric"].startswith("BLS signature sets verified/sec") and r["dtype"].startswith("u32")
    # value = the sets of the timed steps over the timed region
    assert r["value"] == pytest.approx(2 * 3 * 64 / (r["ms_per_step"] / 1e3), rel=1e-3)
    for key in ("p50_latency_ms_128", "roofline", "cpu_baseline", "latency_curve", "cfg3", "hw_queues_4"):
        assert key not in r, key
    v = np.load(tmp_path / "out" / "verdicts.npy")
    assert v.dtype == np.float32 and v.shape == (2, 3, 64) == tuple(r["outputs"]["shape"])
    assert (v == 1).all()
