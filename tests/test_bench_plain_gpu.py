"""A plain `bench.py` run (no --full) on the GPU: one JSON line with the headline and the configuration, every leg that --full adds
left null, and the .npy files of --dump-outputs."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_run_prints_the_headline_alone(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2",
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "clip-pairs/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["steps"] == 2 and d["warmup"] == 1 and d["config"]["clips_per_gpu"] == 2
    assert d["value"] == pytest.approx(2 / (d["ms_per_step"] * 1e-3), rel=1e-3)
    assert d["repeat_ms_per_step"] == [d["ms_per_step"]]
    assert d["roofline"]["frac"] > 0 and "dominant_kernel" not in d["roofline"]
    for k in ("parity", "cpu_baseline", "other_configs", "value_f32", "f32_detail"):
        assert d[k] is None, k
    assert "b2" not in d and "rccl_ranks" not in d
    assert any(f.name.startswith("pair0_0_out_a") for f in tmp_path.iterdir())
