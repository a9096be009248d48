"""The plain benchmark line as later measurements read it: `bench.py --gpus 1 --steps K
--warmup W` times K steps of the headline workload and nothing else, and --dump-outputs
writes what the last timed step computed -- the same arrays from run to run (the timed steps
start from the seeded initial state whatever the time-based settle phase took)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs_repeat(dev, tmp_path):
    runs = [_bench("--gpus", "1", "--steps", "3", "--warmup", "1",
                   "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for r in runs:
        assert (r["steps"], r["warmup"], r["n_gpus"], r["unit"]) == (3, 1, 1, "samples/s")
        assert r["higher_is_better"] is True and r["dtype"].startswith("f32")
        assert r["metric"].startswith("samples/sec MSMDFusion")
        # value = global batch (2) per timed step
        assert r["value"] == pytest.approx(2e3 / r["ms_per_step"], rel=1e-2)
        assert "cpu_baseline" not in r and "also" not in r and r["roofline"] is None
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["loss.npy", "output_channel_sum.npy", "output_sample.npy", "params.npy"]
    assert sorted(os.listdir(tmp_path / "b")) == names
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        total += a.nbytes
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=n)
    assert total <= 64 << 20
    params = np.load(tmp_path / "a" / "params.npy")
    assert params.shape == (runs[0]["config"]["trainable_params"],)
