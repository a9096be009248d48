"""bench.py's --dump-outputs writer on CPU tensors: what it writes, in which types, within
its size bound, and the same sample for the same output whatever its memory format."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_samples_a_large_map(tmp_path):
    import bench
    g = torch.Generator().manual_seed(0)
    bev = torch.randn(2, 128, 180, 180, generator=g)        # 8.3 M elements: sampled
    params = [torch.nn.Parameter(torch.randn(27, 64, 64, generator=g)),
              torch.nn.Parameter(torch.randn(64, generator=g))]
    loss = torch.tensor(0.25)
    bench.dump_outputs(str(tmp_path / "a"), loss, bev, params)
    # the same map channels-last (the LC path's layout): the same logical elements
    bench.dump_outputs(str(tmp_path / "b"), loss, bev.contiguous(memory_format=torch.channels_last),
                       params)
    a, b = _read(tmp_path / "a"), _read(tmp_path / "b")
    assert sorted(a) == ["loss", "output_channel_sum", "output_sample", "params"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), (k, a[k].dtype)
        assert np.array_equal(a[k], b[k]), k
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    assert a["loss"].tolist() == [0.25]
    assert a["output_sample"].shape == (bench.DUMP_SAMPLE,)
    assert np.isin(a["output_sample"][:1000], bev.numpy().reshape(-1)).all()
    np.testing.assert_allclose(a["output_channel_sum"], bev.double().sum((2, 3)).numpy(),
                               rtol=1e-12, atol=1e-9)
    want = torch.cat([p.detach().reshape(-1) for p in params]).numpy()
    assert np.array_equal(a["params"], want)


def test_dump_outputs_keeps_a_small_output_whole(tmp_path):
    import bench
    out = torch.arange(24, dtype=torch.float32).reshape(2, 3, 2, 2)
    p = [torch.nn.Parameter(torch.ones(3))]
    bench.dump_outputs(str(tmp_path), torch.tensor(1.5), out, p)
    a = _read(tmp_path)
    assert sorted(a) == ["loss", "output", "output_channel_sum", "params"]
    assert np.array_equal(a["output"], out.numpy().reshape(-1))
    assert a["output_channel_sum"].dtype == np.float64


def test_bench_options():
    """--full gates everything beyond the headline; --dump-outputs takes a directory."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
