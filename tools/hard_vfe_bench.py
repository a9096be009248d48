#!/usr/bin/env python
"""Times HardVFE at the training size of configs/_base_/models/hv_pointpillars_fpn_nus.py
(N = 4 x 30 000 voxels, M = 64 slots, C = 4, two VFELayers 64 wide), forward + backward, two ways:

  * the fused HardVFE (csrc/hard_vfe.hip: moments, statistics, output and backward passes);
  * the reference's op sequence in float32 torch on the same GPU -- the baseline.

num_points is drawn as min(M, 1 + Geometric(p)) with p = 0.2 (mean about 5 points per pillar,
as sparse LiDAR pillars of 0.25 m hold) and every 50th voxel full; `--occupancy full` fills every
voxel, the case in which the padded-slot shortcut saves nothing.

HIP-event medians after warm-up; per pass the algorithmic bytes (the raw table read once, the
[N, U] outputs) against the 8 TB/s HBM peak and the multiply-adds of the rows actually computed
(real rows + one padded row per voxel) against the 157 TFLOP/s float32 vector peak; peak memory
of both paths.  Appends to / writes profiles/hard_vfe_bench.txt.

    python tools/hard_vfe_bench.py [--reps 20] [--occupancy sparse|full] [--out ...]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hard_vfe_fixture as HF  # noqa: E402
from msmdfusion_amd import kernels as K  # noqa: E402

HBM_PEAK_TBPS = 8.0        # MI355X HBM3E spec peak
FP32_PEAK_TFLOPS = 157.3   # MI355X float32 vector peak
N, M, C, U = 4 * 30000, 64, 4, 64


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2**20


def voxels(occupancy, dev):
    feats, num, coors = HF.make_voxels(N, M, C, seed=1, kind="full")
    rng = np.random.RandomState(2)
    if occupancy == "sparse":
        cnt = np.minimum(M, rng.geometric(0.2, N)).astype(np.int32)
        cnt[::50] = M
        num = torch.from_numpy(cnt)
        feats = feats * (torch.arange(M)[None, :] < num[:, None])[:, :, None]
    return feats.to(dev), num.to(dev), coors.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--occupancy", default="sparse", choices=["sparse", "full"])
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hard_vfe_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    mod = HF.encoder(dev, C, (U, U), True)
    inputs = voxels(args.occupancy, dev)
    num = inputs[1]
    go = torch.randn((N, U), device=dev)
    params = [(v.linear.weight, v.norm.weight, v.norm.bias) for v in mod.vfe_layers]

    def fused():
        mod(*inputs).backward(go)

    def torch_sequence():
        HF.reference_sequence(mod, *inputs, torch.float32, params).backward(go)

    geom = mod._geom
    kdec = geom.decorated(C)
    layers = [(v.linear.weight.detach().contiguous(), torch.ones(U, device=dev),
               torch.zeros(U, device=dev)) for v in mod.vfe_layers]
    out, arg, _ = K.hard_vfe_forward(*inputs, geom, layers)
    g2 = (go * (out > 0)).contiguous()
    dp = torch.full((U,), 1e-6, device=dev)
    rows = float((num.clamp(max=M) + (num < M)).sum())            # rows the kernels compute
    table = N * M * C * 4 + N * 4 + N * 16
    l1, l2 = 2 * kdec * U * rows, 2 * U * U * rows + 2 * U * U * N
    kernels = [
        ("moments pass", lambda: K.hard_vfe_moments(*inputs, geom), table, 0.0),
        ("statistics pass (layer 2)", lambda: K.hard_vfe_stats(*inputs, geom, *layers[0],
                                                               layers[1][0]), table, 2 * l1 + l2),
        ("output pass", lambda: K.hard_vfe_forward(*inputs, geom, layers), table + N * U * 9,
         2 * l1 + l2),
        ("backward pass", lambda: K.hard_vfe_backward(*inputs, geom, layers, g2, arg, dp, dp),
         table + N * U * 5, 2 * l1 + 3 * l2 + 2 * kdec * U * rows),
    ]
    lines = ["# HardVFE, N=%d M=%d C=%d widths %d/%d, occupancy %s (mean num_points %.2f, rows "
             "computed %.1f %% of N*M), float32, training mode, forward + backward, HIP-event "
             "median (min .. max) of %d" % (N, M, C, U, U, args.occupancy, float(num.float().mean()),
                                            100 * rows / (N * M), args.reps)]
    f = timed(fused, args.reps)
    t = timed(torch_sequence, max(3, args.reps // 4), warmup=2)
    lines.append("fused HardVFE                 %8.3f ms (%.3f .. %.3f)" % f)
    lines.append("torch op sequence (float32)   %8.3f ms (%.3f .. %.3f)" % t)
    lines.append("speed-up                      %8.2f x" % (t[0] / f[0]))
    lines.append("peak memory above the inputs: fused %.0f MB, torch op sequence %.0f MB "
                 "(one [N, M, 2U] float tensor: %.0f MB)" % (peak_of(fused), peak_of(torch_sequence),
                                                             N * M * 2 * U * 4 / 2**20))
    for name, fn, nbytes, flops in kernels:
        ms = timed(fn, args.reps)
        lines.append("%-29s %8.3f ms (%.3f .. %.3f)  %6.1f MB  %5.2f TB/s (%4.1f %% of %g TB/s)  "
                     "%6.2f GFLOP  %5.2f TFLOP/s (%4.1f %% of %g)" % (
                         name, ms[0], ms[1], ms[2], nbytes / 1e6, nbytes / (ms[0] * 1e-3) / 1e12,
                         100 * nbytes / (ms[0] * 1e-3) / 1e12 / HBM_PEAK_TBPS, HBM_PEAK_TBPS,
                         flops / 1e9, flops / (ms[0] * 1e-3) / 1e12,
                         100 * flops / (ms[0] * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, FP32_PEAK_TFLOPS))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "a" if args.append else "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
