#!/usr/bin/env python
"""Times the pillar encoder at the size of configs/transfusion_nusc_pillar_L.py (N = 60 000
pillars, M = 20 slots, C = 5, U = 64), forward + backward, two ways:

  * the fused PillarFeatureNet (csrc/pillar.hip: moments, forward and backward passes);
  * the reference's op sequence in float32 torch on the GPU (decorate, mask, Linear,
    BatchNorm1d on a permuted copy, ReLU, max) -- what a user would otherwise run.

HIP-event medians after warm-up; the fused kernels' algorithmic bytes (each pass reads the raw
table once, the forward writes out + argmax, the backward reads grad_out + argmax) against the
8 TB/s HBM peak.  Writes profiles/pillar_bench.txt.

    python tools/pillar_bench.py [--reps 50] [--out profiles/pillar_bench.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pillar_fixture as PF  # noqa: E402
from msmdfusion_amd import kernels as K  # noqa: E402
from msmdfusion_amd.pillar_encoder import PillarFeatureNet  # noqa: E402

HBM_PEAK_TBPS = 8.0     # MI355X HBM3E spec peak
N, M, C, U = 60000, 20, 5, 64


def timed(fn, reps, warmup=5):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pillar_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    mod = PF.seed_encoder(PillarFeatureNet(in_channels=C, feat_channels=[U], voxel_size=PF.VOXEL_SIZE,
                                           point_cloud_range=PF.PC_RANGE), 5).to(dev).train()
    inputs = PF.make_pillars(N, M, C, seed=1, device=dev)
    go = torch.randn((N, U), device=dev)
    pfn = mod.pfn_layers[0]
    params = [pfn.linear.weight, pfn.norm.weight, pfn.norm.bias]

    def fused():
        mod(*inputs).backward(go)

    def torch_sequence():
        PF.reference_sequence(mod, *inputs, torch.float32, *params).backward(go)

    geom = mod._geom
    w = pfn.linear.weight.detach().contiguous()
    scale, shift = torch.ones(U, device=dev), torch.zeros(U, device=dev)
    out, arg = K.pillar_pfn_forward(*inputs, geom, w, scale, shift, "max")
    table = N * M * C * 4 + N * 4 + N * 16
    kernels = [
        ("moments pass", lambda: K.pillar_moments(*inputs, geom), table),
        ("forward pass (max)", lambda: K.pillar_pfn_forward(*inputs, geom, w, scale, shift, "max"),
         table + N * U * 5),
        ("backward pass (max)", lambda: K.pillar_pfn_backward(*inputs, geom, w, scale, shift, "max",
                                                              go, arg), table + N * U * 5),
    ]
    lines = ["# pillar encoder, N=%d M=%d C=%d U=%d, float32, forward + backward, HIP-event "
             "median (min .. max) of %d" % (N, M, C, U, args.reps)]
    f = timed(fused, args.reps)
    t = timed(torch_sequence, args.reps)
    lines.append("fused PillarFeatureNet        %8.3f ms (%.3f .. %.3f)" % f)
    lines.append("torch op sequence (float32)   %8.3f ms (%.3f .. %.3f)" % t)
    lines.append("speed-up                      %8.2f x" % (t[0] / f[0]))
    for name, fn, nbytes in kernels:
        ms = timed(fn, args.reps)
        lines.append("%-29s %8.3f ms (%.3f .. %.3f)  %6.1f MB  %5.2f TB/s  %4.1f %% of %g TB/s" % (
            name, ms[0], ms[1], ms[2], nbytes / 1e6, nbytes / (ms[0] * 1e-3) / 1e12,
            100 * nbytes / (ms[0] * 1e-3) / 1e12 / HBM_PEAK_TBPS, HBM_PEAK_TBPS))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
