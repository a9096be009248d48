#!/usr/bin/env python
"""Times the PointNet++ kernels (csrc/pointnet.hip) at B 4, N 16384, npoint 4096, nsample 32,
C 64 beside the torch composition each replaces on the same GPU:

  * group_points forward          vs  torch.gather
  * group / interpolate backward  vs  index_add_ (float atomics)
  * the inverse index build (once per index tensor)
  * three_nn, knn (k = 16)        vs  cdist + topk
  * three_interpolate forward     vs  gather + weighted sum

HIP-event medians after warm-up; algorithmic bytes against the 8 TB/s HBM peak.  With
--ours-only only the library's kernels run (for a rocprofv3 --kernel-trace --stats run).
Writes profiles/pointnet_bench.txt.

    python tools/pointnet_bench.py [--reps 30] [--ours-only] [--out profiles/pointnet_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msmdfusion_amd import kernels as K  # noqa: E402

HBM_PEAK_TBPS = 8.0     # MI355X HBM3E spec peak
B, N, NPOINT, NSAMPLE, C, KNN = 4, 16384, 4096, 32, 64, 16


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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--ours-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointnet_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(8)
    xyz = torch.from_numpy(rs.randint(-16, 17, size=(B, N, 3)).astype(np.float32) / 4).to(dev)
    centres = xyz[:, :NPOINT].contiguous()
    feat = torch.randn((B, C, N), device=dev)
    idx = K.ball_query(0, 0.6, NSAMPLE, xyz, centres)
    m = NPOINT * NSAMPLE
    idx64 = idx.long().view(B, 1, m).expand(B, C, m)
    go = torch.randn((B, C, NPOINT, NSAMPLE), device=dev)
    inv = K.point_inverse_index(idx, N)
    dist2, idx3 = K.three_nn(xyz, centres)
    w3 = torch.rand((B, N, 3), device=dev)
    pooled = torch.randn((B, C, NPOINT), device=dev)
    go3 = torch.randn((B, C, N), device=dev)
    inv3 = K.point_inverse_index(idx3, NPOINT)
    idx3_64 = idx3.long().view(B, 1, N * 3).expand(B, C, N * 3)

    def torch_group_bwd():
        out = torch.zeros((B, C, N), device=dev)
        for b in range(B):
            out[b].index_add_(1, idx[b].view(-1).long(), go[b].view(C, m))
        return out

    def torch_interp():
        g = torch.gather(pooled, 2, idx3_64).view(B, C, N, 3)
        return (g * w3[:, None]).sum(-1)

    def torch_interp_bwd():
        out = torch.zeros((B, C, NPOINT), device=dev)
        src = (go3[..., None] * w3[:, None]).view(B, C, N * 3)
        for b in range(B):
            out[b].index_add_(1, idx3[b].view(-1).long(), src[b])
        return out

    f4 = 4
    rows = [
        ("group_points fwd", lambda: K.group_points(feat, idx),
         lambda: torch.gather(feat, 2, idx64), B * (m * f4 + C * N * f4 + C * m * f4)),
        ("inverse index (group)", lambda: K.point_inverse_index(idx, N), None,
         B * m * f4 * 6),
        ("group_points bwd", lambda: K.point_scatter_backward(go, inv), torch_group_bwd,
         B * (m * f4 + C * m * f4 + C * N * f4)),
        ("three_nn", lambda: K.three_nn(xyz, centres),
         lambda: torch.cdist(xyz, centres).topk(3, dim=2, largest=False),
         B * (N * 3 * f4 + NPOINT * 3 * f4 + N * 6 * f4)),
        ("three_interpolate fwd", lambda: K.three_interpolate(pooled, idx3, w3), torch_interp,
         B * (N * 6 * f4 + C * NPOINT * f4 + C * N * f4)),
        ("three_interpolate bwd",
         lambda: K.point_scatter_backward(go3, inv3, weight=w3, dest_per_out=3),
         torch_interp_bwd, B * (N * 6 * f4 + C * N * f4 + C * NPOINT * f4)),
        ("knn k=16", lambda: K.knn(KNN, xyz, centres),
         lambda: torch.cdist(centres, xyz).topk(KNN, dim=2, largest=False),
         B * (N * 3 * f4 + NPOINT * 3 * f4 + KNN * NPOINT * 8)),
    ]
    lines = ["# PointNet++ kernels, B=%d N=%d npoint=%d nsample=%d C=%d, float32, HIP-event median "
             "(min .. max) of %d; bytes = algorithmic traffic" % (B, N, NPOINT, NSAMPLE, C,
                                                                   args.reps)]
    for name, ours, theirs, nbytes in rows:
        o = timed(ours, args.reps)
        line = "%-24s %8.3f ms (%.3f .. %.3f)  %7.1f MB  %5.2f TB/s  %4.1f %% of %g TB/s" % (
            name, o[0], o[1], o[2], nbytes / 1e6, nbytes / (o[0] * 1e-3) / 1e12,
            100 * nbytes / (o[0] * 1e-3) / 1e12 / HBM_PEAK_TBPS, HBM_PEAK_TBPS)
        if theirs is not None and not args.ours_only:
            t = timed(theirs, args.reps)
            line += "   torch %8.3f ms (%.3f .. %.3f)  %5.2fx" % (t[0], t[1], t[2], t[0] / o[0])
        lines.append(line)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
