#!/usr/bin/env python
"""Times dynamic voxelization's scatter (csrc/dynamic_voxel.hip): the index half
(scatter_index) and the feature half (mean and max at C = 5 and C = 64, forward and
backward) at two sizes -- the LC size (2 nuScenes-shaped clouds, 0.075 m) and the configs[4]
stress size (4 x 10-sweep ~290k-point clouds, 0.05 m) -- against the torch composition a
user would otherwise write (torch.unique(dim=0, return_inverse, return_counts) + index_add_ /
scatter_reduce("amax")) and against HBM bandwidth (algorithmic bytes: every input read once,
every output written once; the sort's passes are not counted).

    python tools/dynamic_scatter_bench.py [--reps 50]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/dynamic_scatter_bench.py --reps 20

One JSON line per measurement on stdout.  Times are HIP-event medians per call."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msmdfusion_amd import kernels as K  # noqa: E402
from msmdfusion_amd import synthetic as S  # noqa: E402

HBM_PEAK_TBPS = 8.0     # MI355X HBM3E spec peak


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
    return ts[len(ts) // 2]


def coords(clouds, vs):
    cs = [torch.nn.functional.pad(K.dynamic_voxelize(p, vs, S.POINT_CLOUD_RANGE), (1, 0), value=b)
          for b, p in enumerate(clouds)]
    return torch.cat(cs)


def torch_index(coors):
    valid = (coors >= 0).all(1)
    uniq, inv, cnt = torch.unique(coors[valid], dim=0, return_inverse=True, return_counts=True)
    return valid, uniq, inv, cnt


def torch_reduce(feats, valid, inv, m, reduce):
    f = feats[valid]
    if reduce == "mean":
        cnt = torch.bincount(inv, minlength=m).clamp_min(1)
        return torch.zeros((m, f.shape[1]), device=f.device).index_add_(0, inv, f) / cnt[:, None]
    return torch.full((m, f.shape[1]), -float("inf"), device=f.device).scatter_reduce(
        0, inv[:, None].expand(-1, f.shape[1]), f, "amax")


def row(size, what, ms, nbytes, **kw):
    r = dict(size=size, what=what, ms=round(ms, 4), **kw)
    if nbytes:
        r["bytes"] = int(nbytes)
        r["frac_hbm"] = round(nbytes / (ms * 1e-3) / 1e12 / HBM_PEAK_TBPS, 4)
    print(json.dumps(r), flush=True)
    return r


def case(name, clouds, vs, reps):
    dev = clouds[0].device
    coors = coords(clouds, vs).contiguous()
    n, nd = coors.shape
    idx = K.scatter_index(coors)
    m = idx.num_voxels
    print(json.dumps(dict(size=name, points=n, voxels=m)), flush=True)
    ms = timed(lambda: K.scatter_index(coors), reps)
    row(name, "index half (scatter_index)", ms, n * nd * 4 + 3 * n * 4 + m * (nd + 2) * 4)
    ms = timed(lambda: torch_index(coors), reps)
    row(name, "index half, torch.unique(dim=0) baseline", ms, 0)
    valid, _, inv, _ = torch_index(coors)
    for c in (5, 64):
        feats = torch.randn((n, c), device=dev)
        for reduce in ("mean", "max"):
            out_b = m * c * 4 * (2 if reduce == "max" else 1)
            ms = timed(lambda: K.scatter_reduce(feats, idx, reduce), reps)
            row(name, "%s fwd C=%d" % (reduce, c), ms, n * c * 4 + n * 4 + m * 4 + out_b)
            ms = timed(lambda: torch_reduce(feats, valid, inv, m, reduce), reps)
            row(name, "%s fwd C=%d, torch baseline (index_add_ / scatter_reduce amax)" % (reduce, c),
                ms, 0)
            out, arg = K.scatter_reduce(feats, idx, reduce)
            g = torch.randn_like(out)
            ms = timed(lambda: K.scatter_reduce_backward(g, idx.point2voxel, reduce,
                                                         counts=idx.counts, argmax=arg), reps)
            row(name, "%s bwd C=%d" % (reduce, c), ms,
                n * 4 + n * c * 4 + (m * c * 4 if reduce == "max" else m * 4) + m * c * 4)
        ms = timed(lambda: K.scatter_gather(out, idx.point2voxel), reps)
        row(name, "voxel->point gather C=%d" % c, ms, n * 4 + m * c * 4 + n * c * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lc = [torch.from_numpy(S.lidar_sweep(i)).to(dev) for i in range(2)]
    case("LC: 2 clouds, 0.075 m", lc, S.VOXEL_SIZE, args.reps)
    stress = [torch.from_numpy(S.lidar_sweep(10 + i, sweeps=10)).to(dev) for i in range(4)]
    case("configs[4]: 4 x 10-sweep ~290k pts, 0.05 m", stress, [0.05, 0.05, 0.2], args.reps)


if __name__ == "__main__":
    main()
