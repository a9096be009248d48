#!/usr/bin/env python
"""Times the transposed / inverse sparse convs and sparse max-pool (csrc/rulebook.hip
msmd_rulebook_deconv3d_*, csrc/pool.hip) at two sizes -- the LC size (2 nuScenes-shaped clouds,
0.075 m) and the configs[4] stress size (4 x 10-sweep ~290k-point clouds, 0.05 m):

  - the transposed rulebook (coarse -> fine, k3 s2 p1) against the strided rulebook of the
    mirrored geometry (fine -> coarse);
  - max-pool forward and backward (k3 s2 p1) at C = 16 / 64 against the torch composition a
    user would write (reference-format pairs + scatter_reduce("amax") / index_add_), with
    algorithmic bytes (every input, output and table entry touched once) against HBM peak;
  - the inverse conv forward against its couple conv's dgrad (same kernel, same table).

    python tools/sparse_updown_bench.py [--reps 50]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/sparse_updown_bench.py --reps 20

One JSON line per measurement on stdout.  Times are HIP-event medians per call."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msmdfusion_amd import kernels as K  # noqa: E402
from msmdfusion_amd import spconv  # noqa: E402
from msmdfusion_amd import synthetic as S  # noqa: E402
from msmdfusion_amd.spconv import functional as Fsp  # noqa: E402

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


def row(size, what, ms, nbytes=0, **kw):
    r = dict(size=size, what=what, ms=round(ms, 4), **kw)
    if nbytes:
        r["bytes"] = int(nbytes)
        r["frac_hbm"] = round(nbytes / (ms * 1e-3) / 1e12 / HBM_PEAK_TBPS, 4)
    print(json.dumps(r), flush=True)
    return r


def voxel_set(clouds, vs):
    rows = []
    for b, p in enumerate(clouds):
        c = K.dynamic_voxelize(p, vs, S.POINT_CLOUD_RANGE)
        c = torch.unique(c[(c >= 0).all(1)], dim=0)
        rows.append(torch.nn.functional.pad(c, (1, 0), value=b))
    idx = torch.cat(rows).int().contiguous()
    grid = [round((S.POINT_CLOUD_RANGE[3 + i] - S.POINT_CLOUD_RANGE[i]) / vs[i]) for i in range(3)]
    return idx, [grid[2] + 1, grid[1], grid[0]]


def torch_pool(f, i_of, o_of, m):
    c = f.shape[1]
    return torch.zeros((m, c), device=f.device).scatter_reduce(
        0, o_of[:, None].expand(-1, c), f[i_of], "amax", include_self=True)


def torch_pool_bwd(f, out, g, i_of, o_of):
    hit = (out[o_of] == f[i_of]).float()
    return torch.zeros_like(f).index_add_(0, i_of, g[o_of] * hit)


def case(name, clouds, vs, reps):
    idx, shape = voxel_set(clouds, vs)
    batch = len(clouds)
    n = idx.shape[0]
    ks, st, pd = [3, 3, 3], [2, 2, 2], [1, 1, 1]
    out_idx, nbr_fwd, nbr_bwd, out_shape = K.rulebook_conv(idx, batch, shape, ks, st, pd)
    m = out_idx.shape[0]
    print(json.dumps(dict(size=name, voxels=n, coarse_voxels=m, shape=shape,
                          coarse_shape=out_shape)), flush=True)

    # transposed rulebook (coarse -> fine) vs the strided one (fine -> coarse)
    up = K.rulebook_deconv(out_idx, batch, out_shape, ks, st, pd)
    ms = timed(lambda: K.rulebook_deconv(out_idx, batch, out_shape, ks, st, pd), reps)
    row(name, "transposed rulebook k3 s2 p1 (coarse -> fine)", ms, out_voxels=up[0].shape[0],
        out_shape=up[3])
    ms = timed(lambda: K.rulebook_conv(idx, batch, shape, ks, st, pd), reps)
    row(name, "strided rulebook k3 s2 p1 (fine -> coarse), mirrored geometry", ms)

    # max-pool over the strided rulebook
    kvol = nbr_bwd.shape[0]
    live = nbr_bwd >= 0
    i_of = torch.arange(n, device=idx.device)[None, :].expand(kvol, n)[live]
    o_of = nbr_bwd[live].long()
    pairs = int(live.sum())
    for c in (16, 64):
        f = torch.randn((n, c), device=idx.device)
        ms = timed(lambda: K.maxpool_fwd(f, nbr_bwd, m), reps)
        row(name, "max-pool fwd C=%d" % c, ms, n * c * 4 + kvol * n * 4 + m * c * 4, pairs=pairs)
        ms = timed(lambda: torch_pool(f, i_of, o_of, m), reps)
        row(name, "max-pool fwd C=%d, torch baseline (pairs + scatter_reduce amax)" % c, ms)
        out = K.maxpool_fwd(f, nbr_bwd, m)
        g = torch.randn_like(out)
        ms = timed(lambda: K.maxpool_bwd(f, out, g, nbr_bwd), reps)
        row(name, "max-pool bwd C=%d" % c, ms, 2 * n * c * 4 + kvol * n * 4 + 2 * m * c * 4)
        ms = timed(lambda: torch_pool_bwd(f, out, g, i_of, o_of), reps)
        row(name, "max-pool bwd C=%d, torch baseline (compare + index_add_)" % c, ms)

    # inverse conv forward vs its couple's dgrad: the same kernel over the same table
    for c in (16, 64):
        x = spconv.SparseConvTensor(torch.randn((n, c), device=idx.device), idx, shape, batch)
        couple = spconv.SparseConv3d(c, c, 3, 2, 1, bias=False, indice_key="d").to(idx.device)
        inv = spconv.SparseInverseConv3d(c, c, 3, indice_key="d", bias=False).to(idx.device)
        couple.weight.requires_grad_(False)
        inv.weight.requires_grad_(False)
        with torch.no_grad():
            mid = couple(x)
        rb = mid.indice_dict["d"]
        feats = x.features.clone().requires_grad_()
        y = Fsp.sparse_conv(feats, couple.weight, rb, krsc=True)
        g = torch.randn_like(y)
        dgrad = timed(lambda: torch.autograd.grad(y, feats, g, retain_graph=True), reps)
        row(name, "couple conv C=%d dgrad (autograd backward, weight frozen)" % c, dgrad)
        with torch.no_grad():
            ms = timed(lambda: inv(mid), reps)
        row(name, "inverse conv C=%d fwd (module)" % c, ms, vs_dgrad=round(ms / dgrad, 3))


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
