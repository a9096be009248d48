#!/usr/bin/env python
"""Times RoI-aware pooling (csrc/roiaware.hip) at the Part-A2 RoI-head size: B = 2 samples,
128 RoIs and ~16k points each, out_size 14, max_pts_per_voxel 128; max at C = 16 (seg
features), avg at C = 4 (part features):

  - the index half (count, one host read, emit, sorts, inverse) for the whole batch;
  - pooling forward and backward, with algorithmic bytes (every index entry, feature, output
    and gradient element touched once) against HBM peak;
  - the device memory of the compact index against what the reference allocates (the
    per-sample N_rois x N_points mask at its peak, and the padded [N, 14, 14, 14, 128] tables
    of both extractors, which the reference keeps for the backward);
  - the torch composition a user would otherwise write (broadcast predicate, nonzero, stable
    sort for the cap, scatter_reduce / index_add_) at the same sizes.

    python tools/roiaware_bench.py [--reps 50]

One JSON line per measurement on stdout.  Times are HIP-event medians per call."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msmdfusion_amd import kernels as K  # noqa: E402
from msmdfusion_amd.roiaware_pool3d import roi_point_index  # noqa: E402

HBM_PEAK_TBPS = 8.0     # MI355X HBM3E spec peak
OUT, MAX_PTS = 14, 128


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


def row(what, ms, nbytes=0, **kw):
    r = dict(size="parta2", what=what, ms=round(ms, 4), **kw)
    if nbytes:
        r["bytes"] = int(nbytes)
        r["frac_hbm"] = round(nbytes / (ms * 1e-3) / 1e12 / HBM_PEAK_TBPS, 4)
    print(json.dumps(r), flush=True)
    return r


def scene(batch=2, rois_per=128, pts_per=16384, seed=0):
    """KITTI-like: car-sized RoIs (jittered proposals around 24 objects per sample), half the
    points on the objects, half spread over the 70 x 80 m range."""
    g = torch.Generator().manual_seed(seed)
    rois, rb, pts, pb = [], [], [], []
    for b in range(batch):
        obj = torch.rand((24, 2), generator=g) * torch.tensor([70.0, 80.0]) - torch.tensor([0.0, 40.0])
        pick = torch.randint(0, 24, (rois_per,), generator=g)
        r = torch.zeros((rois_per, 7))
        r[:, :2] = obj[pick] + torch.randn((rois_per, 2), generator=g) * 0.5
        r[:, 2] = -1.7 + torch.randn(rois_per, generator=g) * 0.1
        r[:, 3:6] = torch.tensor([1.6, 3.9, 1.56]) * (1 + torch.randn((rois_per, 3), generator=g) * 0.1)
        r[:, 6] = torch.rand(rois_per, generator=g) * 2 * math.pi - math.pi
        half = pts_per // 2
        on = obj[torch.randint(0, 24, (half,), generator=g)] + torch.randn((half, 2), generator=g)
        p = torch.cat([torch.cat([on, torch.rand((half, 1), generator=g) * 2 - 1.8], 1),
                       torch.rand((pts_per - half, 3), generator=g) * torch.tensor([70.0, 80.0, 4.0])
                       - torch.tensor([0.0, 40.0, 3.0])])
        rois.append(r)
        pts.append(p)
        rb.append(torch.full((rois_per,), b, dtype=torch.int32))
        pb.append(torch.full((pts_per,), b, dtype=torch.int32))
    return [torch.cat(x).cuda().contiguous() for x in (rois, rb, pts, pb)]


def torch_composition(rois, rb, pts, pb, feats, mode):
    """What a user without the kernels writes: the predicate broadcast over (RoI, point),
    nonzero, the cap by a stable sort of the cells, then scatter_reduce / index_add_."""
    x, y, z = pts[None, :, 0], pts[None, :, 1], pts[None, :, 2]
    cx, cy, zb, w, l, h, rz = (rois[:, j:j + 1] for j in range(7))
    rot = rz + math.pi / 2
    ca, sa = torch.cos(rot), torch.sin(rot)
    sx, sy = x - cx, y - cy
    lx, ly = sx * ca - sy * sa, sx * sa + sy * ca
    inside = ((z - (zb + h / 2)).abs() <= h / 2) & (lx.abs() < l / 2) & (ly.abs() < w / 2) & \
        (rb[:, None] == pb[None, :])
    r, p = inside.nonzero(as_tuple=True)
    ix = ((lx[r, p] + l[r, 0] / 2) / (l[r, 0] / OUT)).long().clamp_(0, OUT - 1)
    iy = ((ly[r, p] + w[r, 0] / 2) / (w[r, 0] / OUT)).long().clamp_(0, OUT - 1)
    iz = ((z[0, p] - zb[r, 0]) / (h[r, 0] / OUT)).long().clamp_(0, OUT - 1)
    cell = r * OUT ** 3 + (ix * OUT + iy) * OUT + iz
    cell, order = torch.sort(cell, stable=True)
    p = p[order]
    first = torch.searchsorted(cell, cell)
    keep = torch.arange(cell.numel(), device=cell.device) - first < MAX_PTS - 1
    cell, p = cell[keep], p[keep]
    c = feats.shape[1]
    out = torch.zeros((rois.shape[0] * OUT ** 3, c), device=feats.device)
    if mode == "max":
        out.scatter_reduce_(0, cell[:, None].expand(-1, c), feats[p], "amax", include_self=False)
    else:
        out.index_add_(0, cell, feats[p])
        cnt = torch.bincount(cell, minlength=out.shape[0]).clamp_(min=1)
        out /= cnt[:, None]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    rois, rb, pts, pb = scene()
    nr, n = rois.shape[0], pts.shape[0]
    cells = nr * OUT ** 3
    index = roi_point_index(rois, pts, OUT, MAX_PTS, rb, pb)
    h = index.hit_pts.numel()
    kept = int(index.pt_start[-1])
    print(json.dumps(dict(size="parta2", rois=nr, points=n, hits=h, kept=kept,
                          occupied_cells=int((index.counts() > 0).sum()), cells=cells)), flush=True)

    ms = timed(lambda: roi_point_index(rois, pts, OUT, MAX_PTS, rb, pb), args.reps)
    row("index (count + host read + emit + sorts + inverse)", ms,
        n * 16 + nr * 32 + h * 12 + (cells + 1) * 4 + (n + 1) * 4)

    idx_bytes = sum(t.numel() * t.element_size()
                    for t in (index.hit_pts, index.inv_cell, index.vox_start, index.pt_start))
    # the reference pools sample by sample: its RoI x point mask lives for one call (peak =
    # the largest sample's), its padded tables stay saved for the backward (every sample's, two
    # extractors)
    table = cells * MAX_PTS * 4
    mask = max(int((rb == b).sum()) * int((pb == b).sum()) for b in range(int(rb.max()) + 1)) * 4
    print(json.dumps(dict(size="parta2", what="device memory", index_bytes=idx_bytes,
                          reference_mask_peak_bytes=mask, reference_table_bytes=table,
                          reference_two_extractors_bytes=2 * table + mask,
                          ratio=round((2 * table + mask) / idx_bytes, 1))), flush=True)

    for mode, c in (("max", 16), ("avg", 4)):
        feats = torch.randn((n, c), device="cuda")
        pooled, arg = K.roiaware_pool(feats, index, mode)
        ms = timed(lambda: K.roiaware_pool(feats, index, mode), args.reps)
        out_b = cells * c * 4 * (2 if mode == "max" else 1)
        row("forward %s C=%d" % (mode, c), ms, kept * (c * 4 + 4) + (cells + 1) * 4 + out_b)
        g = torch.randn_like(pooled)
        ms = timed(lambda: K.roiaware_pool_backward(g, index, mode, argmax=arg), args.reps)
        row("backward %s C=%d" % (mode, c), ms,
            kept * (8 + c * 4 * (2 if mode == "max" else 1)) + (n + 1) * 4 + n * c * 4 +
            (kept * 8 if mode == "avg" else 0))
        ms = timed(lambda: torch_composition(rois, rb, pts, pb, feats, mode), max(5, args.reps // 5))
        row("torch composition forward %s C=%d (index + pool)" % (mode, c), ms)


if __name__ == "__main__":
    main()
