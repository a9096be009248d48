#!/usr/bin/env python
"""The image stage of TransFusionHeadLC at the nuScenes LC shape (batch 2, 6 views, 200
proposals, 56 x 100 feature maps, 128 channels in 8 heads): the fused path
(`_image_stage_fused`: geometry kernel, batched self-attention, Gaussian-window attention
kernel) beside the composition (`_image_stage_composed`: the reference's double loop) on the
same inputs, forward and forward + backward.  One JSON line per quantity, with the kernel
launches and the host synchronisations of one call.

    python tools/img_fusion_timing.py [--repeat 20] [--rounds 5] [--out FILE]

Times are device events around `repeat` back-to-back calls, after warm-up calls of the same
shape; the two versions alternate round by round and the median round is reported.  Needs a
GPU: there is no fallback.
"""
import argparse
import json
import math
import os
import statistics
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msmdfusion_amd import configs as C  # noqa: E402

BATCH, VIEWS, PROPOSALS, MAP_H, MAP_W = 2, 6, 200, 56, 100


def ring_metas(pad_h, pad_w):
    """Six cameras 1.5 m above the origin, 60 degrees apart, 70 degrees wide."""
    mats = []
    f = 0.5 * pad_w / math.tan(math.radians(35.0))
    for v in range(VIEWS):
        yaw = 2 * math.pi * v / VIEWS
        c, s = math.cos(yaw), math.sin(yaw)
        ext = np.eye(4)
        ext[:3, :3] = np.array([[s, -c, 0], [0, 0, -1.0], [c, s, 0]])
        ext[:3, 3] = -ext[:3, :3] @ np.array([0.0, 0.0, 1.5])
        k = np.eye(4)
        k[0, 0] = k[1, 1] = f
        k[0, 2], k[1, 2] = pad_w / 2, pad_h / 2
        mats.append(k @ ext)
    return [dict(lidar2img=[m.copy() for m in mats], img_shape=(pad_h, pad_w, 3),
                 input_shape=(pad_h, pad_w), pcd_scale_factor=1.02, pcd_horizontal_flip=True,
                 transformation_3d_flow=["S", "HF"]) for _ in range(BATCH)]


def stage_inputs(head, dev):
    rs = np.random.RandomState(0)
    r, a = rs.uniform(4, 45, (BATCH, PROPOSALS)), rs.uniform(0, 2 * math.pi, (BATCH, PROPOSALS))
    xyz = np.stack([r * np.cos(a), r * np.sin(a), rs.uniform(-1, 1, r.shape)], 1)
    dims = rs.uniform((1.5, 0.6, 1.2), (5.0, 2.2, 2.5), (BATCH, PROPOSALS, 3))
    boxes = np.concatenate([np.moveaxis(xyz, 1, -1), dims, rs.uniform(-3, 3, (BATCH, PROPOSALS, 1)),
                            np.zeros((BATCH, PROPOSALS, 2))], -1)
    boxes[..., 2] -= dims[..., 2] / 2
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
    hid = head.shared_conv.weight.shape[0]
    prev = torch.randn(BATCH, hid, PROPOSALS, device=dev)
    feat = torch.randn(BATCH, VIEWS, hid, MAP_H * MAP_W, device=dev, requires_grad=True)
    pos = head._img_feat_pos(MAP_H, MAP_W, dev, torch.float32)
    metas = ring_metas(MAP_H * 4, MAP_W * 4)
    return prev, t(xyz), [b for b in t(boxes)], feat, pos, metas


def window(fn, repeat):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(repeat):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / repeat


def launches(fn):
    """Device kernels of one call, counted by the profiler."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def host_syncs(fn):
    """Synchronising calls of one call, counted by torch's sync-debug mode."""
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum(1 for w in caught if "synchroniz" in str(w.message)
               and "prototype feature" not in str(w.message))


def compare(name, ours, theirs, repeat, rounds):
    for fn in (ours, theirs):
        for _ in range(3):
            fn()
    a, b = [], []
    for _ in range(rounds):
        a.append(window(ours, repeat))
        b.append(window(theirs, max(1, repeat // 4)))
    row = dict(quantity=name, repeat=repeat, rounds=rounds, fused_ms_median=statistics.median(a),
               fused_ms_min=min(a), composition_ms_median=statistics.median(b),
               composition_ms_min=min(b), fused_launches=launches(ours),
               composition_launches=launches(theirs), fused_host_syncs=host_syncs(ours),
               composition_host_syncs=host_syncs(theirs))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    head = C.build_head(C.TRANSFUSION_VOXEL_LC).to(dev).train()
    for m in head.modules():                        # compare like with like: no random masks
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    prev, pos3d, boxes, feat, pos, metas = stage_inputs(head, dev)

    def fused():
        return head._image_stage_fused(prev, pos3d, boxes, feat, pos, metas, (MAP_H, MAP_W))

    def composed():
        return head._image_stage_composed(prev, pos3d, boxes, feat, pos, metas)

    def backward(fn):
        def run():
            feat.grad = None
            out, _ = fn()
            out.square().sum().backward()
        return run

    with torch.no_grad():
        (a, ma), (b, mb) = fused(), composed()
    assert torch.equal(ma, mb) and int(ma.sum()) > PROPOSALS
    err = float((a - b).abs().max())
    print(json.dumps(dict(quantity="agreement", on_image=int(ma.sum()), rows=ma.numel(),
                          max_abs_difference=err)), flush=True)
    assert err < 1e-3
    rows = []
    with torch.no_grad():
        rows.append(compare("image stage, forward", fused, composed, args.repeat, args.rounds))
    rows.append(compare("image stage, forward + backward", backward(fused), backward(composed),
                        args.repeat, args.rounds))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
