#!/usr/bin/env python
"""SSD3DHead at a KITTI-like shape: get_targets (batch 4, 256 candidates, about 30 ground truths
per sample) and get_bboxes (256 boxes x 4 samples), each beside the reference's structure -- the
per-sample loop of tests/ssd3d_ref.py -- on the same device.  One JSON line per quantity
(DESIGN section 20).

    python tools/ssd3d_timing.py [--repeat 20] [--rounds 5] [--out FILE]

The loop's two points-in-boxes passes per sample run on the device (msmd_points_in_boxes_f32, as
the reference's points_in_boxes_gpu does), and its NMS is the same native pair test called once
per sample with a host read of the kept list, as mmcv's nms does.  Times are device-synchronised
host clocks around `repeat` back-to-back calls, after warm-up calls of the same shape; the two
versions alternate round by round and the median round is reported.  Launches are counted by
torch.profiler over one call (null where the profiler reports none).  Needs a GPU.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssd3d_ref as S  # noqa: E402
from msmdfusion_amd import configs as C  # noqa: E402
from msmdfusion_amd import iou3d  # noqa: E402
from msmdfusion_amd import kernels as K  # noqa: E402
from msmdfusion_amd.head_loss import LiDARBoxes  # noqa: E402
from msmdfusion_amd.registry import build_head  # noqa: E402

BATCH, SEEDS, CANDIDATES, GTS, CLASSES, BINS = 4, 512, 256, 30, 3, 12


def window(fn, repeat):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeat):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / repeat


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if "LaunchKernel" in e.name)
        return n or None
    except Exception:                                   # noqa: BLE001 -- a count, not a result
        return None


def compare(name, ours, theirs, repeat, rounds, extra):
    for fn in (ours, theirs):
        for _ in range(2):
            fn()
    a, b = [], []
    for _ in range(rounds):
        a.append(window(ours, repeat))
        b.append(window(theirs, max(1, repeat // 4)))
    row = dict(quantity=name, repeat=repeat, rounds=rounds, fused_ms_median=statistics.median(a),
               fused_ms_min=min(a), loop_ms_median=statistics.median(b), loop_ms_min=min(b),
               fused_launches=launches(ours), loop_launches=launches(theirs), **extra)
    print(json.dumps(row), flush=True)
    return row


def device_first_box(points, boxes):
    return K.points_in_boxes(boxes[None, :, :7].contiguous(), points[None].contiguous(), False)[0]


def bboxes_loop(head, preds):
    """SSD3DHead.get_bboxes / multiclass_nms_single per sample (ssd_3d_head.py:439-543): one NMS
    call and one host read per sample."""
    cfg = head.test_cfg
    sem_scores = torch.sigmoid(preds["obj_scores"]).transpose(1, 2)
    obj_scores = sem_scores.max(-1)[0]
    bbox3d = head.bbox_coder.decode(preds)
    results = []
    for b in range(bbox3d.shape[0]):
        bbox = LiDARBoxes(bbox3d[b].clone(), origin=(0.5, 0.5, 1.0))
        corner3d = bbox.corners
        minmax = torch.cat([corner3d.min(1)[0], corner3d.max(1)[0]], 1)[:, [0, 1, 3, 4]]
        classes = torch.argmax(sem_scores[b], -1)
        shifted = minmax + (classes.to(minmax) * (minmax.max() + 1))[:, None]
        offsets = torch.tensor([0, len(bbox)], dtype=torch.int32).to(minmax.device, non_blocking=True)
        keep, num = iou3d.nms_batched("mmcv", shifted, obj_scores[b], offsets,
                                      cfg["nms_cfg"]["iou_thr"])
        keep = keep[0, :int(num[0])][:cfg["max_output_num"]]            # the host read
        mask = torch.zeros_like(classes).scatter(0, keep, 1)
        selected = mask.bool() & (obj_scores[b] >= cfg["score_thr"])
        results.append((bbox.tensor[selected], obj_scores[b][selected], classes[selected]))
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ssd3d_timing needs a GPU"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    m = copy.deepcopy(C.SSD3D_KITTI_CAR["model"])
    m["bbox_head"]["num_classes"] = CLASSES
    torch.manual_seed(0)
    head = build_head(dict(m["bbox_head"], train_cfg=dict(m["train_cfg"], pos_distance_thr=1.5),
                           test_cfg=dict(m["test_cfg"], per_class_proposal=False))).to(dev)
    t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)   # noqa: E731

    counts = [GTS - 3, GTS, GTS + 2, GTS + 1]
    gt_rows, gt_labels = [], []
    for n in counts:
        gt_rows.append(t(np.concatenate([rng.uniform(0, 60, (n, 2)), rng.uniform(-1.5, -0.5, (n, 1)),
                                         rng.uniform(1.4, 4.5, (n, 3)), rng.uniform(-3.1, 3.1, (n, 1))],
                                        1)))
        labels = rng.integers(0, CLASSES, n)
        labels[rng.integers(0, n, 2)] = -1
        gt_labels.append(t(labels, np.int64))
    gt_boxes = [LiDARBoxes(r) for r in gt_rows]
    pick = [r[torch.from_numpy(rng.integers(0, len(r), CANDIDATES)).to(dev)] for r in gt_rows]
    aggregated = torch.stack([p[:, :3] + t(rng.normal(0, 0.8, (CANDIDATES, 3))) for p in pick])
    aggregated[..., 2] += 0.7
    seeds = torch.cat([aggregated + t(rng.normal(0, 0.3, (BATCH, CANDIDATES, 3))),
                       t(rng.uniform(0, 60, (BATCH, SEEDS - CANDIDATES, 3)))], 1)
    preds = dict(aggregated_points=aggregated.contiguous(), seed_points=seeds.contiguous())
    rows = []

    # ---- get_targets
    S.FIRST_BOX = device_first_box
    ours = lambda: head.get_targets(None, gt_boxes, gt_labels, None, None, preds)        # noqa: E731
    theirs = lambda: S.targets(gt_rows, gt_labels, aggregated, seeds, CANDIDATES, CLASSES, BINS,  # noqa: E731
                               1.5, 0.05)
    got, want = ours(), theirs()
    same = all(torch.equal(got[i], want[i]) for i in (3, 5, 9, 10)) and \
        torch.equal(got[8] > 0, want[8] > 0)
    err = float((got[6] - want[6]).abs().max())
    rows.append(compare("get_targets", ours, theirs, args.repeat, args.rounds,
                        dict(equal_to_loop=bool(same), centerness_max_abs_diff=err,
                             positives=int(got[9].sum()), negatives=int(got[10].sum()),
                             voted=int((got[8] > 0).sum()), host_reads_fused=0,
                             host_reads_loop="one per sample (valid_gt.sum() == 0)")))

    # ---- get_bboxes
    g = torch.Generator().manual_seed(1)
    box_preds = dict(
        center=aggregated, size=(torch.rand((BATCH, CANDIDATES, 3), generator=g) * 1.5 + 0.5).to(dev),
        dir_class=torch.randn((BATCH, CANDIDATES, BINS), generator=g).to(dev),
        dir_res=(torch.randn((BATCH, CANDIDATES, BINS), generator=g) * 0.1).to(dev),
        obj_scores=torch.randn((BATCH, CLASSES, CANDIDATES), generator=g).to(dev))
    ours = lambda: head.get_bboxes(None, box_preds, None)                                # noqa: E731
    theirs = lambda: bboxes_loop(head, box_preds)                                        # noqa: E731
    got, want = ours(), theirs()
    same = all(torch.equal(a[0].tensor, b[0]) and torch.equal(a[2], b[2]) for a, b in zip(got, want))
    rows.append(compare("get_bboxes", ours, theirs, args.repeat, args.rounds,
                        dict(equal_to_loop=bool(same), kept=[len(a[0]) for a in got],
                             host_reads_fused=1, host_reads_loop=BATCH)))
    if args.out:
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
