#!/usr/bin/env python
"""Timings of DESIGN 32 on one GPU, in one process: PartAggregationROIHead._assign_and_sample +
PartA2BboxHead.get_targets, fused (msmd_roi_assign3d_f32 + msmd_roi_sample_targets_f32 and the one
read of the counts) against the fused=False loop (the reference's per-sample, per-class loop on
K.boxes_iou3d matrices with its host reads), at the config's shape (B 2, 512 proposals and 30
boxes per sample, 3 classes, num 128); and PartA2BboxHead.get_bboxes, batched (one NMS call over
the B x C lists) against the per-sample, per-class multi_class_nms loop at the test shape (100
RoIs per sample).  The yardstick is the composition path.  Warm-up, then device events around
groups of calls; median with min / max over the rounds.

    python tools/parta2_roi_timing.py --out profiles/parta2_roi_timing.txt
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import parta2_roi_cases as RC
from msmdfusion_amd import configs as C
from msmdfusion_amd import registry
from msmdfusion_amd.parta2_roi_head import PartAggregationROIHead
from msmdfusion_amd.semantic_head import PointwiseSemanticHead

assert torch.cuda.is_available(), "parta2_roi_timing.py needs a GPU"
dev = torch.device("cuda:0")
parser = argparse.ArgumentParser()
parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "parta2_roi_timing.txt"))
out = open(parser.parse_args().out, "w")
def say(*a):
    line = " ".join(str(x) for x in a); print(line, flush=True); out.write(line + "\n"); out.flush()

def timed(fn, warm, rounds, per_round):
    """Median, min and max over `rounds` of the device time per call (events around per_round calls)."""
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(per_round): fn()
        stop.record(); torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / per_round)
    return "median %.3f ms (min %.3f, max %.3f; %d rounds of %d after %d warm-up)" % (
        statistics.median(times), min(times), max(times), rounds, per_round, warm)

# ---- _assign_and_sample + get_targets ------------------------------------------------------
B, P, G, CLASSES = 2, 512, 30, 3
model = C.PARTA2_SECFPN_KITTI_3CLASS["model"]
rcnn = model["train_cfg"]["rcnn"]
case = RC.make_case(77, (P,) * B, (G,) * B, classes=CLASSES)
proposals = [dict(boxes_3d=torch.from_numpy(p).to(dev), labels_3d=torch.from_numpy(l).to(dev))
             for p, l in zip(case["props"], case["prop_labels"])]
gts = [torch.from_numpy(g).to(dev) for g in case["gt"]]
gt_labels = [torch.from_numpy(l).to(dev) for l in case["gt_labels"]]
bbox_cfg = dict(model["roi_head"]["bbox_head"], roi_feat_size=4, shared_fc_channels=[256, 32])   # (targets only)
bbox_head = registry.build_head(bbox_cfg)
heads = {f: PartAggregationROIHead(PointwiseSemanticHead(16, CLASSES), CLASSES, train_cfg=rcnn, fused=f)
         for f in (True, False)}
keys = heads[True].draw_keys([p["boxes_3d"] for p in proposals], torch.Generator(device=dev).manual_seed(0))

def step(fused):
    return bbox_head.get_targets(heads[fused]._assign_and_sample(proposals, gts, gt_labels, keys=keys), rcnn)

a, b = step(True), step(False)
say("_assign_and_sample + get_targets, B %d, %d proposals and %d boxes per sample, %d classes, num %d: %d sampled rows, "
    "%d positive; tensors equal between the two paths: %s; largest bbox_targets difference: %.3e" % (
        B, P, G, CLASSES, rcnn["sampler"]["num"], a[0].numel(), int(a[3].sum()),
        all(torch.equal(x, y) for k, (x, y) in enumerate(zip(a, b)) if k != 1),
        float((a[1] - b[1]).abs().max()) if a[1].numel() else 0.0))
say("fused (memset + 3 launches, 1 host read):", timed(lambda: step(True), 10, 7, 50))
say("fused=False loop (per sample and class: mask gathers, an IoU matrix, the loop over ground truths, the sampler's chain):",
    timed(lambda: step(False), 2, 5, 3))

# ---- get_bboxes ----------------------------------------------------------------------------
N = model["test_cfg"]["rpn"]["nms_post"]
test_cfg = model["test_cfg"]["rcnn"]
rng = np.random.RandomState(3)
rois, labels, preds = [], [], []
for s in range(B):
    centres, _ = RC.make_gt(rng, 25, CLASSES)
    box = centres[rng.randint(0, 25, N)].astype(np.float64)
    box[:, :2] += rng.uniform(-0.8, 0.8, (N, 2))
    rois.append(np.concatenate([np.full((N, 1), s), box], 1).astype(np.float32))
    labels.append(torch.from_numpy(rng.randint(0, CLASSES, N)).to(dev))
    preds.append(torch.from_numpy(rng.uniform(0, 1, (N, CLASSES)).astype(np.float32)).to(dev))
rois = torch.from_numpy(np.concatenate(rois)).to(dev)
cls_score = torch.from_numpy(rng.normal(size=(B * N, 1)).astype(np.float32)).to(dev)
bbox_pred = torch.from_numpy((rng.normal(size=(B * N, 7)) * 0.05).astype(np.float32)).to(dev)

def loop():
    decoded = bbox_head.decode_rois(rois, bbox_pred)
    res = []
    for s in range(B):
        cur = decoded[s * N:(s + 1) * N]
        sel = bbox_head.multi_class_nms(preds[s], cur, test_cfg["score_thr"], test_cfg["nms_thr"], None,
                                        test_cfg["use_rotate_nms"])
        res.append((cur[sel], cls_score[s * N:(s + 1) * N].view(-1)[sel], labels[s][sel]))
    return res

with torch.no_grad():
    got, want = bbox_head.get_bboxes(rois, cls_score, bbox_pred, labels, preds, None, cfg=test_cfg), loop()
    say("get_bboxes, test cfg %s, %d RoIs per sample, B %d, %d classes: kept %s; results equal to the per-sample, per-class loop: %s"
        % (test_cfg, N, B, CLASSES, [int(r[1].numel()) for r in got],
           all(torch.equal(x, y) for g, w in zip(got, want) for x, y in zip(g, w))))
    say("batched get_bboxes (one NMS call, 1 host read):",
        timed(lambda: bbox_head.get_bboxes(rois, cls_score, bbox_pred, labels, preds, None, cfg=test_cfg), 5, 7, 20))
    say("per-sample, per-class multi_class_nms loop (a host read and an NMS call per class):", timed(loop, 3, 5, 5))
