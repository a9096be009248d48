#!/usr/bin/env python
"""Timings of DESIGN 31 on one GPU: PointwiseSemanticHead.get_targets, fused (padding + one
launch of msmd_semantic_targets_f32) against the composition path (the reference's per-sample,
per-box loop on LiDARBoxes.points_in_boxes, with its host reads), at the config's shape (B 2,
16 000 voxels and 30 boxes per sample); and PartA2RPNHead.get_bboxes with the train proposal cfg
(nms_pre 9000, nms_post 512, normal NMS at 0.8) on the 200 x 176 map against the per-sample loop
over the single-list NMS.  Warm-up, then device events around groups of calls; medians.

    python tools/parta2_timing.py --out profiles/parta2_timing.txt
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
import parta2_cases as PC
from msmdfusion_amd import configs as C
from msmdfusion_amd import iou3d
from msmdfusion_amd import kernels as K
from msmdfusion_amd.head_loss import LiDARBoxes
from msmdfusion_amd.parta2_rpn_head import PartA2RPNHead
from msmdfusion_amd.semantic_head import PointwiseSemanticHead, pad_ground_truths

assert torch.cuda.is_available(), "parta2_timing.py needs a GPU"
dev = torch.device("cuda:0")
parser = argparse.ArgumentParser()
parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "parta2_timing.txt"))
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

# ---- get_targets ---------------------------------------------------------------------------
B, ROWS, G, CLASSES = 2, 16000, 30, 3
rng = np.random.default_rng(0)
tables = [PC.make_boxes(rng, G, cell=3.0 * b) for b in range(B)]
centres = np.concatenate([PC.draw_centres(rng, ROWS, t) for t in tables])
coors = np.zeros((B * ROWS, 4), np.int32); coors[:, 0] = np.repeat(np.arange(B), ROWS)
voxels = dict(coors=torch.from_numpy(coors).to(dev), voxel_centers=torch.from_numpy(centres).to(dev))
boxes = [LiDARBoxes(torch.from_numpy(t).to(dev)) for t in tables]
labels = [torch.from_numpy(rng.integers(0, CLASSES, size=G)).long().to(dev) for _ in range(B)]
fused, composed = PointwiseSemanticHead(16, CLASSES), PointwiseSemanticHead(16, CLASSES, fused=False)
a, b = fused.get_targets(voxels, boxes, labels), composed.get_targets(voxels, boxes, labels)
pos = (a["seg_targets"] >= 0) & (a["seg_targets"] < CLASSES)
say("get_targets, B %d, %d voxels and %d boxes per sample: %d positive rows, %d ignored; seg targets that differ "
    "between the two paths: %d; largest part-target difference: %.3e" % (
        B, ROWS, G, int(pos.sum()), int((a["seg_targets"] == -1).sum()),
        int((a["seg_targets"] != b["seg_targets"]).sum()), float((a["part_targets"] - b["part_targets"]).abs().max())))
say("fused get_targets (padding + enlarged table + one launch), 0 host reads:",
    timed(lambda: fused.get_targets(voxels, boxes, labels), 10, 7, 50))
table, lab, counts = pad_ground_truths(boxes, labels, dev)
big = LiDARBoxes(table.view(-1, 7)).enlarged_box(0.2).tensor.view(table.shape).contiguous()
ids = voxels["coors"][:, 0].contiguous()
say("the launch alone:", timed(lambda: K.semantic_targets(voxels["voxel_centers"], ids, table, big, lab, counts, CLASSES), 10, 7, 200))
say("composition path (per sample two points_in_boxes launches and the loop over boxes, %d host reads per step):" % (B * G),
    timed(lambda: composed.get_targets(voxels, boxes, labels), 3, 5, 5))

# ---- get_bboxes ----------------------------------------------------------------------------
model = C.PARTA2_SECFPN_KITTI_3CLASS["model"]
cfg = model["train_cfg"]["rpn_proposal"]
args = dict(model["rpn_head"], train_cfg=model["train_cfg"]["rpn"], test_cfg=model["test_cfg"]["rpn"])
args.pop("type")
head = PartA2RPNHead(**args).to(dev).eval()
gen = torch.Generator().manual_seed(1)
H, W, A = 200, 176, head.num_anchors
outs = [[(torch.randn((B, A * c, H, W), generator=gen) * s).to(dev)] for c, s in ((3, 1.5), (7, 0.1), (2, 1.0))]

def nms(kind, bx, sc, thr):
    fn = iou3d.nms_gpu if kind == "rotate" else iou3d.nms_normal_gpu
    return fn(bx.contiguous(), sc.contiguous(), thr)

with torch.no_grad():
    got = head.get_bboxes(*outs, [None] * B, cfg)
    want = PC.rpn_loop(head, *outs, cfg, nms=nms)
    say("get_bboxes, train proposal cfg %s, %d x %d map, %d anchors per sample, B %d: kept %s; results equal to the per-sample loop: %s"
        % (cfg, H, W, H * W * A, B, [int(r["scores_3d"].numel()) for r in got],
           all(torch.equal(g[k], w[k]) for g, w in zip(got, want) for k in g)))
    say("batched get_bboxes (one NMS call, 1 host read):", timed(lambda: head.get_bboxes(*outs, [None] * B, cfg), 3, 5, 10))
    say("per-sample loop over the single-list NMS (boolean-mask compaction and len(selected) per sample):",
        timed(lambda: PC.rpn_loop(head, *outs, cfg, nms=nms), 2, 5, 5))
