#!/usr/bin/env python
"""Times FreeAnchor3DHead.loss (forward + backward) and its four library calls against the
torch matrix restatement of the reference's algorithm (tests/free_anchor_ref.py: per sample the
two [num_gt, num_anchors] IoU matrices, a sort, the per-class maximum) on the same device.

    python tools/free_anchor_timing.py [--repeat 20] [--warmup 3] [--only fused|restatement]
                                       [--batch 4] [--boxes 64] [--scale 1]

Shape: the head of configs.FREE_ANCHOR_HEAD_NUS (levels 200^2, 100^2, 50^2 x 8 anchors =
420 000 anchors, 10 classes, k = 25, code size 9), batch 4, 64 boxes per sample; --scale divides
the map sides (a rehearsal size).  Predictions near a third of the boxes are encode(anchor, gt)
plus noise, so the box probability is not empty.  Prints one JSON line: median milliseconds
(device synchronised around each run) of the loss and of each piece on both paths, the peak
memory each path adds, and whether the two paths agree on what they time.  `--only` runs one
path, for a kernel trace of it alone.
"""
import argparse
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
import free_anchor_ref as R  # noqa: E402
from msmdfusion_amd import anchor_head as A  # noqa: E402
from msmdfusion_amd import configs as C  # noqa: E402
from msmdfusion_amd import kernels as K  # noqa: E402
from msmdfusion_amd.registry import build_head  # noqa: E402


def timed(fn, repeat, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 3)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--boxes", type=int, default=64)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--only", choices=["fused", "restatement"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    head = build_head(dict(C.FREE_ANCHOR_HEAD_NUS, in_channels=8, feat_channels=8,
                           train_cfg=C.FREE_ANCHOR_TRAIN_CFG_NUS["pts"], test_cfg=None)).to(dev)
    sizes = [(200 // args.scale // s, 200 // args.scale // s) for s in (1, 2, 4)]
    levels = head.anchor_generator.grid_anchors(sizes, dev)
    code, ncls, k, B = head.box_code_size, head.num_classes, head.pre_anchor_topk, args.batch
    anchors = torch.cat([a.reshape(-1, code) for a in levels])
    A_ = anchors.shape[0]
    rs = np.random.RandomState(0)
    g = torch.Generator().manual_seed(0)
    boxes, labels = [], []
    deltas = (torch.randn((B, A_, code), generator=g) * 0.1).to(dev)
    bev = A.nearest_bev(anchors)
    for b in range(B):
        pick = anchors[torch.from_numpy(rs.randint(0, A_, args.boxes)).to(dev)].clone()
        pick[:, :2] += torch.from_numpy(rs.uniform(-0.3, 0.3, (args.boxes, 2)).astype(np.float32)).to(dev)
        pick[:, 3:6] *= torch.from_numpy(rs.uniform(0.9, 1.15, (args.boxes, 3)).astype(np.float32)).to(dev)
        pick[:, 6] = torch.from_numpy(rs.uniform(-3, 3, args.boxes).astype(np.float32)).to(dev)
        boxes.append(pick)
        labels.append(torch.from_numpy(rs.randint(0, ncls, args.boxes)).to(dev))
        near = pick[::3]
        bag = K.free_anchor_topk(bev, A.nearest_bev(near), k).long()
        enc = A.DeltaXYZWLHRBBoxCoder.encode(anchors[bag], near[:, None].expand(-1, k, -1))
        deltas[b][bag.reshape(-1)] = (enc + torch.randn(enc.shape, generator=g).to(dev) * 0.05
                                      ).reshape(-1, code)
    na = head.num_anchors
    split = lambda flat, c: [t.reshape(B, h, w, na * c).permute(0, 3, 1, 2).contiguous()
                             for t, (h, w) in zip(flat.split([h * w * na for h, w in sizes], 1),
                                                  sizes)]
    preds = [split(torch.randn((B, A_, ncls), generator=g).to(dev) - 3.0, ncls), split(deltas, code),
             split(torch.randn((B, A_, 2), generator=g).to(dev), 2)]
    gt = torch.cat(boxes)
    gt_bev, gt_labels = A.nearest_bev(gt).contiguous(), torch.cat(labels)
    counts = [args.boxes] * B
    offsets = torch.tensor(np.cumsum([0] + counts), dtype=torch.int32).to(dev)
    flat_deltas = deltas.reshape(B * A_, code).contiguous()
    logits = R._flatten(preds[0], ncls).reshape(B * A_, ncls).contiguous()

    def loss_of(fn):
        def run():
            leaves = [[v.detach().requires_grad_() for v in lv] for lv in preds]
            losses = fn(leaves)
            (losses["positive_bag_loss"] + losses["negative_bag_loss"]).backward()
            return losses, leaves
        return run

    fused = loss_of(lambda lv: head.loss(*lv, boxes, labels, None))
    plain = loss_of(lambda lv: R.loss_restatement(head, anchors, *lv, boxes, labels)[0])
    out = dict(anchors=A_, batch=B, boxes=args.boxes, classes=ncls, k=k, repeat=args.repeat,
               matrix_bytes=B * args.boxes * A_ * 4)
    pred_bev = K.decode_nearest_bev(anchors, flat_deltas)
    box_prob = K.free_anchor_box_prob(pred_bev, gt_bev, gt_labels, offsets, ncls, head.bbox_thr)

    def neg(fn):
        def run():
            x = logits.detach().requires_grad_()
            fn(x).backward()
            return x.grad
        return run
    pieces = dict(
        decode=(lambda: K.decode_nearest_bev(anchors, flat_deltas),
                lambda: R.decode_bev_restatement(anchors, flat_deltas)),
        box_prob=(lambda: K.free_anchor_box_prob(pred_bev, gt_bev, gt_labels, offsets, ncls,
                                                 head.bbox_thr),
                  lambda: R.box_prob_restatement(pred_bev, gt_bev, gt_labels, counts, ncls,
                                                 head.bbox_thr)),
        topk=(lambda: K.free_anchor_topk(bev, gt_bev, k),
              lambda: torch.cat([R.topk_restatement(bev, gt_bev[b * args.boxes:(b + 1) * args.boxes],
                                                    k) for b in range(B)])),
        negative_fwd_bwd=(neg(lambda x: head.negative_bag_loss(x, box_prob)),
                          neg(lambda x: R.negative_restatement(x, box_prob, head.gamma,
                                                               head.alpha))))
    for which, idx in (("fused", 0), ("restatement", 1)):
        if args.only and args.only != which:
            continue
        run = fused if idx == 0 else plain
        run()
        out[which + "_loss_ms"] = timed(run, args.repeat, args.warmup)
        out[which + "_loss_peak_bytes"] = peak_of(run)
        for name, pair in pieces.items():
            out["%s_%s_ms" % (which, name)] = timed(pair[idx], args.repeat, args.warmup)
    if args.only is None:
        (lf, gf), (lp, gp) = fused(), plain()
        out["loss_fused"] = {key: float(v.detach()) for key, v in lf.items()}
        out["loss_restatement"] = {key: float(v.detach()) for key, v in lp.items()}
        out["max_grad_difference"] = max(float((a.grad - b.grad).abs().max())
                                         for x, y in zip(gf, gp) for a, b in zip(x, y))
        out["topk_equal"] = bool(torch.equal(pieces["topk"][0]().long(), pieces["topk"][1]()))
        out["box_prob_equal"] = bool(torch.equal(pieces["box_prob"][0](), pieces["box_prob"][1]()))
        out["box_prob_nonzero"] = int((box_prob > 0).sum())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
