#!/usr/bin/env python
"""VoteHead at the SUN RGB-D training shape (batch 8, 20 000 points, 1024 seeds, 256 proposals,
64 ground truths per sample): get_targets, the two Chamfer losses (forward + backward) and
get_bboxes, each beside the same quantity computed by the loop / expanded-matrix restatements
the tests use, on the same device.  One JSON line per quantity.

    python tools/vote_timing.py [--repeat 20] [--rounds 5] [--out FILE]

Times are device-synchronised host clocks around `repeat` back-to-back calls, after warm-up
calls of the same shape; the two versions alternate round by round and the median round is
reported.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vote_ref as V  # noqa: E402
from msmdfusion_amd import configs as C  # noqa: E402
from msmdfusion_amd import losses as L  # noqa: E402
from msmdfusion_amd.head_loss import DepthBoxes  # noqa: E402
from msmdfusion_amd.registry import build_head  # noqa: E402

BATCH, POINTS, SEEDS, PROPOSALS, GTS, CLASSES, BINS = 8, 20000, 1024, 256, 64, 10, 12


def window(fn, repeat):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeat):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / repeat


def compare(name, ours, theirs, repeat, rounds, extra):
    for fn in (ours, theirs):
        for _ in range(2):
            fn()
    a, b = [], []
    for _ in range(rounds):
        a.append(window(ours, repeat))
        b.append(window(theirs, max(1, repeat // 4)))
    row = dict(quantity=name, repeat=repeat, rounds=rounds, kernel_ms_median=statistics.median(a),
               kernel_ms_min=min(a), restatement_ms_median=statistics.median(b),
               restatement_ms_min=min(b), **extra)
    print(json.dumps(row), flush=True)
    return row


def targets_loop(head, points, gt_boxes, gt_labels, aggregated):
    """VoteHead.get_targets_single per sample: the inclusion table, the reference's loop over
    ground truths and slots, the expanded Chamfer matrix (tests/test_gpu_vote_head.py)."""
    coder, cfg, out = head.bbox_coder, head.train_cfg, []
    for b in range(len(gt_labels)):
        boxes, labels = gt_boxes[b], gt_labels[b]
        inside = boxes.points_in_boxes(points[b][:, :3])
        votes, mask = V.vote_targets_loop(points[b], inside, boxes.gravity_center)
        center, size_class, size_res, dir_class, dir_res = coder.encode(boxes, labels)
        d1, _, assignment, _ = L.chamfer_distance_expanded(aggregated[b][None], center[None], "l2")
        assignment, dist = assignment[0], torch.sqrt(d1[0] + 1e-6)
        objectness = (dist < cfg["pos_distance_thr"]).long()
        size_class = size_class[assignment]
        out.append((votes, mask, size_class, size_res[assignment] / coder.mean_size_tensor(
            size_res)[size_class], dir_class[assignment], dir_res[assignment] / (np.pi / BINS),
            center[assignment], labels[assignment], objectness))
    return [torch.stack(x) for x in zip(*out)]


def aligned_3d_nms_loop(boxes, scores, classes, thresh):
    """box3d_nms.py:91-138 as written: a while loop with one host read per kept box."""
    x1, y1, z1, x2, y2, z2 = (boxes[:, i] for i in range(6))
    area = (x2 - x1) * (y2 - y1) * (z2 - z1)
    zero = boxes.new_zeros(1, )
    score_sorted = torch.argsort(scores)
    pick = []
    while score_sorted.shape[0] != 0:
        last = score_sorted.shape[0]
        i = score_sorted[-1]
        pick.append(i)
        rest = score_sorted[:last - 1]
        xx1, yy1, zz1 = torch.max(x1[i], x1[rest]), torch.max(y1[i], y1[rest]), \
            torch.max(z1[i], z1[rest])
        xx2, yy2, zz2 = torch.min(x2[i], x2[rest]), torch.min(y2[i], y2[rest]), \
            torch.min(z2[i], z2[rest])
        inter = torch.max(zero, xx2 - xx1) * torch.max(zero, yy2 - yy1) * torch.max(zero, zz2 - zz1)
        iou = inter / (area[i] + area[rest] - inter)
        iou = iou * (classes[i] == classes[rest]).float()
        score_sorted = score_sorted[torch.nonzero(iou <= thresh, as_tuple=False).flatten()]
    return boxes.new_tensor(pick, dtype=torch.long)


def bboxes_loop(head, points, preds):
    """VoteHead.get_bboxes / multiclass_nms_single per sample (vote_head.py:566-666)."""
    obj_scores = F.softmax(preds["obj_scores"], dim=-1)[..., -1]
    sem_scores = F.softmax(preds["sem_scores"], dim=-1)
    bbox3d = head.bbox_coder.decode(preds)
    results = []
    for b in range(bbox3d.shape[0]):
        bbox = DepthBoxes(bbox3d[b], box_dim=7, with_yaw=True, origin=(0.5, 0.5, 0.5))
        box_indices = bbox.points_in_boxes(points[b, :, :3])
        corner3d = bbox.corners
        minmax = torch.cat([torch.min(corner3d, dim=1)[0], torch.max(corner3d, dim=1)[0]], 1)
        nonempty = box_indices.T.sum(1) > 5
        classes = torch.argmax(sem_scores[b], -1)
        picked = aligned_3d_nms_loop(minmax[nonempty], obj_scores[b][nonempty], classes[nonempty],
                                     head.test_cfg["nms_thr"])
        inds = torch.nonzero(nonempty, as_tuple=False).flatten()
        mask = torch.zeros_like(classes).scatter(0, inds[picked], 1)
        selected = mask.bool() & (obj_scores[b] > head.test_cfg["score_thr"])
        results.append((bbox.tensor[selected], obj_scores[b][selected], classes[selected]))
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "vote_timing needs a GPU"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    m = C.VOTENET_SUNRGBD["model"]
    torch.manual_seed(0)
    head = build_head(dict(m["bbox_head"], train_cfg=m["train_cfg"],
                           test_cfg=dict(m["test_cfg"], per_class_proposal=False))).to(dev)
    t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)   # noqa: E731

    points = t(np.concatenate([rng.uniform(-4, 4, (BATCH, POINTS, 2)),
                               rng.uniform(0, 2.5, (BATCH, POINTS, 1)),
                               rng.uniform(0, 1, (BATCH, POINTS, 1))], 2))
    sizes = np.asarray(head.bbox_coder.mean_sizes)
    gt_labels_np = rng.integers(0, CLASSES, (BATCH, GTS))
    gt_np = np.concatenate([rng.uniform(-3.5, 3.5, (BATCH, GTS, 2)), rng.uniform(0, 0.8, (BATCH, GTS, 1)),
                            sizes[gt_labels_np] * rng.uniform(0.8, 1.2, (BATCH, GTS, 3)),
                            rng.uniform(-3.1, 3.1, (BATCH, GTS, 1))], 2)
    gt_boxes = [DepthBoxes(t(gt_np[b])) for b in range(BATCH)]
    gt_labels = [t(gt_labels_np[b], np.int64) for b in range(BATCH)]
    centers = torch.stack([g.gravity_center for g in gt_boxes])
    pick = t(rng.integers(0, GTS, (BATCH, PROPOSALS)), np.int64)
    aggregated = torch.gather(centers, 1, pick[..., None].expand(-1, -1, 3)) + \
        t(rng.normal(0, 0.25, (BATCH, PROPOSALS, 3)))
    preds = dict(aggregated_points=aggregated.contiguous())
    rows = []

    # ---- get_targets
    ours = lambda: head.get_targets(points, gt_boxes, gt_labels, None, None, preds)      # noqa: E731
    theirs = lambda: targets_loop(head, points, gt_boxes, gt_labels, aggregated)        # noqa: E731
    got, want = ours(), theirs()
    same = all(torch.equal(got[i], want[j]) for i, j in ((1, 1), (2, 2), (4, 4), (8, 7), (10, 8)))
    same = same and bool(torch.equal(got[0], want[0]))
    rows.append(compare("get_targets", ours, theirs, args.repeat, args.rounds,
                        dict(equal_to_restatement=bool(same),
                             positives=int(got[10].sum()), voted_points=int(got[1].sum()))))

    # ---- the two Chamfer losses, forward + backward
    for name, shape, mode in (("center_loss_chamfer", (BATCH, PROPOSALS, GTS), "l2"),
                              ("vote_loss_chamfer", (BATCH * SEEDS, 1, 3), "l1")):
        b, n, k = shape
        src, dst = t(rng.normal(0, 1.5, (b, n, 3))), t(rng.normal(0, 1.5, (b, k, 3)))
        w1, w2 = t(rng.uniform(0, 1, (b, n))), t(rng.uniform(0, 1, (b, k)))

        def run(fn, src=src, dst=dst, w1=w1, w2=w2, mode=mode):
            s, d = src.clone().requires_grad_(), dst.clone().requires_grad_()
            a, c = fn(s, d, mode)[:2]
            ((a * w1).sum() + (c * w2).sum()).backward()
            return s.grad, d.grad

        g_ours, g_theirs = run(L.chamfer_min), run(L.chamfer_distance_expanded)
        err = max(float((g_ours[0] - g_theirs[0]).abs().max()),
                  float((g_ours[1] - g_theirs[1]).abs().max()))
        rows.append(compare(name, lambda: run(L.chamfer_min),
                            lambda: run(L.chamfer_distance_expanded), args.repeat, args.rounds,
                            dict(shape=list(shape), mode=mode, grad_max_abs_diff=err)))

    # ---- get_bboxes
    g = torch.Generator().manual_seed(1)
    box_preds = dict(
        center=aggregated, dir_class=torch.randn((BATCH, PROPOSALS, BINS), generator=g).to(dev),
        dir_res=(torch.randn((BATCH, PROPOSALS, BINS), generator=g) * 0.1).to(dev),
        size_class=torch.randn((BATCH, PROPOSALS, CLASSES), generator=g).to(dev),
        size_res=(torch.randn((BATCH, PROPOSALS, CLASSES, 3), generator=g) * 0.1).to(dev),
        obj_scores=torch.randn((BATCH, PROPOSALS, 2), generator=g).to(dev),
        sem_scores=torch.randn((BATCH, PROPOSALS, CLASSES), generator=g).to(dev))
    ours = lambda: head.get_bboxes(points, box_preds, None)                              # noqa: E731
    theirs = lambda: bboxes_loop(head, points, box_preds)                                # noqa: E731
    got, want = ours(), theirs()
    same = all(torch.equal(a[0].tensor, b[0]) and torch.equal(a[2], b[2]) for a, b in zip(got, want))
    rows.append(compare("get_bboxes", ours, theirs, args.repeat, args.rounds,
                        dict(equal_to_restatement=bool(same), kept=[len(a[0]) for a in got])))
    if args.out:
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
