#!/usr/bin/env python
"""Generates tests/golden/free_anchor_vectors.npz by RUNNING the reference's own

    FreeAnchor3DHead.loss / positive_bag_loss / negative_bag_loss
        mmdet3d/models/dense_heads/free_anchor3d_head.py:42-282

taken from the reference FILE at run time (ast), on top of everything make_anchor_head_golden.py
takes the same way (Anchor3DHead, the generators, the coder, bbox_overlaps_nearest_3d,
get_direction_target, LiDARInstance3DBoxes) and with that script's mmdet stand-ins.  Two of them
gain mmdet's `reduction_override` argument here (SmoothL1Loss / CrossEntropyLoss.forward:
`reduction = reduction_override if reduction_override else self.reduction`).  The head is the
reference's class with its attributes set by hand; `get_anchors` returns the generator's anchors
on the CPU (the reference's loss asks for the default device, 'cuda') in the run's dtype, and
`zip` hands out tensor rows as t[i] (see _zip).

Each case runs the loss twice, in float32 and with float64 leaves and anchors (the reference's
box type keeps the IoUs themselves in float32).  Stored: the inputs, both losses, the per-sample
box_prob (the argument negative_bag_loss receives), every ground truth's bag (what torch.topk
returned, sorted), and the float32 and float64 gradients of the three prediction lists.

Cases (batch 2, k = 6, bbox_thr 0.6):
  k05 / k15   KITTI style: Anchor3DRangeGenerator, code 7, three classes, one 8 x 6 map; samples
              with 0 and 5, and with 1 and 5 ground truths
  n05 / n15   nuScenes style: AlignedAnchor3DRangeGenerator, code 9 with code_weight, maps 8 x 6
              and 4 x 3; the same counts
Predictions of the anchors in a bag are encode(anchor, gt) plus noise (so box_prob is not zero),
except for each sample's last ground truth, whose bag keeps the random predictions (so one
best IoU stays below the threshold).  The script ASSERTS the conditions under which the
reference is well defined (check()).  Only inputs and outputs are stored.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_anchor_head_golden as MA  # noqa: E402

ML = MA.ML
OUT = os.path.join(ROOT, "tests", "golden", "free_anchor_vectors.npz")
TOPK, BBOX_THR, GAMMA, ALPHA = 6, 0.6, 2.0, 0.5
PATH = MA.REF + "models/dense_heads/free_anchor3d_head.py"


class SmoothL1Loss(MA.SmoothL1Loss):
    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        reduction = reduction_override if reduction_override else self.reduction
        diff = torch.abs(pred - target)
        loss = torch.where(diff < self.beta, 0.5 * diff * diff / self.beta, diff - 0.5 * self.beta)
        return self.loss_weight * ML.weight_reduce_loss(loss, weight, reduction, avg_factor)


class CrossEntropyLoss(MA.CrossEntropyLoss):
    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None):
        reduction = reduction_override if reduction_override else self.reduction
        loss = torch.nn.functional.cross_entropy(cls_score, label, reduction="none")
        if weight is not None:
            weight = weight.float()
        return self.loss_weight * ML.weight_reduce_loss(loss, weight, reduction, avg_factor)


def _zip(*seqs):
    """zip over the rows of a tensor as t[0], t[1], ...: what iterating a tensor gave in the torch
    the reference was written for.  (Today's Tensor.__iter__ unbinds, and autograd refuses the
    reference's in-place write, free_anchor3d_head.py:204, into an unbound view.)"""
    return zip(*[[s[i] for i in range(len(s))] if torch.is_tensor(s) else s for s in seqs])


def reference_namespace():
    ns = MA.reference_namespace()
    ns["zip"] = _zip
    ML._exec(ML._defs(PATH, {"FreeAnchor3DHead"}), PATH, ns)
    return ns


def build_head(ns, kind):
    head = MA.build_head(dict(ns, Anchor3DHead=ns["FreeAnchor3DHead"]), kind)
    if kind == "k":
        head.anchor_generator = ns["Anchor3DRangeGenerator"](
            ranges=MA.K_RANGES, sizes=MA.SIZES, rotations=[0, 1.57], reshape_out=True)
    head.assigner_per_size = False
    head.pre_anchor_topk, head.bbox_thr, head.gamma, head.alpha = TOPK, BBOX_THR, GAMMA, ALPHA
    head.loss_bbox = SmoothL1Loss(beta=1.0 / 9.0, loss_weight=0.8)
    head.loss_dir = CrossEntropyLoss(use_sigmoid=False, loss_weight=0.2)
    return head


def sizes_of(kind):
    return [(8, 6)] if kind == "k" else [(8, 6), (4, 3)]


def ground_truth(flat, n, rs):
    """n boxes near randomly chosen anchors."""
    pick = flat[rs.randint(0, flat.shape[0], n)].copy()
    box = pick.copy()
    box[:, :2] += rs.uniform(-0.3, 0.3, (n, 2))
    box[:, 3:6] *= rs.uniform(0.9, 1.15, (n, 3))
    box[:, 6] = rs.uniform(-3.0, 3.0, n)
    if box.shape[1] > 7:
        box[:, 7:] = rs.normal(size=(n, box.shape[1] - 7))
    return box.astype(np.float32), rs.randint(0, 3, n).astype(np.int64)


def bags(ns, flat, boxes):
    """The reference's match_quality_matrix, sorted: (bag [g, k] ascending, gap between the k-th
    and the (k+1)-th IoU)."""
    ov = ns["bbox_overlaps_nearest_3d"](torch.from_numpy(boxes), flat)
    val, idx = torch.sort(ov, dim=1, descending=True, stable=True)
    return torch.sort(idx[:, :TOPK], dim=1)[0], val[:, TOPK - 1] - val[:, TOPK]


def make_case(ns, head, kind, counts, seed):
    """Inputs of one case, or None when the seed breaks a condition that can be seen before the
    loss runs (ties at the cut, overlapping bags)."""
    rs = np.random.RandomState(seed)
    sizes = sizes_of(kind)
    levels = head.anchor_generator.grid_anchors(sizes, device="cpu")
    flat = torch.cat([a.reshape(-1, head.box_code_size) for a in levels])
    code, na = head.box_code_size, head.num_anchors
    g = torch.Generator().manual_seed(seed)
    preds = ([torch.randn((2, na * 3, *s), generator=g) for s in sizes],
             [torch.randn((2, na * code, *s), generator=g) * 0.3 for s in sizes],
             [torch.randn((2, na * 2, *s), generator=g) for s in sizes])
    truth = []
    for b, n in enumerate(counts):
        boxes, labels = ground_truth(flat.numpy(), n, rs)
        truth.append((boxes, labels))
        if n == 0:
            continue
        bag, gap = bags(ns, flat, boxes)
        if float(gap.min()) <= 0 or len(set(bag.reshape(-1).tolist())) != bag.numel():
            return None
        # the regression maps hold [B, anchors * code, H, W]: write through the flattened view
        per_level = [p[b].permute(1, 2, 0).reshape(-1, code) for p in preds[1]]
        rows = torch.cat(per_level)
        for i in range(n - 1 if n > 1 else n):          # the last of several keeps random rows
            enc = ns["DeltaXYZWLHRBBoxCoder"].encode(flat[bag[i]],
                                                     torch.from_numpy(boxes[i])[None].expand(TOPK, -1))
            rows[bag[i]] = enc + torch.from_numpy(rs.normal(size=enc.shape).astype(np.float32)) * 0.05
        start = 0
        for p, lv in zip(preds[1], per_level):
            h, w = p.shape[-2:]
            p[b] = rows[start:start + lv.shape[0]].reshape(h, w, na * code).permute(2, 0, 1)
            start += lv.shape[0]
    return levels, flat, preds, truth


def run(ns, head, levels, preds, truth, dtype):
    box = ns["LiDARInstance3DBoxes"]
    code = head.box_code_size
    lv = [a.to(dtype) for a in levels]
    head.get_anchors = lambda featmap_sizes, input_metas, device="cpu": [list(lv) for _ in truth]
    seen = dict(box_prob=None, matched=[])
    cls = type(head)

    def negative(cls_prob, box_prob):
        seen["box_prob"] = box_prob.detach().clone()
        return cls.negative_bag_loss(head, cls_prob, box_prob)
    head.negative_bag_loss = negative
    topk = torch.topk

    def recording_topk(*a, **kw):
        out = topk(*a, **kw)
        seen["matched"].append(torch.sort(out[1], dim=1)[0].clone())
        return out
    leaves = [[v.clone().to(dtype).requires_grad_() for v in per_level] for per_level in preds]
    gts = [box(torch.from_numpy(b).reshape(-1, code), box_dim=code) for b, _ in truth]
    labs = [torch.from_numpy(l) for _, l in truth]
    torch.topk = recording_topk
    try:
        losses = head.loss(*leaves, gts, labs, [None] * len(truth))
    finally:
        torch.topk = topk
    (losses["positive_bag_loss"] + losses["negative_bag_loss"]).backward()
    return losses, leaves, seen


def check(ns, head, flat, preds, truth, seen):
    """What makes the reference well defined on this case."""
    code = head.box_code_size
    above = below = 0
    for b, (boxes, _) in enumerate(truth):
        deltas = torch.cat([p[b].permute(1, 2, 0).reshape(-1, code) for p in preds[1]])
        decoded = ns["DeltaXYZWLHRBBoxCoder"].decode(flat, deltas)
        rot = decoded[:, 6].double()
        normed = (rot - torch.floor(rot / np.pi + 0.5) * np.pi).abs()
        assert float((normed - np.pi / 4).abs().min()) >= 1e-3, "a rotation at the pi/4 swap"
        if boxes.shape[0] == 0:
            continue
        bag, gap = bags(ns, flat, boxes)
        assert float(gap.min()) > 0, "the k-th and (k+1)-th IoU tie"
        assert len(set(bag.reshape(-1).tolist())) == bag.numel(), "bags overlap"
        iou = ns["bbox_overlaps_nearest_3d"](torch.from_numpy(boxes), decoded)
        assert not bool((iou == np.float32(BBOX_THR)).any()), "an IoU equals t1"
        t2 = iou.max(dim=1).values
        above += int((t2 > BBOX_THR).sum())
        below += int((t2 < BBOX_THR).sum())
    assert above >= 1 and below >= 1, (above, below)
    assert float(seen["box_prob"].max()) > 0


def main():
    ns = reference_namespace()
    out = dict(topk=np.asarray(TOPK), bbox_thr=np.asarray(BBOX_THR), gamma=np.asarray(GAMMA),
               alpha=np.asarray(ALPHA))
    for kind in ("k", "n"):
        for counts in ((0, 5), (1, 5)):
            tag = "%s%d%d" % (kind, *counts)
            head = build_head(ns, kind)
            for seed in range(200):
                case = make_case(ns, head, kind, counts, seed)
                if case is None:
                    continue
                levels, flat, preds, truth = case
                l32, g32, seen32 = run(ns, head, levels, preds, truth, torch.float32)
                try:
                    check(ns, head, flat, preds, truth, seen32)
                except AssertionError:
                    continue
                break
            else:
                raise SystemExit("no seed satisfies the conditions for " + tag)
            l64, g64, seen64 = run(ns, head, levels, preds, truth, torch.float64)
            for a, b in zip(seen32["matched"], seen64["matched"]):
                assert torch.equal(a, b), tag             # the float64 run formed the same bags
            out[tag + "_seed"] = np.asarray(seed)
            for b, (boxes, labels) in enumerate(truth):
                out["%s_gt_boxes_%d" % (tag, b)], out["%s_gt_labels_%d" % (tag, b)] = boxes, labels
                out["%s_matched_%d" % (tag, b)] = seen32["matched"][b].numpy().astype(np.int64)
            for name, per_level, gr32, gr64 in zip(("cls", "bbox", "dir"), preds, g32, g64):
                for lvl, v in enumerate(per_level):
                    out["%s_pred_%s_l%d" % (tag, name, lvl)] = v.numpy().copy()
                    out["%s_grad32_%s_l%d" % (tag, name, lvl)] = gr32[lvl].grad.numpy()
                    out["%s_grad64_%s_l%d" % (tag, name, lvl)] = gr64[lvl].grad.numpy()
            for key in ("positive_bag_loss", "negative_bag_loss"):
                out["%s_%s32" % (tag, key)] = np.asarray(float(l32[key].detach()), np.float32)
                out["%s_%s64" % (tag, key)] = np.asarray(float(l64[key].detach()), np.float64)
            out[tag + "_box_prob32"] = seen32["box_prob"].numpy()
            out[tag + "_box_prob64"] = seen64["box_prob"].numpy()
            print(tag, "seed", seed, {k: (float(l32[k].detach()), float(l64[k].detach()))
                                      for k in l32},
                  "box_prob > 0:", int((seen32["box_prob"] > 0).sum()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
