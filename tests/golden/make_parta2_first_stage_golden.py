#!/usr/bin/env python
"""Generates tests/golden/parta2_first_stage_vectors.npz by RUNNING the reference's own code on
the CPU:

    PointwiseSemanticHead (constructor, forward, get_targets, get_targets_single, loss)
                                  mmdet3d/models/roi_heads/mask_heads/pointwise_semantic_head.py
    PartA2RPNHead (loss, get_bboxes_single, class_agnostic_nms) on Anchor3DHead.get_bboxes
                                  mmdet3d/models/dense_heads/parta2_rpn_head.py, anchor3d_head.py
    LiDARInstance3DBoxes, rotation_3d_in_axis, limit_period, xywhr2xyxyr, the anchor generator,
    the coder and the assigner machinery as make_anchor_head_golden.py takes them

mmcv / mmdet are absent: the definitions are taken from the reference FILES at run time (ast,
the machinery of make_head_loss_golden.py / make_anchor_head_golden.py) and executed as they
stand.  What they import from mmdet is written out there from its published definitions
(FocalLoss's python branch, CrossEntropyLoss with binary_cross_entropy, multi_apply, ...).  The
CUDA-only ops are served as make_ssd3d_head_golden.py serves them: points_in_boxes_gpu by
tests/roiaware_ref.points_in_boxes_first, nms_gpu / nms_normal_gpu by tests/iou3d_ref.py on a
stable descending order.  Only stubs, inputs and recorded outputs are here.

Semantic head cases (16 input channels, 3 classes, extra_width 0.2):
  b2     two samples with 5 and 7 boxes, 150 and 170 voxels
  b1     one sample with 6 boxes, 130 voxels
  empty  two samples, the FIRST without ground truth
  nopos  two samples whose voxels all lie far from every box: no positive row
For each: weights, forward outputs, get_targets (float32), get_targets_single per sample with
float64 centres and boxes, the two loss terms and the parameter gradients in float32 and float64.
main() ASSERTS the margins (tests/parta2_cases.assert_margins): every centre is at least 1e-3
from every face of every box and enlarged box, so the discrete targets are well defined.

RPN head (an 8 x 6 map, 3 sizes x 2 rotations = 288 anchors, batch 2, three assigners): weights,
the maps its forward gives, loss, and get_bboxes under
  train  normal NMS, nms_pre 100 < 288 (the top-k branch), nms_post 12 < the survivors (the
         final sort)
  test   rotate NMS, score_thr 0.9 removing some candidates
  quirk  nms_pre 1000 > 288: the carried cls_preds are the raw logits
  none   the second sample's class maps lowered by 30: nothing passes score_thr there
main() ASSERTS that all candidate scores are pairwise distinct and none within 1e-6 of
score_thr, and that no pair IoU lies within 1e-4 of nms_thr.
"""
import inspect
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import iou3d_ref as IR  # noqa: E402
import make_anchor_head_golden as MA  # noqa: E402
import make_ssd3d_head_golden as MS  # noqa: E402
import parta2_cases as PC  # noqa: E402
import roiaware_ref as RR  # noqa: E402

ML = MA.ML
REF = ML.REF
OUT = os.path.join(HERE, "parta2_first_stage_vectors.npz")
IN_CHANNELS, NUM_CLASSES = 16, 3
SEM_CASES = dict(b2=dict(seed=11, counts=(5, 7), rows=(150, 170)),
                 b1=dict(seed=12, counts=(6,), rows=(130,)),
                 empty=dict(seed=13, counts=(0, 6), rows=(90, 110)),
                 nopos=dict(seed=14, counts=(4, 3), rows=(80, 70)))
RPN_CFGS, RPN_FEAT, RPN_MAP = PC.RPN_CFGS, PC.RPN_FEAT, PC.RPN_MAP
assert (MA.SIZES, MA.K_RANGES, MA.K_THR, MA.DIR_OFFSET) == (PC.RPN_SIZES, PC.RPN_RANGES, PC.RPN_THR,
                                                            PC.RPN_DIR_OFFSET)


def points_in_boxes_gpu(points, boxes):
    """ops/roiaware_pool3d points_in_boxes_gpu: [B, M, 3], [B, T, 7] -> int32 [B, M]."""
    if boxes.shape[1] == 0 or points.shape[1] == 0:
        return torch.full(points.shape[:2], -1, dtype=torch.int32)
    return torch.from_numpy(RR.points_in_boxes_first(
        points.detach().float().numpy(), boxes.detach().float().numpy()))


def reference_namespace():
    ns = MA.reference_namespace()
    losses = {"FocalLoss": ML.FocalLoss, "CrossEntropyLoss": MS.CrossEntropyLoss}
    ns.update(torch=torch, nn=nn, F=F, np=np, points_in_boxes_gpu=points_in_boxes_gpu,
              force_fp32=lambda **kw: (lambda f: f), multi_apply=ML.multi_apply)
    ns["build_loss"] = lambda cfg: losses[cfg["type"]](
        **{k: v for k, v in cfg.items() if k != "type"})
    for path, names in (
            ("models/roi_heads/mask_heads/pointwise_semantic_head.py", {"PointwiseSemanticHead"}),
            ("models/dense_heads/parta2_rpn_head.py", {"PartA2RPNHead"})):
        ML._exec(ML._defs(REF + path, names), REF + path, ns)
    return ns


def _np(t):
    return t.detach().cpu().numpy()


# --------------------------------------------------------------------------- semantic head
def semantic_case(tag, spec):
    case = PC.make_case(spec["seed"], spec["counts"], spec["rows"], NUM_CLASSES)
    if tag == "nopos":
        case["centres"] = (case["centres"] + np.asarray([0, 0, 300.0], np.float32))
        PC.assert_margins(case["centres"], case["ids"], case["boxes"])
    return case


def run_semantic(ns, out):
    LiDAR = ns["LiDARInstance3DBoxes"]

    class Double(LiDAR):
        """The reference's boxes holding float64: its constructor (and with it .to and
        .enlarged_box) casts to float32, which a float64 run of get_targets_single must not."""

        def __init__(self, tensor, box_dim=7, with_yaw=True, origin=(0.5, 0.5, 0)):
            super().__init__(tensor, box_dim=box_dim, with_yaw=with_yaw, origin=origin)
            self.tensor = torch.as_tensor(tensor).double().reshape(-1, box_dim)

        def to(self, device):
            return self

    class Wide(torch.Tensor):
        """Float64 centres whose new_zeros keeps float64: the reference allocates part_targets
        as float32 by name (:97-98), and torch refuses the float64 masked write into it."""

        def new_zeros(self, size, dtype=None, **kw):
            return torch.zeros(size, dtype=torch.float64)

    torch.manual_seed(3)
    head = ns["PointwiseSemanticHead"](in_channels=IN_CHANNELS, num_classes=NUM_CLASSES)
    nn.init.normal_(head.seg_cls_layer.weight, 0, 0.5)
    nn.init.normal_(head.seg_reg_layer.weight, 0, 0.5)
    out["sem_state_keys"] = np.asarray(list(head.state_dict().keys()))
    for k, v in head.state_dict().items():
        out["sem_weight_" + k] = _np(v)
    for attr in ("extra_width", "num_classes", "seg_score_thr"):
        out["sem_default_" + attr] = np.asarray(getattr(
            ns["PointwiseSemanticHead"](in_channels=IN_CHANNELS), attr))
    head64 = ns["PointwiseSemanticHead"](in_channels=IN_CHANNELS, num_classes=NUM_CLASSES).double()
    head64.load_state_dict({k: v.double() for k, v in head.state_dict().items()})
    rs = np.random.RandomState(5)
    for tag, spec in SEM_CASES.items():
        case = semantic_case(tag, spec)
        n = case["centres"].shape[0]
        x = rs.normal(size=(n, IN_CHANNELS)).astype(np.float32)
        p = "sem_%s_" % tag
        out[p + "centres"], out[p + "ids"], out[p + "x"] = case["centres"], case["ids"], x
        for b, (bx, lb) in enumerate(zip(case["boxes"], case["labels"])):
            out[p + "boxes_%d" % b], out[p + "labels_%d" % b] = bx, lb
        coors = np.zeros((n, 4), np.int64)
        coors[:, 0] = case["ids"]
        voxels_dict = dict(coors=torch.from_numpy(coors),
                           voxel_centers=torch.from_numpy(case["centres"]))
        boxes = [LiDAR(torch.from_numpy(b).reshape(-1, 7)) for b in case["boxes"]]
        labels = [torch.from_numpy(l) for l in case["labels"]]
        targets = head.get_targets(voxels_dict, list(boxes), list(labels))
        out[p + "seg_targets"] = _np(targets["seg_targets"])
        out[p + "part_targets"] = _np(targets["part_targets"])
        seg_own, part_own = PC.batch_targets_ref(case["centres"], case["ids"], case["boxes"],
                                                 case["labels"], NUM_CLASSES)
        assert np.array_equal(seg_own, out[p + "seg_targets"]), tag      # ids do not decrease
        assert np.abs(part_own - out[p + "part_targets"]).max() < 1e-5, tag
        pos = (out[p + "seg_targets"] > -1) & (out[p + "seg_targets"] < NUM_CLASSES)
        if tag == "nopos":
            assert not pos.any()
        else:
            assert pos.sum() >= 10 and (out[p + "seg_targets"] == -1).sum() >= 5, tag
            assert (out[p + "seg_targets"] == NUM_CLASSES).sum() >= 5, tag
        # get_targets_single in float64: centres and boxes as doubles of the same numbers
        for b in range(len(boxes)):
            gt = Double(torch.from_numpy(case["boxes"][b]).reshape(-1, 7))
            rows = torch.from_numpy(case["centres"][case["ids"] == b]).double().as_subclass(Wide)
            seg64, part64 = head.get_targets_single(rows, gt, labels[b])
            assert part64.dtype == torch.float64
            out[p + "single64_seg_%d" % b] = _np(seg64.as_subclass(torch.Tensor))
            out[p + "single64_part_%d" % b] = _np(part64.as_subclass(torch.Tensor))
        for dtype, h, sfx in ((torch.float32, head, ""), (torch.float64, head64, "64")):
            h.zero_grad()
            res = h(torch.from_numpy(x).to(dtype))
            for k, v in res.items():
                out[p + "fwd" + sfx + "_" + k] = _np(v)
            tg = dict(seg_targets=targets["seg_targets"],
                      part_targets=targets["part_targets"].to(dtype))
            losses = h.loss(res, tg)
            total = losses["loss_seg"] + losses["loss_part"]
            if total.requires_grad:
                total.backward()
            for k, v in losses.items():
                assert torch.isfinite(v), (tag, k)
                out[p + k + sfx] = _np(v)
            for k, prm in h.named_parameters():
                g = prm.grad if prm.grad is not None else torch.zeros_like(prm)
                out[p + "grad" + sfx + "_" + k] = _np(g)
        if tag == "nopos":
            assert float(out[p + "loss_part"]) == 0.0
        print(tag, "rows", n, "pos", int(pos.sum()), "ignored",
              int((out[p + "seg_targets"] == -1).sum()),
              {k: float(out[p + k]) for k in ("loss_seg", "loss_part")})


# ---------------------------------------------------------------------------------- RPN head
def build_rpn_head(ns):
    head = MA.build_head(ns, "k", per_class=True)
    head.__class__ = ns["PartA2RPNHead"]
    head.feat_channels, head.in_channels = RPN_FEAT, RPN_FEAT
    head._init_layers()
    return head


def assert_rpn_margins(head, cls_scores, bbox_preds, cfg, tag):
    """The candidates of every sample under cfg: scores pairwise distinct, none within 1e-6 of
    score_thr; no pair IoU (of the candidates above score_thr) within 1e-4 of nms_thr."""
    code, C = head.box_code_size, head.num_classes
    (anchors,) = head.anchor_generator.grid_anchors([RPN_MAP], device="cpu")
    anchors = anchors.reshape(-1, code)
    for i in range(cls_scores[0].shape[0]):
        scores = cls_scores[0][i].permute(1, 2, 0).reshape(-1, C).sigmoid().max(1)[0]
        reg = bbox_preds[0][i].permute(1, 2, 0).reshape(-1, code)
        anc = anchors
        if scores.shape[0] > cfg["nms_pre"]:
            scores, inds = scores.topk(cfg["nms_pre"])
            anc, reg = anc[inds], reg[inds]
        s = np.sort(scores.double().numpy())
        assert (np.diff(s) > 0).all(), tag
        assert np.abs(s - cfg["score_thr"]).min() > 1e-6, tag
        boxes = head.bbox_coder.decode(anc, reg)[scores > cfg["score_thr"]]
        if boxes.shape[0] < 2:
            continue
        from msmdfusion_amd.anchor_head import xywhr2xyxyr
        xyxyr = xywhr2xyxyr(boxes[:, [0, 1, 3, 4, 6]]).numpy()
        iou = IR.iou_bev(xyxyr, xyxyr, np.float64) if cfg["use_rotate_nms"] else \
            IR.iou_normal(xyxyr[:, :4], xyxyr[:, :4]).astype(np.float64)
        iou = iou[~np.eye(iou.shape[0], dtype=bool)]
        assert np.abs(iou - cfg["nms_thr"]).min() > 1e-4, tag


def run_rpn(ns, out):
    LiDAR = ns["LiDARInstance3DBoxes"]
    torch.manual_seed(7)
    head = build_rpn_head(ns)
    nn.init.normal_(head.conv_cls.weight, 0, 0.25)
    nn.init.normal_(head.conv_reg.weight, 0, 0.05)
    nn.init.normal_(head.conv_dir_cls.weight, 0, 0.25)
    out["rpn_state_keys"] = np.asarray(list(head.state_dict().keys()))
    for k, v in head.state_dict().items():
        out["rpn_weight_" + k] = _np(v)
    feats = torch.randn(2, RPN_FEAT, *RPN_MAP)
    out["rpn_feats"] = _np(feats)
    (ak,) = head.anchor_generator.grid_anchors([RPN_MAP], device="cpu")
    seven, seven_l = MA.kitti_seven(ak)
    one, one_l = np.asarray([[8.3, 1.0, -1.7, 1.7, 4.0, 1.5, -1.2]], np.float32), np.asarray([2])
    gts = [(seven, seven_l.astype(np.int64)), (one, one_l.astype(np.int64))]
    for b, (bx, lb) in enumerate(gts):
        out["rpn_gt_boxes_%d" % b], out["rpn_gt_labels_%d" % b] = bx, lb

    def forward(h, x):
        return tuple([t] for t in h.forward_single(x))

    for dtype, sfx in ((torch.float32, ""), (torch.float64, "64")):
        h = head.double() if sfx else head
        h.zero_grad()
        preds = forward(h, feats.to(dtype))
        if not sfx:
            for name, per_level in zip(("cls", "bbox", "dir"), preds):
                out["rpn_pred_" + name] = _np(per_level[0])
        losses = h.loss(*preds, [LiDAR(torch.from_numpy(b).to(dtype)) for b, _ in gts],
                        [torch.from_numpy(l) for _, l in gts], [None, None])
        assert sorted(losses) == ["loss_rpn_bbox", "loss_rpn_cls", "loss_rpn_dir"]
        sum(sum(v) for v in losses.values()).backward()
        for k, per_level in losses.items():
            out["rpn_" + k + sfx] = np.asarray([float(v.detach()) for v in per_level], np.float64)
        for k, prm in h.named_parameters():
            out["rpn_grad" + sfx + "_" + k] = _np(prm.grad)
    head.float()

    metas = [dict(box_type_3d=LiDAR)] * 2
    with torch.no_grad():
        base = [[t.clone()] for t in (torch.from_numpy(out["rpn_pred_cls"]),
                                      torch.from_numpy(out["rpn_pred_bbox"]),
                                      torch.from_numpy(out["rpn_pred_dir"]))]
        for tag, cfg in RPN_CFGS.items():
            preds = [[t.clone() for t in per_level] for per_level in base]
            if tag == "none":
                preds[0][0][1] -= 30.0
            assert_rpn_margins(head, preds[0], preds[1], cfg, tag)
            for dtype, sfx in ((torch.float32, ""), (torch.float64, "64")):
                rets = head.get_bboxes(*[[t.to(dtype) for t in per_level] for per_level in preds],
                                       metas, ML.ConfigDict(cfg))
                for i, r in enumerate(rets):
                    p = "rpn_%s_s%d%s_" % (tag, i, sfx)
                    out[p + "boxes_3d"] = _np(r["boxes_3d"].tensor)
                    for k in ("scores_3d", "labels_3d", "cls_preds"):
                        out[p + k] = _np(r[k])
            kept = [out["rpn_%s_s%d_scores_3d" % (tag, i)].shape[0] for i in range(2)]
            for i in range(2):                   # the float64 run made the same selection
                a, b = out["rpn_%s_s%d_labels_3d" % (tag, i)], \
                    out["rpn_%s_s%d64_labels_3d" % (tag, i)]
                assert a.shape == b.shape and np.array_equal(a, b), (tag, i)
            print(tag, "kept", kept)
            if tag == "train":
                assert kept == [12, 12]
                full = head.get_bboxes(*preds, metas, ML.ConfigDict(dict(cfg, nms_post=10 ** 6)))
                assert all(r["scores_3d"].shape[0] > 12 for r in full)
            if tag == "test":
                passed = [(torch.from_numpy(out["rpn_pred_cls"])[i].permute(1, 2, 0).reshape(-1, 3)
                           .sigmoid().max(1)[0].topk(100)[0] > cfg["score_thr"]).sum() for i in range(2)]
                assert all(0 < int(p) < 100 for p in passed) and all(k > 0 for k in kept)
            if tag == "quirk":
                c = out["rpn_quirk_s0_cls_preds"]
                assert c.min() < 0 and np.allclose(                 # raw logits, not sigmoids
                    1 / (1 + np.exp(-c.max(1).astype(np.float64))), out["rpn_quirk_s0_scores_3d"],
                    atol=1e-6)
            if tag == "none":
                assert kept[0] > 0 and kept[1] == 0
                assert out["rpn_none_s1_labels_3d"].dtype == np.float32
                assert out["rpn_none_s1_cls_preds"].shape == (0, 3)


def signature_defaults(cls):
    """The constructor's arguments and defaults as JSON (a required argument: "<required>")."""
    params = list(inspect.signature(cls.__init__).parameters.values())[1:]
    return json.dumps([[q.name, "<required>" if q.default is inspect.Parameter.empty
                        else q.default] for q in params])


def main():
    ns = reference_namespace()
    out = {}
    out["sem_signature"] = np.asarray(signature_defaults(ns["PointwiseSemanticHead"]))
    out["rpn_signature"] = np.asarray(signature_defaults(ns["PartA2RPNHead"]))
    run_semantic(ns, out)
    run_rpn(ns, out)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "(%d arrays, %d bytes)" % (len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
