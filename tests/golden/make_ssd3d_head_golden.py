#!/usr/bin/env python
"""Generates tests/golden/ssd3d_head_vectors.npz by RUNNING the reference's own code:

    AnchorFreeBBoxCoder (encode, decode, split_pred)
                                  mmdet3d/core/bbox/coders/anchor_free_bbox_coder.py
    SSD3DHead.get_targets / get_targets_single / _assign_targets_by_points_inside / loss /
    multiclass_nms_single / get_bboxes
                                  mmdet3d/models/dense_heads/ssd_3d_head.py
    LiDARInstance3DBoxes (gravity_center, dims, yaw, corners, enlarged_box, new_box, indexing,
    the origin argument)          mmdet3d/core/bbox/structures/lidar_box3d.py, base_box3d.py

mmcv / mmdet are absent: the definitions are taken from the reference FILES at run time (ast,
the machinery of make_vote_head_golden.py) and executed as they stand.  What they import from
mmcv / mmdet is written out from its published definitions: multi_apply, SmoothL1Loss,
weight_reduce_loss and ConfigDict (make_vote_head_golden.py), CrossEntropyLoss with mmdet's
binary_cross_entropy (below), and mmcv.ops `nms` / `batched_nms` -- mmcv is not installed, so
they are written out from mmcv 1.x ops/nms.py and ops/csrc/nms_cuda_kernel.cuh (offset 0, the
multiply form of the IoU test) in tests/ssd3d_ref.py and wrapped below.  points_in_boxes_gpu is
CUDA-only in the reference and is served by tests/roiaware_ref.points_in_boxes_first.  The head
is the reference's class with its attributes set by hand (its constructor would build the CUDA
set-abstraction layer); predictions are random maps split by the reference's coder.

Case: batch 3, 64 candidates out of 128 seeds, 3 classes, 12 direction bins.  Sample 0 has no
ground truth (the fake-box path); sample 1 has six boxes, the third labelled -1, with candidates
constructed inside two overlapping boxes, inside only an enlarged box, inside only the -1 box
and outside everything; sample 2 has four boxes all labelled -1 (the empty-scene branch).
main() ASSERTS these constructions.  The literals of the reference's
test_anchor_free_box_coder are read from its file (values only).  Only inputs and outputs are
stored.
"""
import ast
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
import make_vote_head_golden as MV  # noqa: E402
import roiaware_ref as RR  # noqa: E402
import ssd3d_ref as S  # noqa: E402

REF, REF_TESTS = MV.REF, MV.REF_TESTS
OUT = os.path.join(HERE, "ssd3d_head_vectors.npz")

BATCH, NUM_SEED, NUM_CANDIDATES, NUM_CLASSES, NUM_DIR_BINS, NUM_POINTS = 3, 128, 64, 3, 12, 256
TRAIN_CFG = dict(sample_mod="spec", pos_distance_thr=1.0, expand_dims_length=0.05)
TEST_CFGS = dict(
    per_class=dict(nms_cfg=dict(type="nms", iou_thr=0.1), sample_mod="spec", score_thr=0.0,
                   per_class_proposal=True, max_output_num=100),
    cut=dict(nms_cfg=dict(type="nms", iou_thr=0.1), sample_mod="spec", score_thr=0.4,
             per_class_proposal=False, max_output_num=8))
SUM = dict(type="SmoothL1Loss", reduction="sum", loss_weight=1.0)
LOSSES = dict(
    objectness_loss=dict(type="CrossEntropyLoss", use_sigmoid=True, reduction="sum",
                         loss_weight=1.0),
    center_loss=SUM, dir_class_loss=dict(type="CrossEntropyLoss", reduction="sum", loss_weight=1.0),
    dir_res_loss=SUM, size_res_loss=SUM, corner_loss=SUM, vote_loss=SUM)


class CrossEntropyLoss(nn.Module):           # mmdet 2.x cross_entropy_loss.py, both forms
    def __init__(self, use_sigmoid=False, use_mask=False, reduction="mean", class_weight=None,
                 loss_weight=1.0):
        super().__init__()
        assert not use_mask
        self.use_sigmoid, self.reduction = use_sigmoid, reduction
        self.class_weight, self.loss_weight = class_weight, loss_weight

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None):
        reduction = reduction_override if reduction_override else self.reduction
        class_weight = None if self.class_weight is None else \
            cls_score.new_tensor(self.class_weight)
        if weight is not None:
            weight = weight.float()
        if self.use_sigmoid:                 # binary_cross_entropy
            assert cls_score.dim() == label.dim()
            loss = F.binary_cross_entropy_with_logits(cls_score, label.float(),
                                                      pos_weight=class_weight, reduction="none")
        else:
            loss = F.cross_entropy(cls_score, label, weight=class_weight, reduction="none")
        return self.loss_weight * MV.weight_reduce_loss(loss, weight, reduction, avg_factor)


def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """mmcv.ops.batched_nms -> (dets [K, 5], keep)."""
    cfg = dict(nms_cfg)
    assert cfg.pop("type", "nms") == "nms" and not cfg.pop("class_agnostic", class_agnostic)
    keep = torch.from_numpy(S.mmcv_batched_nms(boxes.numpy(), scores.numpy(), idxs.numpy(),
                                               cfg["iou_thr"]))
    return torch.cat([boxes[keep], scores[keep][:, None]], -1), keep


def points_in_boxes_gpu(points, boxes):
    """ops/roiaware_pool3d points_in_boxes_gpu: [B, M, 3], [B, T, 7] -> int32 [B, M]."""
    return torch.from_numpy(RR.points_in_boxes_first(points.detach().numpy(),
                                                     boxes.detach().numpy()))


def reference_namespace():
    from abc import abstractmethod
    reg = MV._Registry()
    ns = {"torch": torch, "nn": nn, "F": F, "np": np, "HEADS": reg, "BBOX_CODERS": reg,
          "BaseBBoxCoder": object, "force_fp32": lambda **kw: (lambda f: f),
          "multi_apply": MV.multi_apply, "abstractmethod": abstractmethod, "BasePoints": None,
          "iou3d_cuda": None, "points_in_boxes_gpu": points_in_boxes_gpu,
          "points_in_boxes_batch": None, "batched_nms": batched_nms, "build_sa_module": None,
          "furthest_point_sample": None, "build_bbox_coder": None, "VoteModule": None,
          "BaseConvBboxHead": None, "aligned_3d_nms": None, "chamfer_distance": None}
    losses = {"CrossEntropyLoss": CrossEntropyLoss, "SmoothL1Loss": MV.SmoothL1Loss}
    ns["build_loss"] = lambda cfg: losses[cfg["type"]](
        **{k: v for k, v in cfg.items() if k != "type"})
    for path, names in (
            ("core/bbox/coders/partial_bin_based_bbox_coder.py", {"PartialBinBasedBBoxCoder"}),
            ("core/bbox/coders/anchor_free_bbox_coder.py", {"AnchorFreeBBoxCoder"}),
            ("core/bbox/structures/utils.py", {"limit_period", "rotation_3d_in_axis"}),
            ("core/bbox/structures/base_box3d.py", {"BaseInstance3DBoxes"}),
            ("core/bbox/structures/lidar_box3d.py", {"LiDARInstance3DBoxes"}),
            ("core/bbox/structures/depth_box3d.py", {"DepthInstance3DBoxes"}),
            ("models/dense_heads/vote_head.py", {"VoteHead"}),
            ("models/dense_heads/ssd_3d_head.py", {"SSD3DHead"})):
        MV._exec(MV._defs(REF + path, names), REF + path, ns)
    return ns


def coder_test_literals():
    """The tensors of the reference's test_anchor_free_box_coder, evaluated from its file."""
    path = REF_TESTS + "test_utils/test_bbox_coders.py"
    fn = MV._defs(path, {"test_anchor_free_box_coder"})[0]
    want = ["gt_bboxes", "gt_labels", "expected_center_target", "expected_size_targets",
            "expected_dir_class_target", "expected_dir_res_target", "center", "size_res",
            "dir_class", "dir_res", "expected_bbox3d"]
    out = {}
    for node in fn.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and \
                isinstance(node.targets[0], ast.Name) and node.targets[0].id in want and \
                node.targets[0].id not in out:
            value = node.value.args[0] if node.targets[0].id == "gt_bboxes" else node.value
            expr = ast.fix_missing_locations(ast.Expression(value))
            got = eval(compile(expr, path, "eval"), {"torch": torch})
            out[node.targets[0].id] = torch.as_tensor(got, dtype=None if torch.is_tensor(got)
                                                      else torch.float32)
    assert sorted(out) == sorted(want), sorted(out)
    return out


def build_head(ns):
    head = ns["SSD3DHead"].__new__(ns["SSD3DHead"])
    nn.Module.__init__(head)
    head.num_classes = NUM_CLASSES
    head.train_cfg = MV.ConfigDict(TRAIN_CFG)
    head.test_cfg = MV.ConfigDict(TEST_CFGS["per_class"])
    head.num_candidates = NUM_CANDIDATES
    for name, cfg in LOSSES.items():
        setattr(head, name, ns["build_loss"](cfg))
    head.bbox_coder = ns["AnchorFreeBBoxCoder"](num_dir_bins=NUM_DIR_BINS, with_rot=True)
    head.num_dir_bins = NUM_DIR_BINS
    return head


def scene():
    """-> boxes (list of [T, 7]), labels (list of [T])."""
    half_pi = float(np.float32(-np.pi / 2))
    boxes1 = np.asarray([[10.0, 2.0, -1.0, 1.6, 3.9, 1.5, 0.3],
                         [10.5, 2.5, -1.0, 1.7, 4.2, 1.6, 0.5],
                         [20.0, -5.0, -1.0, 1.6, 3.9, 1.5, 1.0],
                         [30.0, 8.0, -0.8, 0.6, 0.8, 1.7, -1.2],
                         [25.0, -10.0, -1.2, 1.8, 4.5, 1.9, 7.0],
                         [40.0, 0.0, -1.0, 1.6, 3.9, 1.5, half_pi]], np.float32)
    labels1 = np.asarray([0, 1, -1, 2, 0, 1], np.int64)
    boxes2 = np.asarray([[12.0, 1.0, -1.0, 1.6, 3.9, 1.5, 0.2],
                         [22.0, 3.0, -1.0, 1.7, 4.0, 1.6, -0.4],
                         [32.0, -4.0, -1.0, 1.6, 3.7, 1.4, 2.0],
                         [18.0, -8.0, -1.0, 0.7, 0.9, 1.8, 0.0]], np.float32)
    labels2 = np.full((4,), -1, np.int64)
    return ([np.zeros((0, 7), np.float32), boxes1, boxes2],
            [np.zeros((0,), np.int64), labels1, labels2])


def candidates(rs, boxes):
    """aggregated [3, 64, 3] and seed points [3, 128, 3]: jittered about the boxes of samples 1
    and 2 (sample 0 reuses sample 1's), then the constructed ones of sample 1."""
    agg = np.empty((BATCH, NUM_CANDIDATES, 3), np.float32)
    for b in range(BATCH):
        src = boxes[b] if len(boxes[b]) else boxes[1]
        pick = src[rs.randint(0, len(src), NUM_CANDIDATES)]
        agg[b, :, :2] = pick[:, :2] + rs.uniform(-2.5, 2.5, (NUM_CANDIDATES, 2))
        agg[b, :, 2] = pick[:, 2] + rs.uniform(-0.3, 2.0, NUM_CANDIDATES)
    agg[1, 0] = [10.2, 2.2, -0.3]          # in boxes 0 and 1: the first wins; positive
    agg[1, 1] = [41.98, 0.0, -0.3]         # 0.03 past box 5's end: only its enlarged box
    agg[1, 2] = [60.0, 30.0, 0.0]          # outside everything
    agg[1, 3] = [20.0, -5.0, -0.3]         # in box 2 only, whose label is -1: outside
    agg[1, 4] = [25.0, -10.0, 0.1]         # box 4 (yaw beyond 2 pi)
    agg[1, 5] = [30.0, 8.0, 0.0]           # box 3, positive
    agg[1, 6] = [10.0, 2.0, -0.9]          # box 0, too far below the top centre: not positive
    seeds = np.concatenate(
        [agg + rs.normal(0, 0.3, agg.shape), rs.uniform(-5, 45, (BATCH, NUM_SEED - NUM_CANDIDATES, 3))],
        1).astype(np.float32)
    seeds[1, :4] = agg[1, :4]
    return agg, seeds


def _np(t):
    return t.detach().cpu().numpy()


def main():
    torch.manual_seed(0)
    rs = np.random.RandomState(0)
    ns = reference_namespace()
    LiDAR = ns["LiDARInstance3DBoxes"]
    out = {}

    # ---- coder: the reference test's literals through the reference
    coder = ns["AnchorFreeBBoxCoder"](num_dir_bins=NUM_DIR_BINS, with_rot=True)
    lit = coder_test_literals()
    enc = coder.encode(LiDAR(lit["gt_bboxes"].clone()), lit["gt_labels"].long())
    assert torch.allclose(enc[0], lit["expected_center_target"], atol=1e-4)
    assert torch.allclose(enc[1], lit["expected_size_targets"], atol=1e-4)
    assert torch.all(enc[2] == lit["expected_dir_class_target"])
    assert torch.allclose(enc[3], lit["expected_dir_res_target"], atol=1e-3)
    decoded = coder.decode(dict(center=lit["center"].clone(), size=lit["size_res"].clone(),
                                dir_class=lit["dir_class"].clone(), dir_res=lit["dir_res"].clone()))
    assert torch.allclose(decoded, lit["expected_bbox3d"], atol=1e-4)
    for k, v in lit.items():
        out["coder_lit_" + k] = _np(v)
    for k, v in zip(("center", "size", "dir_class", "dir_res"), enc):
        out["coder_lit_encode_" + k] = _np(v)
    out["coder_lit_decoded"] = _np(decoded)

    # ---- boxes structure
    boxes_np, labels_np = scene()
    gt1 = LiDAR(torch.from_numpy(boxes_np[1]))
    out["gt_boxes_1"], out["gt_labels_1"] = boxes_np[1], labels_np[1]
    out["gt_boxes_2"], out["gt_labels_2"] = boxes_np[2], labels_np[2]
    out["box_gravity_center"] = _np(gt1.gravity_center)
    out["box_dims"], out["box_yaw"] = _np(gt1.dims), _np(gt1.yaw)
    out["box_corners"] = _np(gt1.corners)
    out["box_enlarged"] = _np(gt1.enlarged_box(0.05).tensor)
    out["box_from_gravity_origin"] = _np(LiDAR(torch.from_numpy(boxes_np[1]),
                                               origin=(0.5, 0.5, 0.5)).tensor)
    out["box_from_top_origin"] = _np(LiDAR(torch.from_numpy(boxes_np[1]),
                                           origin=(0.5, 0.5, 1.0)).tensor)
    pick = torch.from_numpy(labels_np[1] != -1)
    out["box_getitem_mask"] = _np(gt1[pick].tensor)
    out["box_new_box"] = _np(gt1.new_box(torch.zeros(1, 7)).tensor)
    enc = coder.encode(gt1, torch.from_numpy(labels_np[1]))
    for k, v in zip(("center", "size", "dir_class", "dir_res"), enc):
        out["encode_" + k] = _np(v)

    # ---- candidates, seeds and the constructions
    agg_np, seeds_np = candidates(rs, boxes_np)
    out["aggregated_points"], out["seed_points"] = agg_np, seeds_np
    first = _np(gt1.points_in_boxes(torch.from_numpy(agg_np[1])))
    out["points_in_boxes_1"] = first.astype(np.int32)
    all_hits = RR.points_in_boxes_all(agg_np[1][None], boxes_np[1][None])[0]
    big = gt1.enlarged_box(0.05)
    big.tensor[:, 2] -= 0.05
    in_big = RR.points_in_boxes_all(agg_np[1][None], _np(big.tensor)[None])[0]
    assert all_hits[0].tolist() == [1, 1, 0, 0, 0, 0] and first[0] == 0
    assert all_hits[1].sum() == 0 and in_big[1].tolist() == [0, 0, 0, 0, 0, 1]
    assert all_hits[2].sum() == 0 and in_big[2].sum() == 0
    assert all_hits[3].tolist() == [0, 0, 1, 0, 0, 0]
    assert first[4] == 4 and first[5] == 3 and first[6] == 0

    # ---- predictions: random maps through the reference coder's split
    head = build_head(ns)
    aggregated = torch.from_numpy(agg_np)
    seed_points = torch.from_numpy(seeds_np)
    cls_preds = torch.randn(BATCH, NUM_CLASSES, NUM_CANDIDATES)
    reg_preds = torch.randn(BATCH, 6 + 2 * NUM_DIR_BINS, NUM_CANDIDATES) * 0.5
    vote_offset = torch.randn(BATCH, 3, NUM_CANDIDATES) * 0.5
    out.update(cls_preds=_np(cls_preds), reg_preds=_np(reg_preds), vote_offset=_np(vote_offset))
    bbox_preds = dict(seed_points=seed_points, aggregated_points=aggregated,
                      vote_offset=vote_offset)
    bbox_preds.update(head.bbox_coder.split_pred(cls_preds, reg_preds, aggregated))
    for k in ("obj_scores", "center_offset", "center", "size", "dir_class", "dir_res_norm",
              "dir_res"):
        out["split_" + k] = _np(bbox_preds[k])

    # ---- targets and losses
    gt_boxes = [LiDAR(torch.from_numpy(b)) for b in boxes_np]
    gt_labels = [torch.from_numpy(v) for v in labels_np]
    points = [torch.from_numpy(rs.uniform(-5, 45, (NUM_POINTS, 4)).astype(np.float32))
              for _ in range(BATCH)]
    out["points"] = np.stack([_np(p) for p in points])
    targets = head.get_targets(points, list(gt_boxes), list(gt_labels), None, None, bbox_preds)
    assert len(targets) == len(S.ALL_TARGET_NAMES)
    for k, v in zip(S.ALL_TARGET_NAMES, targets):
        out["targets_" + k] = _np(v)
        assert np.isfinite(out["targets_" + k].astype(np.float64)).all(), k
    t = dict(zip(S.ALL_TARGET_NAMES, targets))
    pos, neg, vmask = t["positive_mask"], t["negative_mask"], t["vote_mask"] > 0
    assert not pos[0].any() and neg[0].all() and not vmask[0].any()         # the fake box
    assert not pos[2].any() and neg[2].all() and (t["corner3d_targets"][2] == 0).all()
    assert pos[1, :7].tolist() == [True, False, False, False, True, True, False]
    assert neg[1, :7].tolist() == [False, True, True, True, False, False, False]
    assert vmask[1, :4].tolist() == [True, True, False, False]
    assert t["mask_targets"][1, :7].tolist() == [0, 1, 1, 1, 0, 2, 0]       # fallback: box 5
    for b in range(BATCH):
        boxes_b = gt_boxes[b].tensor if len(gt_labels[b]) else torch.zeros(1, 7)
        labels_b = gt_labels[b] if len(gt_labels[b]) else torch.zeros(1, dtype=torch.long)
        assert S.distance_margin(boxes_b, labels_b, aggregated[b], 1.0) > 1e-4
    # the restatement in float32 is the reference: every output equal
    own = S.targets([torch.from_numpy(b) for b in boxes_np], gt_labels, aggregated, seed_points,
                    NUM_CANDIDATES, NUM_CLASSES, NUM_DIR_BINS, 1.0, 0.05)
    for k, a, b in zip(S.ALL_TARGET_NAMES, own, targets):
        assert torch.equal(a.float(), b.float()), k
    metas = [dict(box_type_3d=LiDAR)] * BATCH
    losses = head.loss(bbox_preds, points, list(gt_boxes), list(gt_labels), img_metas=metas)
    for k, v in losses.items():
        assert torch.isfinite(v) and v >= 0, k
        out["loss_" + k] = _np(v)

    # ---- boxes
    points_cat = torch.stack(points)
    preds = {k: v.detach().clone() for k, v in bbox_preds.items()}
    preds["center"][0, 7] = torch.tensor([200.0, 200.0, 50.0])       # far from every point
    preds["obj_scores"][0, :, 7] = 6.0
    out["boxes_in_center"], out["boxes_in_obj_scores"] = _np(preds["center"]), _np(preds["obj_scores"])
    out["boxes_decoded"] = _np(head.bbox_coder.decode(preds))
    for tag, cfg in TEST_CFGS.items():
        head.test_cfg = MV.ConfigDict(cfg)
        results = head.get_bboxes(points_cat, preds, metas)
        for b, (box, score, label) in enumerate(results):
            out["boxes_%s_%d_tensor" % (tag, b)] = _np(box.tensor)
            out["boxes_%s_%d_scores" % (tag, b)] = _np(score)
            out["boxes_%s_%d_labels" % (tag, b)] = _np(label)
    kept = [out["boxes_per_class_%d_tensor" % b].shape[0] // NUM_CLASSES for b in range(BATCH)]
    assert all(1 <= k < NUM_CANDIDATES for k in kept), kept
    assert all(out["boxes_cut_%d_tensor" % b].shape[0] <= 8 for b in range(BATCH))
    far = LiDAR(torch.from_numpy(out["boxes_decoded"][0, 7:8]), origin=(0.5, 0.5, 1.0))
    assert (far.points_in_boxes(points[0][:, :3]) == -1).all()        # it holds no point ...
    assert (torch.from_numpy(out["boxes_per_class_0_tensor"]) == far.tensor[0]).all(1).any()
    print("kept boxes per sample:", kept,
          [out["boxes_cut_%d_tensor" % b].shape[0] for b in range(BATCH)])

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "(%d arrays, %d bytes)" % (len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
