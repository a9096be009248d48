#!/usr/bin/env python
"""Generates tests/golden/vote_head_vectors.npz by RUNNING the reference's own code:

    chamfer_distance, ChamferDistance     mmdet3d/models/losses/chamfer_distance.py
    PartialBinBasedBBoxCoder              mmdet3d/core/bbox/coders/partial_bin_based_bbox_coder.py
    VoteModule (forward, get_loss)        mmdet3d/models/model_utils/vote_module.py
    BaseConvBboxHead                      mmdet3d/models/dense_heads/base_conv_bbox_head.py
    VoteHead.get_targets / get_targets_single / loss / multiclass_nms_single / get_bboxes
                                          mmdet3d/models/dense_heads/vote_head.py
    aligned_3d_nms                        mmdet3d/core/post_processing/box3d_nms.py:91-138
    DepthInstance3DBoxes (gravity_center, corners, points_in_boxes' conversion), Box3DMode
                                          mmdet3d/core/bbox/structures/*.py

mmcv / mmdet are absent: the definitions are taken from the reference FILES at run time (ast)
and executed as they stand (function-local relative imports are dropped: the names are in the
namespace already).  What they import from mmcv / mmdet 2.x is written out below from its
published definitions: ConvModule, build_conv_layer, is_tuple_of, CrossEntropyLoss (softmax form
with class_weight), SmoothL1Loss, weight_reduce_loss, multi_apply, ConfigDict.
points_in_boxes_batch is CUDA-only in the reference and is served by
tests/roiaware_ref.py, the oracle of the roiaware tests.  The head is the reference's class with
its attributes set by hand (its constructor would build the CUDA set-abstraction layer).

Case: batch 2, 256 input points, 32 seeds, 16 proposals, 10 size classes, 12 direction bins;
sample 0 has no ground truth, sample 1 has five.  The five boxes and the proposals are
constructed, and main() ASSERTS what they are for.  The decode literals of the reference's
tests/test_utils/test_bbox_coders.py are read from that file (values only).  Only inputs,
module weights and outputs are stored.

Chamfer: the numpy float32 restatement the GPU tests use (tests/vote_ref.py) is compared here
with the reference's chamfer_distance on every case below: the indices are equal and the
distances are equal BIT FOR BIT (largest difference seen: 0.0) for l2, l1 and smooth_l1, so the
CPU test asks for exact equality.
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import roiaware_ref as RR  # noqa: E402
import vote_ref as V  # noqa: E402

REF = "/root/reference/mmdet3d/"
REF_TESTS = "/root/reference/tests/"
OUT = os.path.join(ROOT, "tests", "golden", "vote_head_vectors.npz")

MEAN_SIZES = [[2.114256, 1.620300, 0.927272], [0.791118, 1.279516, 0.718182],
              [0.923508, 1.867419, 0.845495], [0.591958, 0.552978, 0.827272],
              [0.699104, 0.454178, 0.75625], [0.69519, 1.346299, 0.736364],
              [0.528526, 1.002642, 1.172878], [0.500618, 0.632163, 0.683424],
              [0.404671, 1.071108, 1.688889], [0.76584, 1.398258, 0.472728]]
NUM_CLASSES, NUM_DIR_BINS = 10, 12
NUM_POINTS, NUM_SEED, NUM_PROPOSAL, SEED_CHANNELS, AGG_CHANNELS = 256, 32, 16, 8, 16
TRAIN_CFG = dict(pos_distance_thr=0.3, neg_distance_thr=0.6, sample_mod="vote")
TEST_CFG = dict(sample_mod="seed", nms_thr=0.25, score_thr=0.05, per_class_proposal=True)
VOTE_MODULE_CFG = dict(in_channels=SEED_CHANNELS, vote_per_seed=1, gt_per_seed=3,
                       conv_channels=(8, 8), conv_cfg=dict(type="Conv1d"),
                       norm_cfg=dict(type="BN1d"), norm_feats=True,
                       vote_loss=dict(type="ChamferDistance", mode="l1", reduction="none",
                                      loss_dst_weight=10.0))
PRED_LAYER_CFG = dict(in_channels=AGG_CHANNELS, shared_conv_channels=(16, 16), bias=True)
LOSSES = dict(
    objectness_loss=dict(type="CrossEntropyLoss", class_weight=[0.2, 0.8], reduction="sum",
                         loss_weight=5.0),
    center_loss=dict(type="ChamferDistance", mode="l2", reduction="sum", loss_src_weight=10.0,
                     loss_dst_weight=10.0),
    dir_class_loss=dict(type="CrossEntropyLoss", reduction="sum", loss_weight=1.0),
    dir_res_loss=dict(type="SmoothL1Loss", reduction="sum", loss_weight=10.0),
    size_class_loss=dict(type="CrossEntropyLoss", reduction="sum", loss_weight=1.0),
    size_res_loss=dict(type="SmoothL1Loss", reduction="sum", loss_weight=10.0 / 3.0),
    semantic_loss=dict(type="CrossEntropyLoss", reduction="sum", loss_weight=1.0))


class ConfigDict(dict):                       # mmcv.ConfigDict: keys as attributes
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


# ------------------------------------------------------- mmcv / mmdet 2.x, written out
class _Registry:
    def register_module(self):
        return lambda cls: cls


class ConvModule(nn.Module):       # mmcv.cnn.ConvModule: conv / bn / activate, bias='auto'
    def __init__(self, cin, cout, kernel_size, stride=1, padding=0, bias="auto", conv_cfg=None,
                 norm_cfg=None, act_cfg=dict(type="ReLU"), inplace=True):
        super().__init__()
        assert conv_cfg["type"] == "Conv1d" and norm_cfg["type"] == "BN1d"
        assert act_cfg["type"] == "ReLU"
        self.conv = nn.Conv1d(cin, cout, kernel_size, stride=stride, padding=padding,
                              bias=False if bias == "auto" else bool(bias))
        self.bn = nn.BatchNorm1d(cout)
        self.activate = nn.ReLU(inplace=inplace)

    def forward(self, x):
        return self.activate(self.bn(self.conv(x)))


def build_conv_layer(cfg, *args, **kw):
    return {"Conv1d": nn.Conv1d}[cfg["type"]](*args, **kw)


def is_tuple_of(seq, expected_type):
    return isinstance(seq, tuple) and all(isinstance(s, expected_type) for s in seq)


def multi_apply(func, *args, **kwargs):
    from functools import partial
    pfunc = partial(func, **kwargs) if kwargs else func
    return tuple(map(list, zip(*map(pfunc, *args))))


def weight_reduce_loss(loss, weight=None, reduction="mean", avg_factor=None):
    if weight is not None:
        loss = loss * weight
    if avg_factor is None:
        return loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss
    assert reduction == "mean"
    return loss.sum() / avg_factor


class CrossEntropyLoss(nn.Module):
    def __init__(self, use_sigmoid=False, use_mask=False, reduction="mean", class_weight=None,
                 loss_weight=1.0):
        super().__init__()
        assert not use_sigmoid and not use_mask
        self.reduction, self.class_weight, self.loss_weight = reduction, class_weight, loss_weight

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None):
        reduction = reduction_override if reduction_override else self.reduction
        class_weight = None if self.class_weight is None else \
            cls_score.new_tensor(self.class_weight)
        loss = F.cross_entropy(cls_score, label, weight=class_weight, reduction="none")
        if weight is not None:
            weight = weight.float()
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction, avg_factor)


class SmoothL1Loss(nn.Module):
    def __init__(self, beta=1.0, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.beta, self.reduction, self.loss_weight = beta, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        reduction = reduction_override if reduction_override else self.reduction
        diff = torch.abs(pred - target)
        loss = torch.where(diff < self.beta, 0.5 * diff * diff / self.beta, diff - 0.5 * self.beta)
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction, avg_factor)


def points_in_boxes_batch(points, boxes):
    """ops/roiaware_pool3d points_in_boxes_batch: [B, M, 3], [B, T, 7] -> int [B, M, T]."""
    return torch.from_numpy(RR.points_in_boxes_all(points.detach().numpy(),
                                                   boxes.detach().numpy()))


# ------------------------------------------------------------------ reference definitions
class _DropRelativeImports(ast.NodeTransformer):
    def visit_ImportFrom(self, node):
        return None if node.level > 0 else node


def _defs(path, names=None, kinds=(ast.ClassDef, ast.FunctionDef)):
    tree = _DropRelativeImports().visit(ast.parse(open(path).read()))
    ast.fix_missing_locations(tree)
    return [n for n in tree.body if isinstance(n, kinds) and (names is None or n.name in names)]


def _exec(nodes, path, ns):
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)


def reference_namespace():
    from abc import abstractmethod
    from enum import IntEnum, unique
    reg = _Registry()
    ns = {"torch": torch, "nn": nn, "F": F, "np": np, "LOSSES": reg, "HEADS": reg,
          "BBOX_CODERS": reg, "BaseBBoxCoder": object, "l1_loss": F.l1_loss,
          "mse_loss": F.mse_loss, "smooth_l1_loss": F.smooth_l1_loss,
          "force_fp32": lambda **kw: (lambda f: f), "multi_apply": multi_apply,
          "ConvModule": ConvModule, "build_conv_layer": build_conv_layer,
          "is_tuple_of": is_tuple_of, "abstractmethod": abstractmethod, "IntEnum": IntEnum,
          "unique": unique, "points_in_boxes_batch": points_in_boxes_batch, "BasePoints": None,
          "iou3d_cuda": None, "points_in_boxes_gpu": None, "build_sa_module": None,
          "furthest_point_sample": None, "build_bbox_coder": None}
    losses = {"CrossEntropyLoss": CrossEntropyLoss, "SmoothL1Loss": SmoothL1Loss}
    ns["build_loss"] = lambda cfg: losses[cfg["type"]](
        **{k: v for k, v in cfg.items() if k != "type"})
    for path, names in (
            ("models/losses/chamfer_distance.py", {"chamfer_distance", "ChamferDistance"}),
            ("core/bbox/coders/partial_bin_based_bbox_coder.py", {"PartialBinBasedBBoxCoder"}),
            ("core/bbox/structures/utils.py", {"limit_period", "rotation_3d_in_axis"}),
            ("core/bbox/structures/base_box3d.py", {"BaseInstance3DBoxes"}),
            ("core/bbox/structures/lidar_box3d.py", {"LiDARInstance3DBoxes"}),
            ("core/bbox/structures/depth_box3d.py", {"DepthInstance3DBoxes"}),
            ("core/bbox/structures/box_3d_mode.py", {"Box3DMode"}),
            ("core/post_processing/box3d_nms.py", {"aligned_3d_nms"}),
            ("models/model_utils/vote_module.py", {"VoteModule"}),
            ("models/dense_heads/base_conv_bbox_head.py", {"BaseConvBboxHead"}),
            ("models/dense_heads/vote_head.py", {"VoteHead"})):
        _exec(_defs(REF + path, names), REF + path, ns)
        if "ChamferDistance" in names:
            losses["ChamferDistance"] = ns["ChamferDistance"]
    return ns


def coder_test_literals():
    """The decode inputs and the expected boxes of the reference's
    test_partial_bin_based_box_coder, evaluated from its file (tensor literals only)."""
    path = REF_TESTS + "test_utils/test_bbox_coders.py"
    fn = _defs(path, {"test_partial_bin_based_box_coder"})[0]
    want = ["center", "size_class", "size_res", "dir_class", "dir_res", "expected_bbox3d"]
    out = {}
    for node in fn.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and \
                isinstance(node.targets[0], ast.Name) and node.targets[0].id in want and \
                node.targets[0].id not in out:
            expr = ast.fix_missing_locations(ast.Expression(node.value))
            out[node.targets[0].id] = eval(compile(expr, path, "eval"), {"torch": torch})
    assert sorted(out) == sorted(want)
    return out


def build_head(ns):
    head = ns["VoteHead"].__new__(ns["VoteHead"])
    nn.Module.__init__(head)
    head.num_classes = NUM_CLASSES
    head.train_cfg, head.test_cfg = ConfigDict(TRAIN_CFG), ConfigDict(TEST_CFG)
    head.gt_per_seed, head.num_proposal = VOTE_MODULE_CFG["gt_per_seed"], NUM_PROPOSAL
    for name, cfg in LOSSES.items():
        setattr(head, name, ns["build_loss"](cfg))
    head.iou_loss = None
    head.bbox_coder = ns["PartialBinBasedBBoxCoder"](
        num_dir_bins=NUM_DIR_BINS, num_sizes=NUM_CLASSES, mean_sizes=MEAN_SIZES, with_rot=True)
    head.num_sizes, head.num_dir_bins = NUM_CLASSES, NUM_DIR_BINS
    head.vote_module = ns["VoteModule"](**VOTE_MODULE_CFG)
    head.conv_pred = ns["BaseConvBboxHead"](
        **PRED_LAYER_CFG, num_cls_out_channels=head._get_cls_out_channels(),
        num_reg_out_channels=head._get_reg_out_channels())
    return head


def five_boxes():
    """Depth boxes (x, y, z bottom, x size, y size, z size, yaw): four nested about the origin
    with different heights (so their gravity centres differ), one apart."""
    boxes = np.asarray([[0.0, 0.0, 0.0, 4.0, 4.0, 2.0, 0.0],
                        [0.0, 0.0, 0.0, 3.0, 3.0, 1.8, 0.5],
                        [0.0, 0.0, 0.0, 2.0, 2.0, 1.6, np.pi / 2],
                        [0.0, 0.0, 0.0, 1.0, 1.0, 1.4, -0.3],
                        [5.0, 5.0, 0.2, 1.2, 0.8, 1.0, 2.0]], np.float32)
    labels = np.asarray([0, 2, 5, 7, 9], np.int64)
    return boxes, labels


def make_points(rs):
    """[2, 256, 4]: a dense cluster about the origin (so that proposals there hold more than five
    points), a sparse remainder, and in sample 1 four points placed inside 1, 2, 3 and 4 boxes."""
    pts = np.empty((2, NUM_POINTS, 4), np.float32)
    for b in range(2):
        dense = np.concatenate([rs.uniform(-1.6, 1.6, (150, 2)), rs.uniform(0.05, 1.9, (150, 1))], 1)
        sparse = np.concatenate([rs.uniform(-3, 7, (106, 2)), rs.uniform(0.05, 1.9, (106, 1))], 1)
        pts[b, :, :3] = np.concatenate([dense, sparse])
        pts[b, :, 3] = rs.uniform(0, 1, NUM_POINTS)
    pts[1, 0, :3] = [1.9, 1.9, 1.0]       # box 0 only
    pts[1, 1, :3] = [1.3, 0.0, 1.0]       # boxes 0, 1
    pts[1, 2, :3] = [0.8, 0.0, 1.0]       # boxes 0, 1, 2
    pts[1, 3, :3] = [0.1, 0.1, 1.0]       # boxes 0, 1, 2, 3: slot 2 is overwritten by box 3
    return pts


def _np(t):
    return t.detach().cpu().numpy()


def main():
    torch.manual_seed(0)
    rs = np.random.RandomState(0)
    ns = reference_namespace()
    Depth = ns["DepthInstance3DBoxes"]
    out = {}

    # ---- Chamfer: reference outputs, and the restatement against them
    worst = 0.0
    for tag, (b, n, m) in (("a", (2, 10, 5)), ("b", (3, 70, 33)), ("c", (64, 1, 3))):
        src = (rs.randn(b, n, 3) * 1.2).astype(np.float32)
        dst = (rs.randn(b, m, 3) * 1.2).astype(np.float32)
        dst[:, -1] = dst[:, 0]                                  # a tie: the lowest index wins
        out["chamfer_%s_src" % tag], out["chamfer_%s_dst" % tag] = src, dst
        for mode in ("l2", "l1", "smooth_l1"):
            ref = ns["chamfer_distance"](torch.from_numpy(src), torch.from_numpy(dst),
                                         criterion_mode=mode, reduction="none")
            own = V.chamfer_forward(src, dst, mode)
            assert np.array_equal(own[1], _np(ref[2])) and np.array_equal(own[3], _np(ref[3]))
            worst = max(worst, float(np.abs(own[0] - _np(ref[0])).max()),
                        float(np.abs(own[2] - _np(ref[1])).max()))
            assert own[0].tobytes() == _np(ref[0]).tobytes()
            assert own[2].tobytes() == _np(ref[1]).tobytes()
            for k, v in zip(("d1", "d2", "i1", "i2"), ref):
                out["chamfer_%s_%s_%s" % (tag, mode, k)] = _np(v)
    print("chamfer restatement vs reference: largest difference", worst)
    # the reference's own test_chamfer_disrance relations through its module
    cd = ns["ChamferDistance"](mode="l2", reduction="sum", loss_src_weight=1.0, loss_dst_weight=1.0)
    ls, lt, i1, i2 = cd(torch.from_numpy(out["chamfer_a_src"]), torch.from_numpy(out["chamfer_a_dst"]),
                        return_indices=True)
    assert torch.allclose(ls, torch.from_numpy(out["chamfer_a_l2_d1"]).sum())
    out["chamfer_a_module_sum"] = np.asarray([float(ls), float(lt)], np.float32)

    # ---- coder: the reference test's literals, decode through the reference
    coder = ns["PartialBinBasedBBoxCoder"](num_dir_bins=NUM_DIR_BINS, num_sizes=NUM_CLASSES,
                                           mean_sizes=MEAN_SIZES, with_rot=True)
    lit = coder_test_literals()
    decoded = coder.decode({k: v.clone() for k, v in lit.items() if k != "expected_bbox3d"})
    assert torch.allclose(decoded, lit["expected_bbox3d"], atol=1e-4)
    for k, v in lit.items():
        out["coder_lit_" + k] = _np(v)
    out["coder_lit_decoded"] = _np(decoded)

    # ---- ground truths, boxes structure
    gt_np, labels_np = five_boxes()
    gt_boxes = [Depth(torch.zeros((0, 7))), Depth(torch.from_numpy(gt_np))]
    gt_labels = [torch.zeros((0,), dtype=torch.long), torch.from_numpy(labels_np)]
    out["gt_boxes_1"], out["gt_labels_1"] = gt_np, labels_np
    out["gt_gravity_center_1"] = _np(gt_boxes[1].gravity_center)
    out["gt_corners_1"] = _np(gt_boxes[1].corners)
    out["gt_boxes_lidar_1"] = _np(gt_boxes[1].convert_to(ns["Box3DMode"].LIDAR).tensor)
    shifted = Depth(torch.from_numpy(gt_np), origin=(0.5, 0.5, 0.5))
    out["gt_from_gravity_origin_1"] = _np(shifted.tensor)
    enc = coder.encode(gt_boxes[1], gt_labels[1])
    for k, v in zip(("center", "size_class", "size_res", "dir_class", "dir_res"), enc):
        out["encode_" + k] = _np(v)

    points_np = make_points(rs)
    points = [torch.from_numpy(points_np[0]), torch.from_numpy(points_np[1])]
    out["points"] = points_np
    inside = _np(gt_boxes[1].points_in_boxes(points[1][:, :3]))
    out["points_in_boxes_1"] = inside.astype(np.int32)
    assert inside[:4].sum(1).tolist() == [1, 2, 3, 4], inside[:4]
    assert inside[3].tolist() == [1, 1, 1, 1, 0]

    # ---- head: vote module and prediction layers, forward through the reference
    head = build_head(ns)
    head.train()
    for name, module in (("vote_module", head.vote_module), ("conv_pred", head.conv_pred)):
        for k, v in module.state_dict().items():
            out["weights_%s.%s" % (name, k)] = _np(v)
    seed_indices = torch.from_numpy(rs.randint(0, NUM_POINTS, (2, NUM_SEED)).astype(np.int64))
    seed_indices[1, :4] = torch.arange(4)                       # the four placed points are seeds
    seed_points = torch.stack([points[b][seed_indices[b], :3] for b in range(2)])
    seed_features = torch.randn(2, SEED_CHANNELS, NUM_SEED)
    vote_points, vote_features, vote_offset = head.vote_module(seed_points, seed_features)
    out.update(seed_indices=_np(seed_indices), seed_points=_np(seed_points),
               seed_features=_np(seed_features), vote_points=_np(vote_points),
               vote_features=_np(vote_features), vote_offset=_np(vote_offset))

    # proposals: sample 1 has one within pos_distance_thr of a centre, one between the two
    # thresholds, one beyond both; the rest spread over the scene
    centers = gt_boxes[1].gravity_center
    aggregated = torch.from_numpy(np.concatenate(
        [rs.uniform(-2, 2, (2, NUM_PROPOSAL, 2)), rs.uniform(0.3, 1.5, (2, NUM_PROPOSAL, 1))],
        2).astype(np.float32))
    aggregated[1, 0] = centers[4] + torch.tensor([0.1, 0.0, 0.1])
    aggregated[1, 1] = centers[4] + torch.tensor([0.45, 0.0, 0.0])
    aggregated[1, 2] = torch.tensor([10.0, 10.0, 5.0])
    aggregated[1, 3] = centers[3] + torch.tensor([0.02, -0.02, 0.0])
    agg_features = torch.randn(2, AGG_CHANNELS, NUM_PROPOSAL)
    cls_pred, reg_pred = head.conv_pred(agg_features)
    out.update(aggregated_points=_np(aggregated), aggregated_features=_np(agg_features),
               cls_predictions=_np(cls_pred), reg_predictions=_np(reg_pred))
    bbox_preds = dict(seed_points=seed_points, seed_indices=seed_indices, vote_points=vote_points,
                      vote_features=vote_features, vote_offset=vote_offset,
                      aggregated_points=aggregated)
    bbox_preds.update(head.bbox_coder.split_pred(cls_pred, reg_pred, aggregated))
    for k in ("center", "dir_class", "dir_res_norm", "dir_res", "size_class", "size_res_norm",
              "size_res", "obj_scores", "sem_scores"):
        out["split_" + k] = _np(bbox_preds[k])

    # ---- targets and losses
    names = ("vote_targets", "vote_target_masks", "size_class_targets", "size_res_targets",
             "dir_class_targets", "dir_res_targets", "center_targets", "assigned_center_targets",
             "mask_targets", "valid_gt_masks", "objectness_targets", "objectness_weights",
             "box_loss_weights", "valid_gt_weights")
    single = head.get_targets_single(points[1], gt_boxes[1], gt_labels[1],
                                     aggregated_points=aggregated[1])
    dist = torch.sqrt(((aggregated[1, :, None] - centers[None]) ** 2).sum(-1).min(1)[0] + 1e-6)
    assert dist[0] < 0.3 and 0.3 < dist[1] < 0.6 and dist[2] > 0.6 and dist[3] < 0.3
    assert single[9].tolist()[:4] == [1, 0, 0, 1] and single[10].tolist()[:4] == [1.0, 0.0, 1.0, 1.0]
    votes3 = single[0][3].view(3, 3)                            # the point inside four boxes
    want3 = centers[[0, 1, 3]] - points[1][3, :3]
    assert torch.equal(votes3, want3), (votes3, want3)          # slot 2: the LAST box, not the third
    targets = head.get_targets(points, list(gt_boxes), list(gt_labels), None, None, bbox_preds)
    assert len(targets) == len(names)
    for k, v in zip(names, targets):
        out["targets_" + k] = _np(v)
    assert targets[9].tolist() == [[0, 0, 0, 0, 0], [1, 1, 1, 1, 1]]
    losses = head.loss(bbox_preds, points, list(gt_boxes), list(gt_labels))
    for k, v in losses.items():
        assert torch.isfinite(v), k
        out["loss_" + k] = _np(v)
    vote_loss = head.vote_module.get_loss(seed_points, vote_points, seed_indices, targets[1],
                                          targets[0])
    assert torch.equal(vote_loss, losses["vote_loss"])

    # ---- boxes: hand-set scores over the same predictions
    preds = {k: v.detach().clone() for k, v in bbox_preds.items()}
    preds["center"][:, :8] = torch.from_numpy(
        np.concatenate([rs.uniform(-0.5, 0.5, (2, 8, 2)), rs.uniform(0.8, 1.1, (2, 8, 1))],
                       2).astype(np.float32))                   # eight proposals in the cluster
    preds["size_class"][:, :8, 0] += 10.0                       # ... of the largest mean size
    preds["center"][:, 5] = preds["center"][:, 4] + 0.02        # a near duplicate ...
    preds["sem_scores"][:, 5] = preds["sem_scores"][:, 4]       # ... of the same class
    preds["size_class"][:, 5] = preds["size_class"][:, 4]
    preds["size_res"][:, 5] = preds["size_res"][:, 4]
    preds["obj_scores"] = torch.from_numpy(rs.randn(2, NUM_PROPOSAL, 2).astype(np.float32))
    preds["obj_scores"][:, 4] = torch.tensor([-2.0, 2.0])
    preds["obj_scores"][:, 5] = torch.tensor([-1.0, 1.0])
    preds["obj_scores"][:, 6] = torch.tensor([4.0, -4.0])       # below the score threshold
    for k in ("center", "obj_scores", "sem_scores", "size_class", "size_res"):
        out["boxes_in_" + k] = _np(preds[k])
    points_cat = torch.stack(points)
    metas = [dict(box_type_3d=Depth), dict(box_type_3d=Depth)]
    out["boxes_decoded"] = _np(head.get_bboxes(points_cat, preds, metas, use_nms=False))
    for per_class in (True, False):
        head.test_cfg = ConfigDict(dict(TEST_CFG, per_class_proposal=per_class))
        results = head.get_bboxes(points_cat, preds, metas)
        tag = "boxes_per_class_" if per_class else "boxes_"
        for b, (box, score, label) in enumerate(results):
            out["%s%d_tensor" % (tag, b)] = _np(box.tensor)
            out["%s%d_scores" % (tag, b)] = _np(score)
            out["%s%d_labels" % (tag, b)] = _np(label)
    kept = [out["boxes_%d_tensor" % b].shape[0] for b in range(2)]
    obj = torch.softmax(preds["obj_scores"], -1)[..., -1]
    # in both samples: something is kept, the duplicate went, an empty box went, a low score went
    for b in range(2):
        decoded = Depth(torch.from_numpy(out["boxes_decoded"][b]), origin=(0.5, 0.5, 0.5))
        count = decoded.points_in_boxes(points[b][:, :3]).T.sum(1)
        assert 1 <= kept[b] < NUM_PROPOSAL, kept
        assert (count > 5).any() and (count <= 5).any(), count
        assert count[4] > 5 and count[5] > 5 and obj[b, 6] < 0.05
        got = torch.from_numpy(out["boxes_%d_tensor" % b])
        assert (got == decoded.tensor[4]).all(1).any() and not (got == decoded.tensor[5]).all(1).any()
    print("kept boxes per sample:", kept)

    # ---- aligned_3d_nms on the decoded min-max boxes of sample 1 (through the reference)
    corners = Depth(torch.from_numpy(out["boxes_decoded"][1]), origin=(0.5, 0.5, 0.5)).corners
    minmax = torch.cat([corners.min(1)[0], corners.max(1)[0]], 1)
    classes = torch.argmax(preds["sem_scores"][1], -1)
    pick = ns["aligned_3d_nms"](minmax, obj[1], classes, 0.25)
    out.update(nms_boxes=_np(minmax), nms_scores=_np(obj[1]), nms_classes=_np(classes),
               nms_pick=_np(pick))

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "(%d arrays, %d bytes)" % (len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
