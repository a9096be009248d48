#!/usr/bin/env python
"""Generates tests/golden/h3d_bbox_head_vectors.npz by RUNNING the reference's own code:

    H3DBboxHead.get_targets / get_targets_single
                                mmdet3d/models/roi_heads/bbox_heads/h3d_bbox_head.py:655-932
    H3DBboxHead.__init__ / forward / loss / get_proposal_stage_loss and the suffix-mixed decode
    of get_bboxes               the same file, :56-199, :210-444, :464-476, :552-659
    DepthInstance3DBoxes.get_surface_line_center
                                mmdet3d/core/bbox/structures/depth_box3d.py:277-330
    chamfer_distance, DepthInstance3DBoxes: as make_vote_head_golden.py takes them

mmcv / mmdet are absent: the definitions are taken from the reference FILES at run time, in the
namespace make_vote_head_golden.py builds.  Both functions are plain torch and run on the CPU as
they stand: in float32 through get_targets (the empty-sample padding and the stack included),
and in float64 through get_targets_single with a box stand-in that hands the float32 box
columns over as float64 and runs the reference's get_surface_line_center on them
(DepthInstance3DBoxes itself casts to float32).

forward, loss and the decode run on the reference's own H3DBboxHead, built by its own __init__
("head" without yaw, "head_yaw" with), in float32 and in float64 (a box stand-in keeps the cue
centres in float64, as above).  The two CUDA-only matchers are replaced by _SAMatcher, which has
PointSAModule's parameter names and a forward written out in plain torch; its ball query takes
the neighbours in ascending index with d^2 < r^2, pads a row with its first hit and gives index 0
for an empty ball.  mmdet's MSELoss is written out (mse_loss under weighted_loss).  Stored: the
weights and their key list, the inputs, every forward output, every loss term, the gradients of
the summed loss for every parameter, the proposals and the primitive centres, and the decode.

The inputs come from tests/h3d_cases.py.  main() ASSERTS that the discrete outcomes are well
defined on every case: the restatement tests/h3d_ref.py must agree with the reference exactly
on the discrete outputs in both precisions, and its traces carry the margin assertions (no
compared distance within 1e-3 of its threshold, nearest and second-nearest squared distances
1e-4 apart).  Only inputs and outputs are stored.

    python tests/golden/make_h3d_bbox_head_golden.py
"""
import os
import sys

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_vote_head_golden as G  # noqa: E402
import h3d_cases as HC  # noqa: E402
import h3d_ref as R  # noqa: E402

OUT = os.path.join(HERE, "h3d_bbox_head_vectors.npz")
PROPOSALS, SURFACES, LINES, CLASSES = 16, 40, 30, 18
# name -> (ground truths per sample, with_yaw): B = 2 and B = 1, with and without yaw (six
# distinct non-zero yaws over the samples of "yaw"), an empty sample, 1 .. 5 ground truths
CASES = {"yaw": ((5, 3), True), "no_yaw": ((4, 0), False), "single_yaw": ((2,), True),
         "single": ((1,), False)}


class _Boxes64:
    """What get_targets_single reads of a box set, in float64: the reference's own
    get_surface_line_center runs on these members."""

    def __init__(self, boxes, fn):
        self._t, self._fn = boxes.tensor.double(), fn
        self.gravity_center = boxes.gravity_center.double()

    dims = property(lambda self: self._t[:, 3:6])
    yaw = property(lambda self: self._t[:, 6])

    def to(self, device):
        return self

    def get_surface_line_center(self):
        return self._fn(self)


class _Depth64:
    """What forward and loss read of DepthInstance3DBoxes, without its cast to float32: the
    reference's own get_surface_line_center runs on these members."""
    fn = None

    def __init__(self, tensor, box_dim=7, with_yaw=True, origin=(0.5, 0.5, 0)):
        self.tensor = tensor.clone()
        shift = tensor.new_tensor((0.5, 0.5, 0)) - tensor.new_tensor(origin)
        self.tensor[:, :3] += self.tensor[:, 3:6] * shift

    @property
    def gravity_center(self):
        t = self.tensor
        return torch.cat((t[:, :2], (t[:, 2] + t[:, 5] * 0.5)[:, None]), dim=1)

    dims = property(lambda self: self.tensor[:, 3:6])
    yaw = property(lambda self: self.tensor[:, 6])

    def get_surface_line_center(self):
        return _Depth64.fn(self)


class _SAMatcher(nn.Module):
    """PointSAModule (ops/pointnet_modules/point_sa_module.py) with target_xyz, in plain torch:
    mlps.0.layer{j} = Conv2d without bias + BatchNorm2d + ReLU, max pooling over the group."""

    def __init__(self, mlp_channels, num_point=None, radius=None, num_sample=None, use_xyz=True,
                 normalize_xyz=False, **kw):
        super().__init__()
        assert use_xyz
        self.radius, self.num_sample, self.normalize_xyz = radius, num_sample, normalize_xyz
        spec = list(mlp_channels)
        spec[0] += 3
        mlp = nn.Sequential()
        for j in range(len(spec) - 1):
            layer = nn.Module()
            layer.conv = nn.Conv2d(spec[j], spec[j + 1], 1, bias=False)
            layer.bn = nn.BatchNorm2d(spec[j + 1])
            mlp.add_module("layer%d" % j, layer)
        self.mlps = nn.ModuleList([mlp])
        self.margin = float("inf")        # the closest any d gets to the radius

    def ball_query(self, xyz, new_xyz):
        """Ascending index, d^2 < r^2, the first hit pads the row, an empty ball gives index 0."""
        d2 = ((new_xyz[:, :, None, :] - xyz[:, None, :, :]) ** 2).sum(-1)           # [B, M, N]
        self.margin = min(self.margin, float((d2.detach().sqrt() - self.radius).abs().min()))
        inside = d2 < self.radius ** 2
        n = xyz.shape[1]
        order = torch.where(inside, torch.arange(n).expand_as(inside), torch.full_like(
            inside, n, dtype=torch.long)).sort(dim=-1)[0][..., :self.num_sample]
        if order.shape[-1] < self.num_sample:
            order = torch.cat((order, order.new_full(
                order.shape[:-1] + (self.num_sample - order.shape[-1],), n)), dim=-1)
        first = torch.where(order[..., :1] < n, order[..., :1], torch.zeros_like(order[..., :1]))
        return torch.where(order < n, order, first.expand_as(order))                # [B, M, S]

    def forward(self, points_xyz, features=None, indices=None, target_xyz=None):
        assert indices is None and target_xyz is not None
        idx = self.ball_query(points_xyz.detach(), target_xyz.detach())
        b, m, k = idx.shape
        flat = idx.reshape(b, m * k)
        grouped_xyz = torch.gather(points_xyz, 1, flat[..., None].expand(-1, -1, 3))
        grouped_xyz = grouped_xyz.reshape(b, m, k, 3) - target_xyz[:, :, None, :]
        if self.normalize_xyz:
            grouped_xyz = grouped_xyz / self.radius
        grouped = torch.gather(features, 2, flat[:, None, :].expand(-1, features.shape[1], -1))
        x = torch.cat((grouped_xyz.permute(0, 3, 1, 2), grouped.reshape(b, -1, m, k)), dim=1)
        for layer in self.mlps[0]:
            x = F.relu(layer.bn(layer.conv(x)))
        return target_xyz, x.max(dim=-1)[0], None


class _MSELoss(nn.Module):
    """mmdet/models/losses/mse_loss.py."""

    def __init__(self, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        return self.loss_weight * G.weight_reduce_loss(
            F.mse_loss(pred, target, reduction="none"), weight, self.reduction, avg_factor)


class _ConvModule(G.ConvModule):
    """forward adds the proposal feature to bbox_pred[0]'s output in place (:307).  Current
    torch keeps a ReLU's output for its backward and refuses that; a copy of the output has the
    same values and may be written to."""

    def forward(self, x):
        return super().forward(x).clone()


def namespace():
    ns = G.reference_namespace()
    ns["ConvModule"] = _ConvModule
    rest = lambda cfg: {k: v for k, v in cfg.items() if k != "type"}          # noqa: E731
    build_loss = ns["build_loss"]
    ns.update(build_sa_module=lambda cfg: _SAMatcher(**rest(cfg)),
              build_bbox_coder=lambda cfg: ns["PartialBinBasedBBoxCoder"](**rest(cfg)),
              build_loss=lambda cfg: _MSELoss(**rest(cfg)) if cfg["type"] == "MSELoss"
              else build_loss(cfg))
    path = "models/roi_heads/bbox_heads/h3d_bbox_head.py"
    G._exec(G._defs(G.REF + path, {"H3DBboxHead"}), G.REF + path, ns)
    return ns


def bottom_form(boxes, depth_cls, with_yaw):
    """Gravity-centre rows -> (the reference's box object on bottom-centre rows, the gravity
    form as the reference derives it from them)."""
    bottom = boxes.clone()
    bottom[:, 2] = bottom[:, 2] - bottom[:, 5] * 0.5
    depth = depth_cls(bottom, with_yaw=with_yaw) if len(bottom) else \
        depth_cls(torch.zeros((0, 7)), with_yaw=with_yaw)
    return depth, torch.cat((depth.gravity_center, depth.tensor[:, 3:]), dim=1)


FEATS = 16                       # channels of every feature map of the head cases
# name -> (ground truths per sample, with_yaw, direction bins, seed of the inputs).  The seeds are
# fixed: head_cases asserts the margins on them and fails where one does not hold.
HEAD_CASES = {"head": ((3, 2), False, 1, 701), "head_yaw": ((2, 4), True, 4, 702)}
MEAN_SIZES = [[2.0 + 0.05 * k, 2.2 + 0.04 * k, 2.4 + 0.03 * k] for k in range(CLASSES)]
FORWARD_INPUTS = ("aggregated_points", "aggregated_features", "pred_z_center", "pred_xy_center",
                  "sem_cls_scores_z", "sem_cls_scores_xy", "aggregated_features_z",
                  "aggregated_features_xy", "pred_line_center", "aggregated_features_line",
                  "sem_cls_scores_line", "proposal_list")
GRAD_INPUTS = ("proposal_list", "pred_z_center", "pred_xy_center", "pred_line_center")
RPN_TARGETS = ("vote_targets", "vote_target_masks", "size_class_targets", "size_res_targets",
               "dir_class_targets", "dir_res_targets", "center_targets", "mask_targets",
               "valid_gt_masks", "objectness_targets", "objectness_weights", "box_loss_weights",
               "valid_gt_weights")
RPN_KEYS = ("sem_scores", "dir_class", "size_class")


def head_cfg(with_yaw, bins):
    """H3DBboxHead's arguments for the head cases (tests build this project's head from them)."""
    ce = lambda w, r="sum", **kw: dict(type="CrossEntropyLoss", reduction=r,   # noqa: E731
                                       loss_weight=w, **kw)
    smooth = dict(type="SmoothL1Loss", reduction="sum", loss_weight=10.0)
    matching = lambda rows: dict(type="PointSAModule", num_point=PROPOSALS * rows,  # noqa: E731
                                 radius=0.5, num_sample=4, mlp_channels=[FEATS + rows, 16, 8],
                                 use_xyz=True, normalize_xyz=True)
    return dict(
        num_classes=CLASSES, suface_matching_cfg=matching(6), line_matching_cfg=matching(12),
        bbox_coder=dict(type="PartialBinBasedBBoxCoder", num_sizes=CLASSES, num_dir_bins=bins,
                        with_rot=with_yaw, mean_sizes=MEAN_SIZES),
        train_cfg=dict(HC.CFG), test_cfg=dict(nms_thr=0.25, score_thr=0.05,
                                              per_class_proposal=True),
        gt_per_seed=3, num_proposal=PROPOSALS, primitive_refine_channels=[FEATS, FEATS, FEATS],
        objectness_loss=ce(5.0, class_weight=[0.2, 0.8]),
        center_loss=dict(type="ChamferDistance", mode="l2", reduction="sum",
                         loss_src_weight=10.0, loss_dst_weight=10.0),
        dir_class_loss=ce(0.1), dir_res_loss=dict(smooth), size_class_loss=ce(0.1),
        size_res_loss=dict(smooth), semantic_loss=ce(0.1),
        cues_objectness_loss=ce(5.0, "mean", class_weight=[0.3, 0.7]),
        cues_semantic_loss=ce(5.0, "mean", class_weight=[0.3, 0.7]),
        proposal_objectness_loss=ce(5.0, "none", class_weight=[0.2, 0.8]),
        primitive_center_loss=dict(type="MSELoss", reduction="none", loss_weight=1.0))


def head_inputs(seed, counts, with_yaw, bins):
    """-> (forward inputs, the rpn head's 13 targets and its unsuffixed predictions, ground-truth
    boxes in gravity form, labels), all float32 / long."""
    case = HC.draw_case(seed, counts, PROPOSALS, SURFACES, LINES, CLASSES, with_yaw)
    rs = np.random.default_rng(seed + 7)
    rand = lambda *shape: torch.from_numpy(rs.normal(size=shape)).float()     # noqa: E731
    batch, half = len(counts), SURFACES // 2
    proposals = []
    for b in range(batch):                      # each proposal: its nearest box, perturbed
        g = case["gt_boxes"][b]
        near = R.first_min(R.sq_dist(case["aggregated"][b], g[:, :3]))[1]
        box = g[near].clone()
        box[:, :3] = case["aggregated"][b] + 0.05 * rand(PROPOSALS, 3)
        box[:, 3:6] *= 1 + 0.1 * rand(PROPOSALS, 3).clamp(-2, 2)
        box[:, 6] = box[:, 6] + 0.1 * rand(PROPOSALS) if with_yaw else 0
        proposals.append(box)
    ins = dict(aggregated_points=case["aggregated"], aggregated_features=rand(batch, FEATS, PROPOSALS),
               pred_z_center=case["surface_pred"][:, :half].contiguous(),
               pred_xy_center=case["surface_pred"][:, half:].contiguous(),
               sem_cls_scores_z=case["surface_sem"][:, :half].contiguous(),
               sem_cls_scores_xy=case["surface_sem"][:, half:].contiguous(),
               aggregated_features_z=rand(batch, FEATS, half),
               aggregated_features_xy=rand(batch, FEATS, half),
               pred_line_center=case["line_pred"], aggregated_features_line=rand(batch, FEATS, LINES),
               sem_cls_scores_line=case["line_sem"], proposal_list=torch.stack(proposals))
    g = max(counts)
    # the rpn head's centre targets are the ground-truth centres (a short sample repeats its
    # first): every proposal lies near one, as in training, and the centre loss is of order one
    centers = torch.stack([torch.cat((c[:, :3], c[:1, :3].expand(g - len(c), 3)))
                           for c in case["gt_boxes"]])
    integers = lambda high, *shape: torch.from_numpy(rs.integers(0, high, size=shape)).long()  # noqa: E731
    uniform = lambda *shape: torch.from_numpy(rs.random(shape)).float()       # noqa: E731
    rpn = dict(vote_targets=torch.zeros(batch, 8, 9), vote_target_masks=torch.zeros(batch, 8).long(),
               size_class_targets=integers(CLASSES, batch, PROPOSALS),
               size_res_targets=0.3 * rand(batch, PROPOSALS, 3),
               dir_class_targets=integers(bins, batch, PROPOSALS),
               dir_res_targets=0.3 * rand(batch, PROPOSALS),
               center_targets=centers,
               mask_targets=integers(CLASSES, batch, PROPOSALS),
               valid_gt_masks=torch.ones(batch, g).long(),
               objectness_targets=integers(2, batch, PROPOSALS),
               objectness_weights=uniform(batch, PROPOSALS) / PROPOSALS,
               box_loss_weights=uniform(batch, PROPOSALS) / PROPOSALS,
               valid_gt_weights=uniform(batch, g) / g)
    rpn_preds = dict(sem_scores=rand(batch, PROPOSALS, CLASSES), dir_class=rand(batch, PROPOSALS, bins),
                     size_class=rand(batch, PROPOSALS, CLASSES))
    return ins, rpn, rpn_preds, case["gt_boxes"], case["gt_labels"]


def run_head(ns, head, ins, rpn, rpn_preds, boxes, labels, dtype):
    """The reference's forward, loss and suffix-mixed decode in `dtype` -> (outputs, losses,
    gradients, decode, targets)."""
    Depth = ns["DepthInstance3DBoxes"]
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t             # noqa: E731
    head = head.to(dtype).train()
    head.zero_grad()
    feats = {k: cast(v).clone().requires_grad_(k in GRAD_INPUTS) for k, v in ins.items()}
    if dtype == torch.float64:
        _Depth64.fn = staticmethod(Depth.get_surface_line_center)
        ns["DepthInstance3DBoxes"] = _Depth64
    try:
        out = head(feats, "vote")
        preds = dict(feats, **out)
        preds.update({k: cast(v) for k, v in rpn_preds.items()})
        gt = []
        for g in boxes:
            depth, _ = bottom_form(g, Depth, True)
            gt.append(_Boxes64(depth, Depth.get_surface_line_center) if dtype == torch.float64
                      else depth)
        points = [preds["aggregated_points"][b] for b in range(len(gt))]
        losses = head.loss(preds, points, gt, [l.clone() for l in labels],
                           rpn_targets=tuple(cast(rpn[k]) for k in RPN_TARGETS))
        targets = head.get_targets(points, list(gt), [l.clone() for l in labels], None, None,
                                   {k: v.detach() for k, v in preds.items()})
        mixed = dict(center=preds["center_optimized"], dir_class=preds["dir_class"],
                     dir_res=preds["dir_res_optimized"], size_class=preds["size_class"],
                     size_res=preds["size_res_optimized"])                     # :469-476
        decode = head.bbox_coder.decode(mixed)
    finally:
        ns["DepthInstance3DBoxes"] = Depth
    sum(losses.values()).backward()
    grads = {"param/" + k: v.grad for k, v in head.named_parameters()}
    grads.update({"input/" + k: feats[k].grad for k in GRAD_INPUTS})
    assert all(g is not None for g in grads.values())
    return out, losses, grads, decode, targets


def head_cases(ns, put):
    Head = ns["H3DBboxHead"]
    for k, (name, (counts, with_yaw, bins, seed)) in enumerate(HEAD_CASES.items()):
        torch.manual_seed(40 + k)
        head = Head(**head_cfg(with_yaw, bins))
        for module in head.modules():                 # BatchNorm away from its identity start
            if isinstance(module, (nn.BatchNorm1d, nn.BatchNorm2d)):
                nn.init.uniform_(module.weight, 0.5, 1.5)
                nn.init.normal_(module.bias, std=0.2)
        state = {k: v.clone() for k, v in head.state_dict().items()}
        put(name + "/state_keys", np.array(list(state)))
        for k, v in state.items():
            put("%s/state/%s" % (name, k), v)
        ins, rpn, rpn_preds, boxes, labels = head_inputs(seed, counts, with_yaw, bins)
        put(name + "/with_yaw", int(with_yaw))
        put(name + "/num_dir_bins", bins)
        for group, items in (("in", ins), ("rpn", rpn), ("rpn_pred", rpn_preds)):
            for k, v in items.items():
                put("%s/%s/%s" % (name, group, k), v)
        for b in range(len(counts)):
            depth, _ = bottom_form(boxes[b], ns["DepthInstance3DBoxes"], True)
            put("%s/%d/boxes" % (name, b), depth.tensor)
            put("%s/%d/labels" % (name, b), labels[b])
        runs = {}
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            head.load_state_dict(state)
            for m in (head.surface_center_matcher, head.line_center_matcher):
                m.margin = float("inf")
            out, losses, grads, decode, targets = runs[tag] = run_head(
                ns, head, ins, rpn, rpn_preds, boxes, labels, dtype)
            for group, items in (("out", out), ("loss", losses), ("grad", grads)):
                for k, v in items.items():
                    put("%s/%s/%s/%s" % (name, tag, group, k), v)
            put("%s/%s/decode" % (name, tag), decode)
            for k, v in zip(R.TARGET_NAMES, targets):
                put("%s/%s/target/%s" % (name, tag, k), v)
            # the ball query is well defined: no distance within 1e-4 of the radius
            for m in (head.surface_center_matcher, head.line_center_matcher):
                assert m.margin >= 1e-4, (name, tag, m.margin)
        put(name + "/loss_keys", np.array(list(runs["f32"][1])))
        put(name + "/out_keys", np.array(list(runs["f32"][0])))
        # the discrete outcomes are well defined: the restatement's margins on what get_targets
        # read, and one answer in both precisions
        out64 = runs["f64"][0]
        case = dict(aggregated=ins["aggregated_points"],
                    surface_pred=out64["surface_center_pred"].detach().float(),
                    line_pred=ins["pred_line_center"],
                    surface_sem=out64["surface_sem_pred"].detach().float(),
                    line_sem=ins["sem_cls_scores_line"],
                    cue_obj=torch.cat((runs["f32"][0]["surface_center_object"],
                                       runs["f32"][0]["line_center_object"]), 1).detach(),
                    gt_boxes=[bottom_form(g, ns["DepthInstance3DBoxes"], True)[1] for g in boxes],
                    gt_labels=labels)
        r32, r64 = HC.reference(case)
        for k, key in enumerate(R.TARGET_NAMES[:7]):
            assert torch.equal(runs["f32"][4][k].double(), runs["f64"][4][k].double()), (name, key)
            assert torch.equal(runs["f32"][4][k].double(), r32[k].double()), (name, key)
        t32 = runs["f32"][4]
        assert t32[0].sum() > 0 and t32[6].sum() > 0 and 0 < t32[2].float().mean() < 1, name
        for tag in runs:
            assert all(torch.isfinite(v).all() for v in runs[tag][1].values()), name


def main():
    ns = namespace()
    Head, Depth = ns["H3DBboxHead"], ns["DepthInstance3DBoxes"]
    head = Head.__new__(Head)
    nn.Module.__init__(head)
    head.train_cfg = dict(HC.CFG)
    store = {}

    def put(key, value):
        store[key] = value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)

    put("cfg", [HC.CFG[k] for k in R.THRESHOLDS])
    for seed, (name, (counts, with_yaw)) in enumerate(CASES.items()):
        case = HC.make_case(900 + seed, counts, PROPOSALS, SURFACES, LINES, CLASSES, with_yaw)
        depth = []
        for b in range(len(counts)):
            box, gravity = bottom_form(case["gt_boxes"][b], Depth, with_yaw)
            depth.append(box)
            case["gt_boxes"][b] = gravity
        r32, r64 = HC.reference(case)              # the margins, on what is stored
        put(name + "/with_yaw", int(with_yaw))
        for key in ("aggregated", "surface_pred", "line_pred", "surface_sem", "line_sem",
                    "cue_obj"):
            put("%s/%s" % (name, key), case[key])
        p = PROPOSALS
        preds = dict(aggregated_points=case["aggregated"],
                     surface_center_pred=case["surface_pred"],
                     pred_line_center=case["line_pred"],
                     surface_center_object=case["cue_obj"][:, :6 * p],
                     line_center_object=case["cue_obj"][:, 6 * p:],
                     surface_sem_pred=case["surface_sem"], sem_cls_scores_line=case["line_sem"])
        for b, box in enumerate(depth):
            put("%s/%d/boxes" % (name, b), box.tensor)
            put("%s/%d/gravity_boxes" % (name, b), case["gt_boxes"][b])
            put("%s/%d/labels" % (name, b), case["gt_labels"][b])
            if len(box.tensor):
                fn = Depth.get_surface_line_center
                for tag, got in (("f32", box.get_surface_line_center()),
                                 ("f64", _Boxes64(box, fn).get_surface_line_center())):
                    put("%s/%d/%s/surface_center" % (name, b, tag), got[0])
                    put("%s/%d/%s/line_center" % (name, b, tag), got[1])
        points = [case["aggregated"][b] for b in range(len(counts))]
        got32 = head.get_targets(points, list(depth), [l.clone() for l in case["gt_labels"]],
                                 None, None, preds)
        rows = []
        boxes, labels = list(depth), [l.clone() for l in case["gt_labels"]]
        for b in range(len(counts)):
            box, lab = boxes[b], labels[b]
            if len(lab) == 0:                                       # :685-698
                box, lab = box.new_box(box.tensor.new_zeros(1, 7)), lab.new_zeros(1)
            rows.append(head.get_targets_single(
                points[b].double(), _Boxes64(box, Depth.get_surface_line_center), lab, None, None,
                *[preds[k][b].double() for k in (
                    "aggregated_points", "surface_center_pred", "pred_line_center",
                    "surface_center_object", "line_center_object")],
                preds["surface_sem_pred"][b], preds["sem_cls_scores_line"][b]))
        got64 = [torch.stack(col) for col in zip(*rows)]
        for k, key in enumerate(R.TARGET_NAMES):
            if key in R.DISCRETE:
                # the reference and its restatement, both precisions: one answer
                assert torch.equal(got32[k].double(), got64[k].double()), (name, key)
                assert torch.equal(got32[k].double(), r32[k].double()), (name, key)
                assert torch.equal(got64[k].double(), r64[k].double()), (name, key)
            put("%s/f32/%s" % (name, key), got32[k])
            put("%s/f64/%s" % (name, key), got64[k])
        assert float((got64[7] - r64[7]).abs().max()) < 1e-12, name
        assert got32[0].sum() > 0 and got32[6].sum() > 0 and got32[1].sum() > 0, name
        assert 0 < got32[2].float().mean() < 1, name
    # the rotation quirk shows: row 4 of the "yaw" case's first sample (box 0, face +x) is turned
    # by the yaw of box 4 % n, not by box 0's own
    s = store["yaw/0/f64/surface_center"]
    g = store["yaw/0/gravity_boxes"].astype(np.float64)
    n = g.shape[0]
    for own, want in ((4 % n, True), (0, False)):
        turned = g[0, :3] + np.array([np.cos(-g[own, 6]), np.sin(-g[own, 6]), 0.0]) * g[0, 3] / 2
        assert (np.abs(s[4] - turned).max() < 1e-12) == want, own
    head_cases(ns, put)
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(store), "arrays")


if __name__ == "__main__":
    main()
