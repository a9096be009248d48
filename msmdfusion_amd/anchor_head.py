"""Anchor3DHead (mmdet3d/models/dense_heads/anchor3d_head.py with train_mixins.py) and what it
is built from: the range anchor generators (core/anchor/anchor_3d_generator.py),
DeltaXYZWLHRBBoxCoder (core/bbox/coders/delta_xyzwhlr_bbox_coder.py), BboxOverlapsNearest3D
(core/bbox/iou_calculators/iou3d_calculator.py), mmdet's MaxIoUAssigner and
box3d_multiclass_nms (core/post_processing/box3d_nms.py:8-88) -- the reference's constructor
arguments, attribute names and state-dict keys (conv_cls, conv_reg, conv_dir_cls).

What differs from the reference is where the loops run:

  anchor_target_3d  every sample, level and assigner of a batch in one pass on the device: the
                    nearest-BEV boxes are torch arithmetic (cached for the anchors), assignment
                    and targets are two library calls (csrc/anchor.hip) that never form the
                    [num_gt, num_anchors] IoU matrix; nothing is read back.  (The reference:
                    per sample and per assigner a matrix, two reductions, a Python loop over
                    the ground truths with a host branch each, boolean-mask indexing.)
  loss              FocalLoss through the fused kernel; the regression and direction terms as
                    weighted sums over all anchors (weights are zero off the positives), with
                    num_total_samples a device scalar.
  get_bboxes        all (sample, class) lists of a batch through ONE batched NMS call; one host
                    read per call, the kept counts.

Out of scope, refused at construction: a real bbox_sampler (loss_cls other than FocalLoss), the
softmax classification branch, assigner options other than the ones the reference's configs
use (see MaxIoUAssigner).
"""
import math

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import kernels as K
from .registry import HEADS


def _box_tensor(boxes):
    return boxes.tensor if hasattr(boxes, "tensor") else boxes


# ---------------------------------------------------------------------------- anchors
class Anchor3DRangeGenerator:
    """anchor_3d_generator.py:8-209.  Anchors are computed on the host (so that they are the
    same numbers on every device) and cached per (featmap_sizes, device)."""

    def __init__(self, ranges, sizes=[[1.6, 3.9, 1.56]], scales=[1], rotations=[0, 1.5707963],
                 custom_values=(), reshape_out=True, size_per_range=True):
        assert isinstance(ranges, list) and all(isinstance(r, list) for r in ranges)
        if size_per_range:
            if len(sizes) != len(ranges):
                assert len(ranges) == 1
                ranges = ranges * len(sizes)
            assert len(ranges) == len(sizes)
        else:
            assert len(ranges) == 1
        assert isinstance(sizes, list) and all(isinstance(s, list) for s in sizes)
        assert isinstance(scales, list)
        self.sizes, self.scales, self.ranges, self.rotations = sizes, scales, ranges, rotations
        self.custom_values = custom_values
        self.cached_anchors = None
        self.reshape_out, self.size_per_range = reshape_out, size_per_range
        self._cache = {}

    def __repr__(self):
        s = self.__class__.__name__ + "("
        s += f"anchor_range={self.ranges},\n"
        s += f"scales={self.scales},\n"
        s += f"sizes={self.sizes},\n"
        s += f"rotations={self.rotations},\n"
        s += f"reshape_out={self.reshape_out},\n"
        s += f"size_per_range={self.size_per_range})"
        return s

    @property
    def num_base_anchors(self):
        return len(self.rotations) * torch.tensor(self.sizes).reshape(-1, 3).size(0)

    @property
    def num_levels(self):
        return len(self.scales)

    def grid_anchors(self, featmap_sizes, device="cuda"):
        assert self.num_levels == len(featmap_sizes)
        key = (tuple(tuple(int(v) for v in s) for s in featmap_sizes), str(torch.device(device)))
        if key not in self._cache:
            out = []
            for i in range(self.num_levels):
                anchors = self.single_level_grid_anchors(featmap_sizes[i], self.scales[i], "cpu")
                if self.reshape_out:
                    anchors = anchors.reshape(-1, anchors.size(-1))
                out.append(anchors.to(device))
            self._cache[key] = out
        return list(self._cache[key])

    def single_level_grid_anchors(self, featmap_size, scale, device="cuda"):
        if not self.size_per_range:
            return self.anchors_single_range(featmap_size, self.ranges[0], scale, self.sizes,
                                             self.rotations, device=device)
        mr_anchors = [self.anchors_single_range(featmap_size, anchor_range, scale, anchor_size,
                                                self.rotations, device=device)
                      for anchor_range, anchor_size in zip(self.ranges, self.sizes)]
        return torch.cat(mr_anchors, dim=-3)

    def _centers(self, anchor_range, feature_size, device):
        z = torch.linspace(anchor_range[2], anchor_range[5], feature_size[0], device=device)
        y = torch.linspace(anchor_range[1], anchor_range[4], feature_size[1], device=device)
        x = torch.linspace(anchor_range[0], anchor_range[3], feature_size[2], device=device)
        return x, y, z

    def anchors_single_range(self, feature_size, anchor_range, scale=1, sizes=[[1.6, 3.9, 1.56]],
                             rotations=[0, 1.5707963], device="cuda"):
        """-> [*feature_size, num_sizes, num_rots, 7 + custom]"""
        if len(feature_size) == 2:
            feature_size = [1, feature_size[0], feature_size[1]]
        feature_size = [int(v) for v in feature_size]
        anchor_range = torch.tensor(anchor_range, device=device)
        x_centers, y_centers, z_centers = self._centers(anchor_range, feature_size, device)
        sizes = torch.tensor(sizes, device=device).reshape(-1, 3) * scale
        rotations = torch.tensor(rotations, device=device)
        rets = list(torch.meshgrid(x_centers, y_centers, z_centers, rotations, indexing="ij"))
        tile_shape = [1] * 5
        tile_shape[-2] = int(sizes.shape[0])
        for i in range(len(rets)):
            rets[i] = rets[i].unsqueeze(-2).repeat(tile_shape).unsqueeze(-1)
        sizes = sizes.reshape([1, 1, 1, -1, 1, 3])
        tile_size_shape = list(rets[0].shape)
        tile_size_shape[3] = 1
        sizes = sizes.repeat(tile_size_shape)
        rets.insert(3, sizes)
        ret = torch.cat(rets, dim=-1).permute([2, 1, 0, 3, 4, 5])
        if len(self.custom_values) > 0:
            custom = ret.new_zeros([*ret.shape[:-1], len(self.custom_values)])
            ret = torch.cat([ret, custom], dim=-1)
        return ret


class AlignedAnchor3DRangeGenerator(Anchor3DRangeGenerator):
    """anchor_3d_generator.py:212-325: centres on the voxel grid."""

    def __init__(self, align_corner=False, **kwargs):
        super().__init__(**kwargs)
        self.align_corner = align_corner

    def _centers(self, anchor_range, feature_size, device):
        z = torch.linspace(anchor_range[2], anchor_range[5], feature_size[0] + 1, device=device)
        y = torch.linspace(anchor_range[1], anchor_range[4], feature_size[1] + 1, device=device)
        x = torch.linspace(anchor_range[0], anchor_range[3], feature_size[2] + 1, device=device)
        if not self.align_corner:
            z_shift = (z[1] - z[0]) / 2
            y_shift = (y[1] - y[0]) / 2
            x_shift = (x[1] - x[0]) / 2
            z += z_shift
            y += y_shift
            x += x_shift
        return x[:feature_size[2]], y[:feature_size[1]], z[:feature_size[0]]


_ANCHOR_GENERATORS = {"Anchor3DRangeGenerator": Anchor3DRangeGenerator,
                      "AlignedAnchor3DRangeGenerator": AlignedAnchor3DRangeGenerator}


def build_anchor_generator(cfg):
    if not isinstance(cfg, dict):
        return cfg
    args = dict(cfg)
    kind = args.pop("type")
    if kind not in _ANCHOR_GENERATORS:
        raise NotImplementedError("anchor generator %r is not built" % kind)
    return _ANCHOR_GENERATORS[kind](**args)


# ---------------------------------------------------------------------------- coder
class DeltaXYZWLHRBBoxCoder:
    """delta_xyzwhlr_bbox_coder.py."""

    def __init__(self, code_size=7):
        self.code_size = code_size

    @staticmethod
    def encode(src_boxes, dst_boxes):
        box_ndim = src_boxes.shape[-1]
        cas, cgs, cts = [], [], []
        if box_ndim > 7:
            xa, ya, za, wa, la, ha, ra, *cas = torch.split(src_boxes, 1, dim=-1)
            xg, yg, zg, wg, lg, hg, rg, *cgs = torch.split(dst_boxes, 1, dim=-1)
            cts = [g - a for g, a in zip(cgs, cas)]
        else:
            xa, ya, za, wa, la, ha, ra = torch.split(src_boxes, 1, dim=-1)
            xg, yg, zg, wg, lg, hg, rg = torch.split(dst_boxes, 1, dim=-1)
        za = za + ha / 2
        zg = zg + hg / 2
        diagonal = torch.sqrt(la**2 + wa**2)
        xt = (xg - xa) / diagonal
        yt = (yg - ya) / diagonal
        zt = (zg - za) / ha
        lt = torch.log(lg / la)
        wt = torch.log(wg / wa)
        ht = torch.log(hg / ha)
        rt = rg - ra
        return torch.cat([xt, yt, zt, wt, lt, ht, rt, *cts], dim=-1)

    @staticmethod
    def decode(anchors, deltas):
        cas, cts = [], []
        box_ndim = anchors.shape[-1]
        if box_ndim > 7:
            xa, ya, za, wa, la, ha, ra, *cas = torch.split(anchors, 1, dim=-1)
            xt, yt, zt, wt, lt, ht, rt, *cts = torch.split(deltas, 1, dim=-1)
        else:
            xa, ya, za, wa, la, ha, ra = torch.split(anchors, 1, dim=-1)
            xt, yt, zt, wt, lt, ht, rt = torch.split(deltas, 1, dim=-1)
        za = za + ha / 2
        diagonal = torch.sqrt(la**2 + wa**2)
        xg = xt * diagonal + xa
        yg = yt * diagonal + ya
        zg = zt * ha + za
        lg = torch.exp(lt) * la
        wg = torch.exp(wt) * wa
        hg = torch.exp(ht) * ha
        rg = rt + ra
        zg = zg - hg / 2
        cgs = [t + a for t, a in zip(cts, cas)]
        return torch.cat([xg, yg, zg, wg, lg, hg, rg, *cgs], dim=-1)


def build_bbox_coder(cfg):
    if not isinstance(cfg, dict):
        return cfg
    args = dict(cfg)
    kind = args.pop("type")
    if kind != "DeltaXYZWLHRBBoxCoder":
        raise NotImplementedError("Anchor3DHead: bbox_coder %r is not built" % kind)
    return DeltaXYZWLHRBBoxCoder(**args)


# ---------------------------------------------------------------------------- overlaps
def limit_period(val, offset=0.5, period=np.pi):
    """core/bbox/structures/utils.py:5-18."""
    return val - torch.floor(val / period + offset) * period


def xywhr2xyxyr(boxes_xywhr):
    """core/bbox/structures/utils.py xywhr2xyxyr."""
    boxes = torch.zeros_like(boxes_xywhr)
    half_w, half_h = boxes_xywhr[..., 2] / 2, boxes_xywhr[..., 3] / 2
    boxes[..., 0] = boxes_xywhr[..., 0] - half_w
    boxes[..., 1] = boxes_xywhr[..., 1] - half_h
    boxes[..., 2] = boxes_xywhr[..., 0] + half_w
    boxes[..., 3] = boxes_xywhr[..., 1] + half_h
    boxes[..., 4] = boxes_xywhr[..., 4]
    return boxes


def nearest_bev(boxes):
    """LiDARInstance3DBoxes.nearest_bev (lidar_box3d.py:93-111) of [n, >= 7] boxes -> [n, 4]
    (x1, y1, x2, y2).  The period is a tensor operand, so the division is a true float32
    division on every device (a Python-scalar divisor is a multiplication by the reciprocal on
    the GPU)."""
    x, y, w, l, rotations = boxes[:, 0], boxes[:, 1], boxes[:, 3], boxes[:, 4], boxes[:, 6]
    pi = torch.full((), np.pi, dtype=boxes.dtype, device=boxes.device)
    normed = torch.abs(rotations - torch.floor(rotations / pi + 0.5) * pi)
    swap = normed > np.pi / 4
    dx, dy = torch.where(swap, l, w), torch.where(swap, w, l)
    return torch.stack([x - dx / 2, y - dy / 2, x + dx / 2, y + dy / 2], dim=-1)


def bbox_overlaps(bboxes1, bboxes2, mode="iou", is_aligned=False, eps=1e-6):
    """mmdet 2.x core/bbox/iou_calculators/iou2d_calculator.py bbox_overlaps on [n, 4] boxes."""
    assert mode in ("iou", "iof")
    area1 = (bboxes1[..., 2] - bboxes1[..., 0]) * (bboxes1[..., 3] - bboxes1[..., 1])
    area2 = (bboxes2[..., 2] - bboxes2[..., 0]) * (bboxes2[..., 3] - bboxes2[..., 1])
    if is_aligned:
        lt = torch.max(bboxes1[..., :2], bboxes2[..., :2])
        rb = torch.min(bboxes1[..., 2:], bboxes2[..., 2:])
        wh = (rb - lt).clamp(min=0)
        overlap = wh[..., 0] * wh[..., 1]
        union = area1 + area2 - overlap if mode == "iou" else area1
    else:
        lt = torch.max(bboxes1[..., :, None, :2], bboxes2[..., None, :, :2])
        rb = torch.min(bboxes1[..., :, None, 2:], bboxes2[..., None, :, 2:])
        wh = (rb - lt).clamp(min=0)
        overlap = wh[..., 0] * wh[..., 1]
        union = area1[..., None] + area2[..., None, :] - overlap if mode == "iou" \
            else area1[..., None]
    union = torch.max(union, union.new_tensor([eps]))
    return overlap / union


def bbox_overlaps_nearest_3d(bboxes1, bboxes2, mode="iou", is_aligned=False, coordinate="lidar"):
    """iou3d_calculator.py:94-150 for LiDAR boxes."""
    assert bboxes1.size(-1) == bboxes2.size(-1) >= 7
    if coordinate != "lidar":
        raise NotImplementedError("bbox_overlaps_nearest_3d: coordinate %r (lidar only)"
                                  % coordinate)
    return bbox_overlaps(nearest_bev(_box_tensor(bboxes1)), nearest_bev(_box_tensor(bboxes2)),
                         mode=mode, is_aligned=is_aligned)


class BboxOverlapsNearest3D:
    def __init__(self, coordinate="lidar"):
        assert coordinate in ["camera", "lidar", "depth"]
        self.coordinate = coordinate

    def __call__(self, bboxes1, bboxes2, mode="iou", is_aligned=False):
        return bbox_overlaps_nearest_3d(bboxes1, bboxes2, mode, is_aligned, self.coordinate)

    def __repr__(self):
        return self.__class__.__name__ + f"(coordinate={self.coordinate}"


# ---------------------------------------------------------------------------- assigner
class AssignResult:
    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, \
            max_overlaps, labels


class MaxIoUAssigner:
    """mmdet 2.x MaxIoUAssigner as the reference's anchor configs use it, in front of
    msmd_anchor_assign_f32.  The kernel's contract is match_low_quality=True,
    gt_max_assign_all=True, ignore_iof_thr < 0, a scalar neg_iou_thr and the nearest-BEV IoU;
    anything else is refused here."""

    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, gt_max_assign_all=True,
                 ignore_iof_thr=-1, ignore_wrt_candidates=True, match_low_quality=True,
                 gpu_assign_thr=-1, iou_calculator=dict(type="BboxOverlaps2D")):
        if isinstance(neg_iou_thr, (tuple, list)):
            raise NotImplementedError("MaxIoUAssigner: a tuple neg_iou_thr is not built")
        if ignore_iof_thr > 0:
            raise NotImplementedError("MaxIoUAssigner: ignore_iof_thr > 0 is not built")
        if not match_low_quality:
            raise NotImplementedError("MaxIoUAssigner: match_low_quality=False is not built")
        if not gt_max_assign_all:
            raise NotImplementedError("MaxIoUAssigner: gt_max_assign_all=False is not built")
        if isinstance(iou_calculator, dict):
            if iou_calculator.get("type") != "BboxOverlapsNearest3D":
                raise NotImplementedError("MaxIoUAssigner: iou_calculator %r (BboxOverlapsNearest3D "
                                          "only)" % (iou_calculator.get("type"),))
            args = {k: v for k, v in iou_calculator.items() if k != "type"}
            iou_calculator = BboxOverlapsNearest3D(**args)
        elif not isinstance(iou_calculator, BboxOverlapsNearest3D):
            raise NotImplementedError("MaxIoUAssigner: BboxOverlapsNearest3D only")
        if iou_calculator.coordinate != "lidar":
            raise NotImplementedError("MaxIoUAssigner: lidar coordinates only")
        self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou = pos_iou_thr, neg_iou_thr, min_pos_iou
        self.gt_max_assign_all, self.ignore_iof_thr = gt_max_assign_all, ignore_iof_thr
        self.ignore_wrt_candidates, self.match_low_quality = ignore_wrt_candidates, match_low_quality
        self.gpu_assign_thr, self.iou_calculator = gpu_assign_thr, iou_calculator

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        """One list of boxes against one list of ground truths -> AssignResult (gt_inds long:
        -1 / 0 / i + 1), on the device, nothing read back."""
        bboxes, gt_bboxes = _box_tensor(bboxes).float(), _box_tensor(gt_bboxes).float()
        n, g = bboxes.shape[0], gt_bboxes.shape[0]
        gt_offsets = torch.arange(2, device=bboxes.device, dtype=torch.int32) * g
        gt_bev = nearest_bev(gt_bboxes) if g else bboxes.new_zeros((0, 4))
        assigned, overlaps, _ = K.anchor_assign(
            nearest_bev(bboxes), [0, n], gt_bev, gt_offsets, [self.pos_iou_thr],
            [self.neg_iou_thr], [self.min_pos_iou])
        gt_inds = assigned.long()
        labels = None
        if gt_labels is not None:
            labels = gt_inds.new_full((n,), -1)
            if g:
                labels = torch.where(gt_inds > 0, gt_labels[(gt_inds - 1).clamp(min=0)], labels)
        return AssignResult(g, gt_inds, overlaps, labels=labels)


def build_assigner(cfg):
    if not isinstance(cfg, dict):
        return cfg
    args = dict(cfg)
    kind = args.pop("type")
    if kind != "MaxIoUAssigner":
        raise NotImplementedError("Anchor3DHead: assigner %r is not built" % kind)
    return MaxIoUAssigner(**args)


# ---------------------------------------------------------------------------- losses
class _SigmoidFocalSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, weights, gamma, alpha):
        total, grad = K.sigmoid_focal(logits, labels, weights, gamma, alpha,
                                      want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(grad)
        return total[0]

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return grad * grad_out, None, None, None, None


class FocalLoss(nn.Module):
    """mmdet FocalLoss(use_sigmoid=True) on msmd_sigmoid_focal_f32: the weighted sum comes from
    the kernel, the avg_factor division stays here on a device scalar."""

    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="mean",
                 loss_weight=1.0):
        super().__init__()
        if not use_sigmoid:
            raise NotImplementedError("Only sigmoid focal loss supported now.")
        if reduction != "mean":
            raise NotImplementedError("FocalLoss: reduction %r (mean only)" % reduction)
        self.use_sigmoid, self.gamma, self.alpha = use_sigmoid, gamma, alpha
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        pred = pred.float().contiguous()
        if weight is None:
            weight = pred.new_ones((pred.shape[0],))
        total = _SigmoidFocalSum.apply(pred, target.long().contiguous(),
                                       weight.float().contiguous(), self.gamma, self.alpha)
        if avg_factor is None:
            avg_factor = pred.numel()
        return self.loss_weight * (total / avg_factor)


def _weighted_mean(loss, weight, avg_factor):
    """mmdet weight_reduce_loss(reduction='mean', avg_factor): the sum is taken in float64."""
    if weight is not None:
        loss = loss * weight
    if avg_factor is None:
        return loss.mean()
    return (loss.double().sum() / avg_factor).to(loss.dtype)


def _elementwise(loss, weight, reduction, override):
    """mmdet's reduction_override='none' (FreeAnchor3DHead's positive side): the weighted loss,
    not reduced.  -> None when the class's own reduction applies."""
    if override is None or override == reduction:
        return None
    if override != "none":
        raise NotImplementedError("reduction_override %r (None or 'none')" % (override,))
    return loss if weight is None else loss * weight


class SmoothL1Loss(nn.Module):
    def __init__(self, beta=1.0, reduction="mean", loss_weight=1.0):
        super().__init__()
        assert reduction == "mean" and beta > 0
        self.beta, self.reduction, self.loss_weight = beta, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        diff = torch.abs(pred - target)
        loss = torch.where(diff < self.beta, 0.5 * diff * diff / self.beta, diff - 0.5 * self.beta)
        each = _elementwise(loss, weight, self.reduction, reduction_override)
        if each is not None:
            return self.loss_weight * each
        return self.loss_weight * _weighted_mean(loss, weight, avg_factor)


class CrossEntropyLoss(nn.Module):
    """mmdet CrossEntropyLoss, the softmax form (the direction classifier's)."""

    def __init__(self, use_sigmoid=False, use_mask=False, reduction="mean", class_weight=None,
                 loss_weight=1.0):
        super().__init__()
        if use_sigmoid or use_mask or class_weight is not None or reduction != "mean":
            raise NotImplementedError("CrossEntropyLoss: the plain softmax form only")
        self.use_sigmoid, self.reduction, self.loss_weight = use_sigmoid, reduction, loss_weight

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None):
        loss = F.cross_entropy(cls_score, label, reduction="none")
        if weight is not None:
            weight = weight.float()
        each = _elementwise(loss, weight, self.reduction, reduction_override)
        if each is not None:
            return self.loss_weight * each
        return self.loss_weight * _weighted_mean(loss, weight, avg_factor)


_LOSSES = {"FocalLoss": FocalLoss, "SmoothL1Loss": SmoothL1Loss,
           "CrossEntropyLoss": CrossEntropyLoss}


def build_loss(cfg):
    if not isinstance(cfg, dict):
        return cfg
    args = dict(cfg)
    kind = args.pop("type")
    if kind not in _LOSSES:
        raise NotImplementedError("Anchor3DHead: loss %r is not built" % kind)
    return _LOSSES[kind](**args)


# ---------------------------------------------------------------------------- NMS
def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def multiclass_nms_batched(bboxes_for_nms, scores, score_thr, max_num, use_rotate_nms, nms_thr):
    """box3d_multiclass_nms for a whole batch, with no host read.
    bboxes_for_nms [B, M, 5] xyxyr, scores [B, M, C] (foreground classes only).  Per (sample,
    class): score > score_thr, stable descending sort (equal scores keep input order), NMS;
    per sample the classes in order, then, when more than max_num survive, the max_num best by
    score (stable).
    -> rows long [B, C * M] (candidate index in [0, M), front-packed in output order), labels
       long [B, C * M], out_scores [B, C * M], count long [B] (valid entries per sample)."""
    B, M, C = scores.shape
    dev = scores.device
    if M > K.NMS_MAX_SEGMENT:
        raise ValueError("multiclass NMS handles at most %d candidates per class (got %d)"
                         % (K.NMS_MAX_SEGMENT, M))
    if B * C == 0 or M == 0:
        empty = torch.zeros((B, 0), dtype=torch.long, device=dev)
        return empty, empty, scores.new_zeros((B, 0)), torch.zeros((B,), dtype=torch.long,
                                                                   device=dev)
    per_class = scores.permute(0, 2, 1).reshape(B * C, M)
    valid = per_class > score_thr
    counts = valid.sum(1)
    key = torch.where(valid, per_class, torch.full_like(per_class, -math.inf))
    order = torch.sort(key, dim=1, descending=True, stable=True)[1]            # [S, M]
    boxes = bboxes_for_nms.float()[:, None].expand(B, C, M, 5).reshape(B * C, M, 5)
    sorted_boxes = boxes.gather(1, order[:, :, None].expand(-1, -1, 5)).reshape(-1, 5).contiguous()
    offsets = torch.arange(B * C + 1, device=dev, dtype=torch.int32) * M
    thresh = torch.full((B * C,), float(nms_thr), dtype=torch.float32, device=dev)
    keep, _ = K.nms_segments("rotate" if use_rotate_nms else "normal", sorted_boxes, offsets,
                             thresh, M)
    live = (keep >= 0) & (keep < counts[:, None])          # rows past a list's count are padding
    cand = order.gather(1, keep.clamp(min=0))              # candidate index of every kept slot
    cand_scores = per_class.gather(1, cand)
    live, cand, cand_scores = (t.view(B, C * M) for t in (live, cand, cand_scores))
    labels = torch.arange(C, device=dev).repeat_interleave(M)[None].expand(B, -1)
    kept = live.sum(1)
    # class order (front-pack the live slots), or the max_num best by score
    by_class = torch.sort((~live).to(torch.uint8), dim=1, stable=True)[1]
    packed_scores = torch.where(live, cand_scores, torch.full_like(cand_scores, -math.inf))
    packed_scores = packed_scores.gather(1, by_class)
    by_score = by_class.gather(1, torch.sort(packed_scores, dim=1, descending=True,
                                             stable=True)[1])
    pick = torch.where((kept > max_num)[:, None], by_score, by_class)
    count = kept.clamp(max=max_num)
    return cand.gather(1, pick), labels.gather(1, pick), cand_scores.gather(1, pick), count


def box3d_multiclass_nms(mlvl_bboxes, mlvl_bboxes_for_nms, mlvl_scores, score_thr, max_num, cfg,
                         mlvl_dir_scores=None):
    """box3d_nms.py:8-88 for one sample (scores carry the padded background column) on the
    batched kernel path.  Equal scores keep input order."""
    rows, labels, scores, count = multiclass_nms_batched(
        mlvl_bboxes_for_nms[None], mlvl_scores[None, :, :-1], score_thr, max_num,
        _get(cfg, "use_rotate_nms"), _get(cfg, "nms_thr"))
    n = int(count[0])
    rows, labels, scores = rows[0, :n], labels[0, :n], scores[0, :n]
    bboxes = mlvl_bboxes[rows]
    if mlvl_dir_scores is not None:
        dir_scores = mlvl_dir_scores[rows]
    else:
        dir_scores = mlvl_scores.new_zeros((0,)) if n == 0 else []
    return bboxes, scores, labels, dir_scores


# ---------------------------------------------------------------------------- the head
@HEADS.register_module()
class Anchor3DHead(nn.Module):
    """anchor3d_head.py:16-510 with AnchorTrainMixin (train_mixins.py)."""

    def __init__(self, num_classes, in_channels, train_cfg, test_cfg, feat_channels=256,
                 use_direction_classifier=True,
                 anchor_generator=dict(type="Anchor3DRangeGenerator",
                                       range=[0, -39.68, -1.78, 69.12, 39.68, -1.78], strides=[2],
                                       sizes=[[1.6, 3.9, 1.56]], rotations=[0, 1.57],
                                       custom_values=[], reshape_out=False),
                 assigner_per_size=False, assign_per_class=False, diff_rad_by_sin=True,
                 dir_offset=0, dir_limit_offset=1,
                 bbox_coder=dict(type="DeltaXYZWLHRBBoxCoder"),
                 loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=2.0),
                 loss_dir=dict(type="CrossEntropyLoss", loss_weight=0.2)):
        super().__init__()
        self.in_channels, self.num_classes, self.feat_channels = in_channels, num_classes, \
            feat_channels
        self.diff_rad_by_sin = diff_rad_by_sin
        self.use_direction_classifier = use_direction_classifier
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.assigner_per_size, self.assign_per_class = assigner_per_size, assign_per_class
        self.dir_offset, self.dir_limit_offset = dir_offset, dir_limit_offset
        self.fp16_enabled = False
        self.anchor_generator = build_anchor_generator(anchor_generator)
        self.num_anchors = self.anchor_generator.num_base_anchors
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.box_code_size = self.bbox_coder.code_size
        self.use_sigmoid_cls = loss_cls.get("use_sigmoid", False)
        self.sampling = loss_cls["type"] not in ["FocalLoss", "GHMC"]
        if self.sampling:
            raise NotImplementedError("Anchor3DHead: loss_cls %r needs a bbox_sampler, which is "
                                      "not built (FocalLoss only)" % loss_cls["type"])
        if not self.use_sigmoid_cls:
            raise NotImplementedError("Anchor3DHead: the softmax classification branch "
                                      "(use_sigmoid=False) is not built")
        self.loss_cls = build_loss(loss_cls)
        self.loss_bbox = build_loss(loss_bbox)
        self.loss_dir = build_loss(loss_dir)
        self._init_layers()
        self._init_assigner_sampler()
        self._const = {}

    def _init_assigner_sampler(self):
        if self.train_cfg is None:
            return
        assigner = _get(self.train_cfg, "assigner")
        if isinstance(assigner, dict):
            self.bbox_assigner = build_assigner(assigner)
        elif isinstance(assigner, list):
            self.bbox_assigner = [build_assigner(res) for res in assigner]

    def _init_layers(self):
        self.cls_out_channels = self.num_anchors * self.num_classes
        self.conv_cls = nn.Conv2d(self.feat_channels, self.cls_out_channels, 1)
        self.conv_reg = nn.Conv2d(self.feat_channels, self.num_anchors * self.box_code_size, 1)
        if self.use_direction_classifier:
            self.conv_dir_cls = nn.Conv2d(self.feat_channels, self.num_anchors * 2, 1)

    def init_weights(self):
        """bias_init_with_prob(0.01) / normal_init(std=0.01) of mmcv."""
        bias_cls = float(-np.log((1 - 0.01) / 0.01))
        nn.init.normal_(self.conv_cls.weight, 0, 0.01)
        nn.init.constant_(self.conv_cls.bias, bias_cls)
        nn.init.normal_(self.conv_reg.weight, 0, 0.01)
        nn.init.constant_(self.conv_reg.bias, 0)

    def forward_single(self, x):
        cls_score = self.conv_cls(x)
        bbox_pred = self.conv_reg(x)
        dir_cls_preds = self.conv_dir_cls(x) if self.use_direction_classifier else None
        return cls_score, bbox_pred, dir_cls_preds

    def forward(self, feats):
        """feats: list of levels -> (cls_scores, bbox_preds, dir_cls_preds), a list per level
        each (multi_apply(self.forward_single, feats))."""
        return tuple(map(list, zip(*[self.forward_single(x) for x in feats])))

    def get_anchors(self, featmap_sizes, input_metas, device="cuda"):
        multi_level_anchors = self.anchor_generator.grid_anchors(featmap_sizes, device=device)
        return [multi_level_anchors for _ in range(len(input_metas))]

    def _constant(self, key, make):
        if key not in self._const:
            self._const[key] = make()
        return self._const[key]

    # ------------------------------------------------------------------ targets
    def _anchor_plan(self, levels):
        """What depends on the anchors only, built once per anchor set: the anchors in segment
        order (one run per assigner), their nearest-BEV boxes, the run boundaries and the
        permutation back to the reference's order."""
        assigners = self.bbox_assigner if isinstance(self.bbox_assigner, list) \
            else [self.bbox_assigner]
        key = ("plan",) + tuple((tuple(a.shape), a.data_ptr()) for a in levels) + tuple(
            (a.pos_iou_thr, a.neg_iou_thr, a.min_pos_iou) for a in assigners)
        if key in self._const:
            return self._const[key]
        code = self.box_code_size
        dev = levels[0].device
        if isinstance(self.bbox_assigner, list):
            if len(levels) != 1 or levels[0].dim() != 6:
                raise NotImplementedError("a list of assigners takes one level of anchors "
                                          "[1, H, W, sizes, rotations, code] (reshape_out=False)")
            anchors = levels[0]
            sizes, rots = anchors.size(-3), anchors.size(-2)
            assert len(self.bbox_assigner) == sizes
            cells = anchors.size(0) * anchors.size(1) * anchors.size(2)
            flat = anchors.reshape(cells, sizes, rots, code).permute(1, 0, 2, 3)
            flat = flat.reshape(-1, code).contiguous()
            bounds = [g * cells * rots for g in range(sizes + 1)]
            g, c, r = torch.meshgrid(torch.arange(sizes), torch.arange(cells), torch.arange(rots),
                                     indexing="ij")
            dest = ((c * sizes + g) * rots + r).reshape(-1).to(dev, torch.int32)
            assigners = self.bbox_assigner
            num_level_anchors = [flat.shape[0]]
        else:
            flat = torch.cat([a.reshape(-1, code) for a in levels]).contiguous()
            bounds, dest, assigners = [0, flat.shape[0]], None, [self.bbox_assigner]
            num_level_anchors = [a.reshape(-1, code).size(0) for a in levels]
        plan = dict(anchors=flat, bev=nearest_bev(flat).contiguous(), bounds=bounds, dest=dest,
                    pos=[a.pos_iou_thr for a in assigners], neg=[a.neg_iou_thr for a in assigners],
                    min_pos=[a.min_pos_iou for a in assigners],
                    num_level_anchors=num_level_anchors,
                    levels=levels)        # keeps the storage the key names alive
        self._const[key] = plan
        return plan

    def _gt_lists(self, plan, boxes, labels, dev):
        """The per-segment ground-truth lists of samples boxes[0..n), on the device: segment
        (b, g) holds sample b's boxes, or under assign_per_class those with label g (a stable
        partition).  -> (gt_index int32 | None, gt_offsets int32 [S + 1])"""
        groups = len(plan["bounds"]) - 1
        segments = len(boxes) * groups
        start, index, seg = 0, [], []
        for b, bx in enumerate(boxes):
            n = bx.shape[0]
            rows = torch.arange(start, start + n, device=dev)
            if self.assign_per_class and groups > 1:
                lab = labels[b]
                known = (lab >= 0) & (lab < groups)
                index.append(rows)
                seg.append(torch.where(known, b * groups + lab.clamp(0, groups - 1),
                                       torch.full_like(lab, segments)))
            else:
                index.append(rows.repeat(groups))
                seg.append((b * groups + torch.arange(groups, device=dev)).repeat_interleave(n))
            start += n
        index, seg = torch.cat(index), torch.cat(seg)
        if self.assign_per_class and groups > 1:
            seg, order = torch.sort(seg, stable=True)
            index = index[order]
        counts = torch.zeros(segments + 2, dtype=torch.long, device=dev)
        counts.index_add_(0, seg + 1, torch.ones_like(seg))
        offsets = torch.cumsum(counts, 0)[:segments + 1].int()
        if groups == 1:
            return None, offsets
        return index.int(), offsets

    def anchor_target_3d(self, anchor_list, gt_bboxes_list, input_metas, gt_bboxes_ignore_list=None,
                         gt_labels_list=None, label_channels=1, num_classes=1, sampling=True):
        """train_mixins.py:11-99 for the whole batch, every level and every assigner, with no
        host read.  -> (labels_list, label_weights_list, bbox_targets_list, bbox_weights_list,
        dir_targets_list, dir_weights_list, num_total_pos, num_total_neg): per level [B, n] /
        [B, n, code] tensors; the two totals are device scalars, each sample counted as
        max(n, 1) as the reference does."""
        if sampling:
            raise NotImplementedError("anchor_target_3d: sampling is not built")
        if gt_labels_list is None:
            raise NotImplementedError("anchor_target_3d needs gt_labels_list")
        plan = self._anchor_plan(list(anchor_list[0]))
        dev = plan["anchors"].device
        code, rows = self.box_code_size, plan["anchors"].shape[0]
        groups = len(plan["bounds"]) - 1
        boxes = [_box_tensor(b).to(dev).float().reshape(-1, code) for b in gt_bboxes_list]
        labels = [l.to(dev).long() for l in gt_labels_list]
        B = len(boxes)
        per_call = max(K.ANCHOR_MAX_SEGMENTS // groups, 1)
        pos_weight = _get(self.train_cfg, "pos_weight", -1)
        out, num_pos, num_neg = [], [], []
        for b0 in range(0, B, per_call):
            bx, lb = boxes[b0:b0 + per_call], labels[b0:b0 + per_call]
            nb = len(bx)
            gt = torch.cat(bx)
            gt_labels = torch.cat(lb)
            gt_index, gt_offsets = self._gt_lists(plan, bx, lb, dev)
            gt_bev = nearest_bev(gt) if gt.shape[0] else gt.new_zeros((0, 4))
            offs = [b * rows + v for b in range(nb) for v in plan["bounds"][:-1]] + [nb * rows]
            assigned, _, pos = K.anchor_assign(
                plan["bev"], offs, gt_bev, gt_offsets, plan["pos"] * nb, plan["neg"] * nb,
                plan["min_pos"] * nb, gt_index=gt_index)
            tg = K.anchor_targets(assigned, plan["anchors"], offs, gt, gt_labels, gt_offsets,
                                  num_classes, pos_weight, self.dir_offset, gt_index=gt_index,
                                  dest=plan["dest"])
            out.append([t.view(nb, rows, *t.shape[1:]) for t in tg])
            num_pos.append(pos.view(nb, groups).sum(1))
            num_neg.append((assigned.view(nb, rows) == 0).sum(1))
        tensors = [torch.cat(parts) if len(out) > 1 else parts[0] for parts in zip(*out)]
        num_total_pos = torch.cat(num_pos).clamp(min=1).sum()
        num_total_neg = torch.cat(num_neg).clamp(min=1).sum()
        per_level = []
        for t in tensors:                       # images_to_levels
            start, levels = 0, []
            for n in plan["num_level_anchors"]:
                levels.append(t[:, start:start + n])
                start += n
            per_level.append(levels)
        return (*per_level, num_total_pos, num_total_neg)

    # ------------------------------------------------------------------ loss
    def loss_single(self, cls_score, bbox_pred, dir_cls_preds, labels, label_weights, bbox_targets,
                    bbox_weights, dir_targets, dir_weights, num_total_samples):
        """anchor3d_head.py:188-272.  The positives are not gathered: the box and direction
        weights are zero off them, so the weighted sums over all anchors are the reference's
        sums over the positives.  Its num_pos == 0 branch (pos_bbox_pred.sum(), an empty sum
        that keeps the graph connected) is selected on the device."""
        if num_total_samples is None:
            num_total_samples = int(cls_score.shape[0])
        labels = labels.reshape(-1)
        label_weights = label_weights.reshape(-1)
        cls_score = cls_score.permute(0, 2, 3, 1).reshape(-1, self.num_classes)
        loss_cls = self.loss_cls(cls_score, labels, label_weights, avg_factor=num_total_samples)

        bbox_pred = bbox_pred.permute(0, 2, 3, 1).reshape(-1, self.box_code_size)
        bbox_targets = bbox_targets.reshape(-1, self.box_code_size)
        bbox_weights = bbox_weights.reshape(-1, self.box_code_size)
        pos = (labels >= 0) & (labels < self.num_classes)
        has_pos = pos.any()
        pos_f = pos.to(bbox_pred.dtype)
        code_weight = _get(self.train_cfg, "code_weight", None)
        if code_weight:
            cw = self._constant(("code_weight", bbox_pred.device), lambda: torch.tensor(
                code_weight, dtype=torch.float32, device=bbox_pred.device))
            bbox_weights = bbox_weights * cw
        if self.diff_rad_by_sin:
            bbox_pred_s, bbox_targets = self.add_sin_difference(bbox_pred, bbox_targets)
        else:
            bbox_pred_s = bbox_pred
        loss_bbox = self.loss_bbox(bbox_pred_s, bbox_targets, bbox_weights,
                                   avg_factor=num_total_samples)
        loss_bbox = torch.where(has_pos, loss_bbox, (bbox_pred * pos_f[:, None]).sum())
        loss_dir = None
        if self.use_direction_classifier:
            dir_cls_preds = dir_cls_preds.permute(0, 2, 3, 1).reshape(-1, 2)
            loss_dir = self.loss_dir(dir_cls_preds, dir_targets.reshape(-1), dir_weights.reshape(-1),
                                     avg_factor=num_total_samples)
            loss_dir = torch.where(has_pos, loss_dir, (dir_cls_preds * pos_f[:, None]).sum())
        return loss_cls, loss_bbox, loss_dir

    @staticmethod
    def add_sin_difference(boxes1, boxes2):
        rad_pred_encoding = torch.sin(boxes1[..., 6:7]) * torch.cos(boxes2[..., 6:7])
        rad_tg_encoding = torch.cos(boxes1[..., 6:7]) * torch.sin(boxes2[..., 6:7])
        boxes1 = torch.cat([boxes1[..., :6], rad_pred_encoding, boxes1[..., 7:]], dim=-1)
        boxes2 = torch.cat([boxes2[..., :6], rad_tg_encoding, boxes2[..., 7:]], dim=-1)
        return boxes1, boxes2

    def loss(self, cls_scores, bbox_preds, dir_cls_preds, gt_bboxes, gt_labels, input_metas=None,
             gt_bboxes_ignore=None):
        """anchor3d_head.py:299-368 -> dict(loss_cls, loss_bbox, loss_dir), a list per level."""
        featmap_sizes = [featmap.size()[-2:] for featmap in cls_scores]
        assert len(featmap_sizes) == self.anchor_generator.num_levels
        device = cls_scores[0].device
        input_metas = input_metas if input_metas is not None else [None] * len(gt_bboxes)
        anchor_list = self.get_anchors(featmap_sizes, input_metas, device=device)
        label_channels = self.cls_out_channels if self.use_sigmoid_cls else 1
        (labels_list, label_weights_list, bbox_targets_list, bbox_weights_list, dir_targets_list,
         dir_weights_list, num_total_pos, num_total_neg) = self.anchor_target_3d(
            anchor_list, gt_bboxes, input_metas, gt_bboxes_ignore_list=gt_bboxes_ignore,
            gt_labels_list=gt_labels, num_classes=self.num_classes, label_channels=label_channels,
            sampling=self.sampling)
        num_total_samples = num_total_pos.float()
        if dir_cls_preds is None or not self.use_direction_classifier:
            dir_cls_preds = [None] * len(cls_scores)
        losses = [self.loss_single(c.float(), b.float(), None if d is None else d.float(), *t,
                                   num_total_samples=num_total_samples)
                  for c, b, d, *t in zip(cls_scores, bbox_preds, dir_cls_preds, labels_list,
                                         label_weights_list, bbox_targets_list, bbox_weights_list,
                                         dir_targets_list, dir_weights_list)]
        losses_cls, losses_bbox, losses_dir = map(list, zip(*losses))
        return dict(loss_cls=losses_cls, loss_bbox=losses_bbox, loss_dir=losses_dir)

    # ------------------------------------------------------------------ inference
    def _check_nms_bound(self, cfg, level_sizes):
        nms_pre = _get(cfg, "nms_pre", -1)
        if nms_pre <= 0 or len(level_sizes) * nms_pre > K.NMS_MAX_SEGMENT:
            raise NotImplementedError(
                "Anchor3DHead.get_bboxes: nms_pre=%r over %d levels can exceed the NMS kernel's "
                "%d candidates per class" % (nms_pre, len(level_sizes), K.NMS_MAX_SEGMENT))
        return nms_pre

    def get_bboxes(self, cls_scores, bbox_preds, dir_cls_preds, input_metas, cfg=None,
                   rescale=False):
        """anchor3d_head.py:370-510 for the whole batch: per level the nms_pre top-k and the
        decode, then ONE multiclass NMS call over every (sample, class) list, the direction fix,
        and one host read (the kept counts).  -> per sample (bboxes, scores, labels); bboxes is
        wrapped in input_metas[i]['box_type_3d'] when that is given."""
        cfg = self.test_cfg if cfg is None else cfg
        assert len(cls_scores) == len(bbox_preds) == len(dir_cls_preds)
        featmap_sizes = [c.shape[-2:] for c in cls_scores]
        device = cls_scores[0].device
        code, B = self.box_code_size, cls_scores[0].shape[0]
        mlvl_anchors = [a.reshape(-1, code) for a in
                        self.anchor_generator.grid_anchors(featmap_sizes, device=device)]
        nms_pre = self._check_nms_bound(cfg, featmap_sizes)
        mlvl_bboxes, mlvl_scores, mlvl_dir = [], [], []
        for cls_score, bbox_pred, dir_cls_pred, anchors in zip(cls_scores, bbox_preds,
                                                               dir_cls_preds, mlvl_anchors):
            assert cls_score.size()[-2:] == bbox_pred.size()[-2:] == dir_cls_pred.size()[-2:]
            dir_cls_pred = dir_cls_pred.detach().permute(0, 2, 3, 1).reshape(B, -1, 2)
            dir_cls_score = torch.max(dir_cls_pred, dim=-1)[1]
            scores = cls_score.detach().permute(0, 2, 3, 1).reshape(B, -1, self.num_classes)
            scores = scores.sigmoid()
            bbox_pred = bbox_pred.detach().permute(0, 2, 3, 1).reshape(B, -1, code)
            anchors = anchors[None].expand(B, -1, -1)
            if scores.shape[1] > nms_pre:
                max_scores, _ = scores.max(dim=2)
                _, topk_inds = max_scores.topk(nms_pre, dim=1)
                anchors = anchors.gather(1, topk_inds[:, :, None].expand(-1, -1, code))
                bbox_pred = bbox_pred.gather(1, topk_inds[:, :, None].expand(-1, -1, code))
                scores = scores.gather(1, topk_inds[:, :, None].expand(-1, -1, self.num_classes))
                dir_cls_score = dir_cls_score.gather(1, topk_inds)
            mlvl_bboxes.append(self.bbox_coder.decode(anchors, bbox_pred))
            mlvl_scores.append(scores)
            mlvl_dir.append(dir_cls_score)
        mlvl_bboxes = torch.cat(mlvl_bboxes, dim=1)                     # [B, M, code]
        mlvl_scores = torch.cat(mlvl_scores, dim=1)
        mlvl_dir = torch.cat(mlvl_dir, dim=1)
        # LiDARInstance3DBoxes.bev, column by column (a list index would be copied from the host)
        for_nms = xywhr2xyxyr(torch.stack([mlvl_bboxes[..., k] for k in (0, 1, 3, 4, 6)], dim=-1))
        rows, labels, scores, count = multiclass_nms_batched(
            for_nms, mlvl_scores, _get(cfg, "score_thr", 0), _get(cfg, "max_num"),
            _get(cfg, "use_rotate_nms"), _get(cfg, "nms_thr"))
        bboxes = mlvl_bboxes.gather(1, rows[:, :, None].expand(-1, -1, code)).clone()
        dir_scores = mlvl_dir.gather(1, rows)
        dir_rot = limit_period(bboxes[..., 6] - self.dir_offset, self.dir_limit_offset, np.pi)
        bboxes[..., 6] = dir_rot + self.dir_offset + np.pi * dir_scores.to(bboxes.dtype)
        result_list = []
        for i, n in enumerate(count.tolist()):                          # the one host read
            b = bboxes[i, :n]
            meta = input_metas[i] if input_metas is not None else None
            if meta is not None and "box_type_3d" in meta:
                b = meta["box_type_3d"](b, box_dim=code)
            result_list.append((b, scores[i, :n], labels[i, :n]))
        return result_list

    def get_bboxes_single(self, cls_scores, bbox_preds, dir_cls_preds, mlvl_anchors, input_meta,
                          cfg=None, rescale=False):
        """anchor3d_head.py:421-510: one sample's [C, H, W] maps (the anchors come from the
        generator's cache; mlvl_anchors is accepted for the reference's signature)."""
        return self.get_bboxes([c[None] for c in cls_scores], [b[None] for b in bbox_preds],
                               [d[None] for d in dir_cls_preds], [input_meta], cfg, rescale)[0]
