"""FreeAnchor3DHead (mmdet3d/models/dense_heads/free_anchor3d_head.py): Anchor3DHead with the
FreeAnchor training loss (https://arxiv.org/abs/1909.02466) -- the reference's constructor
arguments, `forward`, `get_bboxes` and state-dict keys are Anchor3DHead's, unchanged.

Only `loss` differs, and where the reference builds, per sample, two [num_gt, num_anchors] IoU
matrices, a torch.topk over one and a sparse_coo_tensor / sparse.sum / nonzero detour over the
other, this one makes four library calls for the whole batch (csrc/free_anchor.hip), none of
which forms such a matrix, and reads nothing back:

  negative side  msmd_decode_nearest_bev_f32 -> msmd_free_anchor_box_prob_f32 (no_grad, as in
                 the reference) -> msmd_free_anchor_negative_f32 behind an autograd function.
  positive side  msmd_free_anchor_topk once for all ground truths (the anchors are shared by
                 the samples); the [G, k, .] work -- gathers, encode, get_direction_target,
                 smooth-L1, direction cross-entropy, exp, the mean-max bag -- stays in torch on
                 tensors of a few thousand rows.

ONE DELIBERATE DEVIATION.  The reference writes the sin-difference encoding back in place,
`bbox_preds_[matched], ... = add_sin_difference(bbox_preds_[matched], ...)`
(free_anchor3d_head.py:203-206), through an index that repeats whenever an anchor sits in two
bags of a sample; which write survives is undefined on a GPU, and the survivor is then used for
both bags.  This head is the functional form: every (ground truth, anchor) pair uses its own
encoding.  For pairwise disjoint bags the two are equal.

Ties of the top-k (the normal case: every anchor of one size inside a large box has the same
IoU, most pairs are exactly 0) go to the lower anchor index; torch.topk leaves them open.
"""
import numpy as np
import torch
from torch.nn import functional as F

from . import kernels as K
from .anchor_head import Anchor3DHead, _box_tensor, _get, limit_period, nearest_bev
from .registry import HEADS


class _NegativeBagSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, box_prob, gamma, alpha):
        total, grad = K.free_anchor_negative(logits, box_prob, gamma, alpha,
                                             want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(grad)
        return total[0]

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return grad * grad_out, None, None, None


def get_direction_target(anchors, reg_targets, dir_offset=0, num_bins=2):
    """train_mixins.py:317-346 with one_hot=False."""
    rot_gt = reg_targets[..., 6] + anchors[..., 6]
    offset_rot = limit_period(rot_gt - dir_offset, 0, 2 * np.pi)
    dir_cls_targets = torch.floor(offset_rot / (2 * np.pi / num_bins)).long()
    return torch.clamp(dir_cls_targets, min=0, max=num_bins - 1)


def _device_ints(values, device, dtype):
    """A short vector of host integers on the device without a host-to-device copy (which
    would wait for the stream): one fill per entry."""
    return torch.cat([torch.full((1,), int(v), dtype=dtype, device=device) for v in values])


@HEADS.register_module()
class FreeAnchor3DHead(Anchor3DHead):
    """free_anchor3d_head.py:11-282.  pre_anchor_topk: anchors per bag; bbox_thr: the threshold
    t1 of the saturated linear function; gamma, alpha: of the focal terms; everything else is
    Anchor3DHead's (its assigners, if the train_cfg names any, are not used).

    Deviation from the reference (see the module docstring): the sin-difference encoding is
    computed per (ground truth, anchor) pair, not written back through a repeating index."""

    def __init__(self, pre_anchor_topk=50, bbox_thr=0.6, gamma=2.0, alpha=0.5, **kwargs):
        super().__init__(**kwargs)
        self.pre_anchor_topk = pre_anchor_topk
        self.bbox_thr = bbox_thr
        self.gamma = gamma
        self.alpha = alpha

    def _bag_plan(self, levels):
        """What depends on the anchors only, once per anchor set: the anchors of all levels in
        the order of the flattened predictions, and their nearest-BEV boxes.  As with
        `_anchor_plan`, an entry is kept for the life of the head: every distinct set of
        feature-map sizes adds one (at the config's 420 000 anchors, code 9: 15 MB of anchors and
        7 MB of BEV boxes), so a training run with a few fixed input sizes holds a few."""
        key = ("bags",) + tuple((tuple(a.shape), a.data_ptr()) for a in levels)
        if key not in self._const:
            flat = torch.cat([a.reshape(-1, self.box_code_size) for a in levels]).float()
            flat = flat.contiguous()
            self._const[key] = dict(anchors=flat, bev=nearest_bev(flat).contiguous(),
                                    levels=levels)   # keeps the storage the key names alive
        return self._const[key]

    def positive_bag_loss(self, matched_cls_prob, matched_box_prob):
        """free_anchor3d_head.py:244-264: -alpha log(Mean-max(P_cls P_loc))."""
        matched_prob = matched_cls_prob * matched_box_prob
        weight = 1 / torch.clamp(1 - matched_prob, 1e-12, None)
        weight = weight / weight.sum(dim=1).unsqueeze(dim=-1)
        bag_prob = (weight * matched_prob).sum(dim=1).clamp(0, 1)
        return self.alpha * F.binary_cross_entropy(bag_prob, torch.ones_like(bag_prob),
                                                   reduction="none")

    def negative_bag_loss(self, cls_logits, box_prob):
        """free_anchor3d_head.py:266-282, summed, on the LOGITS [N, C] (the sigmoid is inside
        the kernel)."""
        return _NegativeBagSum.apply(cls_logits, box_prob, float(self.gamma), float(self.alpha))

    def loss(self, cls_scores, bbox_preds, dir_cls_preds, gt_bboxes, gt_labels, input_metas=None,
             gt_bboxes_ignore=None):
        """free_anchor3d_head.py:42-242 -> dict(positive_bag_loss, negative_bag_loss), for the
        whole batch at once and with no host read."""
        featmap_sizes = [featmap.size()[-2:] for featmap in cls_scores]
        assert len(featmap_sizes) == self.anchor_generator.num_levels
        dev = cls_scores[0].device
        input_metas = input_metas if input_metas is not None else [None] * len(gt_bboxes)
        plan = self._bag_plan(list(self.get_anchors(featmap_sizes, input_metas, device=dev)[0]))
        anchors = plan["anchors"]
        B, A, C, code = cls_scores[0].size(0), anchors.shape[0], self.num_classes, \
            self.box_code_size
        k = int(self.pre_anchor_topk)
        flatten = lambda maps, c: torch.cat(
            [m.float().permute(0, 2, 3, 1).reshape(B, -1, c) for m in maps], dim=1).reshape(B * A, c)
        cls_flat, bbox_flat = flatten(cls_scores, C), flatten(bbox_preds, code)

        boxes = [_box_tensor(b).to(dev).float().reshape(-1, code) for b in gt_bboxes]
        counts = [int(b.shape[0]) for b in boxes]
        assert len(boxes) == B
        num_pos = sum(counts)                              # known to the host
        gt = torch.cat(boxes)
        labels = torch.cat([l.to(dev).long().reshape(-1) for l in gt_labels])
        gt_offsets = _device_ints(np.cumsum([0] + counts), dev, torch.int32)
        gt_bev = nearest_bev(gt).contiguous() if num_pos else gt.new_zeros((0, 4))

        # ---- negative side: P{a_j in A+} and the focal term, all anchors of the batch
        with torch.no_grad():
            pred_bev = K.decode_nearest_bev(anchors, bbox_flat.detach())
            box_prob = K.free_anchor_box_prob(pred_bev, gt_bev, labels, gt_offsets, C, self.bbox_thr)
        negative_loss = self.negative_bag_loss(cls_flat, box_prob) / max(1, num_pos * k)

        # ---- positive side: the bags, [G, k] rows into the flattened predictions
        matched = K.free_anchor_topk(plan["bev"], gt_bev, k).long()                   # [G, k]
        sample = torch.cat([torch.full((n,), b, dtype=torch.long, device=dev)
                            for b, n in enumerate(counts)]) if B else labels
        rows = sample[:, None] * A + matched
        matched_cls_prob = torch.sigmoid(cls_flat)[rows, labels[:, None]]
        matched_anchors = anchors[matched]                                            # [G, k, code]
        targets = self.bbox_coder.encode(matched_anchors,
                                         gt.unsqueeze(dim=1).expand_as(matched_anchors))
        loss_dir = None
        if self.use_direction_classifier:
            dir_flat = flatten(dir_cls_preds, 2)
            dir_targets = get_direction_target(matched_anchors, targets, self.dir_offset)
            loss_dir = self.loss_dir(dir_flat[rows].transpose(-2, -1), dir_targets,
                                     reduction_override="none")
        matched_preds = bbox_flat[rows]
        if self.diff_rad_by_sin:                            # functional: one encoding per pair
            matched_preds, targets = self.add_sin_difference(matched_preds, targets)
        bbox_weights = matched_anchors.new_ones(matched_anchors.size())
        code_weight = _get(self.train_cfg, "code_weight", None)
        if code_weight:
            bbox_weights = bbox_weights * self._constant(
                ("code_weight", dev), lambda: torch.tensor(code_weight, dtype=torch.float32,
                                                           device=dev))
        loss_bbox = self.loss_bbox(matched_preds, targets, bbox_weights,
                                   reduction_override="none").sum(-1)
        if loss_dir is not None:
            loss_bbox = loss_bbox + loss_dir
        matched_box_prob = torch.exp(-loss_bbox)
        positive_loss = self.positive_bag_loss(matched_cls_prob, matched_box_prob).sum() \
            / max(1, num_pos)
        return dict(positive_bag_loss=positive_loss, negative_bag_loss=negative_loss)
