"""mmdet3d/models/losses/chamfer_distance.py on the matrix-free kernels of csrc/vote.hip.

The reference expands both sets to [B, N, M, C], applies the criterion and takes two
``torch.min``; autograd then runs back through the [B, N, M] matrix.  Here one autograd
function wraps msmd_chamfer_fwd_f32 / msmd_chamfer_bwd_f32: nothing of size N x M exists in
either direction.  The weights and the reduction stay in torch around it, so autograd handles
them.  Sets with C != 3 and CPU tensors (which the kernels refuse) take the reference's own
formulation, `chamfer_distance_expanded`.
"""
import torch
from torch import nn
from torch.nn import functional as F

from . import kernels as K

CRITERIA = {"smooth_l1": F.smooth_l1_loss, "l1": F.l1_loss, "l2": F.mse_loss}


def chamfer_distance_expanded(src, dst, criterion_mode="l2"):
    """chamfer_distance.py:50-55 as written -> (src2dst [B, N], dst2src [B, M], indices1,
    indices2)."""
    criterion = CRITERIA[criterion_mode]
    src_expand = src.unsqueeze(2).repeat(1, 1, dst.shape[1], 1)
    dst_expand = dst.unsqueeze(1).repeat(1, src.shape[1], 1, 1)
    distance = criterion(src_expand, dst_expand, reduction="none").sum(-1)
    src2dst, indices1 = torch.min(distance, dim=2)
    dst2src, indices2 = torch.min(distance, dim=1)
    return src2dst, dst2src, indices1, indices2


class _ChamferMin(torch.autograd.Function):
    """(src [B, N, 3], dst [B, M, 3]) -> (d1 [B, N], d2 [B, M], i1, i2)."""

    @staticmethod
    def forward(ctx, src, dst, mode):
        src, dst = src.contiguous(), dst.contiguous()
        d1, i1, d2, i2 = K.chamfer_forward(src, dst, mode)
        ctx.save_for_backward(src, dst, i1, i2)
        ctx.mode = mode
        ctx.mark_non_differentiable(i1, i2)
        return d1, d2, i1, i2

    @staticmethod
    def backward(ctx, g1, g2, _i1, _i2):
        src, dst, i1, i2 = ctx.saved_tensors
        g1 = torch.zeros(i1.shape, dtype=src.dtype, device=src.device) if g1 is None else g1
        g2 = torch.zeros(i2.shape, dtype=src.dtype, device=src.device) if g2 is None else g2
        grad_src, grad_dst = K.chamfer_backward(
            src, dst, g1.contiguous(), g2.contiguous(), i1, i2, ctx.mode,
            want_src=ctx.needs_input_grad[0], want_dst=ctx.needs_input_grad[1])
        return grad_src, grad_dst, None


def chamfer_min(src, dst, criterion_mode="l2"):
    """The unweighted, unreduced pair of minima and their indices: (src2dst [B, N], dst2src
    [B, M], indices1 long [B, N], indices2 long [B, M])."""
    if criterion_mode not in CRITERIA:
        raise NotImplementedError
    if src.dim() != 3 or dst.dim() != 3:
        raise ValueError("chamfer_distance: src [B, N, C] and dst [B, M, C] expected")
    on_kernel = (src.is_cuda and dst.is_cuda and src.shape[2] == 3 and dst.shape[2] == 3
                 and src.dtype == torch.float32 and dst.dtype == torch.float32)
    if not on_kernel:
        return chamfer_distance_expanded(src, dst, criterion_mode)
    return _ChamferMin.apply(src, dst, criterion_mode)


def chamfer_distance(src, dst, src_weight=1.0, dst_weight=1.0, criterion_mode="l2",
                     reduction="mean"):
    """chamfer_distance.py:8-71: -> (loss_src, loss_dst, indices1, indices2)."""
    src2dst, dst2src, indices1, indices2 = chamfer_min(src, dst, criterion_mode)
    loss_src = src2dst * src_weight
    loss_dst = dst2src * dst_weight
    if reduction == "sum":
        loss_src, loss_dst = torch.sum(loss_src), torch.sum(loss_dst)
    elif reduction == "mean":
        loss_src, loss_dst = torch.mean(loss_src), torch.mean(loss_dst)
    elif reduction != "none":
        raise NotImplementedError
    return loss_src, loss_dst, indices1, indices2


class ChamferDistance(nn.Module):
    """chamfer_distance.py:74-146."""

    def __init__(self, mode="l2", reduction="mean", loss_src_weight=1.0, loss_dst_weight=1.0):
        super().__init__()
        assert mode in ["smooth_l1", "l1", "l2"]
        assert reduction in ["none", "sum", "mean"]
        self.mode = mode
        self.reduction = reduction
        self.loss_src_weight = loss_src_weight
        self.loss_dst_weight = loss_dst_weight

    def forward(self, source, target, src_weight=1.0, dst_weight=1.0, reduction_override=None,
                return_indices=False, **kwargs):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        loss_source, loss_target, indices1, indices2 = chamfer_distance(
            source, target, src_weight, dst_weight, self.mode, reduction)
        loss_source = loss_source * self.loss_src_weight
        loss_target = loss_target * self.loss_dst_weight
        if return_indices:
            return loss_source, loss_target, indices1, indices2
        return loss_source, loss_target


def weight_reduce_loss(loss, weight=None, reduction="mean", avg_factor=None):
    """mmdet/models/losses/utils.py weight_reduce_loss."""
    if weight is not None:
        loss = loss * weight
    if avg_factor is None:
        if reduction == "mean":
            return loss.mean()
        return loss.sum() if reduction == "sum" else loss
    if reduction == "mean":
        return loss.sum() / avg_factor
    if reduction != "none":
        raise ValueError('avg_factor can not be used with reduction="sum"')
    return loss


class CrossEntropyLoss(nn.Module):
    """mmdet CrossEntropyLoss, with class_weight and every reduction (the VoteNet configs use
    reduction='sum' and, for objectness, class_weight=[0.2, 0.8]).  use_sigmoid=True (3DSSD's
    centerness loss) is mmdet's binary_cross_entropy: binary_cross_entropy_with_logits on a
    float target of the prediction's shape, then weight, reduction, loss_weight.
    anchor_head.py keeps its own mean-only form: it takes the weighted sum over ~10^5 anchors in
    float64, which these per-proposal sums do not need."""

    def __init__(self, use_sigmoid=False, use_mask=False, reduction="mean", class_weight=None,
                 loss_weight=1.0):
        super().__init__()
        if use_mask:
            raise NotImplementedError("CrossEntropyLoss: the mask form is not built")
        self.use_sigmoid, self.use_mask = use_sigmoid, use_mask
        self.reduction, self.loss_weight, self.class_weight = reduction, loss_weight, class_weight

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None,
                **kwargs):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        # (uploaded without blocking: Tensor.new_tensor on a device tensor is a blocking copy)
        class_weight = None if self.class_weight is None else torch.tensor(
            self.class_weight, dtype=cls_score.dtype).to(cls_score.device, non_blocking=True)
        if weight is not None:
            weight = weight.float()
        if self.use_sigmoid:
            # mmdet binary_cross_entropy (cross_entropy_loss.py): its label expansion serves class
            # indices; 3DSSD passes a target of the prediction's shape, which goes through as is
            if cls_score.dim() != label.dim():
                raise NotImplementedError("CrossEntropyLoss(use_sigmoid=True): the target must "
                                          "have the prediction's shape")
            loss = F.binary_cross_entropy_with_logits(cls_score, label.float(),
                                                      pos_weight=class_weight, reduction="none")
        else:
            loss = F.cross_entropy(cls_score, label, weight=class_weight, reduction="none")
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction, avg_factor)


class SmoothL1Loss(nn.Module):
    """mmdet SmoothL1Loss (smooth_l1_loss under weighted_loss)."""

    def __init__(self, beta=1.0, reduction="mean", loss_weight=1.0):
        super().__init__()
        assert beta > 0
        self.beta, self.reduction, self.loss_weight = beta, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None,
                **kwargs):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        assert pred.size() == target.size() and target.numel() > 0
        diff = torch.abs(pred - target)
        loss = torch.where(diff < self.beta, 0.5 * diff * diff / self.beta,
                           diff - 0.5 * self.beta)
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction, avg_factor)


class MSELoss(nn.Module):
    """mmdet MSELoss (mse_loss under weighted_loss): the element-wise squared error, then
    weight, reduction / avg_factor, loss_weight.  H3DBboxHead's cues_semantic_loss uses
    reduction='none' with a weight."""

    def __init__(self, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None,
                **kwargs):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        loss = F.mse_loss(pred, target, reduction="none")
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction, avg_factor)


_LOSSES = {"ChamferDistance": ChamferDistance, "CrossEntropyLoss": CrossEntropyLoss,
           "SmoothL1Loss": SmoothL1Loss, "MSELoss": MSELoss}


def build_loss(cfg):
    """dict(type='ChamferDistance' | 'CrossEntropyLoss' | 'SmoothL1Loss' | 'MSELoss', ...) -> the
    module (the LOSSES registry entries the VoteNet and H3DNet configs name)."""
    if not isinstance(cfg, dict):
        return cfg
    args = dict(cfg)
    kind = args.pop("type")
    if kind not in _LOSSES:
        raise NotImplementedError("loss %r is not built here" % kind)
    return _LOSSES[kind](**args)
