"""VoteNet's head (COVERAGE n4): PartialBinBasedBBoxCoder, VoteModule, BaseConvBboxHead and
VoteHead with the reference's constructor arguments, attribute names and state-dict keys.

Reference: mmdet3d/models/dense_heads/vote_head.py, base_conv_bbox_head.py,
mmdet3d/models/model_utils/vote_module.py, mmdet3d/core/bbox/coders/
partial_bin_based_bbox_coder.py.

What differs from the reference is where its Python loops and expanded matrices were:

  get_targets   one pass for the whole batch, nothing read back.  The ground truths of all
                samples are padded to the batch maximum with a validity mask (the reference
                pads its results the same way); vote targets come from msmd_vote_targets_f32
                (the per-box, per-slot nonzero loop in closed form); the proposal -> ground
                truth assignment and its distance come from msmd_chamfer_fwd_f32 on the
                aggregated points against the padded centres, with the padding rows moved to
                infinity so that nothing is assigned to them; the rest is gathers.
  losses        ChamferDistance (losses.py) runs on the matrix-free kernels, forward and back.
  get_bboxes    decode for the whole batch, points per box from
                msmd_points_in_boxes_count_f32, ONE aligned3d NMS call for all samples, one
                host read for the variable-length results.
"""
import copy

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import kernels as K
from .head import Conv1d, ConvModule
from .head_loss import DepthBoxes
from .losses import build_loss
from .pointnet_modules import build_sa_module
from .pointnet_ops import furthest_point_sample
from .registry import HEADS


# ------------------------------------------------------------------------------------ coder
class PartialBinBasedBBoxCoder:
    """partial_bin_based_bbox_coder.py: direction in `num_dir_bins` bins plus a residual, size
    as one of `num_sizes` mean sizes plus a residual."""

    def __init__(self, num_dir_bins, num_sizes, mean_sizes, with_rot=True):
        assert len(mean_sizes) == num_sizes
        self.num_dir_bins = num_dir_bins
        self.num_sizes = num_sizes
        self.mean_sizes = mean_sizes
        self.with_rot = with_rot
        self._mean_size_tensors = {}

    def mean_size_tensor(self, like):
        """mean_sizes as a tensor beside `like`, made once per device and dtype (the reference's
        `new_tensor(self.mean_sizes)` is a blocking upload at every call)."""
        key = (like.device, like.dtype)
        if key not in self._mean_size_tensors:
            self._mean_size_tensors[key] = torch.tensor(self.mean_sizes, dtype=like.dtype).to(
                like.device, non_blocking=True)
        return self._mean_size_tensors[key]

    def encode_tensors(self, boxes, labels):
        """encode on plain tensors of any leading shape: boxes [..., 7] (bottom centre), labels
        [...] -> (gravity centre, size class, size residual, direction class, direction
        residual).  Element-wise, so one call serves a padded batch."""
        center_target = torch.cat([boxes[..., :2], (boxes[..., 2] + boxes[..., 5] * 0.5)[..., None]],
                                  dim=-1)
        size_class_target = labels
        size_res_target = boxes[..., 3:6] - self.mean_size_tensor(boxes)[size_class_target]
        if self.with_rot:
            dir_class_target, dir_res_target = self.angle2class(boxes[..., 6])
        else:
            dir_class_target = labels.new_zeros(labels.shape)
            dir_res_target = boxes.new_zeros(labels.shape)
        return center_target, size_class_target, size_res_target, dir_class_target, dir_res_target

    def encode(self, gt_bboxes_3d, gt_labels_3d):
        """:27-56 -- (center, size class, size residual, direction class, direction residual)."""
        return self.encode_tensors(gt_bboxes_3d.tensor, gt_labels_3d)

    def decode(self, bbox_out, suffix=""):
        """:58-99 -- predictions -> [batch, n, 7] (gravity centre, size, angle)."""
        center = bbox_out["center" + suffix]
        batch_size, num_proposal = center.shape[:2]
        if self.with_rot:
            dir_class = torch.argmax(bbox_out["dir_class" + suffix], -1)
            dir_res = torch.gather(bbox_out["dir_res" + suffix], 2, dir_class.unsqueeze(-1))
            dir_res = dir_res.squeeze(2)
            dir_angle = self.class2angle(dir_class, dir_res).reshape(batch_size, num_proposal, 1)
        else:
            dir_angle = center.new_zeros(batch_size, num_proposal, 1)
        size_class = torch.argmax(bbox_out["size_class" + suffix], -1, keepdim=True)
        size_res = torch.gather(bbox_out["size_res" + suffix], 2,
                                size_class.unsqueeze(-1).repeat(1, 1, 1, 3))
        mean_sizes = self.mean_size_tensor(center)
        size_base = torch.index_select(mean_sizes, 0, size_class.reshape(-1))
        bbox_size = size_base.reshape(batch_size, num_proposal, -1) + size_res.squeeze(2)
        return torch.cat([center, bbox_size, dir_angle], dim=-1)

    def decode_corners(self, center, size_res, size_class):
        """:101-137 -- axis-aligned (x1, y1, z1, x2, y2, z2) from normalised size residuals."""
        if len(size_class.shape) == 2 or size_class.shape[-1] == 1:
            batch_size, proposal_num = size_class.shape[:2]
            one_hot_size_class = size_res.new_zeros((batch_size, proposal_num, self.num_sizes))
            if len(size_class.shape) == 2:
                size_class = size_class.unsqueeze(-1)
            one_hot_size_class.scatter_(2, size_class, 1)
            one_hot_size_class_expand = one_hot_size_class.unsqueeze(-1).repeat(
                1, 1, 1, 3).contiguous()
        else:
            one_hot_size_class_expand = size_class
        if len(size_res.shape) == 4:
            size_res = torch.sum(size_res * one_hot_size_class_expand, 2)
        mean_sizes = self.mean_size_tensor(size_res)
        mean_sizes = torch.sum(mean_sizes * one_hot_size_class_expand, 2)
        size_full = (size_res + 1) * mean_sizes
        size_full = torch.clamp(size_full, 0)
        half_size_full = size_full / 2
        return torch.cat([center - half_size_full, center + half_size_full], dim=-1)

    def split_pred(self, cls_preds, reg_preds, base_xyz):
        """:139-201 -- the head's two maps [B, C, P] -> the prediction dict."""
        results = {}
        start, end = 0, 0
        cls_preds_trans = cls_preds.transpose(2, 1)
        reg_preds_trans = reg_preds.transpose(2, 1)
        end += 3
        results["center"] = base_xyz + reg_preds_trans[..., start:end].contiguous()
        start = end
        end += self.num_dir_bins
        results["dir_class"] = reg_preds_trans[..., start:end].contiguous()
        start = end
        end += self.num_dir_bins
        dir_res_norm = reg_preds_trans[..., start:end].contiguous()
        start = end
        results["dir_res_norm"] = dir_res_norm
        results["dir_res"] = dir_res_norm * (np.pi / self.num_dir_bins)
        end += self.num_sizes
        results["size_class"] = reg_preds_trans[..., start:end].contiguous()
        start = end
        end += self.num_sizes * 3
        size_res_norm = reg_preds_trans[..., start:end]
        batch_size, num_proposal = reg_preds_trans.shape[:2]
        size_res_norm = size_res_norm.reshape([batch_size, num_proposal, self.num_sizes, 3])
        start = end
        results["size_res_norm"] = size_res_norm.contiguous()
        mean_sizes = self.mean_size_tensor(reg_preds)
        results["size_res"] = size_res_norm * mean_sizes.unsqueeze(0).unsqueeze(0)
        results["obj_scores"] = cls_preds_trans[..., 0:2].contiguous()
        results["sem_scores"] = cls_preds_trans[..., 2:].contiguous()
        return results

    def angle2class(self, angle):
        """:203-222."""
        angle = angle % (2 * np.pi)
        angle_per_class = 2 * np.pi / float(self.num_dir_bins)
        shifted_angle = (angle + angle_per_class / 2) % (2 * np.pi)
        angle_cls = shifted_angle // angle_per_class
        angle_res = shifted_angle - (angle_cls * angle_per_class + angle_per_class / 2)
        return angle_cls.long(), angle_res

    def class2angle(self, angle_cls, angle_res, limit_period=True):
        """:224-240."""
        angle_per_class = 2 * np.pi / float(self.num_dir_bins)
        angle_center = angle_cls.float() * angle_per_class
        angle = angle_center + angle_res
        if limit_period:
            angle = torch.where(angle > np.pi, angle - 2 * np.pi, angle)
        return angle


class AnchorFreeBBoxCoder(PartialBinBasedBBoxCoder):
    """anchor_free_bbox_coder.py (3DSSD): no size classes -- the size target is the half size,
    the direction residual is normalised by the bin width."""

    def __init__(self, num_dir_bins, with_rot=True):
        super().__init__(num_dir_bins, 0, [], with_rot=with_rot)

    def encode(self, gt_bboxes_3d, gt_labels_3d):
        """:23-51 -- (gravity centre, half sizes, direction class, normalised residual).
        Element-wise, so one call serves the concatenated boxes of a batch."""
        center_target = gt_bboxes_3d.gravity_center
        size_res_target = gt_bboxes_3d.dims / 2
        box_num = gt_labels_3d.shape[0]
        if self.with_rot:
            dir_class_target, dir_res_target = self.angle2class(gt_bboxes_3d.yaw)
            dir_res_target /= (2 * np.pi / self.num_dir_bins)
        else:
            dir_class_target = gt_labels_3d.new_zeros(box_num)
            dir_res_target = gt_bboxes_3d.tensor.new_zeros(box_num)
        return center_target, size_res_target, dir_class_target, dir_res_target

    def decode(self, bbox_out):
        """:53-85 -- predictions -> [batch, n, 7] (centre, size, angle)."""
        center = bbox_out["center"]
        batch_size, num_proposal = center.shape[:2]
        if self.with_rot:
            dir_class = torch.argmax(bbox_out["dir_class"], -1)
            dir_res = torch.gather(bbox_out["dir_res"], 2, dir_class.unsqueeze(-1))
            dir_res = dir_res.squeeze(2)
            dir_angle = self.class2angle(dir_class, dir_res).reshape(batch_size, num_proposal, 1)
        else:
            dir_angle = center.new_zeros(batch_size, num_proposal, 1)
        bbox_size = torch.clamp(bbox_out["size"] * 2, min=0.1)
        return torch.cat([center, bbox_size, dir_angle], dim=-1)

    def split_pred(self, cls_preds, reg_preds, base_xyz):
        """:87-129 -- the head's two maps [B, C, P] -> the prediction dict."""
        results = {"obj_scores": cls_preds}
        reg_preds_trans = reg_preds.transpose(2, 1)
        bins = self.num_dir_bins
        results["center_offset"] = reg_preds_trans[..., 0:3]
        results["center"] = base_xyz.detach() + reg_preds_trans[..., 0:3]
        results["size"] = reg_preds_trans[..., 3:6]
        results["dir_class"] = reg_preds_trans[..., 6:6 + bins]
        dir_res_norm = reg_preds_trans[..., 6 + bins:6 + 2 * bins]
        results["dir_res_norm"] = dir_res_norm
        results["dir_res"] = dir_res_norm * (2 * np.pi / bins)
        return results


_BBOX_CODERS = {"PartialBinBasedBBoxCoder": PartialBinBasedBBoxCoder,
                "AnchorFreeBBoxCoder": AnchorFreeBBoxCoder}


def build_bbox_coder(cfg):
    if not isinstance(cfg, dict):
        return cfg
    args = dict(cfg)
    kind = args.pop("type")
    if kind not in _BBOX_CODERS:
        raise NotImplementedError("VoteHead: bbox coder %r is not built" % kind)
    return _BBOX_CODERS[kind](**args)


def _conv_module(in_channels, out_channels, conv_cfg, norm_cfg, act_cfg, bias):
    """mmcv's ConvModule(kernel_size 1, padding 0, conv_cfg, norm_cfg, act_cfg, bias) on
    head.ConvModule (attribute names conv / bn / activate)."""
    if conv_cfg.get("type") != "Conv1d" or (act_cfg or {}).get("type", "ReLU") != "ReLU":
        raise NotImplementedError("VoteNet's layers are Conv1d + norm + ReLU")
    norm, norm_kwargs = None, None
    if norm_cfg is not None:
        norm_kwargs = dict(norm_cfg)
        norm = norm_kwargs.pop("type")
        norm_kwargs.pop("requires_grad", None)
    return ConvModule(in_channels, out_channels, 1, padding=0, bias=bias, conv="Conv1d",
                      norm=norm, norm_kwargs=norm_kwargs)


# ------------------------------------------------------------------------------ vote module
class VoteModule(nn.Module):
    """vote_module.py: every seed predicts `vote_per_seed` offsets (and feature residuals)."""

    def __init__(self, in_channels, vote_per_seed=1, gt_per_seed=3, num_points=-1,
                 conv_channels=(16, 16), conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d"),
                 act_cfg=dict(type="ReLU"), norm_feats=True, with_res_feat=True,
                 vote_xyz_range=None, vote_loss=None):
        super().__init__()
        self.in_channels = in_channels
        self.vote_per_seed = vote_per_seed
        self.gt_per_seed = gt_per_seed
        self.num_points = num_points
        self.norm_feats = norm_feats
        self.with_res_feat = with_res_feat
        assert vote_xyz_range is None or (isinstance(vote_xyz_range, tuple) and all(
            isinstance(v, float) for v in vote_xyz_range))
        self.vote_xyz_range = vote_xyz_range
        if vote_loss is not None:
            self.vote_loss = build_loss(vote_loss)
        prev_channels = in_channels
        vote_conv_list = list()
        for k in range(len(conv_channels)):
            vote_conv_list.append(_conv_module(prev_channels, conv_channels[k], conv_cfg, norm_cfg,
                                               act_cfg, bias=True))
            prev_channels = conv_channels[k]
        self.vote_conv = nn.Sequential(*vote_conv_list)
        if with_res_feat:
            out_channel = (3 + in_channels) * self.vote_per_seed
        else:
            out_channel = 3 * self.vote_per_seed
        self.conv_out = Conv1d(prev_channels, out_channel, 1)

    def forward(self, seed_points, seed_feats):
        """seed_points (B, N, 3), seed_feats (B, C, N) -> vote_points (B, M, 3), vote_feats
        (B, C, M), offset (B, 3, M), M = N * vote_per_seed."""
        if self.num_points != -1:
            assert self.num_points < seed_points.shape[1], \
                f"Number of vote points ({self.num_points}) should be " \
                f"smaller than seed points size ({seed_points.shape[1]})"
            seed_points = seed_points[:, :self.num_points]
            seed_feats = seed_feats[..., :self.num_points]
        batch_size, feat_channels, num_seed = seed_feats.shape
        num_vote = num_seed * self.vote_per_seed
        x = self.vote_conv(seed_feats)
        votes = self.conv_out(x)
        votes = votes.transpose(2, 1).reshape(batch_size, num_seed, self.vote_per_seed, -1)
        offset = votes[:, :, :, 0:3]
        if self.vote_xyz_range is not None:
            limited_offset_list = []
            for axis in range(len(self.vote_xyz_range)):
                limited_offset_list.append(offset[..., axis].clamp(
                    min=-self.vote_xyz_range[axis], max=self.vote_xyz_range[axis]))
            limited_offset = torch.stack(limited_offset_list, -1)
            vote_points = (seed_points.unsqueeze(2) + limited_offset).contiguous()
        else:
            vote_points = (seed_points.unsqueeze(2) + offset).contiguous()
        vote_points = vote_points.view(batch_size, num_vote, 3)
        offset = offset.reshape(batch_size, num_vote, 3).transpose(2, 1)
        if self.with_res_feat:
            res_feats = votes[:, :, :, 3:]
            vote_feats = (seed_feats.transpose(2, 1).unsqueeze(2) + res_feats).contiguous()
            vote_feats = vote_feats.view(batch_size, num_vote,
                                         feat_channels).transpose(2, 1).contiguous()
            if self.norm_feats:
                features_norm = torch.norm(vote_feats, p=2, dim=1)
                vote_feats = vote_feats.div(features_norm.unsqueeze(1))
        else:
            vote_feats = seed_feats
        return vote_points, vote_feats, offset

    def get_loss(self, seed_points, vote_points, seed_indices, vote_targets_mask, vote_targets):
        """vote_module.py:152-185.  The Chamfer call is B * num_seed batches of vote_per_seed x
        gt_per_seed points: the flat shape of the kernel."""
        batch_size, num_seed = seed_points.shape[:2]
        seed_indices = seed_indices.long()
        seed_gt_votes_mask = torch.gather(vote_targets_mask, 1, seed_indices).float()
        seed_indices_expand = seed_indices.unsqueeze(-1).repeat(1, 1, 3 * self.gt_per_seed)
        seed_gt_votes = torch.gather(vote_targets, 1, seed_indices_expand)
        seed_gt_votes += seed_points.repeat(1, 1, self.gt_per_seed)
        weight = seed_gt_votes_mask / (torch.sum(seed_gt_votes_mask) + 1e-6)
        distance = self.vote_loss(vote_points.view(batch_size * num_seed, -1, 3),
                                  seed_gt_votes.view(batch_size * num_seed, -1, 3),
                                  dst_weight=weight.view(batch_size * num_seed, 1))[1]
        return torch.sum(torch.min(distance, dim=1)[0])


# -------------------------------------------------------------------------- prediction layers
@HEADS.register_module()
class BaseConvBboxHead(nn.Module):
    """base_conv_bbox_head.py: shared convs, then optional class / regression branches, then a
    1 x 1 convolution each."""

    def __init__(self, in_channels=0, shared_conv_channels=(), cls_conv_channels=(),
                 num_cls_out_channels=0, reg_conv_channels=(), num_reg_out_channels=0,
                 conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d"),
                 act_cfg=dict(type="ReLU"), bias="auto"):
        super().__init__()
        assert in_channels > 0
        assert num_cls_out_channels > 0
        assert num_reg_out_channels > 0
        self.in_channels = in_channels
        self.shared_conv_channels = shared_conv_channels
        self.cls_conv_channels = cls_conv_channels
        self.num_cls_out_channels = num_cls_out_channels
        self.reg_conv_channels = reg_conv_channels
        self.num_reg_out_channels = num_reg_out_channels
        self.conv_cfg = conv_cfg
        self.norm_cfg = norm_cfg
        self.act_cfg = act_cfg
        self.bias = bias
        if len(self.shared_conv_channels) > 0:
            self.shared_convs = self._add_conv_branch(self.in_channels, self.shared_conv_channels)
            out_channels = self.shared_conv_channels[-1]
        else:
            out_channels = self.in_channels
        prev_channel = out_channels
        if len(self.cls_conv_channels) > 0:
            self.cls_convs = self._add_conv_branch(prev_channel, self.cls_conv_channels)
            prev_channel = self.cls_conv_channels[-1]
        self.conv_cls = Conv1d(prev_channel, num_cls_out_channels, kernel_size=1)
        prev_channel = out_channels
        if len(self.reg_conv_channels) > 0:
            self.reg_convs = self._add_conv_branch(prev_channel, self.reg_conv_channels)
            prev_channel = self.reg_conv_channels[-1]
        self.conv_reg = Conv1d(prev_channel, num_reg_out_channels, kernel_size=1)

    def _add_conv_branch(self, in_channels, conv_channels):
        conv_spec = [in_channels] + list(conv_channels)
        conv_layers = nn.Sequential()
        for i in range(len(conv_spec) - 1):
            conv_layers.add_module(f"layer{i}", _conv_module(
                conv_spec[i], conv_spec[i + 1], self.conv_cfg, self.norm_cfg, self.act_cfg,
                self.bias))
        return conv_layers

    def init_weights(self):
        pass

    def forward(self, feats):
        """feats (B, C, P) -> class scores (B, num_cls_out_channels, P), box predictions
        (B, num_reg_out_channels, P)."""
        x = feats
        if len(self.shared_conv_channels) > 0:
            x = self.shared_convs(feats)
        x_cls = x
        x_reg = x
        if len(self.cls_conv_channels) > 0:
            x_cls = self.cls_convs(x_cls)
        cls_score = self.conv_cls(x_cls)
        if len(self.reg_conv_channels) > 0:
            x_reg = self.reg_convs(x_reg)
        bbox_pred = self.conv_reg(x_reg)
        return cls_score, bbox_pred


def _cfg_get(cfg, key):
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


def instance_vote_targets(points, pts_semantic_mask, pts_instance_mask, num_classes, gt_per_seed):
    """The instance-mask form of the vote targets (vote_head.py:502-516, ScanNet) for a stacked
    batch, without a loop over instances: points [B, N, >= 3], masks long [B, N] ->
    (vote_targets [B, N, 3 * gt_per_seed], vote_target_masks long [B, N]).  An instance counts
    when the semantic label of its FIRST point is a detection class; its votes point at the
    centre of its points' bounding box.  torch.unique compacts the (sample, instance) pairs --
    the one host read of this branch."""
    batch, n = pts_instance_mask.shape
    xyz = points[..., :3].reshape(batch * n, 3)
    inst = pts_instance_mask.reshape(-1).long()
    sample = torch.arange(batch, device=inst.device).repeat_interleave(n)
    pairs = torch.stack([sample, inst], 1)
    _, group = torch.unique(pairs, dim=0, return_inverse=True)
    groups = batch * n                                  # an upper bound known without a read
    index3 = group[:, None].expand(-1, 3)
    low = xyz.new_zeros((groups, 3)).scatter_reduce_(0, index3, xyz, "amin", include_self=False)
    high = xyz.new_zeros((groups, 3)).scatter_reduce_(0, index3, xyz, "amax", include_self=False)
    row = torch.arange(batch * n, device=inst.device)
    first = row.new_zeros((groups,)).scatter_reduce_(0, group, row, "amin", include_self=False)
    counts = pts_semantic_mask.reshape(-1)[first] < num_classes
    center = 0.5 * (low + high)
    member = counts[group]
    votes = torch.where(member[:, None], center[group] - xyz, xyz.new_zeros(()))
    vote_targets = votes.reshape(batch, n, 3).repeat(1, 1, gt_per_seed)
    return vote_targets, member.long().reshape(batch, n)


# ------------------------------------------------------------------------------------- head
def multiclass_nms_batch(obj_scores, sem_scores, bbox3d, points, with_yaw, test_cfg):
    """multiclass_nms_single (vote_head.py:614-666, h3d_bbox_head.py:492-550) for the whole batch:
    objectness [B, P], class scores [B, P, C], decoded boxes [B, P, 7] (gravity centre) and points
    [B, N, >= 3] -> a list of (DepthBoxes, scores, labels) per sample.  test_cfg holds nms_thr,
    score_thr and per_class_proposal.  VoteHead and H3DBboxHead share it."""
    if not torch.is_tensor(points):
        points = torch.stack(list(points))
    batch, proposals = bbox3d.shape[:2]
    device = bbox3d.device
    # the decoded centre is the gravity centre
    boxes = DepthBoxes(bbox3d.reshape(batch * proposals, -1), box_dim=bbox3d.shape[-1],
                       with_yaw=with_yaw, origin=(0.5, 0.5, 0.5))
    count = K.points_in_boxes_count(
        DepthBoxes.boxes_to_lidar(boxes.tensor).view(batch, proposals, 7).contiguous(),
        DepthBoxes.points_to_lidar(points.float()).contiguous())
    nonempty = (count > 5).reshape(-1)
    corner3d = boxes.corners
    minmax_box3d = torch.cat([torch.min(corner3d, dim=1)[0], torch.max(corner3d, dim=1)[0]], 1)
    bbox_classes = torch.argmax(sem_scores, -1).reshape(-1)
    flat_scores = obj_scores.reshape(-1)

    # one NMS call.  Rows in (non-empty first, sample, descending score) order; the segment of
    # sample b covers its non-empty boxes only, the empty ones lie past the last segment.
    sample = torch.arange(batch, device=device).repeat_interleave(proposals)
    by_score = torch.sort(flat_scores, descending=True, stable=True)[1]
    key = torch.where(nonempty, sample, sample + batch)[by_score]
    order = by_score[torch.sort(key, stable=True)[1]]
    offsets = torch.cat([count.new_zeros(1, dtype=torch.long),
                         torch.cumsum(nonempty.view(batch, proposals).sum(1), 0)]).int()
    rows = torch.cat([minmax_box3d, bbox_classes.float()[:, None]], 1)[order].contiguous()
    thresh = torch.full((batch,), float(_cfg_get(test_cfg, "nms_thr")),
                        dtype=torch.float32, device=device)
    keep, _ = K.nms_segments("aligned3d", rows, offsets, thresh, proposals, order=order)
    nms_mask = torch.zeros(batch * proposals + 1, dtype=torch.bool, device=device)
    nms_mask[(keep + 1).reshape(-1)] = True                      # -1 lands in the spare slot
    selected = nms_mask[1:] & (flat_scores > _cfg_get(test_cfg, "score_thr"))

    chosen = selected.view(batch, proposals).cpu()               # the one host read
    results = []
    per_class = _cfg_get(test_cfg, "per_class_proposal")
    for b in range(batch):
        index = (torch.nonzero(chosen[b]).flatten() + b * proposals).to(device)
        box_b, obj_b = boxes.tensor[index], flat_scores[index]
        if per_class:
            sem_b = sem_scores.reshape(batch * proposals, -1)[index]
            classes = sem_b.shape[-1]
            bbox_selected = box_b.repeat(classes, 1)
            score_selected = (obj_b[None, :] * sem_b.t()).reshape(-1)
            labels = torch.arange(classes, device=device).repeat_interleave(index.numel())
        else:
            bbox_selected, score_selected, labels = box_b, obj_b, bbox_classes[index]
        results.append((DepthBoxes(bbox_selected, box_dim=bbox_selected.shape[-1],
                                   with_yaw=with_yaw), score_selected, labels))
    return results


@HEADS.register_module()
class VoteHead(nn.Module):
    """vote_head.py: votes from the seeds, a set-abstraction layer over the votes, the
    prediction layers, the coder's split."""

    def __init__(self, num_classes, bbox_coder, train_cfg=None, test_cfg=None,
                 vote_module_cfg=None, vote_aggregation_cfg=None, pred_layer_cfg=None,
                 conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d"), objectness_loss=None,
                 center_loss=None, dir_class_loss=None, dir_res_loss=None, size_class_loss=None,
                 size_res_loss=None, semantic_loss=None, iou_loss=None):
        super().__init__()
        if iou_loss is not None:
            raise NotImplementedError(
                "VoteHead: iou_loss (AxisAlignedIoULoss, the votenet_iouloss config) is not built")
        self.num_classes = num_classes
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        self.gt_per_seed = vote_module_cfg["gt_per_seed"]
        self.num_proposal = vote_aggregation_cfg["num_point"]
        self.objectness_loss = build_loss(objectness_loss)
        self.center_loss = build_loss(center_loss)
        self.dir_res_loss = build_loss(dir_res_loss)
        self.dir_class_loss = build_loss(dir_class_loss)
        self.size_res_loss = build_loss(size_res_loss)
        if size_class_loss is not None:
            self.size_class_loss = build_loss(size_class_loss)
        if semantic_loss is not None:
            self.semantic_loss = build_loss(semantic_loss)
        self.iou_loss = None
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.num_sizes = self.bbox_coder.num_sizes
        self.num_dir_bins = self.bbox_coder.num_dir_bins
        self.vote_module = VoteModule(**vote_module_cfg)
        # (a copy: the SA module adds the xyz channels to its mlp_channels list in place)
        self.vote_aggregation = build_sa_module(copy.deepcopy(vote_aggregation_cfg))
        self.fp16_enabled = False
        self.conv_pred = BaseConvBboxHead(
            **pred_layer_cfg, num_cls_out_channels=self._get_cls_out_channels(),
            num_reg_out_channels=self._get_reg_out_channels())

    def init_weights(self):
        pass

    def _get_cls_out_channels(self):
        return self.num_classes + 2                       # classes + objectness (2)

    def _get_reg_out_channels(self):
        # centre residual (3), direction class + residual, size class + residual (3 each)
        return 3 + self.num_dir_bins * 2 + self.num_sizes * 4

    def _extract_input(self, feat_dict):
        if "seed_points" in feat_dict and "seed_features" in feat_dict and \
                "seed_indices" in feat_dict:
            return feat_dict["seed_points"], feat_dict["seed_features"], feat_dict["seed_indices"]
        return feat_dict["fp_xyz"][-1], feat_dict["fp_features"][-1], feat_dict["fp_indices"][-1]

    def forward(self, feat_dict, sample_mod):
        """:138-222."""
        assert sample_mod in ["vote", "seed", "random", "spec"]
        seed_points, seed_features, seed_indices = self._extract_input(feat_dict)
        vote_points, vote_features, vote_offset = self.vote_module(seed_points, seed_features)
        results = dict(seed_points=seed_points, seed_indices=seed_indices,
                       vote_points=vote_points, vote_features=vote_features,
                       vote_offset=vote_offset)
        if sample_mod == "vote":
            aggregation_inputs = dict(points_xyz=vote_points, features=vote_features)
        elif sample_mod == "seed":
            sample_indices = furthest_point_sample(seed_points, self.num_proposal)
            aggregation_inputs = dict(points_xyz=vote_points, features=vote_features,
                                      indices=sample_indices)
        elif sample_mod == "random":
            batch_size, num_seed = seed_points.shape[:2]
            sample_indices = torch.randint(0, num_seed, (batch_size, self.num_proposal)).to(
                device=seed_points.device, dtype=torch.int32)
            aggregation_inputs = dict(points_xyz=vote_points, features=vote_features,
                                      indices=sample_indices)
        else:
            aggregation_inputs = dict(points_xyz=seed_points, features=seed_features,
                                      target_xyz=vote_points)
        aggregated_points, features, aggregated_indices = \
            self.vote_aggregation(**aggregation_inputs)
        results["aggregated_points"] = aggregated_points
        results["aggregated_features"] = features
        results["aggregated_indices"] = aggregated_indices
        cls_predictions, reg_predictions = self.conv_pred(features)
        results.update(self.bbox_coder.split_pred(cls_predictions, reg_predictions,
                                                  aggregated_points))
        return results

    def loss(self, bbox_preds, points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask=None,
             pts_instance_mask=None, img_metas=None, gt_bboxes_ignore=None, ret_target=False):
        """:225-351."""
        targets = self.get_targets(points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask,
                                   pts_instance_mask, bbox_preds)
        (vote_targets, vote_target_masks, size_class_targets, size_res_targets,
         dir_class_targets, dir_res_targets, center_targets, assigned_center_targets,
         mask_targets, valid_gt_masks, objectness_targets, objectness_weights,
         box_loss_weights, valid_gt_weights) = targets
        vote_loss = self.vote_module.get_loss(bbox_preds["seed_points"], bbox_preds["vote_points"],
                                              bbox_preds["seed_indices"], vote_target_masks,
                                              vote_targets)
        objectness_loss = self.objectness_loss(bbox_preds["obj_scores"].transpose(2, 1),
                                               objectness_targets, weight=objectness_weights)
        source2target_loss, target2source_loss = self.center_loss(
            bbox_preds["center"], center_targets, src_weight=box_loss_weights,
            dst_weight=valid_gt_weights)
        center_loss = source2target_loss + target2source_loss
        dir_class_loss = self.dir_class_loss(bbox_preds["dir_class"].transpose(2, 1),
                                             dir_class_targets, weight=box_loss_weights)
        batch_size, proposal_num = size_class_targets.shape[:2]
        heading_label_one_hot = vote_targets.new_zeros(
            (batch_size, proposal_num, self.num_dir_bins))
        heading_label_one_hot.scatter_(2, dir_class_targets.unsqueeze(-1), 1)
        dir_res_norm = torch.sum(bbox_preds["dir_res_norm"] * heading_label_one_hot, -1)
        dir_res_loss = self.dir_res_loss(dir_res_norm, dir_res_targets, weight=box_loss_weights)
        size_class_loss = self.size_class_loss(bbox_preds["size_class"].transpose(2, 1),
                                               size_class_targets, weight=box_loss_weights)
        one_hot_size_targets = vote_targets.new_zeros((batch_size, proposal_num, self.num_sizes))
        one_hot_size_targets.scatter_(2, size_class_targets.unsqueeze(-1), 1)
        one_hot_size_targets_expand = one_hot_size_targets.unsqueeze(-1).repeat(
            1, 1, 1, 3).contiguous()
        size_residual_norm = torch.sum(bbox_preds["size_res_norm"] * one_hot_size_targets_expand, 2)
        box_loss_weights_expand = box_loss_weights.unsqueeze(-1).repeat(1, 1, 3)
        size_res_loss = self.size_res_loss(size_residual_norm, size_res_targets,
                                           weight=box_loss_weights_expand)
        semantic_loss = self.semantic_loss(bbox_preds["sem_scores"].transpose(2, 1), mask_targets,
                                           weight=box_loss_weights)
        losses = dict(vote_loss=vote_loss, objectness_loss=objectness_loss,
                      semantic_loss=semantic_loss, center_loss=center_loss,
                      dir_class_loss=dir_class_loss, dir_res_loss=dir_res_loss,
                      size_class_loss=size_class_loss, size_res_loss=size_res_loss)
        if ret_target:
            losses["targets"] = targets
        return losses

    def get_targets(self, points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask=None,
                    pts_instance_mask=None, bbox_preds=None):
        """:353-564 for the whole batch at once; returns the reference's 14-tuple.

        points: a list of [N, >= 3] tensors of one length (the reference stacks its per-sample
        results, so it needs that too) or the stacked [B, N, >= 3] tensor.  Nothing is read
        back in the box form; the lengths used are shapes."""
        batch = len(gt_labels_3d)
        if not torch.is_tensor(points):
            points = torch.stack(list(points))
        points = points.float()
        num_points = points.shape[1]
        device = points.device
        assert self.bbox_coder.with_rot or pts_semantic_mask is not None

        # an empty sample gets the reference's single all-zero box with label 0, marked invalid
        counts = [max(int(labels.shape[0]), 1) for labels in gt_labels_3d]
        put = lambda t: t.to(device, non_blocking=True)                          # noqa: E731
        box_rows = [put(boxes.tensor) if len(labels) else
                    put(boxes.tensor.new_zeros((1, boxes.tensor.shape[-1])))
                    for boxes, labels in zip(gt_bboxes_3d, gt_labels_3d)]
        label_rows = [put(labels) if len(labels) else put(labels.new_zeros(1))
                      for labels in gt_labels_3d]
        valid_rows = [put(labels.new_ones(labels.shape)) if len(labels) else
                      put(labels.new_zeros(1)) for labels in gt_labels_3d]
        gt_boxes = nn.utils.rnn.pad_sequence(box_rows, batch_first=True)[..., :7]     # [B, G, 7]
        gt_labels = nn.utils.rnn.pad_sequence(label_rows, batch_first=True)           # [B, G]
        valid_gt_masks = nn.utils.rnn.pad_sequence(valid_rows, batch_first=True)      # [B, G]
        count = torch.tensor(counts, dtype=torch.int32).to(device, non_blocking=True)
        exists = torch.arange(gt_boxes.shape[1], device=device)[None, :] < count[:, None]

        (center_targets, size_class_all, size_res_all, dir_class_all, dir_res_all) = \
            self.bbox_coder.encode_tensors(gt_boxes, gt_labels)
        center_targets = center_targets * exists[..., None]          # padding rows: zeros

        if self.bbox_coder.with_rot:
            flat_boxes = torch.cat(box_rows)[:, :7]
            flat_centers = torch.cat([flat_boxes[:, :2],
                                      (flat_boxes[:, 2] + flat_boxes[:, 5] * 0.5)[:, None]], 1)
            box_offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]),
                                       dtype=torch.int32).to(device, non_blocking=True)
            point_offsets = torch.arange(batch + 1, dtype=torch.int32, device=device) * num_points
            flat_points = points.reshape(batch * num_points, -1)
            # both sides in the predicate's frame (DepthBoxes.points_in_boxes); a vote is a
            # difference of depth coordinates, so the centres go in that frame as well and the
            # result is turned back
            lidar_points = DepthBoxes.points_to_lidar(flat_points).contiguous()
            lidar_centers = DepthBoxes.points_to_lidar(flat_centers).contiguous()
            votes, vote_target_masks = K.vote_targets(
                lidar_points, point_offsets, DepthBoxes.boxes_to_lidar(flat_boxes).contiguous(),
                lidar_centers, box_offsets, max_points=num_points, gt_per_seed=self.gt_per_seed)
            votes = votes.view(batch, num_points, self.gt_per_seed, 3)
            vote_targets = torch.stack([0.0 - votes[..., 1], votes[..., 0], votes[..., 2]], -1).reshape(
                batch, num_points, 3 * self.gt_per_seed)
            vote_target_masks = vote_target_masks.view(batch, num_points)
        else:
            semantic = pts_semantic_mask if torch.is_tensor(pts_semantic_mask) \
                else torch.stack(list(pts_semantic_mask))
            instance = pts_instance_mask if torch.is_tensor(pts_instance_mask) \
                else torch.stack(list(pts_instance_mask))
            vote_targets, vote_target_masks = instance_vote_targets(
                points, semantic.to(device), instance.to(device), self.num_classes,
                self.gt_per_seed)

        # proposals -> ground truths: the nearest centre, padding rows out of reach
        aggregated_points = bbox_preds["aggregated_points"].detach().float().contiguous()
        reachable = torch.where(exists[..., None], center_targets,
                                center_targets.new_full((), float("inf"))).contiguous()
        distance1, assignment, _, _ = K.chamfer_forward(aggregated_points, reachable, "l2")
        euclidean_distance1 = torch.sqrt(distance1 + 1e-6)

        positive = euclidean_distance1 < _cfg_get(self.train_cfg, "pos_distance_thr")
        negative = euclidean_distance1 > _cfg_get(self.train_cfg, "neg_distance_thr")
        objectness_targets = positive.long()
        objectness_masks = (positive | negative).float()

        dir_class_targets = torch.gather(dir_class_all, 1, assignment)
        dir_res_targets = torch.gather(dir_res_all, 1, assignment)
        dir_res_targets = dir_res_targets / (np.pi / self.num_dir_bins)
        size_class_targets = torch.gather(size_class_all, 1, assignment)
        assignment3 = assignment[..., None].expand(-1, -1, 3)
        size_res_targets = torch.gather(size_res_all, 1, assignment3)
        pos_mean_sizes = self.bbox_coder.mean_size_tensor(size_res_targets)[size_class_targets]
        size_res_targets = size_res_targets / pos_mean_sizes
        mask_targets = torch.gather(gt_labels, 1, assignment).long()
        assigned_center_targets = torch.gather(center_targets, 1, assignment3)

        objectness_weights = objectness_masks / (torch.sum(objectness_masks) + 1e-6)
        box_loss_weights = objectness_targets.float() / (
            torch.sum(objectness_targets).float() + 1e-6)
        valid_gt_weights = valid_gt_masks.float() / (torch.sum(valid_gt_masks.float()) + 1e-6)
        return (vote_targets, vote_target_masks, size_class_targets, size_res_targets,
                dir_class_targets, dir_res_targets, center_targets, assigned_center_targets,
                mask_targets, valid_gt_masks, objectness_targets, objectness_weights,
                box_loss_weights, valid_gt_weights)

    def get_bboxes(self, points, bbox_preds, input_metas=None, rescale=False, use_nms=True):
        """:566-666 for the whole batch: points [B, N, >= 3] -> a list of (DepthBoxes, scores,
        labels) per sample; use_nms=False returns the decoded [B, P, 7] tensor."""
        obj_scores = F.softmax(bbox_preds["obj_scores"], dim=-1)[..., -1]
        sem_scores = F.softmax(bbox_preds["sem_scores"], dim=-1)
        bbox3d = self.bbox_coder.decode(bbox_preds)
        if not use_nms:
            return bbox3d
        return multiclass_nms_batch(obj_scores, sem_scores, bbox3d, points,
                                    self.bbox_coder.with_rot, self.test_cfg)
