"""H3DNet's PrimitiveHead (mmdet3d/models/roi_heads/mask_heads/primitive_head.py): votes for
box-face centres (modes 'z', 'xy') and box-edge centres (mode 'line').  Attribute and parameter
names are the reference's (flag_conv, flag_pred, vote_module, vote_aggregation,
conv_pred.{0,1,conv_out}), so its checkpoints load, and the result dict carries its keys.

The targets -- in the reference a host loop over the instances of every sample with about
fourteen host reads each, run once per head -- are one index per step
(kernels.primitive_index, shared by the three heads through `prepare_primitive_inputs`) and
one launch per head (kernels.primitive_targets); nothing is read back."""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import kernels as K
from .head import Conv1d
from .head_loss import DepthBoxes  # noqa: F401  (the box type get_targets takes)
from .losses import build_loss
from .pointnet_modules import build_sa_module
from .pointnet_ops import furthest_point_sample
from .registry import HEADS
from .vote_head import VoteModule, _cfg_get, _conv_module


def prepare_primitive_inputs(points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask=None,
                             pts_instance_mask=None, num_classes=18, label_bound=None):
    """What every PrimitiveHead of a step needs of the ground truth, built once: flat points,
    masks (derived from the boxes where they are None, primitive_head.py:358-369), box corners,
    offsets and the instance index.  An empty sample gets the reference's single zero box with
    label 0 (:282-287; the caller's lists are left alone).  No host read: lengths are shapes."""
    batch = len(gt_labels_3d)
    if not torch.is_tensor(points):
        points = torch.stack(list(points))
    points = points.float()
    device, num_points = points.device, points.shape[1]
    boxes, labels = [], []
    for b, l in zip(gt_bboxes_3d, gt_labels_3d):
        if len(l) == 0:
            b = b.new_box(b.tensor.new_zeros((1, b.tensor.shape[-1])))
            l = l.new_zeros(1)
        boxes.append(b.to(device))
        labels.append(l.to(device, non_blocking=True))
    with_yaw = boxes[0].with_yaw
    assert all(b.with_yaw == with_yaw for b in boxes)
    if pts_semantic_mask is None:
        pts_semantic_mask = [None] * batch
    if pts_instance_mask is None:
        pts_instance_mask = [None] * batch
    sems, insts = [], []
    for i in range(batch):
        sem, inst = pts_semantic_mask[i], pts_instance_mask[i]
        if sem is None or inst is None:
            in_box = boxes[i].points_in_boxes(points[i])                  # [N, G]
            assignment = in_box.argmax(1)
            background = in_box.max(1)[0] == 0
            if sem is None:
                sem = torch.where(background, labels[i].new_full((), num_classes),
                                  labels[i][assignment])
            if inst is None:
                inst = torch.where(background, assignment.new_full((), labels[i].shape[0]),
                                   assignment)
        sems.append(sem.to(device).long())
        insts.append(inst.to(device).long())
    counts = [len(b) for b in boxes]
    flat_sem = torch.cat(sems).contiguous()
    flat_inst = torch.cat(insts).contiguous()
    point_offsets = torch.arange(batch + 1, dtype=torch.int32, device=device) * num_points
    box_offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]),
                               dtype=torch.int32).to(device, non_blocking=True)
    index = K.primitive_index(flat_sem, flat_inst, point_offsets, num_classes,
                              label_bound=label_bound, max_points=num_points,
                              max_instances=max(counts))
    return dict(points=points.reshape(batch * num_points, -1).contiguous(), sem=flat_sem,
                inst=flat_inst, corners=torch.cat([b.corners for b in boxes]).contiguous(),
                point_offsets=point_offsets, box_offsets=box_offsets, index=index,
                with_yaw=with_yaw, batch=batch, num_points=num_points, max_boxes=max(counts),
                num_classes=num_classes, label_bound=label_bound)


@HEADS.register_module()
class PrimitiveHead(nn.Module):
    """primitive_head.py:13-111."""

    def __init__(self, num_dims, num_classes, primitive_mode, train_cfg=None, test_cfg=None,
                 vote_module_cfg=None, vote_aggregation_cfg=None, feat_channels=(128, 128),
                 upper_thresh=100.0, surface_thresh=0.5, conv_cfg=dict(type="Conv1d"),
                 norm_cfg=dict(type="BN1d"), objectness_loss=None, center_loss=None,
                 semantic_reg_loss=None, semantic_cls_loss=None, label_bound=None):
        super().__init__()
        assert primitive_mode in ["z", "xy", "line"]
        self.num_dims = num_dims
        self.num_classes = num_classes
        self.primitive_mode = primitive_mode
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        self.gt_per_seed = vote_module_cfg["gt_per_seed"]
        self.num_proposal = vote_aggregation_cfg["num_point"]
        self.upper_thresh = upper_thresh
        self.surface_thresh = surface_thresh
        self.label_bound = label_bound      # None: kernels.PRIMITIVE_MAX_LABELS

        self.objectness_loss = build_loss(objectness_loss)
        self.center_loss = build_loss(center_loss)
        self.semantic_reg_loss = build_loss(semantic_reg_loss)
        self.semantic_cls_loss = build_loss(semantic_cls_loss)

        assert vote_aggregation_cfg["mlp_channels"][0] == vote_module_cfg["in_channels"]

        last = vote_module_cfg["conv_channels"][-1]
        self.flag_conv = _conv_module(last, last // 2, conv_cfg, norm_cfg, None, bias=True)
        self.flag_pred = Conv1d(last // 2, 2, 1)

        self.vote_module = VoteModule(**vote_module_cfg)
        aggregation = dict(vote_aggregation_cfg)
        aggregation["mlp_channels"] = list(aggregation["mlp_channels"])   # the module grows it
        self.vote_aggregation = build_sa_module(aggregation)

        prev_channel = vote_aggregation_cfg["mlp_channels"][-1]
        conv_pred_list = list()
        for k in range(len(feat_channels)):
            conv_pred_list.append(_conv_module(prev_channel, feat_channels[k], conv_cfg, norm_cfg,
                                               None, bias=True))
            prev_channel = feat_channels[k]
        self.conv_pred = nn.Sequential(*conv_pred_list)
        self.conv_pred.add_module("conv_out", Conv1d(prev_channel, 3 + num_dims + num_classes, 1))

    def init_weights(self):
        pass

    def forward(self, feats_dict, sample_mod):
        """:117-186."""
        assert sample_mod in ["vote", "seed", "random"]
        mode = self.primitive_mode
        seed_points = feats_dict["fp_xyz_net0"][-1]
        seed_features = feats_dict["hd_feature"]
        results = {}
        primitive_flag = self.flag_pred(self.flag_conv(seed_features))
        results["pred_flag_" + mode] = primitive_flag
        vote_points, vote_features, _ = self.vote_module(seed_points, seed_features)
        results["vote_" + mode] = vote_points
        results["vote_features_" + mode] = vote_features
        if sample_mod == "vote":
            sample_indices = None
        elif sample_mod == "seed":
            sample_indices = furthest_point_sample(seed_points, self.num_proposal)
        else:
            batch_size, num_seed = seed_points.shape[:2]
            sample_indices = torch.randint(0, num_seed, (batch_size, self.num_proposal),
                                           dtype=torch.int32, device=seed_points.device)
        aggregated_points, features, aggregated_indices = self.vote_aggregation(
            vote_points, vote_features, sample_indices)
        results["aggregated_points_" + mode] = aggregated_points
        results["aggregated_features_" + mode] = features
        results["aggregated_indices_" + mode] = aggregated_indices
        predictions = self.conv_pred(features)
        decode_ret = self.primitive_decode_scores(predictions, aggregated_points)
        results.update(decode_ret)
        center, pred_ind = self.get_primitive_center(primitive_flag, decode_ret["center_" + mode])
        results["pred_" + mode + "_ind"] = pred_ind
        results["pred_" + mode + "_center"] = center
        return results

    def primitive_decode_scores(self, predictions, aggregated_points):
        """:603-629."""
        mode = self.primitive_mode
        ret_dict = {}
        pred_transposed = predictions.transpose(2, 1)
        ret_dict["center_" + mode] = aggregated_points + pred_transposed[:, :, 0:3]
        if mode in ["z", "xy"]:
            ret_dict["size_residuals_" + mode] = pred_transposed[:, :, 3:3 + self.num_dims]
        ret_dict["sem_cls_scores_" + mode] = pred_transposed[:, :, 3 + self.num_dims:]
        return ret_dict

    def get_primitive_center(self, pred_flag, center):
        """:784-801."""
        ind_normal = F.softmax(pred_flag, dim=1)
        pred_indices = (ind_normal[:, 1, :] > self.surface_thresh).detach().float()
        selected = (ind_normal[:, 1, :] <= self.surface_thresh).detach().float()
        offset = torch.ones_like(center) * self.upper_thresh
        center = center + offset * selected.unsqueeze(-1)
        return center, pred_indices

    def get_targets(self, points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask=None,
                    pts_instance_mask=None, bbox_preds=None, prepared=None):
        """:259-325 for the whole batch: one index (or the `prepared` one a step's three heads
        share, prepare_primitive_inputs), one kernel launch, the seed gathers.  points: a list of
        [N, >= 3] tensors of one length or the stacked tensor.  Nothing is read back."""
        if prepared is None:
            prepared = prepare_primitive_inputs(points, gt_bboxes_3d, gt_labels_3d,
                                                pts_semantic_mask, pts_instance_mask,
                                                self.num_classes, self.label_bound)
        p = prepared
        cfg = {k: _cfg_get(self.train_cfg, k) for k in
               ("dist_thresh", "var_thresh", "lower_thresh", "num_point", "num_point_line",
                "line_thresh")}
        point_mask, point_offset, point_sem = K.primitive_targets(
            p["points"], p["sem"], p["point_offsets"], p["corners"], p["box_offsets"], p["index"],
            self.primitive_mode, p["with_yaw"], cfg, label_bound=p["label_bound"],
            max_points=p["num_points"], max_boxes=p["max_boxes"])
        batch_size, n = p["batch"], p["num_points"]
        point_mask = point_mask.view(batch_size, n)
        point_offset = point_offset.view(batch_size, n, 3)
        point_sem = point_sem.view(batch_size, n, 4 + self.num_dims)

        num_proposal = bbox_preds["aggregated_points_" + self.primitive_mode].shape[1]
        num_seed = bbox_preds["seed_points"].shape[1]
        seed_inds = bbox_preds["seed_indices"].long()
        seed_inds_expand = seed_inds.view(batch_size, num_seed, 1).repeat(1, 1, 3)
        seed_gt_votes = torch.gather(point_offset, 1, seed_inds_expand)
        seed_gt_votes += bbox_preds["seed_points"]
        gt_primitive_center = seed_gt_votes.view(batch_size * num_proposal, 1, 3)
        seed_inds_expand_sem = seed_inds.view(batch_size, num_seed, 1).repeat(
            1, 1, 4 + self.num_dims)
        seed_gt_sem = torch.gather(point_sem, 1, seed_inds_expand_sem)
        gt_primitive_semantic = seed_gt_sem[:, :, 3:3 + self.num_dims].view(
            batch_size * num_proposal, 1, self.num_dims).contiguous()
        gt_sem_cls_label = seed_gt_sem[:, :, -1].long()
        gt_votes_mask = torch.gather(point_mask, 1, seed_inds)
        return (point_mask, point_offset, gt_primitive_center, gt_primitive_semantic,
                gt_sem_cls_label, gt_votes_mask)

    def loss(self, bbox_preds, points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask=None,
             pts_instance_mask=None, img_metas=None, gt_bboxes_ignore=None, prepared=None):
        """:188-257."""
        targets = self.get_targets(points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask,
                                   pts_instance_mask, bbox_preds, prepared=prepared)
        return self.loss_from_targets(bbox_preds, targets)

    def loss_from_targets(self, bbox_preds, targets):
        mode = self.primitive_mode
        (point_mask, point_offset, gt_primitive_center, gt_primitive_semantic,
         gt_sem_cls_label, gt_primitive_mask) = targets
        losses = {}
        pred_flag = bbox_preds["pred_flag_" + mode]
        losses["flag_loss_" + mode] = self.objectness_loss(pred_flag, gt_primitive_mask.long())
        losses["vote_loss_" + mode] = self.vote_module.get_loss(
            bbox_preds["seed_points"], bbox_preds["vote_" + mode], bbox_preds["seed_indices"],
            point_mask, point_offset)
        num_proposal = bbox_preds["aggregated_points_" + mode].shape[1]
        primitive_center = bbox_preds["center_" + mode]
        primitive_semantic = bbox_preds["size_residuals_" + mode].contiguous() \
            if mode != "line" else None
        semantic_scores = bbox_preds["sem_cls_scores_" + mode].transpose(2, 1)
        gt_primitive_mask = gt_primitive_mask / (gt_primitive_mask.sum() + 1e-6)
        center_loss, size_loss, sem_cls_loss = self.compute_primitive_loss(
            primitive_center, primitive_semantic, semantic_scores, num_proposal,
            gt_primitive_center, gt_primitive_semantic, gt_sem_cls_label, gt_primitive_mask)
        losses["center_loss_" + mode] = center_loss
        losses["size_loss_" + mode] = size_loss
        losses["sem_loss_" + mode] = sem_cls_loss
        return losses

    def compute_primitive_loss(self, primitive_center, primitive_semantic, semantic_scores,
                               num_proposal, gt_primitive_center, gt_primitive_semantic,
                               gt_sem_cls_label, gt_primitive_mask):
        """:735-782."""
        batch_size = primitive_center.shape[0]
        vote_xyz_reshape = primitive_center.reshape(batch_size * num_proposal, -1, 3)
        weight = gt_primitive_mask.reshape(batch_size * num_proposal, 1)
        center_loss = self.center_loss(vote_xyz_reshape, gt_primitive_center,
                                       dst_weight=weight)[1]
        if self.primitive_mode != "line":
            size_xyz_reshape = primitive_semantic.reshape(
                batch_size * num_proposal, -1, self.num_dims).contiguous()
            size_loss = self.semantic_reg_loss(size_xyz_reshape, gt_primitive_semantic,
                                               dst_weight=weight)[1]
        else:
            size_loss = center_loss.new_zeros(())
        sem_cls_loss = self.semantic_cls_loss(semantic_scores, gt_sem_cls_label,
                                              weight=gt_primitive_mask)
        return center_loss, size_loss, sem_cls_loss
