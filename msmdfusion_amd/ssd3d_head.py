"""3DSSD's head (COVERAGE n5): SSD3DHead on VoteHead with the reference's constructor
arguments, attribute names and state-dict keys.

Reference: mmdet3d/models/dense_heads/ssd_3d_head.py, mmdet3d/core/bbox/coders/
anchor_free_bbox_coder.py (the coder is in vote_head.py beside its base class).

What differs from the reference is where its per-sample Python was:

  get_targets   the reference calls get_targets_single per sample: about sixty small ops, two
                points_in_boxes_gpu launches, a gt[valid] compaction and a host read each.  Here
                what depends on a box alone (the coder's encode, corners, sin / cos of -yaw, the
                enlarged table) is a handful of element-wise torch ops over the batch's
                concatenated boxes, and everything per candidate is ONE launch of
                msmd_ssd3d_targets_f32.  Nothing is read back.
  get_bboxes    decode, corners and the class shift for the whole batch, ONE NMS call over all
                samples (msmd_nms_mmcv_f32: mmcv.ops.batched_nms's pair test), one host read
                for the variable-length results.

Reference behaviour kept as written is marked `as written` where it is implemented.
"""
import numpy as np
import torch

from . import kernels as K
from .head_loss import LiDARBoxes
from .losses import build_loss
from .registry import HEADS
from .vote_head import VoteHead, _cfg_get

NMS_SPLIT_THR = 10000       # mmcv batched_nms: at or above this it runs per class instead


def box_tables(coder, boxes, labels, expand_dims_length):
    """What get_targets_single computes from the ground truths alone, for concatenated boxes (a
    LiDARBoxes) and their labels: -> (gt table [T, 7], vote table [T, 7], per-box float table
    [T, 33], direction class long [T]) as msmd_ssd3d_targets_f32 reads them.  Element-wise torch
    ops on the boxes' device, the reference's own expressions, so every value the kernel copies
    out is the reference's bit for bit."""
    center, half, dir_class, dir_res = coder.encode(boxes, labels)
    yaw = boxes.yaw
    # as written (:424-426): enlarged_box(e) already lowers the bottom by e and the head subtracts
    # e AGAIN, so the vote boxes reach 2e below the box and nothing extra above the enlarged top
    enlarged = boxes.enlarged_box(expand_dims_length)
    enlarged.tensor[:, 2] -= expand_dims_length
    table = torch.cat([center, half, dir_res[:, None], torch.sin(-yaw)[:, None],
                       torch.cos(-yaw)[:, None], boxes.corners.reshape(-1, 24)], 1)
    return (boxes.tensor[:, :7].contiguous(), enlarged.tensor[:, :7].contiguous(),
            table.contiguous(), dir_class.contiguous())


@HEADS.register_module()
class SSD3DHead(VoteHead):
    """ssd_3d_head.py:16-80."""

    def __init__(self, num_classes, bbox_coder, in_channels=256, train_cfg=None, test_cfg=None,
                 vote_module_cfg=None, vote_aggregation_cfg=None, pred_layer_cfg=None,
                 conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d"),
                 act_cfg=dict(type="ReLU"), objectness_loss=None, center_loss=None,
                 dir_class_loss=None, dir_res_loss=None, size_res_loss=None, corner_loss=None,
                 vote_loss=None):
        # (the reference's VoteModule defaults gt_per_seed to 3 and VoteHead reads the key)
        vote_module_cfg = dict(vote_module_cfg)
        vote_module_cfg.setdefault("gt_per_seed", 3)
        super().__init__(num_classes, bbox_coder, train_cfg=train_cfg, test_cfg=test_cfg,
                         vote_module_cfg=vote_module_cfg,
                         vote_aggregation_cfg=vote_aggregation_cfg, pred_layer_cfg=pred_layer_cfg,
                         conv_cfg=conv_cfg, norm_cfg=norm_cfg, objectness_loss=objectness_loss,
                         center_loss=center_loss, dir_class_loss=dir_class_loss,
                         dir_res_loss=dir_res_loss, size_class_loss=None,
                         size_res_loss=size_res_loss, semantic_loss=None)
        self.corner_loss = build_loss(corner_loss)
        self.vote_loss = build_loss(vote_loss)
        self.num_candidates = vote_module_cfg["num_points"]

    def _get_cls_out_channels(self):
        return self.num_classes                           # :83-86

    def _get_reg_out_channels(self):
        return 3 + 3 + self.num_dir_bins * 2              # centre, size, direction class + residual

    def _extract_input(self, feat_dict):
        """:95-110 -- the last set-abstraction level of PointNet2SAMSG."""
        return feat_dict["sa_xyz"][-1], feat_dict["sa_features"][-1], feat_dict["sa_indices"][-1]

    # ---------------------------------------------------------------------------------- loss
    def loss(self, bbox_preds, points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask=None,
             pts_instance_mask=None, img_metas=None, gt_bboxes_ignore=None):
        """:112-217 -- the seven terms.  All torch ops, so autograd carries them."""
        targets = self.get_targets(points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask,
                                   pts_instance_mask, bbox_preds)
        (vote_targets, center_targets, size_res_targets, dir_class_targets, dir_res_targets,
         mask_targets, centerness_targets, corner3d_targets, vote_mask, positive_mask,
         negative_mask, centerness_weights, box_loss_weights, heading_res_loss_weight) = targets

        centerness_loss = self.objectness_loss(bbox_preds["obj_scores"].transpose(2, 1),
                                               centerness_targets, weight=centerness_weights)
        center_loss = self.center_loss(bbox_preds["center_offset"], center_targets,
                                       weight=box_loss_weights.unsqueeze(-1))
        dir_class_loss = self.dir_class_loss(bbox_preds["dir_class"].transpose(1, 2),
                                             dir_class_targets, weight=box_loss_weights)
        dir_res_loss = self.dir_res_loss(
            bbox_preds["dir_res_norm"],
            dir_res_targets.unsqueeze(-1).repeat(1, 1, self.num_dir_bins),
            weight=heading_res_loss_weight)
        size_loss = self.size_res_loss(bbox_preds["size"], size_res_targets,
                                       weight=box_loss_weights.unsqueeze(-1))

        # corner loss: decode with the TARGET direction class (one-hot), centre as the gravity
        # centre (origin (0.5, 0.5, 0.5))
        one_hot_dir_class_targets = dir_class_targets.new_zeros(bbox_preds["dir_class"].shape)
        one_hot_dir_class_targets.scatter_(2, dir_class_targets.unsqueeze(-1), 1)
        pred_bbox3d = self.bbox_coder.decode(dict(
            center=bbox_preds["center"], dir_res=bbox_preds["dir_res"],
            dir_class=one_hot_dir_class_targets, size=bbox_preds["size"]))
        pred_bbox3d = pred_bbox3d.reshape(-1, pred_bbox3d.shape[-1])
        pred_bbox3d = LiDARBoxes(pred_bbox3d.clone(), box_dim=pred_bbox3d.shape[-1],
                                 with_yaw=self.bbox_coder.with_rot, origin=(0.5, 0.5, 0.5))
        pred_corners3d = pred_bbox3d.corners.reshape(-1, 8, 3)
        corner_loss = self.corner_loss(pred_corners3d, corner3d_targets.reshape(-1, 8, 3),
                                       weight=box_loss_weights.view(-1, 1, 1))

        vote_loss = self.vote_loss(bbox_preds["vote_offset"].transpose(1, 2), vote_targets,
                                   weight=vote_mask.unsqueeze(-1))
        return dict(centerness_loss=centerness_loss, center_loss=center_loss,
                    dir_class_loss=dir_class_loss, dir_res_loss=dir_res_loss,
                    size_res_loss=size_loss, corner_loss=corner_loss, vote_loss=vote_loss)

    # ------------------------------------------------------------------------------- targets
    def get_targets(self, points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask=None,
                    pts_instance_mask=None, bbox_preds=None):
        """:219-305 -- the reference's 14-tuple, from one kernel call for the batch and no host
        read.  Unlike the reference the caller's lists are left as they are.  The per-box tables
        are computed where the ground truths live: on the host when the loader left them there
        (one small upload each, bit for bit the reference's CPU values), else on the device."""
        assert self.bbox_coder.with_rot or pts_semantic_mask is not None
        aggregated = bbox_preds["aggregated_points"]
        device = aggregated.device
        put = lambda t: t.to(device, non_blocking=True)                          # noqa: E731
        rows, labels, counts = [], [], []
        for boxes, lab in zip(gt_bboxes_3d, gt_labels_3d):
            if not isinstance(boxes, LiDARBoxes):
                # the Depth-box branch of _assign_targets_by_points_inside is not built
                raise NotImplementedError("SSD3DHead: ground truths must be LiDARBoxes")
            if len(lab) == 0:
                # :243-248 the fake box of a sample without labels (a length the host knows): one
                # all-zero box of label 0.  It holds no point, so every candidate is a negative
                rows.append(boxes.tensor.new_zeros(1, boxes.tensor.shape[-1]))
                labels.append(lab.new_zeros(1))
            else:
                rows.append(boxes.tensor)
                labels.append(lab)
            counts.append(int(rows[-1].shape[0]))
        if any(t.is_cuda for t in rows + labels):
            rows, labels = [put(t) for t in rows], [put(t) for t in labels]
        flat_labels = torch.cat(labels).long()
        tables = box_tables(self.bbox_coder, LiDARBoxes(torch.cat(rows)), flat_labels,
                            _cfg_get(self.train_cfg, "expand_dims_length"))
        gt_table, vote_table, box_table, dir_class = [put(t) for t in tables]
        flat_labels = put(flat_labels).contiguous()
        box_offsets = put(torch.tensor(np.concatenate([[0], np.cumsum(counts)]),
                                       dtype=torch.int32))

        agg = aggregated.detach().float().contiguous()
        seeds = bbox_preds["seed_points"].detach().float()
        # as written: a candidate outside every box is assigned the sample's last valid box and
        # still computes centerness against it (almost always 0) -- the kernel does the same
        (vote_targets, center_targets, size_res_targets, dir_class_targets, dir_res_targets,
         mask_targets, centerness_targets, corner3d_targets, vote_mask, positive_mask,
         negative_mask) = K.ssd3d_targets(
            agg, seeds, gt_table, vote_table, flat_labels, box_offsets, box_table, dir_class,
            self.num_classes, _cfg_get(self.train_cfg, "pos_distance_thr"))

        # as written (:283): not detached -- the aggregated points are the clamped votes, so the
        # centre loss also reaches the vote layers through its target
        center_targets = center_targets - aggregated
        centerness_weights = (positive_mask + negative_mask).unsqueeze(-1).repeat(
            1, 1, self.num_classes).float()
        centerness_weights = centerness_weights / (centerness_weights.sum() + 1e-6)
        vote_mask = vote_mask / (vote_mask.sum() + 1e-6)
        box_loss_weights = positive_mask / (positive_mask.sum() + 1e-6)
        batch_size, proposal_num = dir_class_targets.shape[:2]
        heading_label_one_hot = dir_class_targets.new_zeros(
            (batch_size, proposal_num, self.num_dir_bins))
        heading_label_one_hot.scatter_(2, dir_class_targets.unsqueeze(-1), 1)
        heading_res_loss_weight = heading_label_one_hot * box_loss_weights.unsqueeze(-1)
        return (vote_targets, center_targets, size_res_targets, dir_class_targets,
                dir_res_targets, mask_targets, centerness_targets, corner3d_targets, vote_mask,
                positive_mask, negative_mask, centerness_weights, box_loss_weights,
                heading_res_loss_weight)

    # --------------------------------------------------------------------------------- boxes
    def nms_keep_mask(self, minmax_bev, obj_scores, bbox_classes):
        """multiclass_nms_single's batched_nms (:511-518) for every sample at once: minmax_bev
        [B, P, 4] (x1, y1, x2, y2), obj_scores [B, P], bbox_classes long [B, P] -> bool [B, P],
        the boxes NMS keeps after the max_output_num cut.  No host read."""
        batch, proposals = obj_scores.shape
        if proposals >= NMS_SPLIT_THR:
            raise NotImplementedError("SSD3DHead: %d boxes per sample; mmcv's batched_nms leaves "
                                      "its single-call branch at %d" % (proposals, NMS_SPLIT_THR))
        device = obj_scores.device
        nms_cfg = dict(_cfg_get(self.test_cfg, "nms_cfg"))
        if nms_cfg.pop("type", "nms") != "nms" or nms_cfg.pop("class_agnostic", False):
            raise NotImplementedError("SSD3DHead: nms_cfg must be dict(type='nms', iou_thr=...)")
        # batched_nms: boxes + class * (boxes.max() + 1), the maximum per call = per sample
        max_coordinate = minmax_bev.reshape(batch, -1).max(1)[0]
        shift = bbox_classes.to(minmax_bev) * (max_coordinate + 1)[:, None]
        boxes_for_nms = (minmax_bev + shift[..., None]).reshape(batch * proposals, 4)
        order = torch.sort(obj_scores, dim=1, descending=True, stable=True)[1]
        order = (order + torch.arange(batch, device=device)[:, None] * proposals).reshape(-1)
        offsets = torch.arange(batch + 1, dtype=torch.int32, device=device) * proposals
        thresh = torch.full((batch,), float(nms_cfg["iou_thr"]), dtype=torch.float32,
                            device=device)
        keep, _ = K.nms_segments(K.NMS_MMCV, boxes_for_nms[order].contiguous(), offsets, thresh,
                                 proposals,
                                 post_max=int(_cfg_get(self.test_cfg, "max_output_num")),
                                 order=order)
        nms_mask = torch.zeros(batch * proposals + 1, dtype=torch.bool, device=device)
        nms_mask[(keep + 1).reshape(-1)] = True                      # -1 lands in the spare slot
        return nms_mask[1:].view(batch, proposals)

    def get_bboxes(self, points, bbox_preds, input_metas=None, rescale=False):
        """:439-543 for the whole batch -> a list of (LiDARBoxes, scores, labels) per sample."""
        sem_scores = torch.sigmoid(bbox_preds["obj_scores"]).transpose(1, 2)
        obj_scores = sem_scores.max(-1)[0]
        bbox3d = self.bbox_coder.decode(bbox_preds)
        batch, proposals = bbox3d.shape[:2]
        device = bbox3d.device
        with_yaw = self.bbox_coder.with_rot
        # as written: the decoded centre is taken as the TOP centre (origin (0.5, 0.5, 1.0))
        boxes = LiDARBoxes(bbox3d.reshape(batch * proposals, -1).clone(),
                           box_dim=bbox3d.shape[-1], with_yaw=with_yaw, origin=(0.5, 0.5, 1.0))
        # as written (:492-502): the reference counts the points in every box and then tests
        # `box_indices >= 0` (the Depth branch: `.sum(1) >= 0`), which holds for every box: no
        # box is ever dropped for being empty.  The points-in-boxes pass is therefore not run.
        corner3d = boxes.corners
        low, high = torch.min(corner3d, dim=1)[0], torch.max(corner3d, dim=1)[0]
        minmax_bev = torch.cat([low[:, :2], high[:, :2]], 1).view(batch, proposals, 4)
        bbox_classes = torch.argmax(sem_scores, -1)
        kept = self.nms_keep_mask(minmax_bev, obj_scores, bbox_classes)
        selected = kept & (obj_scores >= _cfg_get(self.test_cfg, "score_thr"))

        chosen = selected.cpu()                                      # the one host read
        results = []
        per_class = _cfg_get(self.test_cfg, "per_class_proposal")
        flat_scores, flat_classes = obj_scores.reshape(-1), bbox_classes.reshape(-1)
        for b in range(batch):
            index = (torch.nonzero(chosen[b]).flatten() + b * proposals).to(device)
            box_b, obj_b, cls_b = boxes.tensor[index], flat_scores[index], flat_classes[index]
            if per_class:
                # as written (:528-537): the SAME selection once per class, label filled with k
                classes = sem_scores.shape[-1]
                bbox_selected = box_b.repeat(classes, 1)
                score_selected = obj_b.repeat(classes)
                labels = torch.arange(classes, device=device).repeat_interleave(index.numel())
            else:
                bbox_selected, score_selected, labels = box_b, obj_b, cls_b
            results.append((LiDARBoxes(bbox_selected.clone(), box_dim=bbox_selected.shape[-1],
                                       with_yaw=with_yaw), score_selected, labels))
        return results
