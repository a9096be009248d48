"""H3DNet's second stage: H3DBboxHead (mmdet3d/models/roi_heads/bbox_heads/h3d_bbox_head.py)
and H3DRoIHead (mmdet3d/models/roi_heads/h3d_roi_head.py), under the reference's attribute and
parameter names (surface_center_matcher, line_center_matcher, matching_conv, matching_pred,
semantic_matching_conv, semantic_matching_pred, surface_feats_aggregation,
line_feats_aggregation, bbox_pred.{0..3}; primitive_z / primitive_xy / primitive_line /
bbox_head), so its checkpoints load.

`get_targets` is H3DBboxHead.get_targets (:655-759) for the whole batch: where the reference
runs get_targets_single (:761-932) once per sample under multi_apply -- three chamfer_distance
calls that expand [1, N, M, 3], two get_surface_line_center calls and about sixty small ops,
seven of them masked assignments with a host read each -- this pads the ground truths once and
makes one call of msmd_h3d_cue_targets_f32 (csrc/h3d.hip), with nothing read back.

Deviation: the reference replaces an empty sample's entries of the caller's gt_bboxes_3d /
gt_labels_3d lists by a zero box and a zero label, in place.  Here the padding happens on the
batch tensor and the caller's lists are left as they were.

Deviation: VoteHead.get_targets returns 14 tensors (assigned_center_targets is the eighth) and
the reference's H3DBboxHead.loss unpacks 13 (:348-351), so its H3DNet.forward_train raises
ValueError as written; its unit test passes a hand-made 13-tuple.  `loss` here takes both: when
14 arrive, assigned_center_targets is dropped.

Quirks kept: get_bboxes(suffix=) mixes the rpn head's unsuffixed sem_scores / dir_class /
size_class with the suffixed centre and residuals (:464-476); forward and loss call
get_surface_line_center on the flattened B * P boxes, so its rotation index runs over the whole
batch.  aug_test is not built.
"""
import copy

import torch
from torch import nn
from torch.nn import functional as F

from . import kernels as K
from .head import Conv1d
from .head_loss import DepthBoxes, _box_tensor
from .losses import build_loss
from .pointnet_modules import build_sa_module
from .primitive_head import prepare_primitive_inputs
from .registry import HEADS, build_head
from .vote_head import _cfg_get, _conv_module, build_bbox_coder, multiclass_nms_batch

TARGET_NAMES = K.H3D_CUE_TARGET_NAMES
# bbox_preds keys get_targets reads (:704-737)
PRED_KEYS = ("aggregated_points", "surface_center_pred", "pred_line_center",
             "surface_center_object", "line_center_object", "surface_sem_pred",
             "sem_cls_scores_line")


def pad_ground_truths(gt_bboxes_3d, gt_labels_3d, device):
    """Lists of per-sample boxes (objects with `.tensor` [G_b, 7] in bottom-centre form, or such
    tensors) and labels long [G_b] -> (boxes float32 [B, G, 7] in GRAVITY-centre form, labels
    long [B, G], counts int32 [B]) on `device`, G = max(1, max G_b), zero padded.  An empty
    sample counts one box: the reference's zero box with label 0 (:685-698).  The counts come
    from the shapes, so nothing is read back; the lists are not modified."""
    if len(gt_bboxes_3d) != len(gt_labels_3d):
        raise ValueError("one label tensor per box set")
    tensors = [_box_tensor(b) for b in gt_bboxes_3d]
    for t, l in zip(tensors, gt_labels_3d):
        if t.dim() != 2 or t.shape[1] != 7 or l.dim() != 1 or l.shape[0] != t.shape[0]:
            raise ValueError("ground truths are [G, 7] boxes with [G] labels, got %s and %s"
                             % (tuple(t.shape), tuple(l.shape)))
    batch = len(tensors)
    width = max([1] + [t.shape[0] for t in tensors])
    boxes = torch.zeros((batch, width, 7), dtype=torch.float32, device=device)
    labels = torch.zeros((batch, width), dtype=torch.long, device=device)
    for b, (t, l) in enumerate(zip(tensors, gt_labels_3d)):
        if t.shape[0]:
            boxes[b, :t.shape[0]] = t.to(device=device, dtype=torch.float32)
            labels[b, :t.shape[0]] = l.to(device=device, dtype=torch.long)
    # DepthBoxes.gravity_center's arithmetic: z_bottom + z_size * 0.5
    boxes[:, :, 2] = boxes[:, :, 2] + boxes[:, :, 5] * 0.5
    counts = torch.tensor([max(1, t.shape[0]) for t in tensors], dtype=torch.int32)
    return boxes, labels, counts.to(device, non_blocking=True)


def get_targets(bbox_preds, gt_bboxes_3d, gt_labels_3d, train_cfg):
    """H3DBboxHead.get_targets for the batch in one kernel call.  bbox_preds holds PRED_KEYS as
    the head's forward and the primitive heads leave them (device tensors); train_cfg holds
    kernels.H3D_CUE_THRESHOLDS.  -> the reference's eight stacked results in its order
    (TARGET_NAMES): cues_objectness_label, cues_sem_label, proposal_objectness_label, cues_mask,
    cues_match_mask, proposal_objectness_mask, cues_matching_label, obj_surface_line_center."""
    preds = [bbox_preds[k].detach().float().contiguous() for k in PRED_KEYS]
    aggregated, surface_pred, line_pred, surface_obj, line_obj, surface_sem, line_sem = preds
    if len(gt_labels_3d) != aggregated.shape[0]:
        raise ValueError("one set of ground truths per sample")
    boxes, labels, counts = pad_ground_truths(gt_bboxes_3d, gt_labels_3d, aggregated.device)
    return K.h3d_cue_targets(aggregated, boxes, counts, labels, surface_pred, line_pred,
                             surface_sem, line_sem, surface_obj, line_obj, train_cfg)


def _face_major(centers, batch_size, per_box):
    """[B * P * k, 3] box-major rows -> [B, k * P, 3], row f * P + p (:253-257)."""
    return centers.reshape(batch_size, -1, per_box, 3).transpose(1, 2).reshape(batch_size, -1, 3)


def _cue_centers(boxes, with_yaw):
    """Decoded boxes [B, P, 7] (gravity centre) -> (surface centres [B, 6P, 3], line centres
    [B, 12P, 3]) of DepthInstance3DBoxes.get_surface_line_center on the flattened B * P boxes."""
    batch_size = boxes.shape[0]
    flat = DepthBoxes(boxes.reshape(-1, 7).clone(), box_dim=boxes.shape[-1], with_yaw=with_yaw,
                      origin=(0.5, 0.5, 0.5))
    surface, line = flat.get_surface_line_center()
    return _face_major(surface, batch_size, 6), _face_major(line, batch_size, 12)


@HEADS.register_module()
class H3DBboxHead(nn.Module):
    """h3d_bbox_head.py:16-199.  Deviation from the reference: `loss` takes the rpn head's
    targets as 13 or as 14 tensors (see the module docstring)."""

    def __init__(self, num_classes, suface_matching_cfg, line_matching_cfg, bbox_coder,
                 train_cfg=None, test_cfg=None, gt_per_seed=1, num_proposal=256,
                 feat_channels=(128, 128), primitive_feat_refine_streams=2,
                 primitive_refine_channels=(128, 128, 128), upper_thresh=100.0,
                 surface_thresh=0.5, line_thresh=0.5, conv_cfg=dict(type="Conv1d"),
                 norm_cfg=dict(type="BN1d"), objectness_loss=None, center_loss=None,
                 dir_class_loss=None, dir_res_loss=None, size_class_loss=None, size_res_loss=None,
                 semantic_loss=None, cues_objectness_loss=None, cues_semantic_loss=None,
                 proposal_objectness_loss=None, primitive_center_loss=None):
        super().__init__()
        self.num_classes = num_classes
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        self.gt_per_seed = gt_per_seed
        self.num_proposal = num_proposal
        self.with_angle = bbox_coder["with_rot"]
        self.upper_thresh = upper_thresh
        self.surface_thresh = surface_thresh
        self.line_thresh = line_thresh

        self.objectness_loss = build_loss(objectness_loss)
        self.center_loss = build_loss(center_loss)
        self.dir_class_loss = build_loss(dir_class_loss)
        self.dir_res_loss = build_loss(dir_res_loss)
        self.size_class_loss = build_loss(size_class_loss)
        self.size_res_loss = build_loss(size_res_loss)
        self.semantic_loss = build_loss(semantic_loss)

        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.num_sizes = self.bbox_coder.num_sizes
        self.num_dir_bins = self.bbox_coder.num_dir_bins

        self.cues_objectness_loss = build_loss(cues_objectness_loss)
        self.cues_semantic_loss = build_loss(cues_semantic_loss)
        self.proposal_objectness_loss = build_loss(proposal_objectness_loss)
        self.primitive_center_loss = build_loss(primitive_center_loss)

        assert suface_matching_cfg["mlp_channels"][-1] == line_matching_cfg["mlp_channels"][-1]
        # (copies: the SA module adds the xyz channels to its mlp_channels list in place)
        self.surface_center_matcher = build_sa_module(copy.deepcopy(suface_matching_cfg))
        self.line_center_matcher = build_sa_module(copy.deepcopy(line_matching_cfg))

        dims = suface_matching_cfg["mlp_channels"][-1]

        def conv(in_channels, out_channels):
            return _conv_module(in_channels, out_channels, conv_cfg, norm_cfg, None, bias=True)

        self.matching_conv = conv(dims, dims)
        self.matching_pred = Conv1d(dims, 2, 1)
        self.semantic_matching_conv = conv(dims, dims)
        self.semantic_matching_pred = Conv1d(dims, 2, 1)
        self.surface_feats_aggregation = nn.Sequential(
            *[conv(dims, dims) for _ in range(primitive_feat_refine_streams)])
        self.line_feats_aggregation = nn.Sequential(
            *[conv(dims, dims) for _ in range(primitive_feat_refine_streams)])

        prev_channel = 18 * dims                         # surface centres (6) + line centres (12)
        self.bbox_pred = nn.ModuleList()
        for channels in primitive_refine_channels:
            self.bbox_pred.append(conv(prev_channel, channels))
            prev_channel = channels
        # objectness (2), centre residual (3), direction class + residual, size class + residual
        conv_out_channel = (2 + 3 + bbox_coder["num_dir_bins"] * 2 + bbox_coder["num_sizes"] * 4 +
                            self.num_classes)
        self.bbox_pred.append(Conv1d(prev_channel, conv_out_channel, 1))

    def init_weights(self, pretrained=None):
        pass

    def forward(self, feats_dict, sample_mod):
        """:210-316."""
        ret_dict = {}
        aggregated_points = feats_dict["aggregated_points"]
        original_feature = feats_dict["aggregated_features"]
        batch_size = original_feature.shape[0]
        object_proposal = original_feature.shape[2]

        z_center = feats_dict["pred_z_center"]
        xy_center = feats_dict["pred_xy_center"]
        z_semantic = feats_dict["sem_cls_scores_z"]
        xy_semantic = feats_dict["sem_cls_scores_xy"]
        z_feature = feats_dict["aggregated_features_z"]
        xy_feature = feats_dict["aggregated_features_xy"]
        line_center = feats_dict["pred_line_center"]
        line_feature = feats_dict["aggregated_features_line"]

        surface_center_pred = torch.cat((z_center, xy_center), dim=1)
        ret_dict["surface_center_pred"] = surface_center_pred
        ret_dict["surface_sem_pred"] = torch.cat((z_semantic, xy_semantic), dim=1)

        # the surface and line centres of the rpn proposals
        obj_surface_center, obj_line_center = _cue_centers(feats_dict["proposal_list"],
                                                           self.with_angle)
        ret_dict["surface_center_object"] = obj_surface_center
        ret_dict["line_center_object"] = obj_line_center

        # primitive z and xy features -> rpn proposals
        surface_center_feature_pred = torch.cat((z_feature, xy_feature), dim=2)
        surface_center_feature_pred = torch.cat(
            (surface_center_feature_pred.new_zeros(
                (batch_size, 6, surface_center_feature_pred.shape[2])),
             surface_center_feature_pred), dim=1)
        _, surface_features, _ = self.surface_center_matcher(
            surface_center_pred, surface_center_feature_pred, target_xyz=obj_surface_center)

        line_feature = torch.cat(
            (line_feature.new_zeros((batch_size, 12, line_feature.shape[2])), line_feature), dim=1)
        _, line_features, _ = self.line_center_matcher(
            line_center, line_feature, target_xyz=obj_line_center)

        combine_features = torch.cat((surface_features, line_features), dim=2)
        matching_score = self.matching_pred(self.matching_conv(combine_features))
        ret_dict["matching_score"] = matching_score.transpose(2, 1)
        semantic_matching_score = self.semantic_matching_pred(
            self.semantic_matching_conv(combine_features))
        ret_dict["semantic_matching_score"] = semantic_matching_score.transpose(2, 1)

        surface_features = self.surface_feats_aggregation(surface_features)
        line_features = self.line_feats_aggregation(line_features)
        surface_features = surface_features.reshape(batch_size, -1, object_proposal)
        line_features = line_features.reshape(batch_size, -1, object_proposal)
        combine_feature = torch.cat((surface_features, line_features), dim=1)

        bbox_predictions = self.bbox_pred[0](combine_feature)
        bbox_predictions = bbox_predictions + original_feature
        for conv_module in self.bbox_pred[1:]:
            bbox_predictions = conv_module(bbox_predictions)

        refine_decode_res = self.bbox_coder.split_pred(
            bbox_predictions[:, :self.num_classes + 2],
            bbox_predictions[:, self.num_classes + 2:], aggregated_points)
        for key in refine_decode_res.keys():
            ret_dict[key + "_optimized"] = refine_decode_res[key]
        return ret_dict

    def loss(self, bbox_preds, points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask=None,
             pts_instance_mask=None, img_metas=None, rpn_targets=None, gt_bboxes_ignore=None):
        """:318-444.  rpn_targets: VoteHead.get_targets' 14 tensors, or the reference's 13
        (without assigned_center_targets)."""
        rpn_targets = tuple(rpn_targets)
        if len(rpn_targets) == 14:
            rpn_targets = rpn_targets[:7] + rpn_targets[8:]
        if len(rpn_targets) != 13:
            raise ValueError("rpn_targets holds 13 or 14 tensors, got %d" % len(rpn_targets))
        (vote_targets, vote_target_masks, size_class_targets, size_res_targets,
         dir_class_targets, dir_res_targets, center_targets, mask_targets, valid_gt_masks,
         objectness_targets, objectness_weights, box_loss_weights, valid_gt_weights) = rpn_targets

        losses = {}
        refined_proposal_loss = self.get_proposal_stage_loss(
            bbox_preds, size_class_targets, size_res_targets, dir_class_targets,
            dir_res_targets, center_targets, mask_targets, objectness_targets,
            objectness_weights, box_loss_weights, valid_gt_weights, suffix="_optimized")
        for key in refined_proposal_loss.keys():
            losses[key + "_optimized"] = refined_proposal_loss[key]

        bbox3d_optimized = self.bbox_coder.decode(bbox_preds, suffix="_optimized")
        targets = self.get_targets(points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask,
                                   pts_instance_mask, bbox_preds)
        (cues_objectness_label, cues_sem_label, proposal_objectness_label, cues_mask,
         cues_match_mask, proposal_objectness_mask, cues_matching_label,
         obj_surface_line_center) = targets

        objectness_scores = bbox_preds["matching_score"]
        objectness_scores_sem = bbox_preds["semantic_matching_score"]
        primitive_objectness_loss = self.cues_objectness_loss(
            objectness_scores.transpose(2, 1), cues_objectness_label, weight=cues_mask,
            avg_factor=cues_mask.sum() + 1e-6)
        primitive_sem_loss = self.cues_semantic_loss(
            objectness_scores_sem.transpose(2, 1), cues_sem_label, weight=cues_mask,
            avg_factor=cues_mask.sum() + 1e-6)

        objectness_scores = bbox_preds["obj_scores_optimized"]
        objectness_loss_refine = self.proposal_objectness_loss(
            objectness_scores.transpose(2, 1), proposal_objectness_label)
        primitive_matching_loss = (objectness_loss_refine * cues_match_mask).sum() / (
            cues_match_mask.sum() + 1e-6) * 0.5
        primitive_sem_matching_loss = (objectness_loss_refine * proposal_objectness_mask).sum() / (
            proposal_objectness_mask.sum() + 1e-6) * 0.5

        pred_surface_line_center = torch.cat(_cue_centers(bbox3d_optimized, self.with_angle), 1)
        square_dist = self.primitive_center_loss(pred_surface_line_center,
                                                 obj_surface_line_center)
        match_dist = torch.sqrt(square_dist.sum(dim=-1) + 1e-6)
        primitive_centroid_reg_loss = torch.sum(match_dist * cues_matching_label) / (
            cues_matching_label.sum() + 1e-6)

        losses.update(dict(primitive_objectness_loss=primitive_objectness_loss,
                           primitive_sem_loss=primitive_sem_loss,
                           primitive_matching_loss=primitive_matching_loss,
                           primitive_sem_matching_loss=primitive_sem_matching_loss,
                           primitive_centroid_reg_loss=primitive_centroid_reg_loss))
        return losses

    def get_targets(self, points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask=None,
                    pts_instance_mask=None, bbox_preds=None):
        """:655-759 for the whole batch: one kernel call, nothing read back, the caller's lists
        untouched (the module's get_targets)."""
        return get_targets(bbox_preds, gt_bboxes_3d, gt_labels_3d, self.train_cfg)

    def get_bboxes(self, points, bbox_preds, input_metas=None, rescale=False, suffix=""):
        """:446-490 for the whole batch.  The class scores, the direction class and the size
        class are the rpn head's, whatever the suffix (:464-476)."""
        obj_scores = F.softmax(bbox_preds["obj_scores" + suffix], dim=-1)[..., -1]
        sem_scores = F.softmax(bbox_preds["sem_scores"], dim=-1)
        prediction_collection = dict(center=bbox_preds["center" + suffix],
                                     dir_class=bbox_preds["dir_class"],
                                     dir_res=bbox_preds["dir_res" + suffix],
                                     size_class=bbox_preds["size_class"],
                                     size_res=bbox_preds["size_res" + suffix])
        bbox3d = self.bbox_coder.decode(prediction_collection)
        return multiclass_nms_batch(obj_scores, sem_scores, bbox3d, points,
                                    self.bbox_coder.with_rot, self.test_cfg)

    def get_proposal_stage_loss(self, bbox_preds, size_class_targets, size_res_targets,
                                dir_class_targets, dir_res_targets, center_targets, mask_targets,
                                objectness_targets, objectness_weights, box_loss_weights,
                                valid_gt_weights, suffix=""):
        """:552-659."""
        objectness_loss = self.objectness_loss(
            bbox_preds["obj_scores" + suffix].transpose(2, 1), objectness_targets,
            weight=objectness_weights)
        source2target_loss, target2source_loss = self.center_loss(
            bbox_preds["center" + suffix], center_targets, src_weight=box_loss_weights,
            dst_weight=valid_gt_weights)
        center_loss = source2target_loss + target2source_loss
        dir_class_loss = self.dir_class_loss(
            bbox_preds["dir_class" + suffix].transpose(2, 1), dir_class_targets,
            weight=box_loss_weights)
        batch_size, proposal_num = size_class_targets.shape[:2]
        heading_label_one_hot = dir_class_targets.new_zeros(
            (batch_size, proposal_num, self.num_dir_bins))
        heading_label_one_hot.scatter_(2, dir_class_targets.unsqueeze(-1), 1)
        dir_res_norm = (bbox_preds["dir_res_norm" + suffix] * heading_label_one_hot).sum(dim=-1)
        dir_res_loss = self.dir_res_loss(dir_res_norm, dir_res_targets, weight=box_loss_weights)
        size_class_loss = self.size_class_loss(
            bbox_preds["size_class" + suffix].transpose(2, 1), size_class_targets,
            weight=box_loss_weights)
        one_hot_size_targets = box_loss_weights.new_zeros(
            (batch_size, proposal_num, self.num_sizes))
        one_hot_size_targets.scatter_(2, size_class_targets.unsqueeze(-1), 1)
        one_hot_size_targets_expand = one_hot_size_targets.unsqueeze(-1).repeat(1, 1, 1, 3)
        size_residual_norm = (bbox_preds["size_res_norm" + suffix] *
                              one_hot_size_targets_expand).sum(dim=2)
        box_loss_weights_expand = box_loss_weights.unsqueeze(-1).repeat(1, 1, 3)
        size_res_loss = self.size_res_loss(size_residual_norm, size_res_targets,
                                           weight=box_loss_weights_expand)
        semantic_loss = self.semantic_loss(
            bbox_preds["sem_scores" + suffix].transpose(2, 1), mask_targets,
            weight=box_loss_weights)
        return dict(objectness_loss=objectness_loss, semantic_loss=semantic_loss,
                    center_loss=center_loss, dir_class_loss=dir_class_loss,
                    dir_res_loss=dir_res_loss, size_class_loss=size_class_loss,
                    size_res_loss=size_res_loss)


@HEADS.register_module()
class H3DRoIHead(nn.Module):
    """h3d_roi_head.py: the three primitive heads and the bbox head, under the reference's
    attribute names.  The ground truth the primitive heads need is prepared once per step and
    shared (prepare_primitive_inputs), where the reference runs get_targets three times over the
    same points."""

    def __init__(self, primitive_list, bbox_head=None, train_cfg=None, test_cfg=None):
        super().__init__()
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        assert len(primitive_list) == 3
        self.primitive_z = build_head(primitive_list[0])
        self.primitive_xy = build_head(primitive_list[1])
        self.primitive_line = build_head(primitive_list[2])
        # (a copy: the reference writes train_cfg / test_cfg into the caller's dict, :43-44)
        self.bbox_head = bbox_head if isinstance(bbox_head, nn.Module) else \
            build_head(dict(bbox_head, train_cfg=train_cfg, test_cfg=test_cfg))

    def init_weights(self, pretrained=None):
        pass

    @property
    def primitive_heads(self):
        return (self.primitive_z, self.primitive_xy, self.primitive_line)

    def _primitives(self, feats_dict, sample_mod):
        assert sample_mod in ["vote", "seed", "random"]
        for head in self.primitive_heads:
            feats_dict.update(head(feats_dict, sample_mod))

    def forward_train(self, feats_dict, img_metas, points, gt_bboxes_3d, gt_labels_3d,
                      pts_semantic_mask=None, pts_instance_mask=None, gt_bboxes_ignore=None):
        """:51-117 -> the losses of the three primitive heads and of the bbox head."""
        losses = dict()
        sample_mod = _cfg_get(self.train_cfg, "sample_mod")
        self._primitives(feats_dict, sample_mod)
        head = self.primitive_z
        prepared = prepare_primitive_inputs(points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask,
                                            pts_instance_mask, head.num_classes, head.label_bound)
        for head in self.primitive_heads:
            targets = head.get_targets(points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask,
                                       pts_instance_mask, feats_dict, prepared=prepared)
            losses.update(head.loss_from_targets(feats_dict, targets))
        targets = feats_dict.pop("targets")
        feats_dict.update(self.bbox_head(feats_dict, sample_mod))
        losses.update(self.bbox_head.loss(feats_dict, points, gt_bboxes_3d, gt_labels_3d,
                                          pts_semantic_mask, pts_instance_mask, img_metas,
                                          targets, gt_bboxes_ignore))
        return losses

    def simple_test(self, feats_dict, img_metas, points, rescale=False):
        """:119-158 (bbox3d2result's fields)."""
        sample_mod = _cfg_get(self.test_cfg, "sample_mod")
        self._primitives(feats_dict, sample_mod)
        feats_dict.update(self.bbox_head(feats_dict, sample_mod))
        bbox_list = self.bbox_head.get_bboxes(points, feats_dict, img_metas, rescale=rescale,
                                              suffix="_optimized")
        return [dict(boxes_3d=b, scores_3d=s, labels_3d=l) for b, s, l in bbox_list]
