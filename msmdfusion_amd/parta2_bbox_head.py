"""Part-A2's RoI box head (COVERAGE n10): PartA2BboxHead with the reference's constructor
arguments, defaults, attribute names and state-dict keys.

Reference: mmdet3d/models/roi_heads/bbox_heads/parta2_bbox_head.py.

  forward      the reference's graph on this package's pieces: `part_feats.sum(-1).nonzero()`
               (one host read: the planning read every sparse conv needs), SubM stacks from
               make_sparse_convmodule with the reference's indice_keys, SparseMaxPool3d(2, 2),
               .dense(), Conv1d ConvModules.  No non-zero cell: decided on the host from that
               count, a RuntimeError, nothing launched on an empty tensor (the reference fails
               inside spconv).
  get_targets  takes the fused RoISampleBatch of PartAggregationROIHead._assign_and_sample (the
               tensors csrc/roi_targets.hip wrote; only the two weight normalisations are left)
               or a list of per-sample sampling results: the composition path, the reference's
               _get_target_single op for op, following the input dtype (a float64 run is the
               yardstick of the kernel's float32 arithmetic).
  loss         no host read.  The reference branches on `pos_inds.any() == 0` and gathers with
               boolean masks (:315-331); here every RoI row goes through the arithmetic with the
               non-positive rows' predictions replaced by zeros, and the terms are masked sums.
               Without a positive row the sums are the reference's fake zero.
  get_bboxes   the decode as written, then the lists of all (sample, class) pairs in ONE
               K.nms_segments call and one host read (the kept counts); only the rows above
               score_thr enter the lists (their lengths stay on the device).  The reference runs
               multi_class_nms per sample with a host read per class; that loop serves samples
               with more RoIs than the batched kernel's list length.

Reference behaviour kept as written: the result's labels come from the RPN's labels_3d, not
from the class of the NMS loop (:547); a box may be selected once per class; the order is
class-major, then NMS order; score_thr is compared against the RPN's cls_preds (:540, 600); an
empty selection gives [0, 7] boxes.

Deviations:
  - loss_corner is the mean over the positive rows (a scalar); the reference returns the
    unreduced [n_pos] vector (:350-352), whose mean the detector's loss parser takes.
  - loss_bbox / loss_corner without a positive row are zeros that depend on the predictions
    (gradient zero) where the reference has constants (:318-320).
  - get_bboxes takes the number of samples from its lists, the reference from
    `roi_batch_id.max().item() + 1` (:521); the RoIs must be grouped by sample in list order,
    which bbox3d2roi produces.
"""
import numpy as np
import torch
from torch import nn

from . import kernels as K
from .anchor_head import _get, build_bbox_coder, xywhr2xyxyr
from .head_loss import LiDARBoxes
from .losses import build_loss
from .registry import HEADS, build_conv_layer, build_norm_layer
from .semantic_head import rotation_3d_in_axis_z
from .sparse_block import make_sparse_convmodule
from . import spconv


class _ConvModule(nn.Module):
    """mmcv.cnn.ConvModule as the head uses it: kernel size 1, bias='auto' (a conv bias only
    without a norm), attribute names conv / bn / activate."""

    def __init__(self, in_channels, out_channels, conv_cfg, norm_cfg=None, act=True):
        super().__init__()
        self.conv = build_conv_layer(conv_cfg, in_channels, out_channels, 1, padding=0,
                                     bias=norm_cfg is None)
        self.bn = None if norm_cfg is None else build_norm_layer(norm_cfg, out_channels)[1]
        self.activate = nn.ReLU(inplace=True) if act else None

    def forward(self, x):
        x = self.conv(x)
        if self.bn is not None:
            x = self.bn(x)
        return x if self.activate is None else self.activate(x)


@HEADS.register_module()
class PartA2BboxHead(nn.Module):
    """parta2_bbox_head.py:16-223."""

    def __init__(self, num_classes, seg_in_channels, part_in_channels, seg_conv_channels=None,
                 part_conv_channels=None, merge_conv_channels=None, down_conv_channels=None,
                 shared_fc_channels=None, cls_channels=None, reg_channels=None, dropout_ratio=0.1,
                 roi_feat_size=14, with_corner_loss=True,
                 bbox_coder=dict(type="DeltaXYZWLHRBBoxCoder"), conv_cfg=dict(type="Conv1d"),
                 norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01),
                 loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=2.0),
                 loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, reduction="none",
                               loss_weight=1.0)):
        super().__init__()
        self.num_classes = num_classes
        self.with_corner_loss = with_corner_loss
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.loss_bbox = build_loss(loss_bbox)
        self.loss_cls = build_loss(loss_cls)
        self.use_sigmoid_cls = loss_cls.get("use_sigmoid", False)
        if self.loss_bbox.reduction not in ("mean", "sum"):
            raise NotImplementedError("PartA2BboxHead: loss_bbox reduction %r (mean or sum)"
                                      % self.loss_bbox.reduction)

        assert down_conv_channels[-1] == shared_fc_channels[0]

        part_channel_last = part_in_channels
        part_conv = []
        for i, channel in enumerate(part_conv_channels):
            part_conv.append(make_sparse_convmodule(part_channel_last, channel, 3, padding=1,
                                                    norm_cfg=norm_cfg, indice_key=f"rcnn_part{i}",
                                                    conv_type="SubMConv3d"))
            part_channel_last = channel
        self.part_conv = spconv.SparseSequential(*part_conv)

        seg_channel_last = seg_in_channels
        seg_conv = []
        for i, channel in enumerate(seg_conv_channels):
            seg_conv.append(make_sparse_convmodule(seg_channel_last, channel, 3, padding=1,
                                                   norm_cfg=norm_cfg, indice_key=f"rcnn_seg{i}",
                                                   conv_type="SubMConv3d"))
            seg_channel_last = channel
        self.seg_conv = spconv.SparseSequential(*seg_conv)

        self.conv_down = spconv.SparseSequential()
        merge_conv_channel_last = part_channel_last + seg_channel_last
        merge_conv = []
        for i, channel in enumerate(merge_conv_channels):
            merge_conv.append(make_sparse_convmodule(merge_conv_channel_last, channel, 3,
                                                     padding=1, norm_cfg=norm_cfg,
                                                     indice_key="rcnn_down0"))
            merge_conv_channel_last = channel
        down_conv_channel_last = merge_conv_channel_last
        conv_down = []
        for i, channel in enumerate(down_conv_channels):
            conv_down.append(make_sparse_convmodule(down_conv_channel_last, channel, 3, padding=1,
                                                    norm_cfg=norm_cfg, indice_key="rcnn_down1"))
            down_conv_channel_last = channel
        self.conv_down.add_module("merge_conv", spconv.SparseSequential(*merge_conv))
        self.conv_down.add_module("max_pool3d", spconv.SparseMaxPool3d(kernel_size=2, stride=2))
        self.conv_down.add_module("down_conv", spconv.SparseSequential(*conv_down))

        shared_fc_list = []
        pool_size = roi_feat_size // 2
        pre_channel = shared_fc_channels[0] * pool_size**3
        for k in range(1, len(shared_fc_channels)):
            shared_fc_list.append(_ConvModule(pre_channel, shared_fc_channels[k], conv_cfg,
                                              norm_cfg))
            pre_channel = shared_fc_channels[k]
            if k != len(shared_fc_channels) - 1 and dropout_ratio > 0:
                shared_fc_list.append(nn.Dropout(dropout_ratio))
        self.shared_fc = nn.Sequential(*shared_fc_list)

        channel_in = shared_fc_channels[-1]
        cls_channel = 1
        cls_layers = []
        pre_channel = channel_in
        for k in range(0, len(cls_channels)):
            cls_layers.append(_ConvModule(pre_channel, cls_channels[k], conv_cfg, norm_cfg))
            pre_channel = cls_channels[k]
        cls_layers.append(_ConvModule(pre_channel, cls_channel, conv_cfg, act=False))
        if dropout_ratio >= 0:
            cls_layers.insert(1, nn.Dropout(dropout_ratio))
        self.conv_cls = nn.Sequential(*cls_layers)

        reg_layers = []
        pre_channel = channel_in
        for k in range(0, len(reg_channels)):
            reg_layers.append(_ConvModule(pre_channel, reg_channels[k], conv_cfg, norm_cfg))
            pre_channel = reg_channels[k]
        reg_layers.append(_ConvModule(pre_channel, self.bbox_coder.code_size, conv_cfg, act=False))
        if dropout_ratio >= 0:
            reg_layers.insert(1, nn.Dropout(dropout_ratio))
        self.conv_reg = nn.Sequential(*reg_layers)

        self.init_weights()

    def init_weights(self):
        """:225-231: xavier-uniform on every dense conv (bias 0), N(0, 0.001) on the last
        regression conv."""
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.xavier_uniform_(m.weight, gain=1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        last = self.conv_reg[-1].conv
        nn.init.normal_(last.weight, 0, 0.001)
        if last.bias is not None:
            nn.init.constant_(last.bias, 0)

    # ------------------------------------------------------------------ forward
    def forward(self, seg_feats, part_feats):
        """:233-281: pooled [R, X, Y, Z, C] features -> (cls_score [R, 1], bbox_pred [R, code])."""
        rcnn_batch_size = part_feats.shape[0]
        sparse_shape = part_feats.shape[1:4]
        sparse_idx = part_feats.sum(dim=-1).nonzero(as_tuple=False)        # the one host read
        if sparse_idx.shape[0] == 0:
            raise RuntimeError("PartA2BboxHead: the pooled part features of all %d RoIs are zero: "
                               "there is no active cell to convolve" % rcnn_batch_size)
        part_features = part_feats[sparse_idx[:, 0], sparse_idx[:, 1], sparse_idx[:, 2],
                                   sparse_idx[:, 3]]
        seg_features = seg_feats[sparse_idx[:, 0], sparse_idx[:, 1], sparse_idx[:, 2],
                                 sparse_idx[:, 3]]
        coords = sparse_idx.int()
        part_features = spconv.SparseConvTensor(part_features, coords, sparse_shape,
                                                rcnn_batch_size)
        seg_features = spconv.SparseConvTensor(seg_features, coords, sparse_shape, rcnn_batch_size)

        x_part = self.part_conv(part_features)
        x_rpn = self.seg_conv(seg_features)
        merged_feature = torch.cat((x_rpn.features, x_part.features), dim=1)
        shared_feature = spconv.SparseConvTensor(merged_feature, coords, sparse_shape,
                                                 rcnn_batch_size)
        x = self.conv_down(shared_feature)
        shared_feature = x.dense().reshape(rcnn_batch_size, -1, 1)
        shared_feature = self.shared_fc(shared_feature)
        cls_score = self.conv_cls(shared_feature).transpose(1, 2).contiguous().squeeze(dim=1)
        bbox_pred = self.conv_reg(shared_feature).transpose(1, 2).contiguous().squeeze(dim=1)
        return cls_score, bbox_pred

    # ------------------------------------------------------------------ loss
    def loss(self, cls_score, bbox_pred, rois, labels, bbox_targets, pos_gt_bboxes, reg_mask,
             label_weights, bbox_weights):
        """:283-354 without a host read (see the module docstring).  bbox_targets /
        pos_gt_bboxes hold one row per positive RoI, in RoI order."""
        losses = dict()
        rcnn_batch_size = cls_score.shape[0]
        cls_flat = cls_score.view(-1)
        losses["loss_cls"] = self.loss_cls(cls_flat, labels, label_weights)

        code_size = self.bbox_coder.code_size
        pos = reg_mask > 0                                              # [R]
        num_pos = bbox_targets.shape[0]                                 # (a shape: no read)
        pred = bbox_pred.view(rcnn_batch_size, -1)
        pred = torch.where(pos[:, None], pred, torch.zeros_like(pred))
        if num_pos:
            slot = (torch.cumsum(pos.long(), 0) - 1).clamp(min=0)       # row -> its positive row
            targets, gts = bbox_targets[slot], pos_gt_bboxes[slot]
        else:
            targets, gts = torch.zeros_like(pred), torch.zeros_like(pred)
        weights = torch.where(pos, bbox_weights, torch.zeros_like(bbox_weights))
        each = self.loss_bbox(pred.unsqueeze(0), targets.unsqueeze(0),
                              weights.view(-1, 1).repeat(1, pred.shape[-1]).unsqueeze(0),
                              reduction_override="none")
        each = torch.where(pos[None, :, None], each, torch.zeros_like(each)).sum()
        if self.loss_bbox.reduction == "mean":
            each = each / max(num_pos * pred.shape[-1], 1)
        losses["loss_bbox"] = each

        if self.with_corner_loss:
            roi_boxes3d = rois[..., 1:].view(-1, code_size)
            batch_anchors = roi_boxes3d.clone().detach()
            rois_rotation = roi_boxes3d[..., 6].view(-1)
            roi_xyz = roi_boxes3d[..., 0:3].view(-1, 3)
            batch_anchors[..., 0:3] = 0
            pred_boxes3d = self.bbox_coder.decode(batch_anchors,
                                                  pred.view(-1, code_size)).view(-1, code_size)
            centre = rotation_3d_in_axis_z(pred_boxes3d[..., 0:3].unsqueeze(1),
                                           rois_rotation + np.pi / 2).squeeze(1) + roi_xyz
            pred_boxes3d = torch.cat([centre, pred_boxes3d[..., 3:]], dim=-1)
            # (a non-positive row's ground truth: the unit box, so its corners are finite)
            gts = torch.where(pos[:, None], gts, torch.ones_like(gts))
            loss_corner = self.get_corner_loss_lidar(pred_boxes3d, gts)
            loss_corner = torch.where(pos, loss_corner, torch.zeros_like(loss_corner)).sum()
            losses["loss_corner"] = loss_corner / max(num_pos, 1)
        return losses

    # ------------------------------------------------------------------ targets
    def get_targets(self, sampling_results, rcnn_train_cfg, concat=True):
        """:356-394.  sampling_results: the fused RoISampleBatch, or per-sample results with
        pos_bboxes / pos_gt_bboxes / iou (the composition path)."""
        from .parta2_roi_head import RoISampleBatch
        if isinstance(sampling_results, RoISampleBatch):
            if not concat:
                raise NotImplementedError("PartA2BboxHead.get_targets: the fused batch is "
                                          "concatenated")
            r = sampling_results
            label_weights = r.label_weights / torch.clamp(r.label_weights.sum(), min=1.0)
            bbox_weights = r.bbox_weights / torch.clamp(r.bbox_weights.sum(), min=1.0)
            return (r.label, r.bbox_targets, r.pos_gt_bboxes, r.reg_mask, label_weights,
                    bbox_weights)
        targets = [self._get_target_single(res.pos_bboxes, res.pos_gt_bboxes, res.iou,
                                           cfg=rcnn_train_cfg) for res in sampling_results]
        (label, bbox_targets, pos_gt_bboxes, reg_mask, label_weights,
         bbox_weights) = [list(t) for t in zip(*targets)]
        if concat:
            label = torch.cat(label, 0)
            bbox_targets = torch.cat(bbox_targets, 0)
            pos_gt_bboxes = torch.cat(pos_gt_bboxes, 0)
            reg_mask = torch.cat(reg_mask, 0)
            label_weights = torch.cat(label_weights, 0)
            label_weights /= torch.clamp(label_weights.sum(), min=1.0)
            bbox_weights = torch.cat(bbox_weights, 0)
            bbox_weights /= torch.clamp(bbox_weights.sum(), min=1.0)
        return (label, bbox_targets, pos_gt_bboxes, reg_mask, label_weights, bbox_weights)

    def _get_target_single(self, pos_bboxes, pos_gt_bboxes, ious, cfg):
        """:396-460 op for op, in the dtype of its inputs.  Note that the reference is handed
        res.pos_bboxes (the positive RoIs) with the IoUs of all sampled rows."""
        cls_pos_mask = ious > _get(cfg, "cls_pos_thr")
        cls_neg_mask = ious < _get(cfg, "cls_neg_thr")
        interval_mask = (cls_pos_mask == 0) & (cls_neg_mask == 0)
        label = (cls_pos_mask > 0).to(ious.dtype)
        label[interval_mask] = ious[interval_mask] * 2 - 0.5
        label_weights = (label >= 0).to(ious.dtype)
        reg_mask = pos_bboxes.new_zeros(ious.size(0)).long()
        reg_mask[0:pos_gt_bboxes.size(0)] = 1
        bbox_weights = (reg_mask > 0).to(ious.dtype)
        if reg_mask.bool().any():
            pos_gt_bboxes_ct = pos_gt_bboxes.clone().detach()
            roi_center = pos_bboxes[..., 0:3]
            roi_ry = pos_bboxes[..., 6] % (2 * np.pi)
            pos_gt_bboxes_ct[..., 0:3] -= roi_center
            pos_gt_bboxes_ct[..., 6] -= roi_ry
            pos_gt_bboxes_ct[..., 0:3] = rotation_3d_in_axis_z(
                pos_gt_bboxes_ct[..., 0:3].unsqueeze(1), -(roi_ry + np.pi / 2)).squeeze(1)
            ry_label = pos_gt_bboxes_ct[..., 6] % (2 * np.pi)
            opposite_flag = (ry_label > np.pi * 0.5) & (ry_label < np.pi * 1.5)
            ry_label[opposite_flag] = (ry_label[opposite_flag] + np.pi) % (2 * np.pi)
            flag = ry_label > np.pi
            ry_label[flag] = ry_label[flag] - np.pi * 2
            ry_label = torch.clamp(ry_label, min=-np.pi / 2, max=np.pi / 2)
            pos_gt_bboxes_ct[..., 6] = ry_label
            rois_anchor = pos_bboxes.clone().detach()
            rois_anchor[:, 0:3] = 0
            rois_anchor[:, 6] = 0
            bbox_targets = self.bbox_coder.encode(rois_anchor, pos_gt_bboxes_ct)
        else:
            bbox_targets = pos_gt_bboxes.new_empty((0, 7))
        return (label, bbox_targets, pos_gt_bboxes, reg_mask, label_weights, bbox_weights)

    def get_corner_loss_lidar(self, pred_bbox3d, gt_bbox3d, delta=1):
        """:462-495 -> [N]."""
        assert pred_bbox3d.shape[0] == gt_bbox3d.shape[0]
        gt_boxes_structure = LiDARBoxes(gt_bbox3d)
        pred_box_corners = LiDARBoxes(pred_bbox3d).corners
        gt_box_corners = gt_boxes_structure.corners
        flipped = gt_boxes_structure.tensor.clone()
        flipped[:, 6] += np.pi
        gt_box_corners_flip = LiDARBoxes(flipped).corners
        corner_dist = torch.min(torch.norm(pred_box_corners - gt_box_corners, dim=2),
                                torch.norm(pred_box_corners - gt_box_corners_flip, dim=2))
        abs_error = torch.abs(corner_dist)
        quadratic = torch.clamp(abs_error, max=delta)
        linear = abs_error - quadratic
        corner_loss = 0.5 * quadratic**2 + delta * linear
        return corner_loss.mean(dim=1)

    # ------------------------------------------------------------------ inference
    def decode_rois(self, rois, bbox_pred):
        """:519-532: the RoI-local predictions back in the LiDAR frame -> [R, code]."""
        roi_boxes = rois[..., 1:]
        roi_ry = roi_boxes[..., 6].view(-1)
        roi_xyz = roi_boxes[..., 0:3].view(-1, 3)
        local_roi_boxes = roi_boxes.clone().detach()
        local_roi_boxes[..., 0:3] = 0
        rcnn_boxes3d = self.bbox_coder.decode(local_roi_boxes, bbox_pred)
        rcnn_boxes3d[..., 0:3] = rotation_3d_in_axis_z(rcnn_boxes3d[..., 0:3].unsqueeze(1),
                                                       roi_ry + np.pi / 2).squeeze(1)
        rcnn_boxes3d[:, 0:3] += roi_xyz
        return rcnn_boxes3d

    @staticmethod
    def _per_class(value, classes):
        return list(value) if isinstance(value, (list, tuple)) else [value] * classes

    def get_bboxes(self, rois, cls_score, bbox_pred, class_labels, class_pred, img_metas,
                   cfg=None):
        """:497-622 for the whole batch: one K.nms_segments call over the B * C lists, one host
        read.  class_labels / class_pred: per sample the RPN's labels_3d [n_b] and cls_preds
        [n_b, C]; RoI rows grouped by sample in that order.
        -> per sample (boxes, scores, labels)."""
        code, classes = self.bbox_coder.code_size, self.num_classes
        batch = len(class_pred)
        sizes = [int(p.shape[0]) for p in class_pred]
        assert sum(sizes) == rois.shape[0], "RoIs must be grouped by sample, in list order"
        rcnn_boxes3d = self.decode_rois(rois.detach(), bbox_pred.detach())
        cls_score = cls_score.detach()
        dev = rois.device
        first = np.cumsum([0] + sizes).tolist()
        widest = max(sizes + [0])
        if widest > K.NMS_MAX_SEGMENT:          # beyond the batched kernel's list length: the loop
            return self._get_bboxes_loop(rcnn_boxes3d, cls_score, class_labels, class_pred,
                                         img_metas, cfg, first)
        score_thresh = self._per_class(_get(cfg, "score_thr"), classes)
        nms_thresh = self._per_class(_get(cfg, "nms_thr"), classes)
        count = [0] * (batch * classes)
        picked = None
        if widest:
            for_nms = xywhr2xyxyr(torch.stack([rcnn_boxes3d[:, k] for k in (0, 1, 3, 4, 6)],
                                              dim=-1)).float()
            thr = torch.tensor(score_thresh, dtype=torch.float32).to(dev, non_blocking=True)
            sorted_boxes, orders, valid_counts, in_list = [], [], [], []
            for b in range(batch):
                n = sizes[b]
                probs = class_pred[b]
                if n == 0:
                    orders.append(torch.zeros((classes, widest), dtype=torch.long, device=dev))
                    valid_counts.append(torch.zeros((classes,), dtype=torch.long, device=dev))
                    continue
                assert probs.shape[1] == classes, f"box_probs shape: {str(probs.shape)}"
                probs = probs.detach().float().t()                           # [C, n]
                valid = probs >= thr[:, None]
                key = torch.where(valid, probs, torch.full_like(probs, -np.inf))
                order = torch.sort(key, dim=1, descending=True, stable=True)[1]     # [C, n]
                sorted_boxes.append(for_nms[first[b]:first[b + 1]][order.reshape(-1)])
                orders.append(nn.functional.pad(order, (0, widest - n)))
                valid_counts.append(valid.sum(1))
                in_list.append((torch.arange(n, device=dev)[None] < valid_counts[-1][:, None])
                               .reshape(-1))
            # Only the rows that pass score_thr go through NMS: they lead their sorted lists, a
            # stable sort on the flag moves them to the front of the buffer list after list, and
            # the lists' lengths are the valid counts, which stay on the device.
            counts = torch.cat(valid_counts)                                 # [B * C]
            front = torch.sort((~torch.cat(in_list)).to(torch.uint8), stable=True)[1]
            offsets = nn.functional.pad(torch.cumsum(counts, 0), (1, 0)).int()
            thresh = torch.tensor(nms_thresh * batch, dtype=torch.float32).to(dev,
                                                                              non_blocking=True)
            keep, _ = K.nms_segments("rotate" if _get(cfg, "use_rotate_nms", True) else "normal",
                                     torch.cat(sorted_boxes)[front].contiguous(), offsets, thresh,
                                     widest)
            live = (keep >= 0) & (keep < counts[:, None])
            picked = torch.cat(orders).gather(1, keep.clamp(min=0))          # [B * C, widest]
            count = live.sum(1).tolist()                                     # the one host read
        result_list = []
        for b in range(batch):
            cur_boxes = rcnn_boxes3d[first[b]:first[b + 1]]
            cur_score = cls_score[first[b]:first[b + 1]].view(-1)
            chosen = [picked[b * classes + k, :count[b * classes + k]] for k in range(classes)
                      if count[b * classes + k]]
            if chosen:
                selected = torch.cat(chosen, dim=0)
                boxes, scores = cur_boxes[selected], cur_score[selected]
                label_preds = class_labels[b][selected]
            else:                                   # :620-621: `selected = []`
                boxes, scores = cur_boxes[:0], cur_score[:0]
                label_preds = class_labels[b][:0]
            meta = img_metas[b] if img_metas is not None else None
            if meta is not None and "box_type_3d" in meta:
                boxes = meta["box_type_3d"](boxes, code)
            result_list.append((boxes, scores, label_preds))
        return result_list

    def _get_bboxes_loop(self, rcnn_boxes3d, cls_score, class_labels, class_pred, img_metas, cfg,
                         first):
        """:535-554 per sample on multi_class_nms, for lists longer than the batched kernel
        takes (each class's candidates above score_thr must still fit K.NMS_MAX_SEGMENT)."""
        result_list = []
        for b in range(len(class_pred)):
            cur_boxes = rcnn_boxes3d[first[b]:first[b + 1]]
            meta = img_metas[b] if img_metas is not None else None
            selected = self.multi_class_nms(class_pred[b], cur_boxes, _get(cfg, "score_thr"),
                                            _get(cfg, "nms_thr"), meta,
                                            _get(cfg, "use_rotate_nms", True))
            boxes = cur_boxes[selected]
            if meta is not None and "box_type_3d" in meta:
                boxes = meta["box_type_3d"](boxes, self.bbox_coder.code_size)
            result_list.append((boxes, cls_score[first[b]:first[b + 1]].view(-1)[selected],
                                class_labels[b][selected]))
        return result_list

    def multi_class_nms(self, box_probs, box_preds, score_thr, nms_thr, input_meta=None,
                        use_rotate_nms=True):
        """:556-622 for one sample, as written: a loop over the classes with a host read and an
        NMS call each (the yardstick of get_bboxes).  -> selected indices (long)."""
        assert box_probs.shape[1] == self.num_classes, f"box_probs shape: {str(box_probs.shape)}"
        selected_list = []
        boxes_for_nms = xywhr2xyxyr(box_preds[:, [0, 1, 3, 4, 6]]).float()
        score_thresh = self._per_class(score_thr, self.num_classes)
        nms_thresh = self._per_class(nms_thr, self.num_classes)
        dev = box_preds.device
        for k in range(0, self.num_classes):
            class_scores_keep = box_probs[:, k] >= score_thresh[k]
            if class_scores_keep.int().sum() > 0:
                original_idxs = class_scores_keep.nonzero(as_tuple=False).view(-1)
                cur_boxes_for_nms = boxes_for_nms[class_scores_keep]
                cur_rank_scores = box_probs[class_scores_keep, k]
                order = torch.sort(cur_rank_scores, descending=True, stable=True)[1]
                n = int(order.numel())
                keep, num = K.nms_segments(
                    "rotate" if use_rotate_nms else "normal",
                    cur_boxes_for_nms[order].contiguous(),
                    torch.tensor([0, n], dtype=torch.int32, device=dev),
                    torch.tensor([nms_thresh[k]], dtype=torch.float32, device=dev), n)
                cur_selected = order[keep[0, :int(num[0])]]
                if cur_selected.shape[0] == 0:
                    continue
                selected_list.append(original_idxs[cur_selected])
        return torch.cat(selected_list, dim=0) if len(selected_list) > 0 else \
            torch.zeros((0,), dtype=torch.long, device=dev)
