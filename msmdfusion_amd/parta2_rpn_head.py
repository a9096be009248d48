"""Part-A2's RPN head (COVERAGE n9): PartA2RPNHead on Anchor3DHead, with the reference's
constructor defaults, state-dict keys and result dict.

Reference: mmdet3d/models/dense_heads/parta2_rpn_head.py.

What differs from the reference is where the loop runs: get_bboxes handles the whole batch --
per level the class maximum, the nms_pre top-k and the decode, then class-agnostic NMS over one
list per sample in ONE K.nms_segments call, the nms_post cut, the direction fix, and one host
read (the kept counts).  The reference calls get_bboxes_single per sample, which compacts the
candidates above score_thr with a boolean mask (a host wait), runs NMS and branches on
`len(selected)` on the host.

Reference behaviour kept as written:
  cls_preds   the comment at :206-210 says "raw" scores, but the nms_pre branch replaces
              cls_score by the post-sigmoid rows (:189) and those are what the result carries
              (:211).  Only when the branch is NOT taken (nms_pre <= 0 or not more anchors than
              nms_pre on that level) does the level carry the raw logits.  Both are reproduced,
              per level.
  empty       a sample without a kept box returns float labels_3d of shape [0] and cls_preds of
              shape [0, C] (:305-311).
"""
import math

import numpy as np
import torch

from . import kernels as K
from .anchor_head import Anchor3DHead, _get, limit_period, xywhr2xyxyr
from .registry import HEADS


@HEADS.register_module()
class PartA2RPNHead(Anchor3DHead):
    """parta2_rpn_head.py:13-83."""

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
        super().__init__(num_classes, in_channels, train_cfg, test_cfg, feat_channels,
                         use_direction_classifier, anchor_generator, assigner_per_size,
                         assign_per_class, diff_rad_by_sin, dir_offset, dir_limit_offset,
                         bbox_coder, loss_cls, loss_bbox, loss_dir)

    def loss(self, cls_scores, bbox_preds, dir_cls_preds, gt_bboxes, gt_labels, input_metas=None,
             gt_bboxes_ignore=None):
        """:85-124: the parent's loss under the keys loss_rpn_cls / loss_rpn_bbox /
        loss_rpn_dir (a list per level each)."""
        loss_dict = super().loss(cls_scores, bbox_preds, dir_cls_preds, gt_bboxes, gt_labels,
                                 input_metas, gt_bboxes_ignore)
        return dict(loss_rpn_cls=loss_dict["loss_cls"], loss_rpn_bbox=loss_dict["loss_bbox"],
                    loss_rpn_dir=loss_dict["loss_dir"])

    # ------------------------------------------------------------------ inference
    def get_bboxes(self, cls_scores, bbox_preds, dir_cls_preds, input_metas, cfg=None,
                   rescale=False):
        """anchor3d_head.py:370-419 over parta2_rpn_head.py:126-311 for the whole batch.
        cls_scores / bbox_preds / dir_cls_preds: per level [B, A * C | A * code | A * 2, H, W].
        -> per sample dict(boxes_3d, scores_3d, labels_3d, cls_preds); boxes_3d is wrapped in
        input_metas[i]['box_type_3d'] when that is given.  One host read: the kept counts."""
        cfg = self.test_cfg if cfg is None else cfg
        assert len(cls_scores) == len(bbox_preds) == len(dir_cls_preds)
        featmap_sizes = [c.shape[-2:] for c in cls_scores]
        device = cls_scores[0].device
        code, B = self.box_code_size, cls_scores[0].shape[0]
        mlvl_anchors = [a.reshape(-1, code) for a in
                        self.anchor_generator.grid_anchors(featmap_sizes, device=device)]
        nms_pre = self._check_nms_bound(cfg, featmap_sizes)
        mlvl_bboxes, mlvl_max_scores, mlvl_label_pred, mlvl_dir_scores, mlvl_cls_score = \
            [], [], [], [], []
        for cls_score, bbox_pred, dir_cls_pred, anchors in zip(cls_scores, bbox_preds,
                                                               dir_cls_preds, mlvl_anchors):
            assert cls_score.size()[-2:] == bbox_pred.size()[-2:] == dir_cls_pred.size()[-2:]
            dir_cls_pred = dir_cls_pred.detach().permute(0, 2, 3, 1).reshape(B, -1, 2)
            dir_cls_score = torch.max(dir_cls_pred, dim=-1)[1]
            cls_score = cls_score.detach().permute(0, 2, 3, 1).reshape(B, -1, self.num_classes)
            scores = cls_score.sigmoid()
            bbox_pred = bbox_pred.detach().permute(0, 2, 3, 1).reshape(B, -1, code)
            max_scores, pred_labels = scores.max(dim=2)
            anchors = anchors[None].expand(B, -1, -1)
            if scores.shape[1] > nms_pre:
                max_scores, topk_inds = max_scores.topk(nms_pre, dim=1)
                wide = topk_inds[:, :, None]
                anchors = anchors.gather(1, wide.expand(-1, -1, code))
                bbox_pred = bbox_pred.gather(1, wide.expand(-1, -1, code))
                # as written (:189): the carried class scores become the post-sigmoid rows
                cls_score = scores.gather(1, wide.expand(-1, -1, self.num_classes))
                dir_cls_score = dir_cls_score.gather(1, topk_inds)
                pred_labels = pred_labels.gather(1, topk_inds)
            mlvl_bboxes.append(self.bbox_coder.decode(anchors, bbox_pred))
            mlvl_max_scores.append(max_scores)
            mlvl_cls_score.append(cls_score)
            mlvl_label_pred.append(pred_labels)
            mlvl_dir_scores.append(dir_cls_score)
        mlvl_bboxes = torch.cat(mlvl_bboxes, dim=1)                     # [B, M, code]
        # LiDARInstance3DBoxes.bev, column by column (a list index would be copied from the host)
        for_nms = xywhr2xyxyr(torch.stack([mlvl_bboxes[..., k] for k in (0, 1, 3, 4, 6)], dim=-1))
        return self._class_agnostic_nms_batched(
            mlvl_bboxes, for_nms, torch.cat(mlvl_max_scores, dim=1),
            torch.cat(mlvl_label_pred, dim=1), torch.cat(mlvl_cls_score, dim=1),
            torch.cat(mlvl_dir_scores, dim=1), _get(cfg, "score_thr", 0), _get(cfg, "nms_post"),
            cfg, input_metas)

    def _class_agnostic_nms_batched(self, bboxes, for_nms, max_scores, label_pred, cls_score,
                                    dir_scores, score_thr, max_num, cfg, input_metas):
        """:222-311 for B samples at once: bboxes [B, M, code], for_nms [B, M, 5] xyxyr,
        max_scores / label_pred / dir_scores [B, M], cls_score [B, M, C].  A sample's list holds
        the candidates with score > score_thr in descending score order (stable); the others
        sort behind them under a -inf key and are cut by the list's count, so nothing is
        compacted.  NMS reports the kept rows in that order, which is the reference's final
        order too: its sort at :289-291 only cuts a list that is already descending."""
        B, M, code = bboxes.shape
        device = bboxes.device
        if M > K.NMS_MAX_SEGMENT:
            raise NotImplementedError("PartA2RPNHead: %d candidates per sample exceed the NMS "
                                      "kernel's %d" % (M, K.NMS_MAX_SEGMENT))
        post = max(min(int(max_num), M), 0)
        if B == 0 or post == 0:
            count = [0] * B
            picked = torch.zeros((B, 0), dtype=torch.long, device=device)
        else:
            valid = max_scores > score_thr
            counts = valid.sum(1)
            key = torch.where(valid, max_scores, torch.full_like(max_scores, -math.inf))
            order = torch.sort(key, dim=1, descending=True, stable=True)[1]            # [B, M]
            sorted_boxes = for_nms.float().gather(1, order[:, :, None].expand(-1, -1, 5))
            offsets = torch.arange(B + 1, device=device, dtype=torch.int32) * M
            thresh = torch.full((B,), float(_get(cfg, "nms_thr")), dtype=torch.float32,
                                device=device)
            keep, _ = K.nms_segments("rotate" if _get(cfg, "use_rotate_nms") else "normal",
                                     sorted_boxes.reshape(-1, 5).contiguous(), offsets, thresh, M,
                                     post_max=post)
            live = (keep >= 0) & (keep < counts[:, None])      # rows past a list's count: padding
            picked = order.gather(1, keep.clamp(min=0))        # candidate index of every slot
            count = live.sum(1).tolist()                       # the one host read
        out_boxes = bboxes.gather(1, picked[:, :, None].expand(-1, -1, code)).clone()
        out_scores = max_scores.gather(1, picked)
        out_labels = label_pred.gather(1, picked)
        out_cls = cls_score.gather(1, picked[:, :, None].expand(-1, -1, cls_score.shape[-1]))
        out_dir = dir_scores.gather(1, picked)
        dir_rot = limit_period(out_boxes[..., 6] - self.dir_offset, self.dir_limit_offset, np.pi)
        out_boxes[..., 6] = dir_rot + self.dir_offset + np.pi * out_dir.to(out_boxes.dtype)
        results = []
        for i, n in enumerate(count):
            meta = input_metas[i] if input_metas is not None else None
            b = out_boxes[i, :n]
            if meta is not None and "box_type_3d" in meta:
                b = meta["box_type_3d"](b, box_dim=code)
            # as written (:305-311): the empty result's labels are float zeros of shape [0]
            labels = out_labels[i, :n] if n else bboxes.new_zeros([0])
            results.append(dict(boxes_3d=b, scores_3d=out_scores[i, :n], labels_3d=labels,
                                cls_preds=out_cls[i, :n]))
        return results

    def get_bboxes_single(self, cls_scores, bbox_preds, dir_cls_preds, mlvl_anchors, input_meta,
                          cfg, rescale=False):
        """:126-220: one sample's [C, H, W] maps (the anchors come from the generator's cache;
        mlvl_anchors is accepted for the reference's signature)."""
        return self.get_bboxes([c[None] for c in cls_scores], [b[None] for b in bbox_preds],
                               [d[None] for d in dir_cls_preds], [input_meta], cfg, rescale)[0]

    def class_agnostic_nms(self, mlvl_bboxes, mlvl_bboxes_for_nms, mlvl_max_scores,
                           mlvl_label_pred, mlvl_cls_score, mlvl_dir_scores, score_thr, max_num,
                           cfg, input_meta):
        """:222-311 for one sample, on the batched body."""
        return self._class_agnostic_nms_batched(
            mlvl_bboxes[None], mlvl_bboxes_for_nms[None], mlvl_max_scores[None],
            mlvl_label_pred[None], mlvl_cls_score[None], mlvl_dir_scores[None], score_thr,
            max_num, cfg, [input_meta])[0]
