"""Part-A2's second stage (COVERAGE n10): PartAggregationROIHead with a 3-D IoU assigner and
IoUNegPiecewiseSampler beside it, under the reference's attribute names.

Reference: mmdet3d/models/roi_heads/part_aggregation_roi_head.py, core/bbox/samplers/
iou_neg_piecewise_sampler.py, mmdet 2.x core/bbox/assigners/max_iou_assigner.py, samplers/
sampling_result.py.

What differs from the reference is where its loops run:

  _assign_and_sample  the reference loops over the samples and inside over the per-class
                assigners: boolean-mask gathers, an IoU matrix, MaxIoUAssigner's Python loop over
                the ground truths and two F.pad index tables per (sample, class), then the
                sampler's chain of nonzero / len() / randperm / unique per sample -- several dozen
                host reads and a few hundred launches per step.  With fused=True (default) the
                whole batch is msmd_roi_assign3d_f32 + msmd_roi_sample_targets_f32
                (csrc/roi_targets.hip): four enqueued operations, then ONE host read (the sampled
                counts, to trim the padded rows).  The result is a RoISampleBatch that already
                carries PartA2BboxHead.get_targets' tensors.  fused=False, CPU tensors or sizes
                above the kernels' caps run the reference's loop (`_assign_and_sample_composed`)
                on K.boxes_iou3d matrices: the yardstick of the kernels.
  randomness    random_choice(gallery, n) is "the n entries with the smallest keys, ties to the
                lower proposal index", the keys one float32 per proposal from torch.rand(...,
                generator=).  That is a uniform subset, as the reference's randperm[:n] is; after
                its .unique() the order is ascending either way.  Both paths draw the keys the
                same way, so one generator seed gives one result.
  one index     _bbox_forward builds ONE RoIPointIndex per step and hands it to both extractors.

Deviations:
  - random stream: the law of the reference's sampling, not its randperm stream (above).
  - a sample without ground truth: mmdet's SamplingResult gives pos_gt_bboxes the shape [0, 4]
    (sampling_result.py:35-38), which the reference's torch.cat in get_targets
    (parta2_bbox_head.py:384) cannot mix with [n, 7]; here it is [0, 7].
  - arg-max ties between ground truths go to the lowest index in both paths (torch.max leaves
    the choice open on the GPU).
  - simple_test returns the result dicts on the device, like the other detectors here.
  - add_gt_as_proposals=True is refused (NotImplementedError); aug_test is not built.
"""
import numpy as np
import torch
from torch import nn

from . import kernels as K
from .anchor_head import AssignResult, _get
from .head_loss import BboxOverlaps3D, _box_tensor
from .registry import BBOX_SAMPLERS, HEADS, build_head, build_roi_extractor, build_sampler


# ---------------------------------------------------------------------------- assigner
class MaxIoUAssigner3D:
    """mmdet 2.x MaxIoUAssigner over BboxOverlaps3D(coordinate='lidar'), as the Part-A2 configs
    use it.  The kernel's contract is match_low_quality=True, gt_max_assign_all=True,
    ignore_iof_thr <= 0 and a float neg_iou_thr; anything else is refused here.  `assign` is the
    composition path (one list against one list, with the reference's host reads)."""

    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, gt_max_assign_all=True,
                 ignore_iof_thr=-1, ignore_wrt_candidates=True, match_low_quality=True,
                 gpu_assign_thr=-1, iou_calculator=dict(type="BboxOverlaps3D")):
        if isinstance(neg_iou_thr, (tuple, list)):
            raise NotImplementedError("MaxIoUAssigner3D: a tuple neg_iou_thr is not built")
        if not isinstance(neg_iou_thr, float):
            # (max_iou_assigner.py:161 applies rule 2 only under isinstance(neg_iou_thr, float))
            raise NotImplementedError("MaxIoUAssigner3D: neg_iou_thr must be a float")
        if ignore_iof_thr > 0:
            raise NotImplementedError("MaxIoUAssigner3D: ignore_iof_thr > 0 is not built")
        if not match_low_quality:
            raise NotImplementedError("MaxIoUAssigner3D: match_low_quality=False is not built")
        if not gt_max_assign_all:
            raise NotImplementedError("MaxIoUAssigner3D: gt_max_assign_all=False is not built")
        if gpu_assign_thr > 0:
            raise NotImplementedError("MaxIoUAssigner3D: gpu_assign_thr is not built")
        if isinstance(iou_calculator, dict):
            if iou_calculator.get("type") != "BboxOverlaps3D":
                raise NotImplementedError("MaxIoUAssigner3D: iou_calculator %r (BboxOverlaps3D only)"
                                          % (iou_calculator.get("type"),))
            iou_calculator = BboxOverlaps3D(**{k: v for k, v in iou_calculator.items()
                                               if k != "type"})
        elif not callable(iou_calculator) or not hasattr(iou_calculator, "coordinate"):
            raise NotImplementedError("MaxIoUAssigner3D: BboxOverlaps3D only")
        if iou_calculator.coordinate != "lidar":
            raise NotImplementedError("MaxIoUAssigner3D: lidar coordinates only")
        self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou = pos_iou_thr, neg_iou_thr, min_pos_iou
        self.gt_max_assign_all, self.ignore_iof_thr = gt_max_assign_all, ignore_iof_thr
        self.ignore_wrt_candidates, self.match_low_quality = ignore_wrt_candidates, match_low_quality
        self.gpu_assign_thr, self.iou_calculator = gpu_assign_thr, iou_calculator

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        """max_iou_assigner.py:80-135 without the ignore branch."""
        if gt_bboxes_ignore is not None:
            raise NotImplementedError("MaxIoUAssigner3D: gt_bboxes_ignore is not built")
        bboxes, gt_bboxes = _box_tensor(bboxes), _box_tensor(gt_bboxes)
        if gt_bboxes.shape[0] and bboxes.shape[0]:
            overlaps = self.iou_calculator(gt_bboxes, bboxes)
        else:
            overlaps = bboxes.new_zeros((gt_bboxes.shape[0], bboxes.shape[0]), dtype=torch.float32)
        return self.assign_wrt_overlaps(overlaps, gt_labels)

    def assign_wrt_overlaps(self, overlaps, gt_labels=None):
        """max_iou_assigner.py:137-212: rules 1-4 with the Python loop over the ground truths."""
        num_gts, num_bboxes = overlaps.size(0), overlaps.size(1)
        assigned_gt_inds = overlaps.new_full((num_bboxes,), -1, dtype=torch.long)
        if num_gts == 0 or num_bboxes == 0:
            max_overlaps = overlaps.new_zeros((num_bboxes,))
            if num_gts == 0:
                assigned_gt_inds[:] = 0
            labels = None if gt_labels is None else overlaps.new_full((num_bboxes,), -1,
                                                                      dtype=torch.long)
            return AssignResult(num_gts, assigned_gt_inds, max_overlaps, labels=labels)
        max_overlaps = overlaps.max(dim=0)[0]
        # the arg-max with ties to the lowest index (torch.max leaves ties open on the GPU)
        rows = torch.arange(num_gts, device=overlaps.device)[:, None]
        argmax_overlaps = torch.where(overlaps == max_overlaps[None], rows,
                                      rows.new_full((), num_gts)).min(dim=0)[0]
        argmax_overlaps = argmax_overlaps.clamp(max=num_gts - 1)       # (a NaN column)
        gt_max_overlaps = overlaps.max(dim=1)[0]
        assigned_gt_inds[(max_overlaps >= 0) & (max_overlaps < self.neg_iou_thr)] = 0
        pos_inds = max_overlaps >= self.pos_iou_thr
        assigned_gt_inds[pos_inds] = argmax_overlaps[pos_inds] + 1
        for i in range(num_gts):
            if gt_max_overlaps[i] >= self.min_pos_iou:
                max_iou_inds = overlaps[i, :] == gt_max_overlaps[i]
                assigned_gt_inds[max_iou_inds] = i + 1
        labels = None
        if gt_labels is not None:
            labels = assigned_gt_inds.new_full((num_bboxes,), -1)
            pos = torch.nonzero(assigned_gt_inds > 0, as_tuple=False).squeeze(1)
            if pos.numel() > 0:
                labels[pos] = gt_labels[assigned_gt_inds[pos] - 1]
        return AssignResult(num_gts, assigned_gt_inds, max_overlaps, labels=labels)


def build_assigner(cfg):
    if not isinstance(cfg, dict):
        return cfg
    args = dict(cfg)
    kind = args.pop("type")
    if kind != "MaxIoUAssigner":
        raise NotImplementedError("PartAggregationROIHead: assigner %r is not built" % kind)
    return MaxIoUAssigner3D(**args)


# ---------------------------------------------------------------------------- sampler
class SamplingResult:
    """mmdet core/bbox/samplers/sampling_result.py for 7-column boxes."""

    def __init__(self, pos_inds, neg_inds, bboxes, gt_bboxes, assign_result, gt_flags):
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.pos_bboxes, self.neg_bboxes = bboxes[pos_inds], bboxes[neg_inds]
        self.pos_is_gt = gt_flags[pos_inds]
        self.num_gts = gt_bboxes.shape[0]
        self.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        if gt_bboxes.numel() == 0:
            assert self.pos_assigned_gt_inds.numel() == 0
            # the documented deviation: [0, 7], where mmdet's view(-1, 4) gives [0, 4]
            self.pos_gt_bboxes = torch.empty_like(gt_bboxes).view(-1, bboxes.shape[-1])
        else:
            self.pos_gt_bboxes = gt_bboxes[self.pos_assigned_gt_inds, :]
        self.pos_gt_labels = None if assign_result.labels is None else \
            assign_result.labels[pos_inds]

    @property
    def bboxes(self):
        return torch.cat([self.pos_bboxes, self.neg_bboxes])


@BBOX_SAMPLERS.register_module()
class IoUNegPiecewiseSampler:
    """iou_neg_piecewise_sampler.py with the key-based random_choice.  `sample` is the
    composition path: the reference's chain op for op, host reads included."""

    def __init__(self, num, pos_fraction=None, neg_piece_fractions=None, neg_iou_piece_thrs=None,
                 neg_pos_ub=-1, add_gt_as_proposals=False, return_iou=False):
        if add_gt_as_proposals:
            raise NotImplementedError("IoUNegPiecewiseSampler: add_gt_as_proposals=True is not "
                                      "built")
        assert isinstance(neg_piece_fractions, list)
        assert len(neg_piece_fractions) == len(neg_iou_piece_thrs)
        self.num, self.pos_fraction, self.neg_pos_ub = num, pos_fraction, neg_pos_ub
        self.add_gt_as_proposals = add_gt_as_proposals
        self.pos_sampler = self.neg_sampler = self
        self.neg_piece_fractions = neg_piece_fractions
        self.neg_iou_thr = neg_iou_piece_thrs
        self.return_iou = return_iou
        self.neg_piece_num = len(self.neg_piece_fractions)

    def fits_kernel(self):
        """msmd_roi_sample_targets_f32's contract beyond its caps: pos_fraction in [0, 1] (the
        positives fit into `num` rows), piece fractions in [0, 1] that (all but the last) sum to
        at most 1 and piece bounds that do not ascend."""
        f, t = self.neg_piece_fractions, self.neg_iou_thr
        return (0.0 <= self.pos_fraction <= 1.0 and all(0.0 <= v <= 1.0 for v in f)
                and sum(f[:-1]) <= 1.0 and all(b <= a for a, b in zip(t, t[1:])))

    @staticmethod
    def random_choice(gallery, num, keys):
        """`num` entries of `gallery` (ascending proposal indices): those with the smallest
        keys[gallery], ties to the lower index."""
        assert len(gallery) >= num
        order = torch.sort(keys[gallery], stable=True)[1]
        return gallery[order[:max(int(num), 0)]]

    def _sample_pos(self, assign_result, num_expected, keys):
        pos_inds = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False)
        if pos_inds.numel() != 0:
            pos_inds = pos_inds.squeeze(1)
        if pos_inds.numel() <= num_expected:
            return pos_inds
        return self.random_choice(pos_inds, num_expected, keys)

    def _sample_neg(self, assign_result, num_expected, keys):
        neg_inds = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False)
        if neg_inds.numel() != 0:
            neg_inds = neg_inds.squeeze(1)
        if len(neg_inds) <= num_expected:
            return neg_inds
        neg_inds_choice = neg_inds.new_zeros([0])
        extend_num = 0
        max_overlaps = assign_result.max_overlaps[neg_inds]
        for piece_inds in range(self.neg_piece_num):
            if piece_inds == self.neg_piece_num - 1:
                piece_expected_num = num_expected - len(neg_inds_choice)
                min_iou_thr = 0
            else:
                piece_expected_num = int(num_expected * self.neg_piece_fractions[piece_inds]) \
                    + extend_num
                min_iou_thr = self.neg_iou_thr[piece_inds + 1]
            max_iou_thr = self.neg_iou_thr[piece_inds]
            piece_neg_inds = torch.nonzero((max_overlaps >= min_iou_thr)
                                           & (max_overlaps < max_iou_thr), as_tuple=False).view(-1)
            if len(piece_neg_inds) < piece_expected_num:
                neg_inds_choice = torch.cat([neg_inds_choice, neg_inds[piece_neg_inds]], dim=0)
                extend_num += piece_expected_num - len(piece_neg_inds)
            else:
                neg_inds_choice = torch.cat([neg_inds_choice, self.random_choice(
                    neg_inds[piece_neg_inds], piece_expected_num, keys)], dim=0)
                extend_num = 0
        return neg_inds_choice

    def sample(self, assign_result, bboxes, gt_bboxes, gt_labels=None, keys=None, generator=None):
        """:98-157.  keys: one float per row of bboxes (drawn from `generator` when absent)."""
        if len(bboxes.shape) < 2:
            bboxes = bboxes[None, :]
        if keys is None:
            keys = torch.rand((bboxes.shape[0],), generator=generator, device=bboxes.device)
        gt_flags = bboxes.new_zeros((bboxes.shape[0],), dtype=torch.bool)
        num_expected_pos = int(self.num * self.pos_fraction)
        pos_inds = self._sample_pos(assign_result, num_expected_pos, keys).unique()
        num_sampled_pos = pos_inds.numel()
        num_expected_neg = self.num - num_sampled_pos
        if self.neg_pos_ub >= 0:
            neg_upper_bound = int(self.neg_pos_ub * max(1, num_sampled_pos))
            if num_expected_neg > neg_upper_bound:
                num_expected_neg = neg_upper_bound
        neg_inds = self._sample_neg(assign_result, num_expected_neg, keys).unique()
        sampling_result = SamplingResult(pos_inds, neg_inds, bboxes, gt_bboxes, assign_result,
                                         gt_flags)
        if self.return_iou:
            sampling_result.iou = assign_result.max_overlaps[torch.cat([pos_inds, neg_inds])]
            sampling_result.iou.detach_()
        return sampling_result


class RoISampleBatch:
    """What the fused _assign_and_sample leaves: the sampled RoIs of the whole batch with
    PartA2BboxHead.get_targets' tensors, trimmed to the sampled rows (a sample's positives in
    ascending proposal order, then its negatives).  label_weights / bbox_weights are not yet
    normalised (get_targets does that).  counts: per sample (positives, negatives), host ints."""

    def __init__(self, rois, iou, label, bbox_targets, pos_gt_bboxes, reg_mask, label_weights,
                 bbox_weights, inds, counts, assign):
        self.rois, self.iou, self.label, self.bbox_targets = rois, iou, label, bbox_targets
        self.pos_gt_bboxes, self.reg_mask = pos_gt_bboxes, reg_mask
        self.label_weights, self.bbox_weights = label_weights, bbox_weights
        self.inds, self.counts, self.assign = inds, counts, assign

    def __len__(self):
        return len(self.counts)


def bbox3d2roi(bbox_list):
    """core/bbox/transforms.py bbox3d2roi: [n_i, 7] per sample -> [sum n_i, 8] (batch id, box).
    An empty sample contributes [0, 8] (the reference's zeros_like gives [0, 7], which its
    torch.cat cannot mix with [n, 8])."""
    rois_list = []
    for img_id, bboxes in enumerate(bbox_list):
        if bboxes.size(0) > 0:
            img_inds = bboxes.new_full((bboxes.size(0), 1), img_id)
            rois = torch.cat([img_inds, bboxes], dim=-1)
        else:
            rois = bboxes.new_zeros((0, bboxes.size(-1) + 1))
        rois_list.append(rois)
    return torch.cat(rois_list, 0)


# ---------------------------------------------------------------------------- the head
@HEADS.register_module()
class PartAggregationROIHead(nn.Module):
    """part_aggregation_roi_head.py:11-61 (on base_3droi_head.py)."""

    def __init__(self, semantic_head, num_classes=3, seg_roi_extractor=None,
                 part_roi_extractor=None, bbox_head=None, train_cfg=None, test_cfg=None,
                 fused=True):
        super().__init__()
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.fused = fused
        if bbox_head is not None:
            self.init_bbox_head(bbox_head)
        self.num_classes = num_classes
        assert semantic_head is not None
        self.semantic_head = semantic_head if isinstance(semantic_head, nn.Module) \
            else build_head(semantic_head)
        if seg_roi_extractor is not None:
            self.seg_roi_extractor = build_roi_extractor(seg_roi_extractor)
        if part_roi_extractor is not None:
            self.part_roi_extractor = build_roi_extractor(part_roi_extractor)
        self.init_assigner_sampler()

    def init_weights(self, pretrained=None):
        pass

    def init_bbox_head(self, bbox_head):
        self.bbox_head = bbox_head if isinstance(bbox_head, nn.Module) else build_head(bbox_head)

    def init_assigner_sampler(self):
        """:60-71."""
        self.bbox_assigner = None
        self.bbox_sampler = None
        if self.train_cfg:
            assigner = _get(self.train_cfg, "assigner")
            if isinstance(assigner, list):
                self.bbox_assigner = [build_assigner(res) for res in assigner]
            else:
                self.bbox_assigner = build_assigner(assigner)
            self.bbox_sampler = build_sampler(_get(self.train_cfg, "sampler"))

    @property
    def with_bbox(self):
        return hasattr(self, "bbox_head") and self.bbox_head is not None

    @property
    def with_semantic(self):
        return hasattr(self, "semantic_head") and self.semantic_head is not None

    # ------------------------------------------------------------------ training
    def forward_train(self, feats_dict, voxels_dict, img_metas, proposal_list, gt_bboxes_3d,
                      gt_labels_3d, generator=None):
        """:79-119 -> the losses of the semantic head and of the bbox head."""
        losses = dict()
        if self.with_semantic:
            semantic_results = self._semantic_forward_train(feats_dict["seg_features"],
                                                            voxels_dict, gt_bboxes_3d,
                                                            gt_labels_3d)
            losses.update(semantic_results["loss_semantic"])
        sample_results = self._assign_and_sample(proposal_list, gt_bboxes_3d, gt_labels_3d,
                                                 generator=generator)
        if self.with_bbox:
            bbox_results = self._bbox_forward_train(feats_dict["seg_features"],
                                                    semantic_results["part_feats"], voxels_dict,
                                                    sample_results)
            losses.update(bbox_results["loss_bbox"])
        return losses

    def simple_test(self, feats_dict, voxels_dict, img_metas, proposal_list, **kwargs):
        """:121-162 -> per sample dict(boxes_3d, scores_3d, labels_3d)."""
        assert self.with_bbox, "Bbox head must be implemented."
        assert self.with_semantic
        semantic_results = self.semantic_head(feats_dict["seg_features"])
        rois = bbox3d2roi([_box_tensor(res["boxes_3d"]) for res in proposal_list])
        labels_3d = [res["labels_3d"] for res in proposal_list]
        cls_preds = [res["cls_preds"] for res in proposal_list]
        bbox_results = self._bbox_forward(feats_dict["seg_features"],
                                          semantic_results["part_feats"], voxels_dict, rois)
        bbox_list = self.bbox_head.get_bboxes(rois, bbox_results["cls_score"],
                                              bbox_results["bbox_pred"], labels_3d, cls_preds,
                                              img_metas, cfg=self.test_cfg)
        return [dict(boxes_3d=bboxes, scores_3d=scores, labels_3d=labels)
                for bboxes, scores, labels in bbox_list]

    def _bbox_forward_train(self, seg_feats, part_feats, voxels_dict, sampling_results):
        """:164-189."""
        if isinstance(sampling_results, RoISampleBatch):
            rois = sampling_results.rois
        else:
            rois = bbox3d2roi([res.bboxes for res in sampling_results])
        bbox_results = self._bbox_forward(seg_feats, part_feats, voxels_dict, rois)
        bbox_targets = self.bbox_head.get_targets(sampling_results, self.train_cfg)
        loss_bbox = self.bbox_head.loss(bbox_results["cls_score"], bbox_results["bbox_pred"],
                                        rois, *bbox_targets)
        bbox_results.update(loss_bbox=loss_bbox)
        return bbox_results

    def _bbox_forward(self, seg_feats, part_feats, voxels_dict, rois):
        """:191-220, with ONE RoIPointIndex for both extractors (they share out_size and
        max_pts_per_voxel in the configs; otherwise each builds its own)."""
        centers, batch_inds = voxels_dict["voxel_centers"], voxels_dict["coors"][..., 0]
        seg_layer, part_layer = self.seg_roi_extractor.roi_layer, self.part_roi_extractor.roi_layer
        index = self.seg_roi_extractor.build_index(centers, batch_inds, rois)
        shared = seg_layer.out_xyz == part_layer.out_xyz and \
            seg_layer.max_pts_per_voxel == part_layer.max_pts_per_voxel
        pooled_seg_feats = self.seg_roi_extractor(seg_feats, centers, batch_inds, rois,
                                                  index=index)
        pooled_part_feats = self.part_roi_extractor(part_feats, centers, batch_inds, rois,
                                                    index=index if shared else None)
        cls_score, bbox_pred = self.bbox_head(pooled_seg_feats, pooled_part_feats)
        return dict(cls_score=cls_score, bbox_pred=bbox_pred, pooled_seg_feats=pooled_seg_feats,
                    pooled_part_feats=pooled_part_feats)

    def _semantic_forward_train(self, x, voxels_dict, gt_bboxes_3d, gt_labels_3d):
        """:296-316."""
        semantic_results = self.semantic_head(x)
        semantic_targets = self.semantic_head.get_targets(voxels_dict, gt_bboxes_3d, gt_labels_3d)
        loss_semantic = self.semantic_head.loss(semantic_results, semantic_targets)
        semantic_results.update(loss_semantic=loss_semantic)
        return semantic_results

    # ------------------------------------------------------------------ assignment
    def _lists(self, proposal_list, gt_bboxes_3d, gt_labels_3d):
        boxes = [_box_tensor(p["boxes_3d"])[:, :7] for p in proposal_list]
        dev = boxes[0].device
        labels = [p["labels_3d"].long() for p in proposal_list]
        gts = [_box_tensor(g).to(dev)[:, :7] for g in gt_bboxes_3d]
        gt_labels = [l.to(dev).long() for l in gt_labels_3d]
        return boxes, labels, gts, gt_labels

    def draw_keys(self, boxes, generator=None):
        """One float32 key per proposal of the batch, sample after sample, in one draw."""
        total = sum(b.shape[0] for b in boxes)
        return torch.rand((total,), generator=generator, device=boxes[0].device)

    def fits_kernels(self, boxes):
        sampler, assigner = self.bbox_sampler, self.bbox_assigner
        classes = len(assigner) if isinstance(assigner, list) else 1
        return (boxes[0].is_cuda and 1 <= len(boxes) <= K.ROI_ASSIGN_MAX_SAMPLES
                and 1 <= classes <= K.ROI_ASSIGN_MAX_CLASSES
                and max(b.shape[0] for b in boxes) <= K.ROI_SAMPLE_MAX_PROPOSALS
                and 1 <= sampler.num <= K.ROI_SAMPLE_MAX_NUM
                and sampler.neg_piece_num <= K.ROI_SAMPLE_MAX_PIECES and sampler.fits_kernel())

    def _assign_and_sample(self, proposal_list, gt_bboxes_3d, gt_labels_3d, generator=None,
                           keys=None):
        """:222-294.  -> RoISampleBatch (fused) or a list of SamplingResult (composition)."""
        boxes, labels, gts, gt_labels = self._lists(proposal_list, gt_bboxes_3d, gt_labels_3d)
        if keys is None:
            keys = self.draw_keys(boxes, generator)
        if not (self.fused and self.fits_kernels(boxes)):
            return self._assign_and_sample_composed(boxes, labels, gts, gt_labels, keys)
        sampler, assigner = self.bbox_sampler, self.bbox_assigner
        single = not isinstance(assigner, list)
        group = [assigner] if single else assigner
        poffs = np.cumsum([0] + [b.shape[0] for b in boxes]).tolist()
        goffs = np.cumsum([0] + [g.shape[0] for g in gts]).tolist()
        props = torch.cat(boxes).float().contiguous()
        gt_all = torch.cat(gts).float().contiguous()
        gt_inds, overlaps, assigned_labels = K.roi_assign3d(
            props, None if single else torch.cat(labels).contiguous(), poffs, gt_all,
            torch.cat(gt_labels).contiguous(), goffs, [a.pos_iou_thr for a in group],
            [a.neg_iou_thr for a in group], [a.min_pos_iou for a in group], single=single)
        res = K.roi_sample_targets(
            props, poffs, gt_inds, overlaps, keys.float().contiguous(), gt_all, goffs, sampler.num,
            int(sampler.num * sampler.pos_fraction), sampler.neg_pos_ub,
            sampler.neg_piece_fractions, sampler.neg_iou_thr, _get(self.train_cfg, "cls_pos_thr"),
            _get(self.train_cfg, "cls_neg_thr"))
        counts = res["counts"].tolist()                    # the one host read
        rows = lambda t: torch.cat([t[s, :p + n] for s, (p, n) in enumerate(counts)])  # noqa: E731
        pos = lambda t: torch.cat([t[s, :p] for s, (p, _) in enumerate(counts)])       # noqa: E731
        return RoISampleBatch(
            rois=rows(res["rois"]), iou=rows(res["iou"]), label=rows(res["label"]),
            bbox_targets=pos(res["bbox_targets"]), pos_gt_bboxes=pos(res["pos_gt_bboxes"]),
            reg_mask=rows(res["reg_mask"]), label_weights=rows(res["label_weights"]),
            bbox_weights=rows(res["bbox_weights"]), inds=rows(res["inds"]),
            counts=[tuple(c) for c in counts],
            assign=dict(gt_inds=gt_inds, max_overlaps=overlaps, labels=assigned_labels,
                        offsets=poffs))

    def _assign_composed(self, cur_boxes, cur_labels_3d, cur_gt_bboxes, cur_gt_labels):
        """:244-287 for one sample: the reference's loop over the per-class assigners."""
        n = cur_boxes.shape[0]
        if isinstance(self.bbox_assigner, list):
            batch_num_gts = 0
            batch_gt_indis = cur_gt_labels.new_full((n,), 0)
            batch_max_overlaps = cur_boxes.new_zeros(n)
            batch_gt_labels = cur_gt_labels.new_full((n,), -1)
            for i, assigner in enumerate(self.bbox_assigner):
                gt_per_cls = (cur_gt_labels == i)
                pred_per_cls = (cur_labels_3d == i)
                cur_assign_res = assigner.assign(cur_boxes[pred_per_cls],
                                                 cur_gt_bboxes[gt_per_cls],
                                                 gt_labels=cur_gt_labels[gt_per_cls])
                batch_num_gts += cur_assign_res.num_gts
                gt_inds_arange_pad = gt_per_cls.nonzero(as_tuple=False).view(-1) + 1
                gt_inds_arange_pad = nn.functional.pad(gt_inds_arange_pad, (1, 0), mode="constant",
                                                       value=0)
                gt_inds_arange_pad = nn.functional.pad(gt_inds_arange_pad, (1, 0), mode="constant",
                                                       value=-1)
                gt_inds_arange_pad += 1
                batch_gt_indis[pred_per_cls] = gt_inds_arange_pad[cur_assign_res.gt_inds + 1] - 1
                batch_max_overlaps[pred_per_cls] = cur_assign_res.max_overlaps
                batch_gt_labels[pred_per_cls] = cur_assign_res.labels
            return AssignResult(batch_num_gts, batch_gt_indis, batch_max_overlaps, batch_gt_labels)
        return self.bbox_assigner.assign(cur_boxes, cur_gt_bboxes, gt_labels=cur_gt_labels)

    def _assign_and_sample_composed(self, boxes, labels, gts, gt_labels, keys):
        """The reference's _assign_and_sample on K.boxes_iou3d matrices, host reads included."""
        sampling_results, first = [], 0
        for cur_boxes, cur_labels_3d, cur_gt, cur_gt_labels in zip(boxes, labels, gts, gt_labels):
            assign_result = self._assign_composed(cur_boxes, cur_labels_3d, cur_gt, cur_gt_labels)
            cur_keys = keys[first:first + cur_boxes.shape[0]]
            first += cur_boxes.shape[0]
            result = self.bbox_sampler.sample(assign_result, cur_boxes, cur_gt, cur_gt_labels,
                                              keys=cur_keys)
            result.assign_result = assign_result
            sampling_results.append(result)
        return sampling_results
