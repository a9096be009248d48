"""Part-A2's point-wise semantic head (COVERAGE n9): PointwiseSemanticHead with the
reference's constructor arguments, attribute names (seg_cls_layer, seg_reg_layer, loss_seg,
loss_part) and state-dict keys.

Reference: mmdet3d/models/roi_heads/mask_heads/pointwise_semantic_head.py; voxel_centers is
mmdet3d/models/detectors/parta2.py:62-65.

What differs from the reference is where its per-sample, per-box Python was:

  get_targets   the reference splits the voxels per sample with a boolean mask, runs two
                points_in_boxes launches per sample and then a loop over the ground-truth boxes
                with a mask, a host read (`k_box_flag.any()`), a gather, an einsum rotation and a
                masked write each, and concatenates.  Here the ground truths are padded to
                [B, G, 7] on the device, the enlarged table is LiDARBoxes.enlarged_box of it
                (torch's float32 arithmetic, not a second definition), and everything per voxel
                is ONE launch of msmd_semantic_targets_f32 (csrc/parta2.hip).  Nothing is read
                back.  `fused=False`, or CPU tensors, run the composition path: the reference's
                loop restated op for op on LiDARBoxes.points_in_boxes, the yardstick of the
                kernel.
  loss          no host read: loss_part is sum(BCE * pos_mask) / clamp(3 * num_pos, 1), which is
                the reference's mean over part_preds[pos_mask] and, without a positive row, its
                fake zero.

Deviations, both in get_targets: the output is in input row order (the reference's torch.cat
whenever coors[:, 0] does not decrease, which is what PartA2.voxelize produces), and a row whose
batch id is outside [0, B) gets seg = -1 and part = 0 where the reference drops it.  The
caller's lists are left as they are.
"""
import torch
from torch import nn
from torch.nn import functional as F

from . import kernels as K
from .head_loss import LiDARBoxes, _constant
from .head_loss import build_loss as build_focal_loss
from .losses import build_loss
from .registry import HEADS


def voxel_centers(coors, voxel_size, point_cloud_range):
    """parta2.py:62-65: voxel coordinates [N, >= 3] whose LAST three columns are (z, y, x) ->
    float32 [N, 3] xyz centres, (coors[:, [2, 1, 0]] + 0.5) * voxel_size + range[0:3].  A batch
    column in front (Voxelization's batched coors) is skipped."""
    zyx = coors[:, -3:]
    xyz = torch.stack([zyx[:, 2], zyx[:, 1], zyx[:, 0]], dim=1)
    size = torch.tensor(list(voxel_size), dtype=torch.float32).to(coors.device, non_blocking=True)
    low = torch.tensor(list(point_cloud_range[0:3]), dtype=torch.float32).to(
        coors.device, non_blocking=True)
    return (xyz + 0.5) * size + low


def rotation_3d_in_axis_z(points, angles):
    """core/bbox/structures/utils.py:36-39, 46-51, 61 (axis=2): points [N, M, 3], angles [N]."""
    rot_sin, rot_cos = torch.sin(angles), torch.cos(angles)
    ones, zeros = torch.ones_like(rot_cos), torch.zeros_like(rot_cos)
    rot_mat_t = torch.stack([torch.stack([rot_cos, -rot_sin, zeros]),
                             torch.stack([rot_sin, rot_cos, zeros]),
                             torch.stack([zeros, zeros, ones])])
    return torch.einsum("aij,jka->aik", (points, rot_mat_t))


def _as_boxes(boxes):
    return boxes if isinstance(boxes, LiDARBoxes) else LiDARBoxes(
        boxes.tensor if hasattr(boxes, "tensor") else boxes)


def pad_ground_truths(gt_bboxes_3d, gt_labels_3d, device):
    """Per-sample boxes ([G_b, >= 7] bottom-centre LiDAR boxes or objects with `.tensor`) and
    labels [G_b] -> (boxes float32 [B, G, 7], labels long [B, G], counts int32 [B]) on `device`,
    G = max G_b (0 when every sample is empty), zero padded.  The counts come from the shapes:
    nothing is read back, and the lists are not modified."""
    if len(gt_bboxes_3d) != len(gt_labels_3d):
        raise ValueError("one label tensor per box set")
    tensors = [_as_boxes(b).tensor for b in gt_bboxes_3d]
    for t, l in zip(tensors, gt_labels_3d):
        if l.dim() != 1 or l.shape[0] != t.shape[0]:
            raise ValueError("ground truths are [G, 7] boxes with [G] labels, got %s and %s"
                             % (tuple(t.shape), tuple(l.shape)))
    batch, width = len(tensors), max([0] + [t.shape[0] for t in tensors])
    boxes = torch.zeros((batch, width, 7), dtype=torch.float32, device=device)
    labels = torch.zeros((batch, width), dtype=torch.long, device=device)
    for b, (t, l) in enumerate(zip(tensors, gt_labels_3d)):
        if t.shape[0]:
            boxes[b, :t.shape[0]] = t[:, :7].to(device=device, dtype=torch.float32,
                                                non_blocking=True)
            labels[b, :t.shape[0]] = l.to(device=device, dtype=torch.long, non_blocking=True)
    counts = torch.tensor([t.shape[0] for t in tensors], dtype=torch.int32)
    return boxes, labels, counts.to(device, non_blocking=True)


@HEADS.register_module()
class PointwiseSemanticHead(nn.Module):
    """pointwise_semantic_head.py:11-50."""

    def __init__(self, in_channels, num_classes=3, extra_width=0.2, seg_score_thr=0.3,
                 loss_seg=dict(type="FocalLoss", use_sigmoid=True, reduction="sum", gamma=2.0,
                               alpha=0.25, loss_weight=1.0),
                 loss_part=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0),
                 fused=True):
        super().__init__()
        self.extra_width = extra_width
        self.num_classes = num_classes
        self.seg_score_thr = seg_score_thr
        self.fused = fused
        self.seg_cls_layer = nn.Linear(in_channels, 1, bias=True)
        self.seg_reg_layer = nn.Linear(in_channels, 3, bias=True)
        self.loss_seg = build_focal_loss(loss_seg)
        self.loss_part = build_loss(loss_part)
        if not self.loss_part.use_sigmoid or self.loss_part.class_weight is not None:
            raise NotImplementedError("PointwiseSemanticHead: loss_part must be "
                                      "CrossEntropyLoss(use_sigmoid=True) without class_weight")

    def forward(self, x):
        """:52-76 -> dict(seg_preds [N, 1], part_preds [N, 3], part_feats [N, 4])."""
        seg_preds = self.seg_cls_layer(x)
        part_preds = self.seg_reg_layer(x)
        seg_scores = torch.sigmoid(seg_preds).detach()
        seg_mask = seg_scores > self.seg_score_thr
        part_offsets = torch.sigmoid(part_preds).clone().detach()
        # part_offsets[seg_mask.view(-1) == 0] = 0, without the boolean-mask index
        part_offsets = torch.where(seg_mask, part_offsets, torch.zeros_like(part_offsets))
        part_feats = torch.cat((part_offsets, seg_scores), dim=-1)
        return dict(seg_preds=seg_preds, part_preds=part_preds, part_feats=part_feats)

    # ----------------------------------------------------------------------------- targets
    def get_targets_single(self, voxel_centers, gt_bboxes_3d, gt_labels_3d):
        """:78-125 as written, one sample: the composition path.  voxel_centers [n, 3] (any
        float dtype; points_in_boxes tests in float32 as the reference's op does), gt_bboxes_3d
        a LiDARBoxes or [G, 7] tensor, gt_labels_3d [G].  -> (seg_targets long [n], part_targets
        [n, 3] in the centres' dtype: the reference names float32 and cannot run in float64).
        The two points_in_boxes passes are the library's kernel, and the loop reads
        `k_box_flag.any()` on the host, as the reference does."""
        gt = _as_boxes(gt_bboxes_3d).to(voxel_centers.device)
        # (the box arithmetic follows the centres' dtype: a float64 run is float64 throughout)
        boxes = gt.tensor.to(voxel_centers.dtype) if voxel_centers.dtype == torch.float64 \
            else gt.tensor
        enlarged = boxes.clone()
        enlarged[:, 3:6] += self.extra_width * 2
        enlarged[:, 2] -= self.extra_width
        part_targets = voxel_centers.new_zeros((voxel_centers.shape[0], 3), dtype=torch.float32)
        box_idx = _points_in_boxes(boxes, voxel_centers)
        enlarge_box_idx = _points_in_boxes(enlarged, voxel_centers).long()
        gt_labels_pad = F.pad(gt_labels_3d.to(voxel_centers.device), (1, 0), mode="constant",
                              value=self.num_classes)
        seg_targets = gt_labels_pad[(box_idx.long() + 1)]
        fg_pt_flag = box_idx > -1
        ignore_flag = fg_pt_flag ^ (enlarge_box_idx > -1)
        seg_targets[ignore_flag] = -1
        part_targets = part_targets.to(voxel_centers.dtype)
        for k in range(boxes.shape[0]):
            k_box_flag = box_idx == k
            if not k_box_flag.any():
                continue
            fg_voxels = voxel_centers[k_box_flag]
            transformed_voxels = fg_voxels - boxes[k, :3]
            transformed_voxels = rotation_3d_in_axis_z(transformed_voxels.unsqueeze(0),
                                                       -boxes[k, 6].view(1))
            part_targets[k_box_flag] = transformed_voxels / boxes[k, 3:6] + _constant(
                transformed_voxels, [0.5, 0.5, 0])
        part_targets = torch.clamp(part_targets, min=0)
        return seg_targets, part_targets

    def _get_targets_composed(self, voxels_dict, gt_bboxes_3d, gt_labels_3d):
        """:146-157 as written (rows of a sample gathered by a boolean mask, then torch.cat)."""
        seg, part = [], []
        for idx in range(len(gt_labels_3d)):
            coords_idx = voxels_dict["coors"][:, 0] == idx
            s, p = self.get_targets_single(voxels_dict["voxel_centers"][coords_idx],
                                           gt_bboxes_3d[idx], gt_labels_3d[idx])
            seg.append(s)
            part.append(p)
        return dict(seg_targets=torch.cat(seg, dim=0), part_targets=torch.cat(part, dim=0))

    def get_targets(self, voxels_dict, gt_bboxes_3d, gt_labels_3d):
        """:127-157 -> dict(seg_targets long [N], part_targets float32 [N, 3]) for
        voxels_dict['voxel_centers'] [N, 3] and voxels_dict['coors'] [N, 4] (batch id first).

        Fused (CUDA tensors and fused=True): the lists are padded on the device and ONE kernel
        call computes both outputs for the batch; nothing is read back and the lists are left
        untouched.  Output is in input row order, which equals the reference's torch.cat
        whenever the batch ids are non-decreasing -- what PartA2.voxelize produces.  A row whose
        batch id is outside [0, B) gets seg = -1 and part = 0 (the reference drops such rows).
        Otherwise (fused=False, or CPU tensors) the composition path restates the reference."""
        centers = voxels_dict["voxel_centers"]
        if not (self.fused and centers.is_cuda):
            return self._get_targets_composed(voxels_dict, gt_bboxes_3d, gt_labels_3d)
        device = centers.device
        boxes, labels, counts = pad_ground_truths(gt_bboxes_3d, gt_labels_3d, device)
        enlarged = LiDARBoxes(boxes.view(-1, 7)).enlarged_box(self.extra_width).tensor
        seg, part = K.semantic_targets(
            centers.detach().float().contiguous(),
            voxels_dict["coors"][:, 0].to(torch.int32).contiguous(), boxes,
            enlarged.view(boxes.shape).contiguous(), labels, counts, self.num_classes)
        return dict(seg_targets=seg, part_targets=part)

    # -------------------------------------------------------------------------------- loss
    def loss(self, semantic_results, semantic_targets):
        """:159-200 -> dict(loss_seg, loss_part), with no host read.  loss_part: the reference
        takes the mean of BCE-with-logits over part_preds[pos_mask] ([num_pos, 3]) when there
        is a positive row and a constant zero otherwise; sum(BCE * pos_mask) / clamp(3 * num_pos,
        1) is both."""
        seg_preds = semantic_results["seg_preds"]
        part_preds = semantic_results["part_preds"]
        seg_targets = semantic_targets["seg_targets"]
        part_targets = semantic_targets["part_targets"]

        pos_mask = (seg_targets > -1) & (seg_targets < self.num_classes)
        binary_seg_target = pos_mask.long()
        pos = pos_mask.float()
        neg = (seg_targets == self.num_classes).float()
        seg_weights = pos + neg
        pos_normalizer = pos.sum()
        seg_weights = seg_weights / torch.clamp(pos_normalizer, min=1.0)
        loss_seg = self.loss_seg(seg_preds, binary_seg_target, seg_weights)

        bce = F.binary_cross_entropy_with_logits(part_preds, part_targets.to(part_preds.dtype),
                                                 reduction="none")
        # (where, not a product: a NaN in a row that is not positive stays out of the sum)
        bce = torch.where(pos_mask[:, None], bce, torch.zeros_like(bce))
        loss_part = self.loss_part.loss_weight * (
            bce.sum() / torch.clamp(3 * pos_normalizer, min=1.0).to(bce.dtype))
        return dict(loss_seg=loss_seg, loss_part=loss_part)


def _points_in_boxes(boxes, points):
    """LiDARInstance3DBoxes.points_in_boxes (lidar_box3d.py:242-257) through
    LiDARBoxes.points_in_boxes (msmd_points_in_boxes_f32, float32): the first box holding each
    point or -1; no launch for an empty box set."""
    if boxes.shape[0] == 0:
        return torch.full((points.shape[0],), -1, dtype=torch.int32, device=points.device)
    return LiDARBoxes(boxes.float()).points_in_boxes(points.float())
