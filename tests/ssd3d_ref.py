"""Restatements the 3DSSD tests compare with (torch on any device, numpy for NMS).

  targets_single   SSD3DHead.get_targets_single (ssd_3d_head.py:307-437) as written, one sample,
                   in the dtype asked for.  float32 is the reference's own arithmetic (its
                   einsum and pow included); float64 is the yardstick both the kernel and the
                   float32 form are measured against.  Which box holds a point is decided once,
                   by the float32 predicate (tests/roiaware_ref.py), in either dtype.
  targets          SSD3DHead.get_targets (:219-305): the per-sample loop, the fake box, the
                   stacking and the weights -- the reference's structure, used as the baseline
                   the fused path is timed against.
  losses           SSD3DHead.loss (:112-217) on given targets, in the dtype of its inputs.
  mmcv_nms / mmcv_batched_nms
                   mmcv 1.x ops/nms.py `nms` / `batched_nms` with ops/csrc/nms_cuda_kernel.cuh's
                   pair test written out from their published definitions (mmcv is not
                   installed): float32, offset 0, scores sorted descending, greedy.
  multiclass_nms_single / get_bboxes
                   ssd_3d_head.py:439-543 as written, per sample.
"""
import numpy as np
import torch
import torch.nn.functional as F

import roiaware_ref as RR

F32 = np.float32
TARGET_NAMES = ("vote_targets", "center_targets", "size_res_targets", "dir_class_targets",
                "dir_res_targets", "mask_targets", "centerness_targets", "corner3d_targets",
                "vote_mask", "positive_mask", "negative_mask")
ALL_TARGET_NAMES = TARGET_NAMES + ("centerness_weights", "box_loss_weights",
                                   "heading_res_loss_weight")


# ------------------------------------------------------------------------ box structure
def rotation_z(points, angles):
    """core/bbox/structures/utils.py rotation_3d_in_axis(points [N, M, 3], angles [N], axis=2)."""
    rot_sin, rot_cos = torch.sin(angles), torch.cos(angles)
    ones, zeros = torch.ones_like(rot_cos), torch.zeros_like(rot_cos)
    rot_mat_t = torch.stack([torch.stack([rot_cos, -rot_sin, zeros]),
                             torch.stack([rot_sin, rot_cos, zeros]),
                             torch.stack([zeros, zeros, ones])])
    return torch.einsum("aij,jka->aik", (points, rot_mat_t))


def gravity_center(boxes):
    return torch.cat([boxes[:, :2], (boxes[:, 2] + boxes[:, 5] * 0.5)[:, None]], 1)


def corners(boxes):
    """lidar_box3d.py:46-84."""
    dims = boxes[:, 3:6]
    unit = torch.tensor([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0],
                         [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]], dtype=boxes.dtype,
                        device=boxes.device)
    unit = unit - torch.tensor([0.5, 0.5, 0], dtype=boxes.dtype, device=boxes.device)
    out = rotation_z(dims.view(-1, 1, 3) * unit.reshape(1, 8, 3), boxes[:, 6])
    return out + boxes[:, :3].view(-1, 1, 3)


def enlarged(boxes, extra):
    out = boxes.clone()
    out[:, 3:6] += extra * 2
    out[:, 2] -= extra
    return out


def from_origin(boxes, origin):
    """base_box3d.py:36-65: the given centre lies at `origin` of the box -> bottom centre."""
    out = boxes.clone()
    dst = torch.tensor((0.5, 0.5, 0), dtype=boxes.dtype, device=boxes.device)
    src = torch.tensor(origin, dtype=boxes.dtype, device=boxes.device)
    out[:, :3] += out[:, 3:6] * (dst - src)
    return out


FIRST_BOX = None     # a timing script may put a device points-in-boxes here (points, boxes) -> [M]


def first_box(points, boxes):
    """points [M, 3], boxes [T, 7] (float32 values) -> long [M] on their device: the first box
    holding each point or -1 (points_in_boxes_gpu), by the float32 / double predicate."""
    if boxes.shape[0] == 0:
        return torch.full((points.shape[0],), -1, dtype=torch.long, device=points.device)
    if FIRST_BOX is not None:
        return FIRST_BOX(points, boxes).long()
    idx = RR.points_in_boxes_first(points.detach().float().cpu().numpy()[None],
                                   boxes.detach().float().cpu().numpy()[None, :, :7])[0]
    return torch.from_numpy(idx.astype(np.int64)).to(points.device)


def assign_by_points_inside(boxes, points):
    """:545-572, the LiDAR branch -> (inside bool [M], assignment long [M])."""
    assignment = first_box(points, boxes)
    inside = assignment >= 0
    assignment = torch.where(inside, assignment, torch.full_like(assignment, boxes.shape[0] - 1))
    return inside, assignment


# ---------------------------------------------------------------------------------- coder
def angle2class(angle, num_dir_bins):
    angle = angle % (2 * np.pi)
    angle_per_class = 2 * np.pi / float(num_dir_bins)
    shifted_angle = (angle + angle_per_class / 2) % (2 * np.pi)
    angle_cls = shifted_angle // angle_per_class
    angle_res = shifted_angle - (angle_cls * angle_per_class + angle_per_class / 2)
    return angle_cls.long(), angle_res


def class2angle(angle_cls, angle_res, num_dir_bins):
    angle_per_class = 2 * np.pi / float(num_dir_bins)
    angle = angle_cls.to(angle_res.dtype) * angle_per_class + angle_res
    return torch.where(angle > np.pi, angle - 2 * np.pi, angle)


def decode(bbox_out, num_dir_bins):
    """anchor_free_bbox_coder.py:53-85."""
    center = bbox_out["center"]
    batch, n = center.shape[:2]
    dir_class = torch.argmax(bbox_out["dir_class"], -1)
    dir_res = torch.gather(bbox_out["dir_res"], 2, dir_class.unsqueeze(-1)).squeeze(2)
    angle = class2angle(dir_class, dir_res, num_dir_bins).reshape(batch, n, 1)
    return torch.cat([center, torch.clamp(bbox_out["size"] * 2, min=0.1), angle], -1)


# -------------------------------------------------------------------------------- targets
def targets_single(boxes, labels, aggregated, seeds, num_classes, num_dir_bins,
                   pos_distance_thr, expand_dims_length, dtype=torch.float32):
    """boxes [T, 7] float32, labels long [T], aggregated / seeds [N, 3] float32 -> the eleven
    results of get_targets_single, floating ones in `dtype`.  Both points_in_boxes calls see
    float32 values: the reference's inputs."""
    n, dev = aggregated.shape[0], aggregated.device
    valid = labels != -1
    boxes32, labels = boxes[valid][:, :7].float(), labels[valid]
    if boxes32.shape[0] == 0:
        z = lambda *s: torch.zeros(s, dtype=dtype, device=dev)                   # noqa: E731
        zl = lambda *s: torch.zeros(s, dtype=torch.long, device=dev)             # noqa: E731
        zb = torch.zeros(n, dtype=torch.bool, device=dev)
        return (z(n, 3), z(n, 3), z(n, 3), zl(n), z(n), zl(n), z(n, num_classes), z(n, 8, 3), zb,
                zb.clone(), ~zb)
    gt = boxes32.to(dtype)
    points, seed = aggregated.to(dtype), seeds.to(dtype)
    center_all = gravity_center(gt)
    size_all = gt[:, 3:6] / 2
    dir_class_all, dir_res_all = angle2class(gt[:, 6], num_dir_bins)
    dir_res_all = dir_res_all / (2 * np.pi / num_dir_bins)

    inside, assignment = assign_by_points_inside(boxes32, aggregated)
    center_targets = center_all[assignment]
    size_res_targets = size_all[assignment]
    mask_targets = labels[assignment]
    dir_class_targets = dir_class_all[assignment]
    dir_res_targets = dir_res_all[assignment]
    corner3d_targets = corners(gt)[assignment]

    top_center_targets = center_targets.clone()
    top_center_targets[:, 2] += size_res_targets[:, 2]
    dist = torch.norm(points - top_center_targets, dim=1)
    positive_mask = inside & (dist < pos_distance_thr)
    negative_mask = ~inside

    canonical_xyz = points - center_targets
    canonical_xyz = rotation_z(canonical_xyz.unsqueeze(0).transpose(0, 1),
                               -gt[:, 6][assignment]).squeeze(1)
    s, c = size_res_targets, canonical_xyz
    front, back = torch.clamp(s[:, 0] - c[:, 0], min=0), torch.clamp(s[:, 0] + c[:, 0], min=0)
    left, right = torch.clamp(s[:, 1] - c[:, 1], min=0), torch.clamp(s[:, 1] + c[:, 1], min=0)
    top, bottom = torch.clamp(s[:, 2] - c[:, 2], min=0), torch.clamp(s[:, 2] + c[:, 2], min=0)
    centerness_l = torch.min(front, back) / torch.max(front, back)
    centerness_w = torch.min(left, right) / torch.max(left, right)
    centerness_h = torch.min(bottom, top) / torch.max(bottom, top)
    centerness = torch.clamp(centerness_l * centerness_w * centerness_h, min=0)
    centerness = centerness.pow(1 / 3.0)
    centerness = torch.clamp(centerness, min=0, max=1)
    one_hot = centerness.new_zeros((n, num_classes))
    one_hot.scatter_(1, mask_targets.unsqueeze(-1), 1)
    centerness_targets = centerness.unsqueeze(1) * one_hot

    # the vote boxes: enlarged, then lowered once more (as the reference does)
    vote32 = enlarged(boxes32, expand_dims_length)
    vote32[:, 2] -= expand_dims_length
    vote_mask, vote_assignment = assign_by_points_inside(vote32, seeds)
    vote_targets = center_all[vote_assignment] - seed
    return (vote_targets, center_targets, size_res_targets, dir_class_targets, dir_res_targets,
            mask_targets, centerness_targets, corner3d_targets, vote_mask, positive_mask,
            negative_mask)


def distance_margin(boxes, labels, aggregated, pos_distance_thr):
    """The smallest |dist / pos_distance_thr - 1| over a sample's candidates, in float64 (inf for
    a sample without a valid box): how far the positive mask is from flipping."""
    valid = labels != -1
    boxes32 = boxes[valid][:, :7].float()
    if boxes32.shape[0] == 0:
        return float("inf")
    gt = boxes32.double()
    _, assignment = assign_by_points_inside(boxes32, aggregated)
    top = gravity_center(gt)[assignment]
    top[:, 2] += gt[:, 5][assignment] / 2
    dist = torch.norm(aggregated.double() - top, dim=1)
    return float((dist / pos_distance_thr - 1).abs().min())


def targets(gt_boxes, gt_labels, aggregated, seed_points, num_candidates, num_classes,
            num_dir_bins, pos_distance_thr, expand_dims_length, dtype=torch.float32):
    """get_targets: gt_boxes a list of [T_b, 7] tensors, gt_labels a list of long [T_b];
    aggregated [B, N, 3]; seed_points [B, >= N, 3] -> the 14-tuple."""
    per_sample = []
    for b, (boxes, labels) in enumerate(zip(gt_boxes, gt_labels)):
        if len(labels) == 0:
            boxes, labels = boxes.new_zeros(1, boxes.shape[-1]), labels.new_zeros(1)
        per_sample.append(targets_single(
            boxes.to(aggregated.device), labels.to(aggregated.device), aggregated[b],
            seed_points[b, :num_candidates], num_classes, num_dir_bins, pos_distance_thr,
            expand_dims_length, dtype))
    (vote_targets, center_targets, size_res_targets, dir_class_targets, dir_res_targets,
     mask_targets, centerness_targets, corner3d_targets, vote_mask, positive_mask,
     negative_mask) = [torch.stack(t) for t in zip(*per_sample)]
    center_targets = center_targets - aggregated.to(dtype)
    centerness_weights = (positive_mask + negative_mask).unsqueeze(-1).repeat(
        1, 1, num_classes).to(dtype)
    centerness_weights = centerness_weights / (centerness_weights.sum() + 1e-6)
    vote_mask = vote_mask.to(dtype) / (vote_mask.sum() + 1e-6)
    box_loss_weights = positive_mask.to(dtype) / (positive_mask.sum() + 1e-6)
    one_hot = torch.zeros(dir_class_targets.shape + (num_dir_bins,), dtype=torch.long,
                          device=aggregated.device)
    one_hot.scatter_(2, dir_class_targets.unsqueeze(-1), 1)
    heading_res_loss_weight = one_hot * box_loss_weights.unsqueeze(-1)
    return (vote_targets, center_targets, size_res_targets, dir_class_targets, dir_res_targets,
            mask_targets, centerness_targets, corner3d_targets, vote_mask, positive_mask,
            negative_mask, centerness_weights, box_loss_weights, heading_res_loss_weight)


# ---------------------------------------------------------------------------------- losses
def smooth_l1_sum(pred, target, weight):
    diff = torch.abs(pred - target)
    return (torch.where(diff < 1.0, 0.5 * diff * diff, diff - 0.5) * weight).sum()


def losses(bbox_preds, all_targets, num_dir_bins):
    """SSD3DHead.loss with the 3DSSD config's loss modules (sum reduction, weight 1)."""
    (vote_targets, center_targets, size_res_targets, dir_class_targets, dir_res_targets,
     mask_targets, centerness_targets, corner3d_targets, vote_mask, positive_mask,
     negative_mask, centerness_weights, box_loss_weights, heading_res_loss_weight) = all_targets
    p = bbox_preds
    centerness_loss = (F.binary_cross_entropy_with_logits(
        p["obj_scores"].transpose(2, 1), centerness_targets, reduction="none")
        * centerness_weights).sum()
    center_loss = smooth_l1_sum(p["center_offset"], center_targets,
                                box_loss_weights.unsqueeze(-1))
    dir_class_loss = (F.cross_entropy(p["dir_class"].transpose(1, 2), dir_class_targets,
                                      reduction="none") * box_loss_weights).sum()
    dir_res_loss = smooth_l1_sum(p["dir_res_norm"],
                                 dir_res_targets.unsqueeze(-1).repeat(1, 1, num_dir_bins),
                                 heading_res_loss_weight)
    size_loss = smooth_l1_sum(p["size"], size_res_targets, box_loss_weights.unsqueeze(-1))
    one_hot = dir_class_targets.new_zeros(p["dir_class"].shape)
    one_hot.scatter_(2, dir_class_targets.unsqueeze(-1), 1)
    pred = decode(dict(center=p["center"], dir_res=p["dir_res"], dir_class=one_hot,
                       size=p["size"]), num_dir_bins)
    pred = from_origin(pred.reshape(-1, 7), (0.5, 0.5, 0.5))
    corner_loss = smooth_l1_sum(corners(pred).reshape(-1, 8, 3),
                                corner3d_targets.reshape(-1, 8, 3),
                                box_loss_weights.view(-1, 1, 1))
    vote_loss = smooth_l1_sum(p["vote_offset"].transpose(1, 2), vote_targets,
                              vote_mask.unsqueeze(-1))
    return dict(centerness_loss=centerness_loss, center_loss=center_loss,
                dir_class_loss=dir_class_loss, dir_res_loss=dir_res_loss,
                size_res_loss=size_loss, corner_loss=corner_loss, vote_loss=vote_loss)


# ------------------------------------------------------------------------------------- NMS
def mmcv_nms_hits(kept, later, thr):
    """nms_cuda_kernel.cuh devIoU(a = kept row, b = later rows [K, 4], offset 0) in float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        left, right = np.fmax(kept[0], later[:, 0]), np.fmin(kept[2], later[:, 2])
        top, bottom = np.fmax(kept[1], later[:, 1]), np.fmin(kept[3], later[:, 3])
        width = np.fmax((right - left).astype(F32), F32(0))
        height = np.fmax((bottom - top).astype(F32), F32(0))
        inter = (width * height).astype(F32)
        sa = F32(F32(kept[2] - kept[0]) * F32(kept[3] - kept[1]))
        sb = ((later[:, 2] - later[:, 0]).astype(F32) * (later[:, 3] - later[:, 1]).astype(F32))
        union = ((sa + sb.astype(F32)).astype(F32) - inter).astype(F32)
        return inter > (F32(thr) * union).astype(F32)


def mmcv_nms(boxes, scores, iou_threshold):
    """mmcv.ops.nms (offset 0) -> kept indices, best score first.  boxes [N, 4] float32."""
    boxes, scores = np.asarray(boxes, F32), np.asarray(scores, F32)
    order = np.argsort(-scores, kind="stable")
    rows = boxes[order]
    removed = np.zeros(len(order), bool)
    keep = []
    for i in range(len(order)):
        if removed[i]:
            continue
        keep.append(order[i])
        if i + 1 < len(order):
            removed[i + 1:] |= mmcv_nms_hits(rows[i], rows[i + 1:], iou_threshold)
    return np.asarray(keep, np.int64)


def class_shift(boxes, idxs):
    """batched_nms: boxes + idxs * (boxes.max() + 1), float32 (torch's max: NaN wins)."""
    boxes = np.asarray(boxes, F32)
    with np.errstate(invalid="ignore"):
        shift = np.asarray(idxs).astype(F32) * F32(np.max(boxes) + F32(1))
        return (boxes + shift[:, None]).astype(F32)


def mmcv_batched_nms(boxes, scores, idxs, iou_thr, split_thr=10000):
    """mmcv.ops.batched_nms(boxes, scores, idxs, dict(type='nms', iou_thr=...)): the single-call
    branch -> kept indices, best score first."""
    assert len(boxes) < split_thr
    return mmcv_nms(class_shift(boxes, idxs), scores, iou_thr)


def multiclass_nms_single(obj_scores, sem_scores, bbox, test_cfg, with_yaw=True):
    """:471-543 for one sample (torch tensors on one device) -> (boxes [K, 7], scores, labels).
    The non-empty mask is `box_indices >= 0`: always true, so it selects everything."""
    boxes = from_origin(bbox, (0.5, 0.5, 1.0))
    corner3d = corners(boxes)
    minmax = torch.cat([corner3d.min(1)[0], corner3d.max(1)[0]], 1)
    bbox_classes = torch.argmax(sem_scores, -1)
    keep = mmcv_batched_nms(minmax[:, [0, 1, 3, 4]].cpu().numpy(), obj_scores.cpu().numpy(),
                            bbox_classes.cpu().numpy(), test_cfg["nms_cfg"]["iou_thr"])
    keep = torch.from_numpy(keep[:test_cfg["max_output_num"]]).to(bbox.device)
    nms_mask = torch.zeros_like(bbox_classes).scatter(0, keep, 1)
    selected = nms_mask.bool() & (obj_scores >= test_cfg["score_thr"])
    if test_cfg["per_class_proposal"]:
        classes = sem_scores.shape[-1]
        return (torch.cat([boxes[selected]] * classes), torch.cat([obj_scores[selected]] * classes),
                torch.cat([torch.zeros_like(bbox_classes[selected]).fill_(k)
                           for k in range(classes)]))
    return boxes[selected], obj_scores[selected], bbox_classes[selected]


def get_bboxes(bbox_preds, num_dir_bins, test_cfg):
    """:439-469: the per-sample loop."""
    sem_scores = torch.sigmoid(bbox_preds["obj_scores"]).transpose(1, 2)
    obj_scores = sem_scores.max(-1)[0]
    bbox3d = decode(bbox_preds, num_dir_bins)
    return [multiclass_nms_single(obj_scores[b], sem_scores[b], bbox3d[b], test_cfg)
            for b in range(bbox3d.shape[0])]
