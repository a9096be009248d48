"""mmdet3d/ops/iou3d (iou3d_utils.py) and circle_nms (core/post_processing/box3d_nms.py:141-181)
on the C ABI, plus the batched form the heads call.

The suppression mask and the greedy reduction both run on the device (csrc/nms.hip): nothing
is copied to the host, and one call handles every (task, sample) list.  Sorting stays in
torch: ``torch.sort(descending=True, stable=True)``, so boxes with EQUAL scores are visited
lower index first.  The reference leaves that order unspecified (``scores.sort`` is not
stable; circle_nms reverses a numpy quicksort), so its result on tied scores is whatever its
sort happened to do; everything else -- pair tests, ``>`` / ``<=``, cut sizes, the order of
the returned indices -- is the reference's.
"""
import torch

from . import kernels as K


def xywhr2xyxyr(boxes_xywhr):
    """core/bbox/structures/utils.py xywhr2xyxyr."""
    boxes = torch.zeros_like(boxes_xywhr)
    half_w, half_h = boxes_xywhr[:, 2] / 2, boxes_xywhr[:, 3] / 2
    boxes[:, 0] = boxes_xywhr[:, 0] - half_w
    boxes[:, 1] = boxes_xywhr[:, 1] - half_h
    boxes[:, 2] = boxes_xywhr[:, 0] + half_w
    boxes[:, 3] = boxes_xywhr[:, 1] + half_h
    boxes[:, 4] = boxes_xywhr[:, 4]
    return boxes


def boxes_iou_bev(boxes_a, boxes_b):
    """iou3d_utils.boxes_iou_bev: (M, 5) x (N, 5) xyxyr -> IoU (M, N)."""
    return K.boxes_iou_bev(boxes_a, boxes_b)


def segment_ids(offsets, total):
    """The segment of each of `total` rows under CSR `offsets` [S + 1] (device, no read)."""
    rows = torch.arange(total, device=offsets.device, dtype=offsets.dtype)
    return torch.searchsorted(offsets[1:].contiguous(), rows, right=True)


def nms_batched(kind, boxes, scores, offsets, thresh, pre_max=None, post_max=None):
    """NMS of S independent lists in one call, with no host read.

    kind: 'rotate' (boxes [N, 5] xyxyr, IoU > thresh), 'normal' (axis-aligned IoU of the
    first four columns > thresh), 'circle' (boxes [N, >= 2] centres, squared distance <=
    thresh) or 'aligned3d' (boxes [N, 7]: x1, y1, z1, x2, y2, z2, class; a later box goes
    unless 3-D IoU * same-class <= thresh, see aligned_3d_nms) or 'mmcv' (boxes [N, 4]: x1, y1,
    x2, y2 already shifted by class * (max + 1) as mmcv's batched_nms does; mmcv.ops.nms's test
    inter > thresh * (area_i + area_j - inter), no division and no floor on the union).
    List s is rows offsets[s] .. offsets[s+1] of boxes / scores (offsets: int
    [S + 1] on the device).  thresh: a float, or one per list (sequence or tensor).
    pre_max: only the pre_max best boxes of a list take part; it also bounds the work, so
    it is required when N exceeds 16384 (a single list: its length is the bound).
    post_max: at most that many are reported per list.

    -> keep long [S, K]: row indices into `boxes`, best score first, -1 past num_keep[s];
       num_keep int32 [S].  Equal scores: lower index first (see the module docstring)."""
    total = boxes.shape[0]
    offsets = offsets.to(device=boxes.device, dtype=torch.int32)
    segments = offsets.numel() - 1
    if pre_max is None:
        if total > K.NMS_MAX_SEGMENT and segments > 1:
            raise ValueError("nms_batched: %d boxes in %d lists need pre_max (a list holds at "
                             "most %d)" % (total, segments, K.NMS_MAX_SEGMENT))
        bound = total
    else:
        bound = min(int(pre_max), total)
    if torch.is_tensor(thresh):
        th = thresh.to(device=boxes.device, dtype=torch.float32).reshape(-1)
        if th.numel() == 1 and segments != 1:
            th = th.expand(segments).contiguous()
    elif isinstance(thresh, (list, tuple)):
        th = torch.tensor([float(t) for t in thresh], dtype=torch.float32, device=boxes.device)
    else:
        th = torch.full((segments,), float(thresh), dtype=torch.float32, device=boxes.device)
    # descending score inside each list, ties by index: a stable sort by score, then a stable
    # sort by list id (lists are contiguous, so the second only regroups)
    by_score = torch.sort(scores.reshape(-1), descending=True, stable=True)[1]
    if segments > 1:
        seg = segment_ids(offsets, total)
        order = by_score[torch.sort(seg[by_score], stable=True)[1]]
    else:
        order = by_score
    sorted_boxes = boxes.float()[order].contiguous()
    return K.nms_segments(kind, sorted_boxes, offsets, th, bound, post_max=post_max, order=order)


def _single(kind, boxes, scores, thresh, pre_max, post_max):
    n = boxes.shape[0]
    offsets = torch.tensor([0, n], dtype=torch.int32).to(boxes.device, non_blocking=True)
    keep, num = nms_batched(kind, boxes, scores, offsets, thresh, pre_max, post_max)
    return keep[0, :int(num[0])].contiguous()     # the reference's return is variable-length


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
    """iou3d_utils.nms_gpu: boxes [N, 5] xyxyr, scores [N] -> kept indices, best first."""
    return _single("rotate", boxes, scores, thresh, pre_maxsize, post_max_size)


def nms_normal_gpu(boxes, scores, thresh):
    """iou3d_utils.nms_normal_gpu: axis-aligned IoU of (x1, y1, x2, y2)."""
    return _single("normal", boxes, scores, thresh, None, None)


def circle_nms(dets, thresh, post_max_size=83):
    """box3d_nms.circle_nms on DEVICE tensors: dets [N, 3] (x, y, score) -> a device long
    tensor of kept indices (the reference takes a numpy array and returns a list).  The
    squared centre distance is evaluated in float32 exactly as numpy does there."""
    return _single("circle", dets[:, :2].contiguous(), dets[:, 2], thresh, None, post_max_size)


def aligned_3d_nms(boxes, scores, classes, thresh):
    """box3d_nms.aligned_3d_nms: boxes [N, 6] (x1, y1, z1, x2, y2, z2), scores [N], classes [N]
    -> kept indices, best first.  A box is dropped by a kept, better one of its class whose IoU
    with it exceeds thresh -- and, as in the reference's `iou <= thresh` selection, by ANY kept
    better box when the IoU is NaN (two disjoint zero-volume boxes)."""
    rows = torch.cat([boxes.float(), classes.to(boxes.device).float().reshape(-1, 1)], 1)
    return _single("aligned3d", rows, scores, thresh, None, None)
