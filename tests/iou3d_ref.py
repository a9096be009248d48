"""Numpy restatements of the reference's NMS family, for the iou3d tests.

  greedy_nms        the host loop of mmdet3d/ops/iou3d/src/iou3d.cpp:128-143 over a pairwise
                    predicate matrix (row i suppresses a later column j)
  circle_nms        mmdet3d/core/post_processing/box3d_nms.py:158-181, float32 scalars, with
                    the visiting order handed in (the reference's own order on tied scores is
                    unspecified; the product sorts stably)
  iou_normal        iou3d_kernel.cu:333-343 in float32
  iou_bev           iou3d_kernel.cu:244-251 over the oracle's rotated overlap
  stable_order      descending score, ties lower index first
"""
import numpy as np

F = np.float32


def stable_order(scores):
    return np.argsort(-np.asarray(scores, np.float64), kind="stable")


def greedy_nms(hit):
    """hit[i, j] (i < j in visiting order): box i, when kept, suppresses box j."""
    n = hit.shape[0]
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        removed[i + 1:] |= hit[i, i + 1:]
    return keep


def circle_nms(dets, thresh, post_max_size=83, order=None):
    dets = np.asarray(dets, F)
    x1, y1 = dets[:, 0], dets[:, 1]
    order = stable_order(dets[:, 2]) if order is None else order
    ndets = dets.shape[0]
    suppressed = np.zeros(ndets, np.int32)
    thresh = F(thresh)
    keep = []
    for _i in range(ndets):
        i = order[_i]
        if suppressed[i] == 1:
            continue
        keep.append(int(i))
        for _j in range(_i + 1, ndets):
            j = order[_j]
            if suppressed[j] == 1:
                continue
            dist = (x1[i] - x1[j]) ** 2 + (y1[i] - y1[j]) ** 2
            if dist <= thresh:
                suppressed[j] = 1
    return keep[:post_max_size]


def circle_hits(xy, thresh):
    """The pair test of circle_nms as a matrix (float32, operand order of :176)."""
    xy = np.asarray(xy, F)
    dx = xy[:, None, 0] - xy[None, :, 0]
    dy = xy[:, None, 1] - xy[None, :, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        return (dx * dx + dy * dy) <= F(thresh)


def iou_normal(a, b):
    a, b = np.asarray(a, F)[:, None, :], np.asarray(b, F)[None, :, :]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        left, right = np.fmax(a[..., 0], b[..., 0]), np.fmin(a[..., 2], b[..., 2])
        top, bottom = np.fmax(a[..., 1], b[..., 1]), np.fmin(a[..., 3], b[..., 3])
        width, height = np.fmax(right - left, F(0)), np.fmax(bottom - top, F(0))
        inter = width * height
        sa = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        sb = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
        return inter / np.fmax(sa + sb - inter, F(1e-8))


def iou_bev(a, b, dtype=F):
    """Rotated IoU of xyxyr boxes; dtype float64 evaluates the division (not the overlap, which
    is the oracle's float32 polygon area) in double, for margin checks."""
    from oracle import head_loss as OH
    a, b = np.asarray(a, F), np.asarray(b, F)
    s = OH.boxes_overlap_bev(a, b).astype(dtype)
    sa = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])).astype(dtype)[:, None]
    sb = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(dtype)[None, :]
    with np.errstate(invalid="ignore"):
        return s / np.fmax(sa + sb - s, dtype(1e-8))


def nms(kind, boxes, thresh, order):
    """Kept ORIGINAL indices, best first, for boxes visited in `order`."""
    b = np.asarray(boxes, F)[order]
    if kind == "circle":
        hit = circle_hits(b[:, :2], thresh)
    elif kind == "normal":
        hit = iou_normal(b[:, :4], b[:, :4]) > F(thresh)
    else:
        with np.errstate(invalid="ignore"):
            hit = iou_bev(b[:, :5], b[:, :5]) > F(thresh)
    return [int(order[i]) for i in greedy_nms(hit)]
