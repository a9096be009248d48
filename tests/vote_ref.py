"""Restatements for the VoteNet op tests (csrc/vote.hip, the aligned3d kind of csrc/nms.hip).

  chamfer_forward     models/losses/chamfer_distance.py:50-55 in numpy float32: the criterion per
                      coordinate, summed (cx + cy) + cz, then torch.min's rule (lowest index on
                      ties, the first NaN wins)
  chamfer_backward    the fixed-order gradient the kernel promises: the point's own term, then
                      the points of the other set that chose it, ascending; float32 differences,
                      products and running sum in float64, rounded to float32 at the end
  vote_targets_loop   VoteHead.get_targets_single, vote_head.py:472-501, as written (torch), over
                      an inclusion table handed in
  aligned_nms         core/post_processing/box3d_nms.py:91-138 over a visiting order handed in
                      (the reference's argsort is not stable), float32
"""
import numpy as np
import torch

F = np.float32

# tests/test_utils/test_nms.py test_aligned_3d_nms of the reference: 30 boxes, their scores and
# classes, and the pick at threshold 0.25
LITERAL_BOXES = [
    [1.2261, 0.6679, -1.2678, 2.6547, 1.0428, 0.1000], [5.0919, 0.6512, 0.7238, 5.4821, 1.2451, 2.1095],
    [6.8392, -1.2205, 0.8570, 7.6920, 0.3220, 3.2223], [3.6900, -0.4235, -1.0380, 4.4415, 0.2671, -0.1442],
    [4.8071, -1.4311, 0.7004, 5.5788, -0.6837, 1.2487], [2.1807, -1.5811, -1.1289, 3.0151, -0.1346, -0.5351],
    [4.4631, -4.2588, -1.1403, 5.3012, -3.4463, -0.3212], [4.7607, -3.3311, 0.5993, 5.2976, -2.7874, 1.2273],
    [3.1265, 0.7113, -0.0296, 3.8944, 1.3532, 0.9785], [5.5828, -3.5350, 1.0105, 8.2841, -0.0405, 3.3614],
    [3.0003, -2.1099, -1.0608, 5.3423, 0.0328, 0.6252], [2.7148, 0.6082, -1.1738, 3.6995, 1.2375, -0.0209],
    [4.9263, -0.2152, 0.2889, 5.6963, 0.3416, 1.3471], [5.0713, 1.3459, -0.2598, 5.6278, 1.9300, 1.2835],
    [4.5985, -2.3996, -0.3393, 5.2705, -1.7306, 0.5698], [4.1386, 0.5658, 0.0422, 4.8937, 1.1983, 0.9911],
    [2.7694, -1.9822, -1.0637, 4.0691, 0.3575, -0.1393], [4.6464, -3.0123, -1.0694, 5.1421, -2.4450, -0.3758],
    [3.4754, 0.4443, -1.1282, 4.6727, 1.3786, 0.2550], [2.5905, -0.3504, -1.1202, 3.1599, 0.1153, -0.3036],
    [4.1336, -3.4813, 1.1477, 6.2091, -0.8776, 2.6757], [3.9966, 0.2069, -1.1148, 5.0841, 1.0525, -0.0648],
    [4.3216, -1.8647, 0.4733, 6.2069, 0.6671, 3.3363], [4.7683, 0.4286, -0.0500, 5.5642, 1.2906, 0.8902],
    [1.7337, 0.7625, -1.0058, 3.0675, 1.3617, 0.3849], [4.7193, -3.3687, -0.9635, 5.1633, -2.7656, 1.1001],
    [4.4704, -2.7744, -1.1127, 5.0971, -2.0228, -0.3150], [2.7027, 0.6122, -0.9169, 3.3083, 1.2117, 0.6129],
    [4.8789, -2.0025, 0.8385, 5.5214, -1.3668, 1.3552], [3.7856, -1.7582, -0.1738, 5.3373, -0.6300, 0.5558]]
LITERAL_SCORES = [
    3.6414e-03, 2.2901e-02, 2.7576e-04, 1.2238e-02, 5.9310e-04, 1.2659e-01, 2.4104e-02, 5.0742e-03,
    2.3581e-03, 2.0946e-07, 8.8039e-01, 1.9127e-01, 5.0469e-05, 9.3638e-03, 3.0663e-03, 9.4350e-03,
    5.3380e-02, 1.7895e-01, 2.0048e-01, 1.1294e-03, 3.0304e-08, 2.0237e-01, 1.0894e-08, 6.7972e-02,
    6.7156e-01, 9.3986e-04, 7.9470e-01, 3.9736e-01, 1.8000e-04, 7.9151e-04]
LITERAL_CLASSES = [8, 8, 8, 3, 3, 1, 3, 3, 7, 8, 0, 6, 7, 8, 3, 7, 2, 7, 6, 3, 8, 6, 6, 7, 6, 8, 7, 6,
                   3, 1]
LITERAL_PICK = [10, 26, 24, 27, 21, 18, 17, 5, 23, 16, 6, 1, 3, 15, 13, 7, 0, 14, 8, 19, 25, 29, 4, 2,
                28, 12, 9, 20, 22]


def criterion(d, mode):
    d = np.asarray(d, F)
    if mode == "l2":
        return d * d
    z = np.abs(d)
    if mode == "l1":
        return z
    with np.errstate(invalid="ignore"):
        return np.where(z < F(1), (F(0.5) * z) * z, z - F(0.5)).astype(F)


def slope(d, mode):
    d = np.asarray(d, F)
    if mode == "l2":
        return F(2) * d
    with np.errstate(invalid="ignore"):
        sign = np.where(d > 0, F(1), np.where(d < 0, F(-1), F(0))).astype(F)
        if mode == "l1":
            return sign
        return np.where(np.abs(d) < F(1), d, sign).astype(F)


def chamfer_matrix(src, dst, mode):
    """[B, N, M] float32 -- test side only; the kernels never hold it."""
    src, dst = np.asarray(src, F), np.asarray(dst, F)
    with np.errstate(invalid="ignore", over="ignore"):
        c = criterion(src[:, :, None, :] - dst[:, None, :, :], mode)
        return (c[..., 0] + c[..., 1]) + c[..., 2]


def chamfer_forward(src, dst, mode):
    """-> d1 [B, N], i1 int64 [B, N], d2 [B, M], i2 int64 [B, M].  numpy's argmin has torch.min's
    rule: the first occurrence of the minimum, and the first NaN when there is one."""
    dist = chamfer_matrix(src, dst, mode)
    i1, i2 = dist.argmin(2), dist.argmin(1)
    d1 = np.take_along_axis(dist, i1[:, :, None], 2)[:, :, 0]
    d2 = np.take_along_axis(dist, i2[:, None, :], 1)[:, 0, :]
    return d1, i1.astype(np.int64), d2, i2.astype(np.int64)


def _side_grad(own, oth, g_own, i_own, g_oth, i_oth, mode):
    b = np.arange(own.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        near = np.take_along_axis(oth, i_own[:, :, None], 1)
        d = np.float64
        acc = 0.0 + g_own[:, :, None].astype(d) * slope(own - near, mode).astype(d)
        for o in range(oth.shape[1]):                 # ascending: the promised order
            at = i_oth[:, o]
            term = g_oth[:, o, None].astype(d) * slope(own[b, at] - oth[:, o], mode).astype(d)
            acc[b, at] = acc[b, at] + term
    return acc.astype(F)


def chamfer_backward(src, dst, g1, g2, i1, i2, mode):
    src, dst, g1, g2 = (np.asarray(a, F) for a in (src, dst, g1, g2))
    return (_side_grad(src, dst, g1, i1, g2, i2, mode),
            _side_grad(dst, src, g2, i2, g1, i1, mode))


def vote_targets_loop(points, inside, centers, gt_per_seed=3):
    """points [N, >= 3], inside [N, T] (0 / 1), centers [T, 3] -> (vote_targets [N, 9],
    vote_target_masks long [N]); the reference loop, statement by statement."""
    num_points = points.shape[0]
    vote_targets = points.new_zeros([num_points, 3 * gt_per_seed])
    vote_target_masks = points.new_zeros([num_points], dtype=torch.long)
    vote_target_idx = points.new_zeros([num_points], dtype=torch.long)
    for i in range(centers.shape[0]):
        box_indices = inside[:, i]
        indices = torch.nonzero(box_indices, as_tuple=False).squeeze(-1)
        selected_points = points[indices]
        vote_target_masks[indices] = 1
        vote_targets_tmp = vote_targets[indices]
        votes = centers[i].unsqueeze(0) - selected_points[:, :3]
        for j in range(gt_per_seed):
            column_indices = torch.nonzero(vote_target_idx[indices] == j,
                                           as_tuple=False).squeeze(-1)
            vote_targets_tmp[column_indices, int(j * 3):int(j * 3 + 3)] = votes[column_indices]
            if j == 0:
                vote_targets_tmp[column_indices] = votes[column_indices].repeat(1, gt_per_seed)
        vote_targets[indices] = vote_targets_tmp
        vote_target_idx[indices] = torch.clamp(vote_target_idx[indices] + 1, max=2)
    return vote_targets, vote_target_masks


def aligned_hits(boxes, classes, thresh):
    """hit[i, j]: box i, when kept, removes box j -- the complement of the reference's
    `iou <= thresh` selection, so a NaN IoU removes.  float32 throughout."""
    b = np.asarray(boxes, F)
    lo, hi = b[:, :3], b[:, 3:6]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ext = np.fmax(F(0), np.fmin(hi[:, None], hi[None]) - np.fmax(lo[:, None], lo[None]))
        inter = (ext[..., 0] * ext[..., 1]) * ext[..., 2]
        size = hi - lo
        vol = (size[:, 0] * size[:, 1]) * size[:, 2]
        iou = inter / ((vol[:, None] + vol[None, :]) - inter)
        cls = np.asarray(classes)
        iou = iou * (cls[:, None] == cls[None, :]).astype(F)
        return ~(iou <= F(thresh))


def aligned_nms(boxes, classes, thresh, order):
    """Kept ORIGINAL indices, best first, for boxes visited in `order`."""
    order = np.asarray(order)
    hit = aligned_hits(np.asarray(boxes, F)[order], np.asarray(classes)[order], thresh)
    n = len(order)
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(int(order[i]))
        removed[i + 1:] |= hit[i, i + 1:]
    return keep
