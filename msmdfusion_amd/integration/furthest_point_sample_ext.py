"""`furthest_point_sample_ext` -- the pybind module of mmdet3d/ops/furthest_point_sample
(src/furthest_point_sample.cpp:32-65) on the C ABI.  `temp` is the reference's scratch of
running minima (the caller fills it with 1e10); the kernels keep the minima in registers
where they fit and use their own scratch otherwise, so it is accepted and left alone."""
import torch

from .. import kernels as K
from ._pointnet_common import check_input, check_shape


def furthest_point_sampling_wrapper(b, n, m, points_tensor, temp_tensor, idx_tensor):
    """idx[b, m] (int32) <- FPS of points[b, n, 3]."""
    dev = check_input(points_tensor=points_tensor, temp_tensor=temp_tensor, idx_tensor=idx_tensor)
    with torch.cuda.device(dev):
        out = K.furthest_point_sample(check_shape("points_tensor", points_tensor, (b, n, 3)), m)
        check_shape("idx_tensor", idx_tensor, (b, m), torch.int32).copy_(out)
    return 1


def furthest_point_sampling_with_dist_wrapper(b, n, m, points_tensor, temp_tensor, idx_tensor):
    """idx[b, m] (int32) <- FPS on the distance matrix points[b, n, n]."""
    dev = check_input(points_tensor=points_tensor, temp_tensor=temp_tensor, idx_tensor=idx_tensor)
    with torch.cuda.device(dev):
        K.furthest_point_sample_with_dist(
            check_shape("points_tensor", points_tensor, (b, n, n)), m,
            out=check_shape("idx_tensor", idx_tensor, (b, m), torch.int32))
    return 1
