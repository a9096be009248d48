"""`group_points_ext` -- the pybind module of mmdet3d/ops/group_points
(src/group_points.cpp:31-62) on the C ABI.  backward adds into the zero-initialised
grad_points it is given, in a fixed order (each source's destinations in ascending (point,
sample) position, float32, then added to grad_points' value) instead of float atomics."""
import torch

from .. import kernels as K
from ._pointnet_common import check_input, check_shape


def forward(b, c, n, npoints, nsample, points_tensor, idx_tensor, out_tensor):
    """out[b, c, npoints, nsample] <- points[b, c, n] at idx[b, npoints, nsample] (int32)."""
    dev = check_input(points_tensor=points_tensor, idx_tensor=idx_tensor, out_tensor=out_tensor)
    with torch.cuda.device(dev):
        K.group_points(check_shape("points_tensor", points_tensor, (b, c, n)),
                       check_shape("idx_tensor", idx_tensor, (b, npoints, nsample), torch.int32),
                       out=check_shape("out_tensor", out_tensor, (b, c, npoints, nsample)))
    return 1


def backward(b, c, n, npoints, nsample, grad_out_tensor, idx_tensor, grad_points_tensor):
    """grad_points[b, c, n] += grad_out[b, c, npoints, nsample] through idx."""
    dev = check_input(grad_out_tensor=grad_out_tensor, idx_tensor=idx_tensor,
                      grad_points_tensor=grad_points_tensor)
    with torch.cuda.device(dev):
        inv = K.point_inverse_index(check_shape("idx_tensor", idx_tensor, (b, npoints, nsample),
                                                torch.int32), n)
        K.point_scatter_backward(
            check_shape("grad_out_tensor", grad_out_tensor, (b, c, npoints, nsample)), inv,
            grad_in=check_shape("grad_points_tensor", grad_points_tensor, (b, c, n)))
    return 1
