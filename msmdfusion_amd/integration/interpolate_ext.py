"""`interpolate_ext` -- the pybind module of mmdet3d/ops/interpolate
(src/interpolate.cpp:46-93) on the C ABI.  three_nn_wrapper writes SQUARED distances, as the
reference's kernel does (three_nn.py takes the root).  three_interpolate_grad_wrapper adds
into the zero-initialised grad_points it is given, in a fixed order (each source's (point,
slot) destinations in ascending position, float32) instead of float atomics."""
import torch

from .. import kernels as K
from ._pointnet_common import check_input, check_shape


def three_nn_wrapper(b, n, m, unknown_tensor, known_tensor, dist2_tensor, idx_tensor):
    """dist2 / idx [b, n, 3] <- the three nearest of known[b, m, 3] to unknown[b, n, 3]."""
    dev = check_input(unknown_tensor=unknown_tensor, known_tensor=known_tensor,
                      dist2_tensor=dist2_tensor, idx_tensor=idx_tensor)
    with torch.cuda.device(dev):
        K.three_nn(check_shape("unknown_tensor", unknown_tensor, (b, n, 3)),
                   check_shape("known_tensor", known_tensor, (b, m, 3)),
                   dist2=check_shape("dist2_tensor", dist2_tensor, (b, n, 3)),
                   idx=check_shape("idx_tensor", idx_tensor, (b, n, 3), torch.int32))


def three_interpolate_wrapper(b, c, m, n, points_tensor, idx_tensor, weight_tensor, out_tensor):
    """out[b, c, n] <- points[b, c, m] at idx[b, n, 3] weighted by weight[b, n, 3]."""
    dev = check_input(points_tensor=points_tensor, idx_tensor=idx_tensor,
                      weight_tensor=weight_tensor, out_tensor=out_tensor)
    with torch.cuda.device(dev):
        K.three_interpolate(check_shape("points_tensor", points_tensor, (b, c, m)),
                            check_shape("idx_tensor", idx_tensor, (b, n, 3), torch.int32),
                            check_shape("weight_tensor", weight_tensor, (b, n, 3)),
                            out=check_shape("out_tensor", out_tensor, (b, c, n)))


def three_interpolate_grad_wrapper(b, c, n, m, grad_out_tensor, idx_tensor, weight_tensor,
                                   grad_points_tensor):
    """grad_points[b, c, m] += weight * grad_out[b, c, n] through idx."""
    dev = check_input(grad_out_tensor=grad_out_tensor, idx_tensor=idx_tensor,
                      weight_tensor=weight_tensor, grad_points_tensor=grad_points_tensor)
    with torch.cuda.device(dev):
        inv = K.point_inverse_index(check_shape("idx_tensor", idx_tensor, (b, n, 3), torch.int32),
                                    m)
        K.point_scatter_backward(
            check_shape("grad_out_tensor", grad_out_tensor, (b, c, n)), inv,
            weight=check_shape("weight_tensor", weight_tensor, (b, n, 3)), dest_per_out=3,
            grad_in=check_shape("grad_points_tensor", grad_points_tensor, (b, c, m)))
