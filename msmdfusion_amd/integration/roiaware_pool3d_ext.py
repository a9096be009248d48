"""`roiaware_pool3d_ext` -- the pybind module of mmdet3d/ops/roiaware_pool3d
(src/roiaware_pool3d.cpp:126-136), on the C ABI: forward / backward with the reference's
argument lists and in-place outputs, and points_in_boxes_gpu / _batch / _cpu.

forward fills the caller's zero-initialised tensors as roiaware_pool3d_launcher does:
pts_idx_of_voxels slot 0 = count, slots 1..count = the points (ascending index, at most
max_pts_per_voxel - 1); pooled_features where a point won (max) or the count is > 0 (avg);
argmax everywhere (max) and not at all (avg).  The table is built from the library's compact
index and is the only padded table on this path.  backward rebuilds that index from the
table it is handed and adds into grad_in in a fixed order -- each point's hits in ascending
RoI order, float32, then added to grad_in's value -- instead of float atomics: bitwise
reproducible.  out sizes above 256 are refused (the reference's 8-bit packing aliases)."""
import torch

from .. import kernels as K
from ..roiaware_pool3d import points_in_boxes_cpu as _pib_cpu

_MODES = {0: "max", 1: "avg"}


def _check_input(**ts):
    dev = None
    for name, t in ts.items():
        if not t.is_cuda:
            raise RuntimeError("%s must be a CUDAtensor" % name)
        if not t.is_contiguous():
            raise RuntimeError("%s must be contiguous" % name)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("%s is on %s, not %s" % (name, t.device, dev))
    return dev


def _mode(pool_method):
    if pool_method not in _MODES:
        raise RuntimeError("pool_method must be 0 (max) or 1 (avg), got %r" % (pool_method,))
    return _MODES[pool_method]


def forward(rois, pts, pts_feature, argmax, pts_idx_of_voxels, pooled_features, pool_method):
    """roiaware_pool3d.cpp:49-90.  rois[N, 7], pts[npoints, 3], pts_feature[npoints, C];
    argmax / pooled_features [N, X, Y, Z, C], pts_idx_of_voxels [N, X, Y, Z, max_pts]."""
    mode = _mode(pool_method)
    dev = _check_input(rois=rois, pts=pts, pts_feature=pts_feature, argmax=argmax,
                       pts_idx_of_voxels=pts_idx_of_voxels, pooled_features=pooled_features)
    if pts_idx_of_voxels.dim() != 5:
        raise RuntimeError("pts_idx_of_voxels must be [N, out_x, out_y, out_z, max_pts]")
    out_xyz = tuple(int(v) for v in pts_idx_of_voxels.shape[1:4])
    with torch.cuda.device(dev):
        index = K.roiaware_index(rois, pts, out_xyz, int(pts_idx_of_voxels.shape[4]))
        K.roiaware_write_table(index, pts_idx_of_voxels)
        K.roiaware_pool(pts_feature, index, mode, pooled=pooled_features,
                        argmax=argmax if mode == "max" else None)
    return 1


def backward(pts_idx_of_voxels, argmax, grad_out, grad_in, pool_method):
    """roiaware_pool3d.cpp:92-124: grad_in[npoints, C] += the gradient of grad_out[N, X, Y, Z,
    C] through the table (avg) or argmax (max).  Both modes walk the inverse of the table:
    max adds grad_out where argmax names the point among the voxel's listed points, so it
    needs the table that forward wrote together with that argmax (the reference's max
    backward reads argmax alone)."""
    mode = _mode(pool_method)
    dev = _check_input(pts_idx_of_voxels=pts_idx_of_voxels, argmax=argmax, grad_out=grad_out,
                       grad_in=grad_in)
    if grad_in.dim() != 2:
        raise RuntimeError("grad_in must be [npoints, C]")
    with torch.cuda.device(dev):
        index = K.roiaware_index_from_table(pts_idx_of_voxels, int(grad_in.shape[0]))
        K.roiaware_pool_backward(grad_out, index, mode,
                                 argmax=argmax if mode == "max" else None, grad_in=grad_in)
    return 1


def points_in_boxes_gpu(boxes_tensor, pts_tensor, box_idx_of_points_tensor):
    """points_in_boxes_cuda.cu:156-179: box_idx_of_points[B, M] <- the first box holding the
    point; points in no box keep the caller's value (points_in_boxes.py fills -1)."""
    dev = _check_input(boxes_tensor=boxes_tensor, pts_tensor=pts_tensor,
                       box_idx_of_points_tensor=box_idx_of_points_tensor)
    with torch.cuda.device(dev):
        res = K.points_in_boxes(boxes_tensor, pts_tensor, all_hits=False)
        if tuple(box_idx_of_points_tensor.shape) != tuple(res.shape) or \
                box_idx_of_points_tensor.dtype != torch.int32:
            raise RuntimeError("box_idx_of_points must be [B, M] int32")
        box_idx_of_points_tensor.copy_(torch.where(res >= 0, res, box_idx_of_points_tensor))
    return 1


def points_in_boxes_batch(boxes_tensor, pts_tensor, box_idx_of_points_tensor):
    """points_in_boxes_cuda.cu:181-203: box_idx_of_points[B, M, T] <- 1 where the point is in
    box k; other entries keep the caller's value (points_in_boxes.py fills 0)."""
    dev = _check_input(boxes_tensor=boxes_tensor, pts_tensor=pts_tensor,
                       box_idx_of_points_tensor=box_idx_of_points_tensor)
    with torch.cuda.device(dev):
        res = K.points_in_boxes(boxes_tensor, pts_tensor, all_hits=True)
        if tuple(box_idx_of_points_tensor.shape) != tuple(res.shape) or \
                box_idx_of_points_tensor.dtype != torch.int32:
            raise RuntimeError("box_idx_of_points must be [B, M, T] int32")
        box_idx_of_points_tensor.masked_fill_(res.bool(), 1)
    return 1


def points_in_boxes_cpu(boxes_tensor, pts_tensor, pts_indices_tensor):
    """points_in_boxes_cpu.cpp:42-69: pts_indices[N, npoints] <- 0 / 1 (every element)."""
    for name, t in (("boxes_tensor", boxes_tensor), ("pts_tensor", pts_tensor),
                    ("pts_indices_tensor", pts_indices_tensor)):
        if not t.is_contiguous():
            raise RuntimeError("%s must be contiguous" % name)
    pts_indices_tensor.copy_(_pib_cpu(pts_tensor, boxes_tensor))
    return 1
