"""`voxel_layer` -- the pybind module of mmdet3d/ops/voxel (voxelization.cpp:6-11),
on the C ABI: hard_voxelize, dynamic_voxelize and dynamic_point_to_voxel_forward /
_backward with the reference's argument lists and outputs (GPU tensors only)."""
import ctypes as C

import torch

from .. import kernels as K
from .._lib import check, float_arr, lib


def hard_voxelize(points, voxels, coors, num_points_per_voxel, voxel_size, coors_range,
                  max_points, max_voxels, NDim=3):
    """voxelization.h:51-69: fills the caller's `voxels[max_voxels,max_points,C]`,
    `coors[max_voxels,3]` (z,y,x) and `num_points_per_voxel[max_voxels]` in place and
    returns the number of voxels (mmdet3d/ops/voxel/voxelize.py:41-59 slices by it).
    Rows [0, voxel_num) are written completely, zero padding included; rows beyond
    keep the caller's contents (voxelize.py:46-50 zero-fills them)."""
    if NDim != 3:
        raise RuntimeError("hard_voxelize: only NDim == 3 is built")
    if not points.is_cuda:
        raise RuntimeError("hard_voxelize: points must live on the GPU (no CPU path)")
    if points.dtype != torch.float32 or voxels.dtype != torch.float32 or \
            coors.dtype != torch.int32 or num_points_per_voxel.dtype != torch.int32:
        raise RuntimeError("hard_voxelize: float32 points/voxels and int32 coors/num_points")
    if not (points.is_contiguous() and voxels.is_contiguous() and coors.is_contiguous()
            and num_points_per_voxel.is_contiguous()):
        raise RuntimeError("hard_voxelize: tensors must be contiguous")
    n, c = points.shape
    if tuple(voxels.shape) != (max_voxels, max_points, c) or tuple(coors.shape) != (max_voxels, 3) \
            or num_points_per_voxel.shape[0] != max_voxels:
        raise RuntimeError("hard_voxelize: output tensors do not match max_voxels / max_points")
    with torch.cuda.device(points.device):
        count = torch.empty((1,), dtype=torch.int32, device=points.device)
        nbytes = lib.msmd_voxelize_workspace_bytes(n, int(max_voxels), int(max_points))
        ws = torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=points.device)
        stream = torch.cuda.current_stream(points.device).cuda_stream
        check(lib.msmd_hard_voxelize(
            C.c_void_p(points.data_ptr()), n, c, float_arr(voxel_size), float_arr(coors_range),
            int(max_points), int(max_voxels), C.c_void_p(voxels.data_ptr()),
            C.c_void_p(coors.data_ptr()), C.c_void_p(num_points_per_voxel.data_ptr()), None,
            C.c_void_p(count.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, C.c_void_p(stream)),
            "msmd_hard_voxelize")
        return int(count.item())      # the one host read the reference has too


def _same_device(points, *ts):
    for t in ts:
        if not t.is_cuda or t.device != points.device:
            raise RuntimeError("all tensors must live on the GPU of the first argument")


def dynamic_voxelize(points, coors, voxel_size, coors_range, NDim=3):
    """voxelization.h:71-83: fills the caller's `coors[N, NDim]` int32 in place with the
    (z, y, x) row of every point; out-of-range points get the reference kernel's -1 pattern
    (voxelization_cuda.cu:25-61) and keep the caller's values in the slots it skips."""
    if not points.is_cuda:
        raise RuntimeError("dynamic_voxelize: points must live on the GPU (no CPU path)")
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] < 3:
        raise RuntimeError("dynamic_voxelize: points must be [N, >=3] float32")
    _same_device(points, coors)
    if NDim < 3 or coors.dtype != torch.int32 or not coors.is_contiguous() or \
            tuple(coors.shape) != (points.shape[0], NDim):
        raise RuntimeError("dynamic_voxelize: coors must be [points.shape[0], NDim] int32 "
                           "contiguous (NDim >= 3)")
    with torch.cuda.device(points.device):
        K.dynamic_voxelize(points.contiguous(), voxel_size, coors_range, coors)


def _check_scatter_inputs(feats, coors):
    if not feats.is_cuda:
        raise RuntimeError("dynamic_point_to_voxel: feats must live on the GPU (no CPU path)")
    _same_device(feats, coors)
    if feats.dtype != torch.float32 or feats.dim() != 2:
        raise RuntimeError("dynamic_point_to_voxel: feats must be [N, C] float32")
    if coors.dtype != torch.int32 or coors.dim() != 2 or coors.shape[0] != feats.shape[0]:
        raise RuntimeError("dynamic_point_to_voxel: coors must be [N, NDim] int32")
    if not (feats.is_contiguous() and coors.is_contiguous()):
        raise RuntimeError("dynamic_point_to_voxel: tensors must be contiguous")


def dynamic_point_to_voxel_forward(feats, coors, reduce_type):
    """voxelization.h:96-108 -> [reduced_feats[M,C], out_coors[M,NDim], coors_map[N],
    reduce_count[M]].  Rows in lexicographic coordinate order (the reference's argsort of
    its linear id); reduce_count is filled for "mean" only and zero otherwise, as
    scatter_points_cuda.cu:278-305 accumulates it for MEAN alone."""
    code = K._reduce_code(reduce_type)
    _check_scatter_inputs(feats, coors)
    with torch.cuda.device(feats.device):
        idx = K.scatter_index(coors)
        reduced, _ = K.scatter_reduce(feats, idx, reduce_type)
        count = idx.counts if code == 1 else torch.zeros_like(idx.counts)
        return [reduced, idx.voxel_coors, idx.point2voxel, count]


def dynamic_point_to_voxel_backward(grad_feats, grad_reduced_feats, feats, reduced_feats,
                                    coors_map, reduce_count, reduce_type):
    """voxelization.h:110-128: fills the caller's `grad_feats[N, C]` in place.  max re-derives
    the argmax from (feats, reduced_feats) as the reference's traceback kernel does: the
    smallest point index whose value equals the maximum takes the gradient."""
    code = K._reduce_code(reduce_type)
    _check_scatter_inputs(feats, coors_map.view(-1, 1) if coors_map.dim() == 1 else coors_map)
    _same_device(feats, grad_feats, grad_reduced_feats, reduced_feats, reduce_count)
    for name, t in (("grad_feats", grad_feats), ("grad_reduced_feats", grad_reduced_feats),
                    ("reduced_feats", reduced_feats)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("dynamic_point_to_voxel_backward: %s must be contiguous float32"
                               % name)
    if grad_feats.shape != feats.shape or grad_reduced_feats.shape != reduced_feats.shape or \
            reduced_feats.dim() != 2 or reduced_feats.shape[1] != feats.shape[1]:
        raise RuntimeError("dynamic_point_to_voxel_backward: shapes do not match")
    if reduce_count.dtype != torch.int32 or coors_map.dim() != 1 or \
            reduce_count.shape[0] != reduced_feats.shape[0]:
        raise RuntimeError("dynamic_point_to_voxel_backward: coors_map[N] / reduce_count[M] "
                           "must be int32")
    with torch.cuda.device(feats.device):
        arg = K.scatter_max_argmax(feats, coors_map, reduced_feats) if code == 2 else None
        K.scatter_reduce_backward(grad_reduced_feats, coors_map, reduce_type,
                                  counts=reduce_count if code == 1 else None, argmax=arg,
                                  out=grad_feats)
