"""DynamicScatter / dynamic_scatter: mmdet3d/ops/voxel/scatter_points.py on the HIP path.

The reference re-derives the voxel of every point on each call (linear id, argsort, float
atomics, a host read) and loops over the batch in Python.  Here the index half -- unique
coordinate rows, point -> voxel map, segment table -- is a `ScatterIndex` computed once per
coordinate set (`scatter_index`) and shared by every reduce and gather on it; a 4-column
(batch, z, y, x) call is one launch set, its rows in lexicographic order, which is the
reference loop's order (sample by sample, each sample's rows sorted) whenever the last
row carries the largest batch id, as every detector's concatenation does.

Reductions accumulate in ascending point index without float atomics: results are
bitwise reproducible.  max's gradient goes to the smallest point index attaining the
maximum, the point the reference's atomicMin traceback picks."""
import torch
from torch import nn

from . import kernels as K
from .kernels import ScatterIndex, scatter_index

__all__ = ["ScatterIndex", "scatter_index", "scatter_reduce", "gather_points", "dynamic_scatter",
           "DynamicScatter"]


class _ScatterReduce(torch.autograd.Function):

    @staticmethod
    def forward(ctx, feats, index, reduce_type):
        out, arg = K.scatter_reduce(feats.contiguous(), index, reduce_type)
        ctx.index, ctx.reduce_type, ctx.argmax = index, reduce_type, arg
        return out

    @staticmethod
    def backward(ctx, grad):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        idx = ctx.index
        g = K.scatter_reduce_backward(grad.contiguous(), idx.point2voxel, ctx.reduce_type,
                                      counts=idx.counts, argmax=ctx.argmax)
        return g, None, None


class _GatherPoints(torch.autograd.Function):

    @staticmethod
    def forward(ctx, voxel_feats, index):
        ctx.index = index
        return K.scatter_gather(voxel_feats, index.point2voxel)

    @staticmethod
    def backward(ctx, grad):
        if not ctx.needs_input_grad[0]:
            return None, None
        # the gather's transpose is the sum reduce on the same segments (no scatter-add)
        g, _ = K.scatter_reduce(grad.contiguous(), ctx.index, "sum")
        return g, None


def scatter_reduce(feats, index, reduce_type="max"):
    """feats[N, C] float32 -> [M, C] (sum | mean | max) over `index`'s voxels (autograd)."""
    K._reduce_code(reduce_type)
    return _ScatterReduce.apply(feats, index, reduce_type)


def gather_points(voxel_feats, index):
    """voxel_feats[M, C] -> [N, C]: every point gets its voxel's row, invalid points 0
    (DynamicVFE.map_voxel_center_to_point; autograd)."""
    return _GatherPoints.apply(voxel_feats, index)


def dynamic_scatter(feats, coors, reduce_type="max", index=None):
    """scatter_points.py:_dynamic_scatter: -> (voxel_feats[M, C], voxel_coors[M, NDim]).
    `index`: a ScatterIndex of `coors` computed before (skips the index half)."""
    if index is None:
        index = scatter_index(coors.contiguous())
    return scatter_reduce(feats, index, reduce_type), index.voxel_coors


class DynamicScatter(nn.Module):
    """scatter_points.py:DynamicScatter: same constructor, same outputs.  forward also takes
    a precomputed `index` of the same coordinates."""

    def __init__(self, voxel_size, point_cloud_range, average_points: bool):
        super().__init__()
        self.voxel_size = voxel_size
        self.point_cloud_range = point_cloud_range
        self.average_points = average_points

    @property
    def reduce_type(self):
        return "mean" if self.average_points else "max"

    def forward_single(self, points, coors, index=None):
        return dynamic_scatter(points.contiguous(), coors.contiguous(), self.reduce_type, index)

    def forward(self, points, coors, index=None):
        """points[N, C], coors[N, 3] or [N, 4] (batch, z, y, x): one launch set either way."""
        return self.forward_single(points, coors, index)

    def __repr__(self):
        return (f"{self.__class__.__name__}(voxel_size={self.voxel_size}, point_cloud_range="
                f"{self.point_cloud_range}, average_points={self.average_points})")
