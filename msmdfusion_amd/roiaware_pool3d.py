"""RoIAwarePool3d, points_in_boxes_* and Single3DRoIAwareExtractor: mmdet3d/ops/roiaware_pool3d
and mmdet3d/models/roi_heads/roi_extractors/single_roiaware_extractor.py on the HIP path.

The reference allocates an N_rois x N_points mask per call, collects the point lists with one
thread per RoI into a padded [N, X, Y, Z, max_pts] table (1.4 MB per RoI at out_size 14), and
adds the backward with float atomics.  Here the point lists are a compact `RoIPointIndex`
(csrc/roiaware.hip) built once per (RoIs, points) -- the Part-A2 seg and part extractors share
it -- in one launch set for the whole batch; pooling reads it, and the backward walks its
inverse (point -> kept hits in ascending RoI order): bitwise reproducible, no padded table.
out_size above 256 per axis is refused (the reference's 8-bit packing aliases there)."""
import math

import torch
from torch import nn

from . import kernels as K
from .kernels import RoIPointIndex
from .registry import ROI_EXTRACTORS

__all__ = ["RoIPointIndex", "roi_point_index", "RoIAwarePool3d", "points_in_boxes_gpu",
           "points_in_boxes_batch", "points_in_boxes_cpu", "Single3DRoIAwareExtractor"]


def roi_point_index(rois, pts, out_size, max_pts_per_voxel=128, roi_batch=None, pts_batch=None):
    """rois[R, 7] (x, y, z bottom, w, l, h, rz), pts[P, 3] float32 on the GPU -> RoIPointIndex.
    roi_batch[R] / pts_batch[P] int32 (None: one sample): a point only joins RoIs of its own
    batch id.  One host read (the hit count)."""
    if not rois.is_cuda:
        raise RuntimeError("RoI-aware pooling needs CUDA/ROCm tensors (there is no CPU path)")
    with torch.cuda.device(rois.device):
        return K.roiaware_index(rois, pts, out_size, max_pts_per_voxel, roi_batch, pts_batch)


class _RoIAwarePool3dFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pts_feature, index, mode):
        pooled, argmax = K.roiaware_pool(pts_feature.contiguous(), index, mode)
        # max keeps the index and argmax[N, X, Y, Z, C]; avg the index alone
        ctx.index, ctx.mode, ctx.argmax = index, mode, argmax
        return pooled

    @staticmethod
    def backward(ctx, grad):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        g = K.roiaware_pool_backward(grad.contiguous(), ctx.index, ctx.mode, argmax=ctx.argmax)
        return g, None, None


class RoIAwarePool3d(nn.Module):
    """roiaware_pool3d.py:RoIAwarePool3d: same constructor and forward.  forward also takes a
    precomputed `index` of the same RoIs and points (skips the index half)."""

    MODES = {"max": 0, "avg": 1}

    def __init__(self, out_size, max_pts_per_voxel=128, mode="max"):
        super().__init__()
        if mode not in self.MODES:
            raise ValueError("RoIAwarePool3d: mode must be 'max' or 'avg', got %r" % (mode,))
        self.out_size = out_size
        self.max_pts_per_voxel = max_pts_per_voxel
        self.mode = self.MODES[mode]          # the reference's pool_method code
        self.out_xyz = K.roiaware_out_size(out_size)
        if not isinstance(max_pts_per_voxel, int) or max_pts_per_voxel < 1:
            raise ValueError("RoIAwarePool3d: max_pts_per_voxel must be an int >= 1")

    @property
    def mode_name(self):
        return "max" if self.mode == 0 else "avg"

    def index(self, rois, pts, roi_batch=None, pts_batch=None):
        return roi_point_index(rois, pts, self.out_xyz, self.max_pts_per_voxel, roi_batch,
                               pts_batch)

    def pool(self, pts_feature, index):
        """pts_feature[P, C] over a RoIPointIndex -> [N, X, Y, Z, C] (autograd)."""
        if index.out_size != self.out_xyz or index.max_pts_per_voxel != self.max_pts_per_voxel:
            raise RuntimeError("RoIAwarePool3d: the index was built for out_size %s, "
                               "max_pts_per_voxel %d" % (index.out_size, index.max_pts_per_voxel))
        with torch.cuda.device(index.vox_start.device):
            return _RoIAwarePool3dFn.apply(pts_feature, index, self.mode_name)

    def forward(self, rois, pts, pts_feature, index=None):
        """rois[N, 7], pts[npoints, 3], pts_feature[npoints, C] -> [N, X, Y, Z, C]."""
        if index is None:
            index = self.index(rois, pts)
        return self.pool(pts_feature, index)

    def extra_repr(self):
        return "out_size=%r, max_pts_per_voxel=%d, mode=%r" % (self.out_size,
                                                              self.max_pts_per_voxel,
                                                              self.mode_name)


def _check_pib(points, boxes, pts_dims):
    assert boxes.shape[0] == points.shape[0], \
        f"Points and boxes should have the same batch size, " \
        f"got {points.shape[0]} and {boxes.shape[0]}"
    assert boxes.shape[2] == 7, \
        f"boxes dimension should be 7, got unexpected shape {boxes.shape[2]}"
    assert points.shape[2] == pts_dims, \
        f"points dimension should be 3, got unexpected shape {points.shape[2]}"
    if not (points.is_cuda and boxes.is_cuda):
        raise RuntimeError("points_in_boxes: points and boxes must live on the GPU "
                           "(points_in_boxes_cpu is the CPU function)")
    assert points.device == boxes.device, "Points and boxes should be put on the same device"


def points_in_boxes_gpu(points, boxes):
    """points[B, M, 3], boxes[B, T, 7] (bottom centre) -> box_idxs_of_pts[B, M] int32: the
    first box holding the point, -1 for background."""
    _check_pib(points, boxes, 3)
    with torch.cuda.device(points.device):
        return K.points_in_boxes(boxes.contiguous(), points.contiguous(), all_hits=False)


def points_in_boxes_batch(points, boxes):
    """points[B, M, 3], boxes[B, T, 7] -> box_idxs_of_pts[B, M, T] int32 0 / 1 flags."""
    _check_pib(points, boxes, 3)
    with torch.cuda.device(points.device):
        return K.points_in_boxes(boxes.contiguous(), points.contiguous(), all_hits=True)


def points_in_boxes_cpu(points, boxes):
    """points[npoints, 3], boxes[N, 7] on the CPU -> point_indices[N, npoints] int32 0 / 1
    (points_in_boxes_cpu.cpp: the same float / double predicate as the GPU kernels, restated
    on float32 tensors)."""
    assert boxes.shape[1] == 7, \
        f"boxes dimension should be 7, got unexpected shape {boxes.shape[1]}"
    assert points.shape[1] == 3, \
        f"points dimension should be 3, got unexpected shape {points.shape[1]}"
    if points.is_cuda or boxes.is_cuda:
        raise RuntimeError("points_in_boxes_cpu takes CPU tensors")
    b = boxes.float()
    p = points.float()
    x, y, z = p[:, 0][None], p[:, 1][None], p[:, 2][None]
    cx, cy, zb, w, l, h, rz = (b[:, j][:, None] for j in range(7))
    h2 = h.double() / 2.0
    cz = (zb.double() + h2).float()
    rot = (rz.double() + math.pi / 2).float()
    ca, sa = torch.cos(rot), torch.sin(rot)
    sx, sy = x - cx, y - cy
    lx = sx * ca + sy * (-sa)
    ly = sx * sa + sy * ca
    hl, hw = l.double() / 2.0, w.double() / 2.0
    lxd, lyd = lx.double(), ly.double()
    inside = ~((z - cz).abs().double() > h2) & (lxd > -hl) & (lxd < hl) & (lyd > -hw) & (lyd < hw)
    return inside.to(torch.int32)


_ROI_LAYERS = {"RoIAwarePool3d": RoIAwarePool3d}


@ROI_EXTRACTORS.register_module()
class Single3DRoIAwareExtractor(nn.Module):
    """single_roiaware_extractor.py: point-wise RoI features.  The reference pools sample by
    sample; here one launch set covers the batch, with the same result: rows grouped by
    ascending batch id, in input order within a batch, and RoIs whose batch id is negative
    or above batch_inds.max() dropped as the loop drops them."""

    def __init__(self, roi_layer=None):
        super().__init__()
        self.roi_layer = self.build_roi_layers(roi_layer)

    def build_roi_layers(self, layer_cfg):
        cfg = dict(layer_cfg)
        layer_type = cfg.pop("type")
        if layer_type not in _ROI_LAYERS:
            raise KeyError("unknown roi layer %r (built: %s)" % (layer_type, sorted(_ROI_LAYERS)))
        return _ROI_LAYERS[layer_type](**cfg)

    def build_index(self, coordinate, batch_inds, rois):
        """The RoIPointIndex of forward's selection; one index serves every extractor with
        the same out_size and max_pts_per_voxel (Part-A2's seg and part extractors).  Two
        host reads: the kept RoI count and the hit count."""
        if not (coordinate.is_cuda and rois.is_cuda and batch_inds.is_cuda):
            raise RuntimeError("Single3DRoIAwareExtractor: tensors must live on the GPU")
        if rois.dim() != 2 or rois.shape[1] != 8:
            raise RuntimeError("rois must be [N, 8] (batch id, x, y, z, w, l, h, rz)")
        pb = batch_inds.int().contiguous()
        rb = rois[:, 0].int()
        keep = (rb >= 0) & (rb <= pb.max())
        key = torch.where(keep, rb, torch.full_like(rb, torch.iinfo(torch.int32).max))
        order = torch.sort(key, stable=True).indices
        rows = order[:int(keep.sum())]
        layer = self.roi_layer
        index = roi_point_index(rois[rows, 1:].contiguous(), coordinate.contiguous(),
                                layer.out_xyz, layer.max_pts_per_voxel,
                                roi_batch=rb[rows].contiguous(), pts_batch=pb)
        index.rows = rows
        return index

    def forward(self, feats, coordinate, batch_inds, rois, index=None):
        """feats[P, C], coordinate[P, 3], batch_inds[P], rois[N, 8] -> [N', X, Y, Z, C].
        `index`: a build_index() of the same coordinate / batch_inds / rois."""
        if index is None:
            index = self.build_index(coordinate, batch_inds, rois)
        elif index.rows is None:
            raise RuntimeError("Single3DRoIAwareExtractor: pass an index from build_index()")
        return self.roi_layer.pool(feats, index)
