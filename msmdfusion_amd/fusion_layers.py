"""MVX-Net's point-image fusion: mmdet3d/models/fusion_layers/point_fusion.py (point_sample
:10-95, PointFusion :98-306) and coord_transform.py (apply_3d_transformation :7-90).

PointFusion lifts image features onto the points: every point is taken back through the 3-D
augmentation, projected with lidar2img, taken through the image augmentation (scale, crop,
flip) and bilinearly sampled from every image level; the concatenated samples and the point
features each pass Linear + BatchNorm1d and are added.

Two paths compute obtain_mlvl_feats:
  * the composition (`obtain_mlvl_feats_composed`): the reference's op sequence around
    F.grid_sample, per (sample, level).  It serves CPU tensors, aligned=False (nearest), the
    non-zero padding modes and points that require grad, and it is the tests' yardstick;
  * the fused path (csrc/point_sample.hip): one launch for all samples and levels on
    channels-last maps, writing the concatenated [N, sum C] rows directly; the backward is
    cell-stationary over an index built lazily on the first backward, without float atomics
    (bitwise reproducible).  The whole affine chain in front of the perspective divide -- the
    reversed T / S / R / HF / VF flow and lidar2img -- is composed on the host in float64 into
    one 3x4 matrix per sample and rounded to float32 once.  The forward makes no host read.
Deviation of the fused path: a point whose pixel coordinate is not finite (NaN / inf rows)
reads zeros in every level and gets no part in the backward; torch's grid_sample result for a
NaN coordinate depends on the backend.  The fused path gives no gradient to the points (the
reference's does, and nothing consumes it): points that require grad take the composition.

img_transform, pts_transform, the add, the ReLU, fuse_conv and the dropout are torch ops.
"""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import kernels as K
from .bev import ConvModule
from .registry import FUSION_LAYERS


def _meta_array(v):
    """A meta value (numpy, list, CPU / GPU tensor, scalar) as a float64 numpy array."""
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().double().numpy()
    return np.asarray(v, dtype=np.float64)


def _flow(img_meta, reverse):
    return list(img_meta.get("transformation_3d_flow", []))[::-1 if reverse else 1]


def apply_3d_transformation(pcd, coords_type, img_meta, reverse=False):
    """coord_transform.py:7-90 for 'LIDAR' points: the T / S / R / HF / VF flow of
    img_meta['transformation_3d_flow'] (reversed, with inverted steps, under reverse=True) on a
    copy of pcd[:, :3].  Missing keys default as in the reference: identity rotation, scale 1,
    zero translation, no flips, an empty flow.  A horizontal flip negates y, a vertical one x
    (LiDARPoints.flip); a rotation is pcd @ rotation (BasePoints.rotate with a matrix)."""
    if coords_type != "LIDAR":
        raise NotImplementedError("apply_3d_transformation: only 'LIDAR' coordinates are built, "
                                  "got %r" % (coords_type,))
    dtype, device = pcd.dtype, pcd.device
    rot = torch.as_tensor(img_meta["pcd_rotation"], dtype=dtype, device=device) \
        if "pcd_rotation" in img_meta else torch.eye(3, dtype=dtype, device=device)
    scale = img_meta["pcd_scale_factor"] if "pcd_scale_factor" in img_meta else 1.
    trans = torch.as_tensor(img_meta["pcd_trans"], dtype=dtype, device=device) \
        if "pcd_trans" in img_meta else torch.zeros(3, dtype=dtype, device=device)
    hflip = img_meta["pcd_horizontal_flip"] if "pcd_horizontal_flip" in img_meta else False
    vflip = img_meta["pcd_vertical_flip"] if "pcd_vertical_flip" in img_meta else False
    if reverse:
        scale, trans, rot = 1.0 / scale, -trans, rot.inverse()
    # (the reference works in place on a clone; out of place here, with the same values, so
    # that points which require grad keep a usable graph)
    xyz = pcd[:, :3].clone()
    for op in _flow(img_meta, reverse):
        if op == "T":
            xyz = xyz + trans.squeeze(0)
        elif op == "S":
            xyz = xyz * scale
        elif op == "R":
            xyz = xyz @ rot
        elif op == "HF":
            if hflip:
                xyz = xyz * xyz.new_tensor([1.0, -1.0, 1.0])
        elif op == "VF":
            if vflip:
                xyz = xyz * xyz.new_tensor([-1.0, 1.0, 1.0])
        else:
            raise AssertionError("This 3D data transformation op (%s) is not supported" % op)
    return xyz


def flow_matrix(img_meta, reverse=False):
    """apply_3d_transformation as one float64 4x4 matrix A (column convention: p' = A [p; 1]).
    Every step is affine, so the product is the flow exactly in real arithmetic."""
    rot = _meta_array(img_meta["pcd_rotation"]) if "pcd_rotation" in img_meta else np.eye(3)
    scale = float(img_meta["pcd_scale_factor"]) if "pcd_scale_factor" in img_meta else 1.0
    trans = _meta_array(img_meta["pcd_trans"]).reshape(3) if "pcd_trans" in img_meta \
        else np.zeros(3)
    hflip = bool(img_meta.get("pcd_horizontal_flip", False))
    vflip = bool(img_meta.get("pcd_vertical_flip", False))
    if reverse:
        scale, trans, rot = 1.0 / scale, -trans, np.linalg.inv(rot)
    a = np.eye(4)
    for op in _flow(img_meta, reverse):
        step = np.eye(4)
        if op == "T":
            step[:3, 3] = trans
        elif op == "S":
            step[:3, :3] *= scale
        elif op == "R":
            step[:3, :3] = rot.T            # rows: p @ rot
        elif op == "HF":
            step[1, 1] = -1.0 if hflip else 1.0
        elif op == "VF":
            step[0, 0] = -1.0 if vflip else 1.0
        else:
            raise AssertionError("This 3D data transformation op (%s) is not supported" % op)
        a = step @ a
    return a


def projection_matrix(img_meta):
    """The float64 3x4 matrix taking a point as the detector sees it to homogeneous pixel
    coordinates: lidar2img's first three rows times the reversed 3-D flow."""
    l2i = _meta_array(img_meta["lidar2img"])
    return l2i[:3, :4] @ flow_matrix(img_meta, reverse=True)


def sample_params(img_meta):
    """One sample's msmd_point_sample_params as 20 float64 numbers (rounded to float32 by the
    caller, once): the 3x4 matrix, scale, crop offset, flip, the flip axis, the padded shape."""
    scale = _meta_array(img_meta["scale_factor"]).reshape(-1)[:2] \
        if "scale_factor" in img_meta else np.ones(2)
    crop = _meta_array(img_meta["img_crop_offset"]).reshape(-1)[:2] \
        if "img_crop_offset" in img_meta else np.zeros(2)
    flip = 1.0 if img_meta.get("flip", False) else 0.0
    pad_h, pad_w = [float(v) for v in img_meta["input_shape"][:2]]
    img_w = float(img_meta["img_shape"][1])
    return np.concatenate([projection_matrix(img_meta).reshape(12), scale, crop,
                           [flip, img_w, pad_h, pad_w]])


def point_sample(img_meta, img_features, points, lidar2img_rt, img_scale_factor, img_crop_offset,
                 img_flip, img_pad_shape, img_shape, aligned=True, padding_mode="zeros",
                 align_corners=True):
    """point_fusion.py:10-95, op for op: img_features (1, C, H, W), points (N, 3) -> (N, C)
    (squeezed as the reference squeezes: (N,) for C == 1)."""
    points = apply_3d_transformation(points, "LIDAR", img_meta, reverse=True)
    num_points = points.shape[0]
    pts_4d = torch.cat([points, points.new_ones(size=(num_points, 1))], dim=-1)
    pts_2d = pts_4d @ lidar2img_rt.t()
    # (the reference clamps and divides in place, which autograd refuses once the points
    # require grad; the same operations out of place give the same values)
    depth = torch.clamp(pts_2d[:, 2:3], min=1e-5)
    img_coors = pts_2d[:, 0:2] / depth * img_scale_factor
    img_coors = img_coors - img_crop_offset
    coor_x, coor_y = torch.split(img_coors, 1, dim=1)
    if img_flip:
        orig_h, orig_w = img_shape
        coor_x = orig_w - coor_x
    h, w = img_pad_shape
    coor_y = coor_y / h * 2 - 1
    coor_x = coor_x / w * 2 - 1
    grid = torch.cat([coor_x, coor_y], dim=1).unsqueeze(0).unsqueeze(0)
    mode = "bilinear" if aligned else "nearest"
    point_features = F.grid_sample(img_features, grid, mode=mode, padding_mode=padding_mode,
                                   align_corners=align_corners)
    return point_features.squeeze().t()


def _channels_last(m):
    """An NCHW map as its [B, H, W, C] channels-last rows: a view where it lies that way."""
    return m.permute(0, 2, 3, 1).contiguous()


class _FusedSample(torch.autograd.Function):
    """out[N, sum C] = the bilinear samples of every level (csrc/point_sample.hip).  maps are
    [B, H, W, C] channels-last tensors; their gradients come back in the same layout."""

    @staticmethod
    def forward(ctx, points, batch, align_corners, *maps):
        out = K.point_sample_forward(points, batch, maps, align_corners)
        ctx.points, ctx.batch, ctx.align_corners = points, batch, align_corners
        ctx.shapes = [tuple(m.shape) for m in maps]     # (the index reads no feature)
        ctx.index = None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.index is None:
            ctx.index = K.point_sample_index(ctx.points, ctx.batch, ctx.shapes, ctx.align_corners)
        grads = K.point_sample_backward(grad_out.contiguous(), ctx.index, ctx.shapes)
        return (None, None, None, *grads)


@FUSION_LAYERS.register_module()
class PointFusion(nn.Module):
    """point_fusion.py:98-306 with the reference's constructor arguments, attributes, state-dict
    keys (`lateral_convs.{i}.conv.*`, `img_transform.{0,1}.*`, `pts_transform.{0,1}.*`,
    `fuse_conv.*`) and Xavier-uniform initialisation of its Conv2d / Linear layers."""

    def __init__(self, img_channels, pts_channels, mid_channels, out_channels, img_levels=3,
                 conv_cfg=None, norm_cfg=None, act_cfg=None, activate_out=True, fuse_out=False,
                 dropout_ratio=0, aligned=True, align_corners=True, padding_mode="zeros",
                 lateral_conv=True):
        super().__init__()
        if isinstance(img_levels, int):
            img_levels = [img_levels]
        if isinstance(img_channels, int):
            img_channels = [img_channels] * len(img_levels)
        assert isinstance(img_levels, list)
        assert isinstance(img_channels, list)
        assert len(img_channels) == len(img_levels)
        self.img_levels = img_levels
        self.act_cfg = act_cfg
        self.activate_out = activate_out
        self.fuse_out = fuse_out
        self.dropout_ratio = dropout_ratio
        self.img_channels = img_channels
        self.aligned = aligned
        self.align_corners = align_corners
        self.padding_mode = padding_mode
        self.lateral_convs = None
        if lateral_conv:
            self.lateral_convs = nn.ModuleList(
                ConvModule(c, mid_channels, 3, padding=1, conv_cfg=conv_cfg, norm_cfg=norm_cfg,
                           act_cfg=self.act_cfg, inplace=False) for c in img_channels)
            img_in = mid_channels * len(img_channels)
        else:
            img_in = sum(img_channels)
        self.img_transform = nn.Sequential(nn.Linear(img_in, out_channels),
                                           nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01))
        self.pts_transform = nn.Sequential(nn.Linear(pts_channels, out_channels),
                                           nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01))
        if self.fuse_out:
            self.fuse_conv = nn.Sequential(nn.Linear(mid_channels, out_channels),
                                           nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01),
                                           nn.ReLU(inplace=False))
        self.init_weights()

    def init_weights(self):
        """mmcv's xavier_init(m, distribution='uniform'): gain 1, bias 0."""
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.xavier_uniform_(m.weight, gain=1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def forward(self, img_feats, pts, pts_feats, img_metas, pts_cat=None):
        """img_feats: the levels' (B, C, H, W) maps; pts: the samples' (N_b, >= 3) clouds;
        pts_feats (sum N_b, pts_channels); pts_cat: the clouds already concatenated (the fused
        path then concatenates nothing) -> (sum N_b, out_channels)."""
        img_pts = self.obtain_mlvl_feats(img_feats, pts, img_metas, pts_cat=pts_cat)
        img_pre_fuse = self.img_transform(img_pts)
        if self.training and self.dropout_ratio > 0:
            img_pre_fuse = F.dropout(img_pre_fuse, self.dropout_ratio)
        pts_pre_fuse = self.pts_transform(pts_feats)
        fuse_out = img_pre_fuse + pts_pre_fuse
        if self.activate_out:
            fuse_out = F.relu(fuse_out)
        if self.fuse_out:
            fuse_out = self.fuse_conv(fuse_out)
        return fuse_out

    def _img_ins(self, img_feats):
        if self.lateral_convs is not None:
            return [conv(img_feats[i]) for i, conv in zip(self.img_levels, self.lateral_convs)]
        return img_feats

    def fused_ok(self, img_ins, pts, pts_cat=None):
        """Whether the HIP sampler serves this call: bilinear, zero padding, float32 maps and
        points on the GPU, points that take no gradient, at most 8 levels."""
        if not self.aligned or self.padding_mode != "zeros":
            return False
        n_levels = len(self.img_levels)
        if not 1 <= n_levels <= K.POINT_SAMPLE_MAX_LEVELS or len(img_ins) < n_levels:
            return False
        clouds = list(pts) + ([] if pts_cat is None else [pts_cat])
        for t in list(img_ins[:n_levels]) + clouds:
            if not t.is_cuda or t.dtype != torch.float32:
                return False
        return not any(p.requires_grad for p in clouds)

    def obtain_mlvl_feats(self, img_feats, pts, img_metas, pts_cat=None):
        """point_fusion.py:239-270 -> (sum N_b, sum C_l)."""
        img_ins = self._img_ins(img_feats)
        if not self.fused_ok(img_ins, pts, pts_cat):
            return self._sample_composed(img_ins, pts, img_metas)
        return self._sample_fused(img_ins, pts, img_metas, pts_cat)

    def obtain_mlvl_feats_composed(self, img_feats, pts, img_metas):
        """obtain_mlvl_feats by the reference's op sequence, whatever the inputs."""
        return self._sample_composed(self._img_ins(img_feats), pts, img_metas)

    def _sample_composed(self, img_ins, pts, img_metas):
        img_feats_per_point = []
        for i in range(len(img_metas)):
            mlvl_img_feats = []
            for level in range(len(self.img_levels)):
                feat = img_ins[level][i:i + 1]
                if pts[i].shape[0] == 0:        # (grid_sample refuses an empty grid)
                    mlvl_img_feats.append(feat.new_zeros((0, feat.shape[1])))
                    continue
                s = self.sample_single(feat, pts[i][:, :3], img_metas[i])
                # the reference's squeeze() drops a single point or channel: put it back
                mlvl_img_feats.append(s.reshape(pts[i].shape[0], feat.shape[1]))
            img_feats_per_point.append(torch.cat(mlvl_img_feats, dim=-1))
        return torch.cat(img_feats_per_point, dim=0)

    def _sample_fused(self, img_ins, pts, img_metas, pts_cat):
        if len(pts) != len(img_metas):
            raise ValueError("PointFusion: %d clouds but %d img_metas" % (len(pts), len(img_metas)))
        starts = [0]
        for p in pts:
            starts.append(starts[-1] + int(p.shape[0]))
        if pts_cat is None:
            pts_cat = pts[0] if len(pts) == 1 else torch.cat([p[:, :3] for p in pts], dim=0)
        elif pts_cat.shape[0] != starts[-1]:
            raise ValueError("PointFusion: pts_cat has %d rows, the clouds %d"
                             % (pts_cat.shape[0], starts[-1]))
        if pts_cat.stride(1) != 1:
            pts_cat = pts_cat.contiguous()
        dev = pts_cat.device
        # one pinned upload: the parameter blocks, then sample_start
        params = np.stack([sample_params(m) for m in img_metas]).astype(np.float32)
        host = np.concatenate([params.reshape(-1).view(np.int32),
                               np.asarray(starts, dtype=np.int32)])
        blob = torch.from_numpy(host).pin_memory().to(dev, non_blocking=True)
        nparam = params.size
        batch = K.PointSampleBatch(starts, blob[nparam:],
                                   blob[:nparam].view(torch.float32).view(len(img_metas), -1))
        maps = [_channels_last(m) for m in img_ins[:len(self.img_levels)]]
        with torch.autocast(device_type="cuda", enabled=False):
            return _FusedSample.apply(pts_cat.detach(), batch, bool(self.align_corners), *maps)

    def sample_single(self, img_feats, pts, img_meta):
        """point_fusion.py:272-306: one level, one sample, by the composition."""
        img_scale_factor = (pts.new_tensor(img_meta["scale_factor"][:2])
                            if "scale_factor" in img_meta.keys() else 1)
        img_flip = img_meta["flip"] if "flip" in img_meta.keys() else False
        img_crop_offset = (pts.new_tensor(img_meta["img_crop_offset"])
                           if "img_crop_offset" in img_meta.keys() else 0)
        return point_sample(img_meta, img_feats, pts, pts.new_tensor(img_meta["lidar2img"]),
                            img_scale_factor, img_crop_offset, img_flip=img_flip,
                            img_pad_shape=img_meta["input_shape"][:2],
                            img_shape=img_meta["img_shape"][:2], aligned=self.aligned,
                            padding_mode=self.padding_mode, align_corners=self.align_corners)
