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

ImVoteNet's VoteFusion (vote_fusion.py, the 2-D transforms of coord_transform.py:93-214 and the
'DEPTH' flow) is the second layer here, with the same two paths: `forward_composed`, the
reference's op sequence sample by sample, and one launch of csrc/vote_fusion.hip for the whole
batch.  Its tie rule and its three deviations are in the class docstring.
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


def _flip_signs(coords_type):
    """The signs a horizontal and a vertical BEV flip multiply (x, y, z) with."""
    if coords_type == "LIDAR":
        return [1.0, -1.0, 1.0], [-1.0, 1.0, 1.0]
    if coords_type == "DEPTH":
        return [-1.0, 1.0, 1.0], [1.0, -1.0, 1.0]
    raise NotImplementedError("apply_3d_transformation: 'LIDAR' and 'DEPTH' coordinates are "
                              "built, got %r" % (coords_type,))


def apply_3d_transformation(pcd, coords_type, img_meta, reverse=False):
    """coord_transform.py:7-90 for 'LIDAR' and 'DEPTH' points: the T / S / R / HF / VF flow of
    img_meta['transformation_3d_flow'] (reversed, with inverted steps, under reverse=True) on a
    copy of pcd[:, :3].  Missing keys default as in the reference: identity rotation, scale 1,
    zero translation, no flips, an empty flow.  A horizontal flip negates y, a vertical one x
    (LiDARPoints.flip) -- for 'DEPTH' points x and y (DepthPoints.flip); a rotation is
    pcd @ rotation (BasePoints.rotate with a matrix)."""
    hf, vf = _flip_signs(coords_type)
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
                xyz = xyz * xyz.new_tensor(hf)
        elif op == "VF":
            if vflip:
                xyz = xyz * xyz.new_tensor(vf)
        else:
            raise AssertionError("This 3D data transformation op (%s) is not supported" % op)
    return xyz


def flow_matrix(img_meta, reverse=False, coords_type="LIDAR"):
    """apply_3d_transformation as one float64 4x4 matrix A (column convention: p' = A [p; 1]).
    Every step is affine, so the product is the flow exactly in real arithmetic."""
    hf, vf = _flip_signs(coords_type)
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
            if hflip:
                step[:3, :3] = np.diag(hf)
        elif op == "VF":
            if vflip:
                step[:3, :3] = np.diag(vf)
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


# ---- ImVoteNet's VoteFusion (vote_fusion.py, coord_transform.py:93-214) ----------------------
def extract_2d_info(img_meta, tensor):
    """coord_transform.py:93-118 without ori_shape (nothing reads it): img_h, img_w, the scale
    factor's first two entries, the flip flag and the crop offset, as tensors like `tensor`."""
    img_h, img_w = img_meta["img_shape"][:2]
    scale = tensor.new_tensor(_meta_array(img_meta["scale_factor"]).reshape(-1)[:2]) \
        if "scale_factor" in img_meta else tensor.new_tensor([1.0, 1.0])
    flip = img_meta["flip"] if "flip" in img_meta else False
    crop = tensor.new_tensor(_meta_array(img_meta["img_crop_offset"]).reshape(-1)[:2]) \
        if "img_crop_offset" in img_meta else tensor.new_tensor([0.0, 0.0])
    return img_h, img_w, scale, flip, crop


def bbox_2d_transform(img_meta, bbox_2d, ori2new):
    """coord_transform.py:121-172: (l, t, r, b, ...) rows between the original and the augmented
    image frame, the reference's operations in its order (scale, crop, flip; or back)."""
    _, img_w, scale, flip, crop = extract_2d_info(img_meta, bbox_2d)
    new = bbox_2d.clone()
    if ori2new:
        new[:, 0:4:2] = new[:, 0:4:2] * scale[0] + crop[0]
        new[:, 1:4:2] = new[:, 1:4:2] * scale[1] + crop[1]
    if flip:
        r, l = img_w - new[:, 0], img_w - new[:, 2]
        new[:, 0], new[:, 2] = l, r
    if not ori2new:
        new[:, 0:4:2] = (new[:, 0:4:2] - crop[0]) / scale[0]
        new[:, 1:4:2] = (new[:, 1:4:2] - crop[1]) / scale[1]
    return new


def coord_2d_transform(img_meta, coord_2d, ori2new):
    """coord_transform.py:175-214: (..., 2) pixel coordinates, likewise."""
    _, img_w, scale, flip, crop = extract_2d_info(img_meta, coord_2d)
    new = coord_2d.clone()
    if ori2new:
        new[..., 0] = new[..., 0] * scale[0] + crop[0]
        new[..., 1] = new[..., 1] * scale[1] + crop[1]
    if flip:
        new[..., 0] = img_w - new[..., 0]
    if not ori2new:
        new[..., 0] = (new[..., 0] - crop[0]) / scale[0]
        new[..., 1] = (new[..., 1] - crop[1]) / scale[1]
    return new


_DEPTH2CAM = [[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]
_CAM2DEPTH = [[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]]


def convert_point_depth_cam(point, rt_mat, to_cam):
    """Coord3DMode.convert_point (coord_3d_mode.py:181-257) between DEPTH and CAM with a 3x3
    Rt: to_cam: p @ ([[1,0,0],[0,0,-1],[0,1,0]] @ Rt^T)^T; back: p @ (Rt @ [[1,0,0],[0,0,1],
    [0,-1,0]])^T."""
    if to_cam:
        m = rt_mat.new_tensor(_DEPTH2CAM) @ rt_mat.transpose(1, 0)
    else:
        m = rt_mat @ rt_mat.new_tensor(_CAM2DEPTH)
    return point[:, :3] @ m.t()


def points_cam2img(points_3d, proj_mat):
    """core/bbox/structures/utils.py:114-144 for a 3x3 / 3x4 / 4x4 matrix -> (N, 2)."""
    d1, d2 = proj_mat.shape[:2]
    if d1 == 3:
        expanded = torch.eye(4, device=proj_mat.device, dtype=proj_mat.dtype)
        expanded[:d1, :d2] = proj_mat
        proj_mat = expanded
    points_4 = torch.cat([points_3d, points_3d.new_ones(points_3d.shape[0], 1)], dim=-1)
    point_2d = torch.matmul(points_4, proj_mat.t())
    return point_2d[..., :2] / point_2d[..., 2:3]


def vote_fusion_params(img_metas, calibs):
    """The batch's msmd_vote_fusion_params as a float32 [B, 41] tensor on the device the
    calibration lives on.  Everything the metas hold is composed on the host in float64; Rt and
    K join in float64 torch operations on their own device (a handful of batched 3x3 products
    when they are GPU tensors, and no read), and the block is rounded to float32 once.
    m_cam = ([[1,0,0],[0,0,-1],[0,1,0]] Rt^T) reversed_flow; m_vote = forward_flow (Rt
    [[1,0,0],[0,0,1],[0,-1,0]]) with the flow's translation in its fourth column."""
    b = len(img_metas)
    host = np.zeros((b, 49))
    host[:, 31:40], host[:, 40:49] = np.reshape(_DEPTH2CAM, 9), np.reshape(_CAM2DEPTH, 9)
    for i, m in enumerate(img_metas):
        host[i, :12] = flow_matrix(m, reverse=True, coords_type="DEPTH")[:3].reshape(12)
        host[i, 12:24] = flow_matrix(m, reverse=False, coords_type="DEPTH")[:3].reshape(12)
        if "scale_factor" in m:
            host[i, 24:26] = _meta_array(m["scale_factor"]).reshape(-1)[:2]
        else:
            host[i, 24:26] = 1.0
        if "img_crop_offset" in m:
            host[i, 26:28] = _meta_array(m["img_crop_offset"]).reshape(-1)[:2]
        host[i, 28] = 1.0 if m.get("flip", False) else 0.0
        host[i, 29:31] = [float(v) for v in m["img_shape"][:2]]
    rt, k = calibs["Rt"], calibs["K"]
    if not isinstance(rt, torch.Tensor):
        rt, k = torch.as_tensor(np.asarray(rt)), torch.as_tensor(np.asarray(k))
    rt, k = rt.double().reshape(b, 3, 3), k.double().reshape(b, 3, 3)
    h = torch.from_numpy(host)
    if rt.is_cuda:
        h = h.pin_memory().to(rt.device, non_blocking=True)
    rev, fwd = h[:, :12].reshape(b, 3, 4), h[:, 12:24].reshape(b, 3, 4)
    # (the two axis permutations travel with the block: a new_tensor on the GPU is a blocking copy)
    d2c, c2d = h[:, 31:40].reshape(b, 3, 3), h[:, 40:49].reshape(b, 3, 3)
    m_cam = (d2c @ rt.transpose(1, 2)) @ rev
    m_vote = torch.cat([fwd[:, :, :3] @ (rt @ c2d), fwd[:, :, 3:]], dim=2)
    return torch.cat([m_cam.reshape(b, 12), k.reshape(b, 9), m_vote.reshape(b, 12), h[:, 24:31],
                      k[:, 0, 0:1]], dim=1).float()


EPS = 1e-6


@FUSION_LAYERS.register_module()
class VoteFusion(nn.Module):
    """vote_fusion.py:11-212 with the reference's constructor: every seed is taken back through
    the 3-D augmentation, into the camera frame and onto the image; the max_imvote_per_pixel
    best 2-D boxes that hold its pixel lift image votes (5 geometric cues: xz, ray_angle), a
    semantic cue (conf at the class row) and the pixel's colour.  Returns (features
    [B, 5 + num_classes + 3, K S], mask [B, K S] bool), slot k of seed s in column k S + s.

    Two paths:
      * the composition (`forward_composed`): the reference's op sequence, sample by sample.  It
        serves CPU tensors and K above the fused path's cap (kernels.VOTE_FUSION_MAX_K), and it
        is the tests' yardstick;
      * the fused path (csrc/vote_fusion.hip): one launch for the whole batch, no
        [seed, box] tensor, no device read (box_offsets comes from the list's shapes).
    Tie rule (ours, both paths): the K pairs are in descending score, and pairs of EQUAL score go
    to the lower box index.  torch.topk leaves that order open; among out-of-box pairs it is
    invisible in the output, among in-box pairs (equal conf) it is not.
    Deviations from the reference (fused path; the third one both paths):
      * a pixel outside img_shape, or not finite, gives a zero texture cue and no read (the
        reference's gather asserts on the device, or wraps into the next row where the flat
        index stays in range);
      * a class index outside [0, num_classes) contributes no semantic cue (the reference's
        scatter faults);
      * the image is never modified (the reference's `img_flatten /= 255.` can write through a
        view into the caller's image).
    The empty-list branch writes 5 + num_classes cue rows (the reference hard-codes 15, its
    value at num_classes = 10)."""

    def __init__(self, num_classes=10, max_imvote_per_pixel=3):
        super().__init__()
        self.num_classes = num_classes
        self.max_imvote_per_pixel = max_imvote_per_pixel

    def fused_ok(self, imgs, bboxes_2d_rescaled, seeds_3d_depth):
        """Whether the HIP kernel serves this call: float32 GPU tensors, K within the cap."""
        if not 1 <= self.max_imvote_per_pixel <= K.VOTE_FUSION_MAX_K:
            return False
        if not torch.is_tensor(seeds_3d_depth) or not torch.is_tensor(imgs):
            return False
        for t in [imgs, seeds_3d_depth] + list(bboxes_2d_rescaled):
            if not t.is_cuda or t.dtype != torch.float32:
                return False
        return True

    def forward(self, imgs, bboxes_2d_rescaled, seeds_3d_depth, img_metas, calibs):
        """imgs (B, 3, Hpad, Wpad) (or a list of (3, Hpad, Wpad)); bboxes_2d_rescaled: B tensors
        (n_b, 6) = (l, t, r, b, conf, class); seeds_3d_depth (B, S, 3); calibs: dict(Rt (B, 3, 3),
        K (B, 3, 3))."""
        if not self.fused_ok(imgs, bboxes_2d_rescaled, seeds_3d_depth):
            return self.forward_composed(imgs, bboxes_2d_rescaled, seeds_3d_depth, img_metas,
                                         calibs)
        b = seeds_3d_depth.shape[0]
        if not (len(bboxes_2d_rescaled) == len(img_metas) == imgs.shape[0] == b):
            raise ValueError("VoteFusion: %d seed sets, %d box lists, %d images, %d img_metas"
                             % (b, len(bboxes_2d_rescaled), imgs.shape[0], len(img_metas)))
        dev = seeds_3d_depth.device
        offsets = [0]
        for bb in bboxes_2d_rescaled:
            offsets.append(offsets[-1] + int(bb.shape[0]))
        boxes = torch.cat([bb.reshape(-1, 6) for bb in bboxes_2d_rescaled], dim=0)
        params = vote_fusion_params(img_metas, calibs)
        if not params.is_cuda:
            params = params.pin_memory().to(dev, non_blocking=True)
        d_off = torch.tensor(offsets, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        with torch.no_grad():
            return K.vote_fusion(seeds_3d_depth.detach().contiguous(), boxes.detach(), d_off,
                                 offsets, imgs.detach().contiguous(), params.to(dev),
                                 self.num_classes, self.max_imvote_per_pixel)

    def forward_composed(self, imgs, bboxes_2d_rescaled, seeds_3d_depth, img_metas, calibs):
        """vote_fusion.py:40-212 by the reference's op sequence, whatever the inputs."""
        img_features, masks = [], []
        k = self.max_imvote_per_pixel
        for i, (img, bbox_2d_rescaled, seed_3d_depth, img_meta) in enumerate(
                zip(imgs, bboxes_2d_rescaled, seeds_3d_depth, img_metas)):
            bbox_num, seed_num = bbox_2d_rescaled.shape[0], seed_3d_depth.shape[0]
            img_shape = img_meta["img_shape"]
            rt = torch.as_tensor(calibs["Rt"][i]).to(seed_3d_depth)
            kmat = torch.as_tensor(calibs["K"][i]).to(seed_3d_depth)
            xyz_depth = apply_3d_transformation(seed_3d_depth, "DEPTH", img_meta, reverse=True)
            xyz_cam = convert_point_depth_cam(xyz_depth, rt, to_cam=True)
            uv_origin = (points_cam2img(xyz_cam, kmat) - 1).round()
            uv_rescaled = coord_2d_transform(img_meta, uv_origin, True)
            bbox_2d_origin = bbox_2d_transform(img_meta, bbox_2d_rescaled, False)
            if bbox_num == 0:
                two_cues = seed_3d_depth.new_zeros((5 + self.num_classes, seed_num * k))
                mask = torch.cat([seed_3d_depth.new_ones(seed_num, dtype=torch.bool),
                                  seed_3d_depth.new_zeros(seed_num * (k - 1), dtype=torch.bool)])
            else:
                bbox_expanded = bbox_2d_origin.view(1, bbox_num, -1).expand(seed_num, -1, -1)
                seed_2d_expanded = uv_origin.view(seed_num, 1, -1).expand(-1, bbox_num, -1)
                sx, sy = seed_2d_expanded.split(1, dim=-1)
                bl, bt, br, bb, bconf, bcls = bbox_expanded.split(1, dim=-1)
                midx, midy = (bl + br) / 2, (bt + bb) / 2
                in_bbox = ((sx > bl) * (sx < br)) * ((sy > bt) * (sy < bb))
                sem_cue = torch.zeros_like(bconf).expand(-1, -1, self.num_classes)
                sem_cue = sem_cue.scatter(-1, bcls.long(), bconf)
                delta_u, delta_v = midx - sx, midy - sy
                seed_3d_expanded = seed_3d_depth.view(seed_num, 1, -1).expand(-1, bbox_num, -1)
                z_cam = xyz_cam[..., 2:3].view(seed_num, 1, 1).expand(-1, bbox_num, -1)
                delta_u = delta_u * z_cam / kmat[0, 0]
                delta_v = delta_v * z_cam / kmat[0, 0]
                imvote = torch.cat([delta_u, delta_v, torch.zeros_like(delta_v)],
                                   dim=-1).view(-1, 3)
                imvote = convert_point_depth_cam(imvote, rt, to_cam=False)
                imvote = apply_3d_transformation(imvote, "DEPTH", img_meta, reverse=False)
                seed_3d_expanded = seed_3d_expanded.reshape(imvote.shape)
                ray_angle = seed_3d_expanded + imvote
                ray_angle = ray_angle / torch.sqrt(torch.sum(ray_angle ** 2, -1) +
                                                   EPS).unsqueeze(-1)
                xz = ray_angle[:, [0, 2]] / (ray_angle[:, [1]] + EPS) \
                    * seed_3d_expanded[:, [1]] - seed_3d_expanded[:, [0, 2]]
                geo_cue = torch.cat([xz, ray_angle], dim=-1).view(seed_num, -1, 5)
                two_cues = torch.cat([geo_cue, sem_cue], dim=-1)
                two_cues = two_cues * in_bbox.float()
                feature_size = two_cues.shape[-1]
                if bbox_num < k:
                    pad = k - bbox_num
                    in_bbox = torch.cat([in_bbox, in_bbox.new_zeros((seed_num, pad, 1))], dim=1)
                    two_cues = torch.cat([two_cues,
                                          two_cues.new_zeros((seed_num, pad, feature_size))], dim=1)
                    bconf = torch.cat([bconf, two_cues.new_zeros((seed_num, pad, 1))], dim=1)
                pair_score = in_bbox.float() + bconf
                # topk(largest, sorted) with the tie rule of the docstring: a stable sort
                mask, indices = torch.sort(pair_score, dim=1, descending=True, stable=True)
                mask, indices = mask[:, :k], indices[:, :k]
                two_cues = two_cues.gather(dim=1, index=indices.expand(-1, -1, feature_size))
                two_cues = two_cues.transpose(1, 0).reshape(-1, feature_size).transpose(
                    1, 0).contiguous()
                mask = mask.floor().int().transpose(1, 0).reshape(-1).bool()
            img = img[:, :img_shape[0], :img_shape[1]]
            # out of place, and by a tensor: torch's GPU division by a Python scalar multiplies
            # by the reciprocal, which is not the true division the CPU (and the kernel) does
            img_flatten = img.reshape(3, -1).float()
            img_flatten = img_flatten / img_flatten.new_tensor(255.)
            uv_flatten = uv_rescaled[:, 1].round() * img_shape[1] + uv_rescaled[:, 0].round()
            uv_expanded = uv_flatten.unsqueeze(0).expand(3, -1).long()
            txt_cue = torch.gather(img_flatten, dim=-1, index=uv_expanded)
            txt_cue = txt_cue.unsqueeze(1).expand(-1, k, -1).reshape(3, -1)
            img_features.append(torch.cat([two_cues, txt_cue], dim=0))
            masks.append(mask)
        return torch.stack(img_features, 0), torch.stack(masks, 0)
