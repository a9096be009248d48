"""The pillar path: mmdet3d/models/voxel_encoders/pillar_encoder.py (PillarFeatureNet :11-150,
DynamicPillarFeatureNet :153-308), mmdet3d/models/voxel_encoders/utils.py (PFNLayer :153-227,
get_paddings_indicator :11-31) and mmdet3d/models/middle_encoders/pillar_scatter.py
(PointPillarsScatter).

PillarFeatureNet with one PFNLayer on a plain BatchNorm1d -- every shipped PointPillars config
-- runs as three HIP passes over the raw [N, M, C] pillar table (csrc/pillar.hip): the moments
of the decorated rows, from which BatchNorm's batch statistics of `W f` follow in closed form,
the fused decoration + Linear + BN + ReLU + max / mean forward, and the backward sums.  The
[N, M, U] activations the reference materialises four times never exist.  Anything else (more
layers, another norm, an input that requires grad, CPU tensors) takes the composition path: the
reference's op sequence in torch.

Deliberate differences from the reference:
  * the reference's legacy=True forward writes x - cx, y - cy into the CALLER's tensor (its
    f_center is a view); here the input is never written, the decorated rows are the same;
  * forward returns [N, U] also for N = 1 (the reference's bare .squeeze() returns [U])."""
import torch
from torch import nn
from torch.nn import functional as F

from . import kernels as K
from .dynamic_scatter import DynamicScatter, gather_points, scatter_index, scatter_reduce
from .registry import MIDDLE_ENCODERS, VOXEL_ENCODERS, build_norm_layer
from .spconv import functional as Fsp


def get_paddings_indicator(actual_num, max_num, axis=0):
    """utils.py:11-31: [N] counts -> [N, max_num] bool, True for slots below the count."""
    actual_num = torch.unsqueeze(actual_num, axis + 1)
    shape = [1] * actual_num.dim()
    shape[axis + 1] = -1
    slots = torch.arange(max_num, dtype=torch.int, device=actual_num.device).view(shape)
    return actual_num.int() > slots


class PFNLayer(nn.Module):
    """utils.py:153-227: Linear (no bias) -> BatchNorm1d over the channel axis -> ReLU -> max /
    mean over the points of a pillar; a non-last layer returns the point features with the
    pillar's reduction repeated behind them."""

    def __init__(self, in_channels, out_channels, norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01),
                 last_layer=False, mode="max"):
        super().__init__()
        self.fp16_enabled = False
        self.name = "PFNLayer"
        self.last_vfe = last_layer
        if not self.last_vfe:
            out_channels = out_channels // 2
        self.units = out_channels
        self.norm = build_norm_layer(norm_cfg, self.units)[1]
        self.linear = nn.Linear(in_channels, self.units, bias=False)
        assert mode in ["max", "avg"]
        self.mode = mode

    def forward(self, inputs, num_voxels=None, aligned_distance=None):
        x = self.linear(inputs)
        x = self.norm(x.permute(0, 2, 1).contiguous()).permute(0, 2, 1).contiguous()
        x = F.relu(x)
        if aligned_distance is not None:
            x = x.mul(aligned_distance.unsqueeze(-1))
        if self.mode == "max":
            x_max = torch.max(x, dim=1, keepdim=True)[0]
        else:
            x_max = x.sum(dim=1, keepdim=True) / num_voxels.type_as(inputs).view(-1, 1, 1)
        if self.last_vfe:
            return x_max
        return torch.cat([x, x_max.repeat(1, inputs.shape[1], 1)], dim=2)


class _FusedPFN(torch.autograd.Function):
    """One PFNLayer on the raw pillar table.  Gradients: linear.weight, norm.weight, norm.bias
    (the pillars are data).  All of the U x K algebra is float64 torch ops on the device; there
    is no host read."""

    @staticmethod
    def forward(ctx, weight, gamma, beta, voxels, num_points, coors, geom, bn, mode):
        w = weight.detach().float().contiguous()
        wd = w.double()
        n = voxels.shape[0] * voxels.shape[1]
        batch_stats = bn.training or bn.running_mean is None
        if batch_stats:
            if n <= 1:
                raise ValueError("Expected more than 1 value per channel when training, got "
                                 "%d pillar slots" % n)
            s, g = K.pillar_moments(voxels, num_points, coors, geom)
            mu = s / n
            sigma = g / n - torch.outer(mu, mu)
            mean = wd @ mu
            var = ((wd @ sigma) * wd).sum(1).clamp_(min=0.0)
            if bn.training and bn.track_running_stats and bn.running_mean is not None:
                Fsp.count_batch(bn.num_batches_tracked)
                mom = bn.momentum
                bn.running_mean.mul_(1 - mom).add_((mean * mom).to(bn.running_mean.dtype))
                bn.running_var.mul_(1 - mom).add_(
                    (var * (n / (n - 1.0)) * mom).to(bn.running_var.dtype))
        else:
            s = g = None
            mean, var = bn.running_mean.double(), bn.running_var.double()
        invstd = torch.rsqrt(var + bn.eps)
        gd = gamma.detach().double()
        scale = gd * invstd
        shift = beta.detach().double() - mean * scale
        scale32, shift32 = scale.float(), shift.float()
        out, arg = K.pillar_pfn_forward(voxels, num_points, coors, geom, w, scale32, shift32, mode)
        ctx.save_for_backward(voxels, num_points, coors, w, scale32, shift32, arg, gd, invstd, mean,
                              s, g)
        ctx.geom, ctx.mode, ctx.rows = geom, mode, n
        ctx.dtypes = (weight.dtype, gamma.dtype, beta.dtype)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        voxels, num_points, coors, w, scale32, shift32, arg, gd, invstd, mean, s, g = \
            ctx.saved_tensors
        a, sg = K.pillar_pfn_backward(voxels, num_points, coors, ctx.geom, w, scale32, shift32,
                                      ctx.mode, grad_out.contiguous().float(), arg)
        wd, n = w.double(), float(ctx.rows)
        dbeta = sg
        dgamma = invstd * ((wd * a).sum(1) - mean * sg)
        if s is not None:         # batch statistics: the mean and the variance depend on W too
            corr = (dbeta / n)[:, None] * s[None, :] + \
                (dgamma * invstd / n)[:, None] * (wd @ g - mean[:, None] * s[None, :])
            dw = (gd * invstd)[:, None] * (a - corr)
        else:
            dw = (gd * invstd)[:, None] * a
        need = ctx.needs_input_grad
        return (dw.to(ctx.dtypes[0]) if need[0] else None,
                dgamma.to(ctx.dtypes[1]) if need[1] else None,
                dbeta.to(ctx.dtypes[2]) if need[2] else None, None, None, None, None, None, None)


@VOXEL_ENCODERS.register_module()
class PillarFeatureNet(nn.Module):
    """pillar_encoder.py:11-150, the reference's constructor, defaults and state-dict keys
    (`pfn_layers.{i}.linear.weight`, `pfn_layers.{i}.norm.*`).

    forward(features[N, M, C], num_points[N], coors[N, 4] (batch, z, y, x)) -> [N, U], always
    2-D: the reference's bare `.squeeze()` collapses N = 1 to [U], here it does not.  The input
    is cast to float32 (force_fp32) and never written; the reference's legacy=True path
    overwrites the caller's x, y with x - cx, y - cy, which the decorated rows here reproduce
    without touching the input.

    Fused (HIP) path: GPU tensors, exactly one PFN layer, a plain affine nn.BatchNorm1d,
    K <= 16 decorated channels, U <= 128, M <= 64 and an input that does not require grad.
    Under autocast it still computes in float32.  Everything else: `forward_composed`, the
    reference's op sequence in torch (CPU too), same results."""

    takes_voxel_table = True      # the detector hands (voxels, num_points, coors), not means

    def __init__(self, in_channels=4, feat_channels=(64, ), with_distance=False,
                 with_cluster_center=True, with_voxel_center=True, voxel_size=(0.2, 0.2, 4),
                 point_cloud_range=(0, -40, -3, 70.4, 40, 1),
                 norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01), mode="max", legacy=True):
        super().__init__()
        assert len(feat_channels) > 0
        self.legacy = legacy
        if with_cluster_center:
            in_channels += 3
        if with_voxel_center:
            in_channels += 2
        if with_distance:
            in_channels += 1
        self._with_distance = with_distance
        self._with_cluster_center = with_cluster_center
        self._with_voxel_center = with_voxel_center
        self.fp16_enabled = False
        self.in_channels = in_channels
        feat_channels = [in_channels] + list(feat_channels)
        pfn_layers = []
        for i in range(len(feat_channels) - 1):
            pfn_layers.append(PFNLayer(feat_channels[i], feat_channels[i + 1], norm_cfg=norm_cfg,
                                       last_layer=i >= len(feat_channels) - 2, mode=mode))
        self.pfn_layers = nn.ModuleList(pfn_layers)
        self.vx = voxel_size[0]
        self.vy = voxel_size[1]
        self.x_offset = self.vx / 2 + point_cloud_range[0]
        self.y_offset = self.vy / 2 + point_cloud_range[1]
        self.point_cloud_range = point_cloud_range
        self._geom = K.PillarGeometry(with_cluster_center, with_voxel_center, with_distance, legacy,
                                      self.vx, self.vy, self.x_offset, self.y_offset)

    def decorate(self, features, num_points, coors):
        """pillar_encoder.py:103-145 without the in-place view: -> masked [N, M, K] rows."""
        raw = features
        ls = [features]
        if self._with_cluster_center:
            points_mean = raw[:, :, :3].sum(dim=1, keepdim=True) / \
                num_points.type_as(raw).view(-1, 1, 1)
            ls.append(raw[:, :, :3] - points_mean)
        if self._with_voxel_center:
            f_center = torch.stack(
                [raw[:, :, 0] - (coors[:, 3].type_as(raw).unsqueeze(1) * self.vx + self.x_offset),
                 raw[:, :, 1] - (coors[:, 2].type_as(raw).unsqueeze(1) * self.vy + self.y_offset)],
                dim=-1)
            if self.legacy:
                # the reference's f_center is a view: its subtraction lands in channels 0, 1 of
                # the first block (and of everything read from the input afterwards)
                features = torch.cat([f_center, raw[:, :, 2:]], dim=-1)
                ls[0] = features
            ls.append(f_center)
        if self._with_distance:
            ls.append(torch.norm(features[:, :, :3], 2, 2, keepdim=True))
        out = torch.cat(ls, dim=-1)
        mask = get_paddings_indicator(num_points, out.shape[1], axis=0)
        return out * torch.unsqueeze(mask, -1).type_as(out)

    def forward_composed(self, features, num_points, coors):
        x = self.decorate(features.float(), num_points, coors)
        for pfn in self.pfn_layers:
            x = pfn(x, num_points)
        return x.squeeze(1)

    def fused_ok(self, features):
        if not features.is_cuda or features.requires_grad or len(self.pfn_layers) != 1:
            return False
        pfn = self.pfn_layers[0]
        bn = pfn.norm
        if type(bn) is not nn.BatchNorm1d or bn.weight is None or bn.bias is None or \
                bn.momentum is None:        # (cumulative averaging: left to torch)
            return False
        if features.dim() != 3 or features.shape[0] == 0:
            return False
        return K.pillar_supported(features.shape[1], features.shape[2],
                                  self._geom.decorated(features.shape[2]), pfn.units)

    def forward(self, features, num_points, coors):
        if not self.fused_ok(features):
            return self.forward_composed(features, num_points, coors)
        pfn = self.pfn_layers[0]
        with torch.autocast(device_type="cuda", enabled=False):
            return _FusedPFN.apply(pfn.linear.weight, pfn.norm.weight, pfn.norm.bias,
                                   features.float().contiguous(), num_points.int().contiguous(),
                                   coors.int().contiguous(), self._geom, pfn.norm, pfn.mode)


@VOXEL_ENCODERS.register_module()
class DynamicPillarFeatureNet(nn.Module):
    """pillar_encoder.py:153-308: the pillar encoder on dynamically voxelized points:
    (features[N, C], coors[N, 4] (batch, z, y, x)) -> (voxel_feats[M, U], voxel_coors[M, 4]).

    Same constructor, attributes and state-dict keys as the reference
    (`pfn_layers.{i}.0.weight`, `pfn_layers.{i}.1.*`), the multi-layer form with its
    `in_filters *= 2` rule included.  One ScatterIndex (computed here, or taken from `index=`
    as DynamicVFE does) is shared by the cluster scatter, every pfn scatter and every
    voxel -> point gather; the reference's map_voxel_center_to_point sizes a dense canvas from
    `pts_coors[-1, 0]`, a host read -- here there is no canvas and no read."""

    def __init__(self, in_channels=4, feat_channels=(64, ), with_distance=False,
                 with_cluster_center=True, with_voxel_center=True, voxel_size=(0.2, 0.2, 4),
                 point_cloud_range=(0, -40, -3, 70.4, 40, 1),
                 norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01), mode="max"):
        super().__init__()
        assert len(feat_channels) > 0
        assert mode in ["max", "avg"]
        if with_cluster_center:
            in_channels += 3
        if with_voxel_center:
            in_channels += 2
        if with_distance:
            in_channels += 1
        self._with_distance = with_distance
        self._with_cluster_center = with_cluster_center
        self._with_voxel_center = with_voxel_center
        self.fp16_enabled = False
        self.legacy = True
        self.in_channels = in_channels
        self.vx = voxel_size[0]
        self.vy = voxel_size[1]
        self.x_offset = self.vx / 2 + point_cloud_range[0]
        self.y_offset = self.vy / 2 + point_cloud_range[1]
        self.point_cloud_range = point_cloud_range
        feat_channels = [self.in_channels] + list(feat_channels)
        pfn_layers = []
        for i in range(len(feat_channels) - 1):
            in_filters = feat_channels[i]
            out_filters = feat_channels[i + 1]
            if i > 0:
                in_filters *= 2
            pfn_layers.append(nn.Sequential(nn.Linear(in_filters, out_filters, bias=False),
                                            build_norm_layer(norm_cfg, out_filters)[1],
                                            nn.ReLU(inplace=True)))
        self.num_pfn = len(pfn_layers)
        self.pfn_layers = nn.ModuleList(pfn_layers)
        self.pfn_scatter = DynamicScatter(voxel_size, point_cloud_range, mode != "max")
        self.cluster_scatter = DynamicScatter(voxel_size, point_cloud_range, average_points=True)

    def map_voxel_center_to_point(self, voxel_feats, index):
        """voxel_feats[M, C] -> [N, C] through the shared index (0 for invalid points)."""
        return gather_points(voxel_feats, index)

    def forward(self, features, coors, index=None):
        features = features.float()
        if index is None:
            index = scatter_index(coors.contiguous())
        features_ls = [features]
        if self._with_cluster_center:
            voxel_mean = scatter_reduce(features[:, :3].contiguous(), index,
                                        self.cluster_scatter.reduce_type)
            features_ls.append(features[:, :3] - self.map_voxel_center_to_point(voxel_mean, index))
        if self._with_voxel_center:
            f_center = features.new_zeros(size=(features.size(0), 2))
            f_center[:, 0] = features[:, 0] - (coors[:, 3].type_as(features) * self.vx +
                                               self.x_offset)
            f_center[:, 1] = features[:, 1] - (coors[:, 2].type_as(features) * self.vy +
                                               self.y_offset)
            features_ls.append(f_center)
        if self._with_distance:
            features_ls.append(torch.norm(features[:, :3], 2, 1, keepdim=True))
        features = torch.cat(features_ls, dim=-1)
        reduce = self.pfn_scatter.reduce_type
        for i, pfn in enumerate(self.pfn_layers):
            point_feats = pfn(features)
            voxel_feats = scatter_reduce(point_feats, index, reduce)
            if i != len(self.pfn_layers) - 1:
                features = torch.cat([point_feats,
                                      self.map_voxel_center_to_point(voxel_feats, index)], dim=1)
        return voxel_feats, index.voxel_coors


class _PillarScatter(torch.autograd.Function):

    @staticmethod
    def forward(ctx, feats, idx, batch_size, ny, nx):
        bev = torch.zeros((batch_size, ny, nx, feats.shape[1]), dtype=torch.float32,
                          device=feats.device)
        K.bev_scatter_nhwc(feats, idx, batch_size, [1, ny, nx], bev, 0)
        ctx.save_for_backward(idx)
        ctx.geometry = (feats.shape[1], batch_size, ny, nx)
        return bev.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad):
        (idx,) = ctx.saved_tensors
        c, batch_size, ny, nx = ctx.geometry
        g = grad.permute(0, 2, 3, 1).contiguous().float()
        return K.bev_gather_nhwc(g, idx, c, batch_size, [1, ny, nx], 0), None, None, None, None


@MIDDLE_ENCODERS.register_module()
class PointPillarsScatter(nn.Module):
    """pillar_scatter.py: pillar features -> the dense pseudo image.

    forward(voxel_features[N, C], coors[N, 4] (batch, z, y, x), batch_size) -> [B, C, ny, nx],
    a channels-last view of the NHWC buffer the BEV scatter kernel fills (what the row-form
    backbone takes as it is); batch_size=None is the reference's single-sample form:
    coors[N, 3] (z, y, x) -> a list holding one [1, C, ny, nx] map.  The z column is ignored,
    as in the reference.

    Coordinates must be unique per sample and inside the canvas -- what Voxelization produces.
    The reference's behaviour on repeated coordinates (last write wins, in an unspecified
    order) is not reproduced."""

    def __init__(self, in_channels, output_shape):
        super().__init__()
        self.output_shape = output_shape
        self.ny = output_shape[0]
        self.nx = output_shape[1]
        self.in_channels = in_channels
        self.fp16_enabled = False

    def forward(self, voxel_features, coors, batch_size=None):
        if voxel_features.dim() != 2 or voxel_features.shape[1] != self.in_channels:
            raise ValueError("PointPillarsScatter: features %s, in_channels=%d"
                             % (tuple(voxel_features.shape), self.in_channels))
        single = batch_size is None
        idx = coors.new_zeros((coors.shape[0], 4), dtype=torch.int32)
        idx[:, 2:] = coors[:, -2:]
        if not single:
            idx[:, 0] = coors[:, 0]
        bev = _PillarScatter.apply(voxel_features.float(), idx, 1 if single else int(batch_size),
                                   int(self.ny), int(self.nx))
        return [bev] if single else bev
