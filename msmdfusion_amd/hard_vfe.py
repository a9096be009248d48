"""HardVFE: mmdet3d/models/voxel_encoders/voxel_encoder.py (HardVFE) on
mmdet3d/models/voxel_encoders/utils.py:34-106 (VFELayer), the voxel encoder of the nuScenes
PointPillars-FPN model (configs/_base_/models/hv_pointpillars_fpn_nus.py) and of every
free_anchor config.

With one or two VFELayers on plain affine BatchNorm1d norms -- the config runs two, 64 wide, on
a [N, 64, 4] table -- the encoder runs as HIP passes over the raw [N, M, C] table
(csrc/hard_vfe.hip): the moments of the decorated rows (layer 1's batch statistics in closed
form), a statistics pass for layer 2's (no closed form: a ReLU and a max lie in between), the
output pass, and ONE dense backward pass.  No [N, M, U] activation is ever written; a voxel's
padded slots are one row, computed once and weighted.  Anything else (more
layers, another norm, an input that requires grad, CPU tensors, wider layers) takes
`forward_composed`: the reference's op sequence in torch.

Deliberate differences from the reference:
  * with_distance=True: the reference's constructor adds 3 input channels and its forward
    appends 1, so its own Linear fails on the shape; the constructor arithmetic is kept (it
    decides the state-dict shapes) and forward raises a ValueError that names the mismatch;
  * fusion_layer (PointFusion) is not built: NotImplementedError."""
import torch
from torch import nn
from torch.nn import functional as F

from . import kernels as K
from .dynamic_scatter import DynamicScatter
from .pillar_encoder import get_paddings_indicator
from .registry import VOXEL_ENCODERS, _NaiveSyncMixin, build_norm_layer
from .spconv import functional as Fsp


class VFELayer(nn.Module):
    """utils.py:34-106: Linear (no bias) -> BatchNorm1d over the channel axis -> ReLU; max_out:
    the max over the points of a voxel, returned alone [N, U] or (cat_max) repeated behind the
    point features [N, M, 2U]; max_out=False returns the point features."""

    def __init__(self, in_channels, out_channels, norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01),
                 max_out=True, cat_max=True):
        super().__init__()
        self.fp16_enabled = False
        self.cat_max = cat_max
        self.max_out = max_out
        self.norm = build_norm_layer(norm_cfg, out_channels)[1]
        self.linear = nn.Linear(in_channels, out_channels, bias=False)

    def forward(self, inputs):
        voxel_count = inputs.shape[1]
        x = self.linear(inputs)
        x = self.norm(x.permute(0, 2, 1).contiguous()).permute(0, 2, 1).contiguous()
        pointwise = F.relu(x)
        if not self.max_out:
            return pointwise
        aggregated = torch.max(pointwise, dim=1, keepdim=True)[0]
        if not self.cat_max:
            return aggregated.squeeze(1)
        return torch.cat([pointwise, aggregated.repeat(1, voxel_count, 1)], dim=2)


def _bn_coefficients(bn, gamma, beta, mean, var, n):
    """The batch (or running) statistics of one BatchNorm1d -> (scale, shift, invstd) float64,
    with nn.BatchNorm1d's running-statistics update when `n` rows of batch statistics are
    given (n=None: mean, var are the running ones)."""
    if n is not None and bn.training and bn.track_running_stats and bn.running_mean is not None:
        Fsp.count_batch(bn.num_batches_tracked)
        mom = bn.momentum
        bn.running_mean.mul_(1 - mom).add_((mean * mom).to(bn.running_mean.dtype))
        bn.running_var.mul_(1 - mom).add_((var * (n / (n - 1.0)) * mom).to(bn.running_var.dtype))
    invstd = torch.rsqrt(var + bn.eps)
    scale = gamma.detach().double() * invstd
    return scale, beta.detach().double() - mean * scale, invstd


def _batch_stats(bn):
    return bn.training or bn.running_mean is None


class _FusedVFE(torch.autograd.Function):
    """One or two VFELayers on the raw voxel table.  Gradients: the layers' linear.weight,
    norm.weight and norm.bias (the voxels are data).  The U x K and U x 2U algebra is float64
    torch ops on the device; there is no host read."""

    @staticmethod
    def forward(ctx, voxels, num_points, coors, geom, norms, *params):
        two = len(norms) == 2
        w1 = params[0].detach().float().contiguous()
        n = voxels.shape[0] * voxels.shape[1]
        if any(_batch_stats(bn) for bn in norms) and n <= 1:
            raise ValueError("Expected more than 1 value per channel when training, got "
                             "%d voxel slots" % n)
        bn1 = norms[0]
        wd = w1.double()
        if _batch_stats(bn1):
            s, g = K.hard_vfe_moments(voxels, num_points, coors, geom)
            mu = s / n
            mean1 = wd @ mu
            var1 = ((wd @ (g / n - torch.outer(mu, mu))) * wd).sum(1).clamp_(min=0.0)
            scale1, shift1, invstd1 = _bn_coefficients(bn1, params[1], params[2], mean1, var1, n)
        else:
            s = g = None
            mean1 = bn1.running_mean.double()
            scale1, shift1, invstd1 = _bn_coefficients(bn1, params[1], params[2], mean1,
                                                       bn1.running_var.double(), None)
        layers = [(w1, scale1.float(), shift1.float())]
        mean2 = invstd2 = None
        if two:
            bn2 = norms[1]
            w2 = params[3].detach().float().contiguous()
            if _batch_stats(bn2):
                pivot, sy, sq = K.hard_vfe_stats(voxels, num_points, coors, geom, *layers[0], w2)
                mean2 = sy / n
                # about the pivot: var = E (y - p)^2 - (mean - p)^2 does not cancel
                var2 = (sq / n - (mean2 - pivot.double()) ** 2).clamp_(min=0.0)
                scale2, shift2, invstd2 = _bn_coefficients(bn2, params[4], params[5], mean2,
                                                           var2, n)
            else:
                mean2 = bn2.running_mean.double()
                scale2, shift2, invstd2 = _bn_coefficients(bn2, params[4], params[5], mean2,
                                                           bn2.running_var.double(), None)
            layers.append((w2, scale2.float(), shift2.float()))
        out, arg, ymax = K.hard_vfe_forward(voxels, num_points, coors, geom, layers)
        ctx.save_for_backward(voxels, num_points, coors, out, arg, ymax, s, g, mean1, invstd1,
                              mean2, invstd2, *[t for layer in layers for t in layer],
                              *[p.detach() for p in params[1::3]])
        ctx.geom, ctx.rows, ctx.two = geom, n, two
        ctx.batch2 = two and _batch_stats(norms[1])
        ctx.dtypes = [p.dtype for p in params]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        voxels, num_points, coors, out, arg, ymax, s, g, mean1, invstd1, mean2, invstd2 = \
            ctx.saved_tensors[:12]
        rest = ctx.saved_tensors[12:]
        nl = 2 if ctx.two else 1
        layers = [tuple(rest[3 * i:3 * i + 3]) for i in range(nl)]
        gammas = rest[3 * nl:]
        n = float(ctx.rows)
        g2 = (grad_out.float() * (out > 0)).contiguous()
        grads = []
        if ctx.two:
            gd = g2.double()
            a2 = gd.sum(0)
            b2 = (gd * ((ymax.double() - mean2) * invstd2)).sum(0)
            scale2 = layers[1][1].double()
            if ctx.batch2:       # dy2 = scale2 (g2 - A2 / n - u2hat B2 / n) = scale2 g2 - dp - dq y2
                dq = scale2 * invstd2 * b2 / n
                dp = scale2 * a2 / n - mean2 * dq
            else:
                dp = dq = torch.zeros_like(a2)
            dw2, a1, sg1 = K.hard_vfe_backward(voxels, num_points, coors, ctx.geom, layers, g2,
                                               arg, dp.float(), dq.float())
            grads = [dw2, b2, a2]
        else:
            _, a1, sg1 = K.hard_vfe_backward(voxels, num_points, coors, ctx.geom, layers, g2, arg)
        # layer 1: section 16.2's closed forms on A1 = sum g1 f and sum g1
        wd = layers[0][0].double()
        gam1 = gammas[0].double()
        dbeta1 = sg1
        dgamma1 = invstd1 * ((wd * a1).sum(1) - mean1 * sg1)
        if s is not None:        # batch statistics: the mean and the variance depend on W1 too
            corr = (dbeta1 / n)[:, None] * s[None, :] + \
                (dgamma1 * invstd1 / n)[:, None] * (wd @ g - mean1[:, None] * s[None, :])
            dw1 = (gam1 * invstd1)[:, None] * (a1 - corr)
        else:
            dw1 = (gam1 * invstd1)[:, None] * a1
        grads = [dw1, dgamma1, dbeta1] + grads
        need = ctx.needs_input_grad[5:]
        return (None, None, None, None, None,
                *[gr.to(dt) if nd else None for gr, dt, nd in zip(grads, ctx.dtypes, need)])


@VOXEL_ENCODERS.register_module()
class HardVFE(nn.Module):
    """voxel_encoder.py (HardVFE): the reference's constructor, defaults, attributes and
    state-dict keys (`vfe_layers.{i}.linear.weight`, `vfe_layers.{i}.norm.*`); layers after the
    first take `2 * feat_channels[i]` inputs, every layer but the last concatenates its max.

    forward(features[N, M, C], num_points[N], coors[N, 4] (batch, z, y, x)) -> [N, U_last]
    float32.  The input is never written.  Decorated row: raw channels, xyz minus (sum over
    ALL M slots) / num_points, xyz minus the voxel centre (three channels), the whole row times
    [slot < num_points].  num_points >= 1 is a precondition; num_points > M is an all-ones mask.

    Fused (HIP) path: GPU tensors, one or two layers, affine nn.BatchNorm1d norms with a
    momentum (the naiveSync subclass where it takes its plain branch), K <= 16 decorated
    channels, widths <= 64, M <= 64 and an input that does not require grad.  Under autocast it
    still computes in float32.  Everything else: `forward_composed` (CPU too, any depth)."""

    takes_voxel_table = True      # the detector hands (voxels, num_points, coors), not means

    def __init__(self, in_channels=4, feat_channels=[], with_distance=False,
                 with_cluster_center=False, with_voxel_center=False, voxel_size=(0.2, 0.2, 4),
                 point_cloud_range=(0, -40, -3, 70.4, 40, 1),
                 norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01), mode="max",
                 fusion_layer=None, return_point_feats=False):
        super().__init__()
        assert len(feat_channels) > 0
        if fusion_layer is not None:
            raise NotImplementedError("HardVFE: fusion_layer (PointFusion) is not built")
        if with_cluster_center:
            in_channels += 3
        if with_voxel_center:
            in_channels += 3
        if with_distance:
            in_channels += 3          # (sic: forward appends ONE channel, see forward)
        self.in_channels = in_channels
        self._with_distance = with_distance
        self._with_cluster_center = with_cluster_center
        self._with_voxel_center = with_voxel_center
        self.return_point_feats = return_point_feats
        self.fp16_enabled = False
        self.mode = mode
        self.vx, self.vy, self.vz = voxel_size[0], voxel_size[1], voxel_size[2]
        self.x_offset = self.vx / 2 + point_cloud_range[0]
        self.y_offset = self.vy / 2 + point_cloud_range[1]
        self.z_offset = self.vz / 2 + point_cloud_range[2]
        self.point_cloud_range = point_cloud_range
        self.scatter = DynamicScatter(voxel_size, point_cloud_range, True)
        feat_channels = [self.in_channels] + list(feat_channels)
        vfe_layers = []
        for i in range(len(feat_channels) - 1):
            in_filters = feat_channels[i]
            if i > 0:
                in_filters *= 2
            last = i == len(feat_channels) - 2
            vfe_layers.append(VFELayer(in_filters, feat_channels[i + 1], norm_cfg=norm_cfg,
                                       max_out=True, cat_max=not last))
        self.vfe_layers = nn.ModuleList(vfe_layers)
        self.num_vfe = len(vfe_layers)
        self.fusion_layer = None
        self._geom = K.HardVFEGeometry(with_cluster_center, with_voxel_center, self.vx, self.vy,
                                       self.vz, self.x_offset, self.y_offset, self.z_offset)

    def decorate(self, features, num_points, coors):
        """voxel_encoder.py (HardVFE.forward, up to the mask) -> masked [N, M, K] rows."""
        ls = [features]
        if self._with_cluster_center:
            points_mean = features[:, :, :3].sum(dim=1, keepdim=True) / \
                num_points.type_as(features).view(-1, 1, 1)
            ls.append(features[:, :, :3] - points_mean)
        if self._with_voxel_center:
            centre = [coors[:, 3].type_as(features).unsqueeze(1) * self.vx + self.x_offset,
                      coors[:, 2].type_as(features).unsqueeze(1) * self.vy + self.y_offset,
                      coors[:, 1].type_as(features).unsqueeze(1) * self.vz + self.z_offset]
            ls.append(torch.stack([features[:, :, i] - centre[i] for i in range(3)], dim=-1))
        out = torch.cat(ls, dim=-1)
        mask = get_paddings_indicator(num_points, out.shape[1], axis=0)
        return out * mask.unsqueeze(-1).type_as(out)

    def _refuse_distance(self, features):
        if self._with_distance:
            have = features.shape[-1] + 3 * bool(self._with_cluster_center) + \
                3 * bool(self._with_voxel_center) + 1
            raise ValueError(
                "HardVFE(with_distance=True): the constructor counts 3 channels for the distance "
                "but forward appends 1, so the decorated row has %d channels where "
                "vfe_layers.0.linear expects %d (the reference fails on the same shape)"
                % (have, self.in_channels))

    def forward_composed(self, features, num_points, coors, img_feats=None, img_metas=None):
        self._refuse_distance(features)
        x = self.decorate(features.float(), num_points, coors)
        for vfe in self.vfe_layers:
            x = vfe(x)
        return x

    def fused_ok(self, features):
        if not features.is_cuda or features.requires_grad or features.dim() != 3 or \
                features.shape[0] == 0:
            return False
        for vfe in self.vfe_layers:
            bn = vfe.norm
            if isinstance(bn, _NaiveSyncMixin):
                if not isinstance(bn, nn.BatchNorm1d) or not bn.plain_branch():
                    return False
            elif type(bn) is not nn.BatchNorm1d:
                return False
            if bn.weight is None or bn.bias is None or bn.momentum is None:
                return False             # (cumulative averaging: left to torch)
        return K.hard_vfe_supported(features.shape[1], features.shape[2],
                                    self._geom.decorated(features.shape[2]),
                                    [vfe.linear.out_features for vfe in self.vfe_layers])

    def forward(self, features, num_points, coors, img_feats=None, img_metas=None):
        self._refuse_distance(features)
        if not self.fused_ok(features):
            return self.forward_composed(features, num_points, coors)
        params = [p for vfe in self.vfe_layers
                  for p in (vfe.linear.weight, vfe.norm.weight, vfe.norm.bias)]
        with torch.autocast(device_type="cuda", enabled=False):
            return _FusedVFE.apply(features.float().contiguous(), num_points.int().contiguous(),
                                   coors.int().contiguous(), self._geom,
                                   [vfe.norm for vfe in self.vfe_layers], *params)
