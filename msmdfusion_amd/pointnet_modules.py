"""PointNet++ set-abstraction and feature-propagation modules with the reference's
constructor signatures and state-dict keys (mmdet3d/ops/pointnet_modules/
{point_sa_module,point_fp_module,builder,registry}.py): `mlps.0.layer0.conv.weight`,
`mlps.0.layer0.bn.weight`, ...  Sampling, grouping and interpolation are the library's
kernels (pointnet_ops); the shared MLPs are 1x1 Conv2d + BatchNorm2d + ReLU."""
import torch
from torch import nn
from torch.nn import functional as F

from .head import ConvModule
from .pointnet_ops import (GroupAll, Points_Sampler, QueryAndGroup, gather_points,
                           three_interpolate, three_nn)
from .registry import Registry

SA_MODULES = Registry("point_sa_module")


class PointwiseConv2d(nn.Conv2d):
    """nn.Conv2d (same parameters, same state-dict keys); the 1x1 convolutions of the shared
    MLPs run as the matrix product they are, as head.Conv1d does: the grouped tensors are
    (B, C, npoint, nsample) or (B, C, n, 1) with a handful of channels, shapes MIOpen serves
    through kernels picked for images."""

    def forward(self, x):
        if self.kernel_size != (1, 1) or self.stride != (1, 1) or self.groups != 1 or \
                self.padding != (0, 0) or x.dim() != 4:
            return super().forward(x)
        y = torch.matmul(self.weight[:, :, 0, 0], x.flatten(2))
        if self.bias is not None:
            y = y + self.bias[:, None]
        return y.view(x.shape[0], self.out_channels, x.shape[2], x.shape[3])


def conv_module(in_channels, out_channels, conv_cfg, norm_cfg, bias="auto"):
    """mmcv's ConvModule(kernel_size 1, stride 1, conv_cfg, norm_cfg, bias) on head.ConvModule:
    the norm_cfg's `type` picks the layer, its other entries (eps, momentum) reach it."""
    norm, norm_kwargs = None, None
    if norm_cfg is not None:
        norm_kwargs = dict(norm_cfg)
        norm = norm_kwargs.pop("type")
        norm_kwargs.pop("requires_grad", None)
    return ConvModule(in_channels, out_channels, 1, stride=1, bias=bias,
                      conv=PointwiseConv2d if conv_cfg["type"] == "Conv2d" else conv_cfg["type"],
                      norm=norm, norm_kwargs=norm_kwargs)


@SA_MODULES.register_module()
class PointSAModuleMSG(nn.Module):
    """Set abstraction with multi-scale grouping (point_sa_module.py:11-179)."""

    def __init__(self, num_point, radii, sample_nums, mlp_channels, fps_mod=["D-FPS"],
                 fps_sample_range_list=[-1], dilated_group=False, norm_cfg=dict(type="BN2d"),
                 use_xyz=True, pool_mod="max", normalize_xyz=False, bias="auto"):
        super().__init__()
        assert len(radii) == len(sample_nums) == len(mlp_channels)
        assert pool_mod in ["max", "avg"]
        assert isinstance(fps_mod, (list, tuple))
        assert isinstance(fps_sample_range_list, (list, tuple))
        assert len(fps_mod) == len(fps_sample_range_list)
        if isinstance(mlp_channels, tuple):
            mlp_channels = list(map(list, mlp_channels))
        if isinstance(num_point, int):
            self.num_point = [num_point]
        elif isinstance(num_point, (list, tuple)):
            self.num_point = num_point
        else:
            raise NotImplementedError("Error type of num_point!")
        self.pool_mod = pool_mod
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        self.fps_mod_list = fps_mod
        self.fps_sample_range_list = fps_sample_range_list
        self.points_sampler = Points_Sampler(self.num_point, self.fps_mod_list,
                                             self.fps_sample_range_list)
        for i in range(len(radii)):
            if num_point is not None:
                min_radius = radii[i - 1] if dilated_group and i != 0 else 0
                grouper = QueryAndGroup(radii[i], sample_nums[i], min_radius=min_radius,
                                        use_xyz=use_xyz, normalize_xyz=normalize_xyz)
            else:
                grouper = GroupAll(use_xyz)
            self.groupers.append(grouper)
            mlp_spec = mlp_channels[i]
            if use_xyz:
                mlp_spec[0] += 3        # in place, as the reference: the caller's list grows
            mlp = nn.Sequential()
            for j in range(len(mlp_spec) - 1):
                mlp.add_module(f"layer{j}", conv_module(mlp_spec[j], mlp_spec[j + 1],
                                                        dict(type="Conv2d"), norm_cfg, bias))
            self.mlps.append(mlp)

    def forward(self, points_xyz, features=None, indices=None, target_xyz=None):
        """points_xyz (B, N, 3), features (B, C, N) -> new_xyz (B, M, 3), new features
        (B, sum_k mlps[k][-1], M), indices (B, M)."""
        new_features_list = []
        xyz_flipped = points_xyz.transpose(1, 2).contiguous()
        if indices is not None:
            assert indices.shape[1] == self.num_point[0]
            new_xyz = gather_points(xyz_flipped, indices).transpose(1, 2).contiguous() \
                if self.num_point is not None else None
        elif target_xyz is not None:
            new_xyz = target_xyz.contiguous()
        else:
            indices = self.points_sampler(points_xyz, features)
            new_xyz = gather_points(xyz_flipped, indices).transpose(1, 2).contiguous() \
                if self.num_point is not None else None
        for grouper, mlp in zip(self.groupers, self.mlps):
            new_features = mlp(grouper(points_xyz, new_xyz, features))
            if self.pool_mod == "max":
                new_features = F.max_pool2d(new_features, kernel_size=[1, new_features.size(3)])
            else:
                new_features = F.avg_pool2d(new_features, kernel_size=[1, new_features.size(3)])
            new_features_list.append(new_features.squeeze(-1))
        return new_xyz, torch.cat(new_features_list, dim=1), indices


@SA_MODULES.register_module()
class PointSAModule(PointSAModuleMSG):
    """Set abstraction with one scale (point_sa_module.py:182-230)."""

    def __init__(self, mlp_channels, num_point=None, radius=None, num_sample=None,
                 norm_cfg=dict(type="BN2d"), use_xyz=True, pool_mod="max", fps_mod=["D-FPS"],
                 fps_sample_range_list=[-1], normalize_xyz=False):
        super().__init__(mlp_channels=[mlp_channels], num_point=num_point, radii=[radius],
                         sample_nums=[num_sample], norm_cfg=norm_cfg, use_xyz=use_xyz,
                         pool_mod=pool_mod, fps_mod=fps_mod,
                         fps_sample_range_list=fps_sample_range_list,
                         normalize_xyz=normalize_xyz)


def build_sa_module(cfg, *args, **kwargs):
    """pointnet_modules/builder.py:4-36: cfg None means PointSAModule."""
    if cfg is None:
        cfg_ = dict(type="PointSAModule")
    else:
        if not isinstance(cfg, dict):
            raise TypeError("cfg must be a dict")
        if "type" not in cfg:
            raise KeyError('the cfg dict must contain the key "type"')
        cfg_ = cfg.copy()
    module_type = cfg_.pop("type")
    if module_type not in SA_MODULES:
        raise KeyError(f"Unrecognized module type {module_type}")
    return SA_MODULES.get(module_type)(*args, **kwargs, **cfg_)


class PointFPModule(nn.Module):
    """Feature propagation (point_fp_module.py:10-77): inverse-distance interpolation of the
    source features at the target points over their three nearest sources, stacked on the
    target's own features, then the shared MLP."""

    def __init__(self, mlp_channels, norm_cfg=dict(type="BN2d")):
        super().__init__()
        self.fp16_enabled = False
        self.mlps = nn.Sequential()
        for i in range(len(mlp_channels) - 1):
            self.mlps.add_module(f"layer{i}", conv_module(mlp_channels[i], mlp_channels[i + 1],
                                                          dict(type="Conv2d"), norm_cfg))

    def forward(self, target, source, target_feats, source_feats):
        """target (B, n, 3), source (B, m, 3), target_feats (B, C1, n), source_feats
        (B, C2, m) -> (B, mlp[-1], n)."""
        if source is not None:
            dist, idx = three_nn(target.contiguous(), source.contiguous())
            dist_reciprocal = 1.0 / (dist + 1e-8)
            norm = torch.sum(dist_reciprocal, dim=2, keepdim=True)
            weight = dist_reciprocal / norm
            interpolated_feats = three_interpolate(source_feats.contiguous(), idx, weight)
        else:
            interpolated_feats = source_feats.expand(*source_feats.size()[0:2], target.size(1))
        if target_feats is not None:
            new_features = torch.cat([interpolated_feats, target_feats], dim=1)
        else:
            new_features = interpolated_feats
        return self.mlps(new_features.unsqueeze(-1)).squeeze(-1)
