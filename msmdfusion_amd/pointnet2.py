"""PointNet++ backbones: PointNet2SASSG (single-scale grouping, with feature propagation) and
PointNet2SAMSG (multi-scale grouping), with the constructor arguments, output dict keys and
index bookkeeping of mmdet3d/models/backbones/pointnet2_sa_{ssg,msg}.py and
base_pointnet.py.  auto_fp16 of the reference is plain float32 here."""
import torch
from torch import nn

from .head import ConvModule
from .pointnet_modules import PointFPModule, build_sa_module
from .registry import BACKBONES


class BasePointNet(nn.Module):
    """base_pointnet.py:7-40."""

    def __init__(self):
        super().__init__()
        self.fp16_enabled = False

    def init_weights(self, pretrained=None):
        """Conv layers keep torch's initialisation, as in the reference; a checkpoint path is
        loaded non-strictly."""
        if isinstance(pretrained, str):
            state = torch.load(pretrained, map_location="cpu")
            self.load_state_dict(state.get("state_dict", state), strict=False)

    @staticmethod
    def _split_point_feats(points):
        """(B, N, 3 + C) -> xyz (B, N, 3), features (B, C, N) or None."""
        xyz = points[..., 0:3].contiguous()
        features = points[..., 3:].transpose(1, 2).contiguous() if points.size(-1) > 3 else None
        return xyz, features


def _input_indices(xyz):
    batch, num_points = xyz.shape[:2]
    return torch.arange(num_points, device=xyz.device).unsqueeze(0).repeat(batch, 1).long()


@BACKBONES.register_module()
class PointNet2SASSG(BasePointNet):
    """pointnet2_sa_ssg.py:10-136."""

    def __init__(self, in_channels, num_points=(2048, 1024, 512, 256),
                 radius=(0.2, 0.4, 0.8, 1.2), num_samples=(64, 32, 16, 16),
                 sa_channels=((64, 64, 128), (128, 128, 256), (128, 128, 256), (128, 128, 256)),
                 fp_channels=((256, 256), (256, 256)), norm_cfg=dict(type="BN2d"),
                 sa_cfg=dict(type="PointSAModule", pool_mod="max", use_xyz=True,
                             normalize_xyz=True)):
        super().__init__()
        self.num_sa = len(sa_channels)
        self.num_fp = len(fp_channels)
        assert len(num_points) == len(radius) == len(num_samples) == len(sa_channels)
        assert len(sa_channels) >= len(fp_channels)
        self.SA_modules = nn.ModuleList()
        sa_in_channel = in_channels - 3
        skip_channel_list = [sa_in_channel]
        for sa_index in range(self.num_sa):
            cur_sa_mlps = [sa_in_channel] + list(sa_channels[sa_index])
            sa_out_channel = cur_sa_mlps[-1]
            self.SA_modules.append(build_sa_module(
                num_point=num_points[sa_index], radius=radius[sa_index],
                num_sample=num_samples[sa_index], mlp_channels=cur_sa_mlps, norm_cfg=norm_cfg,
                cfg=sa_cfg))
            skip_channel_list.append(sa_out_channel)
            sa_in_channel = sa_out_channel
        self.FP_modules = nn.ModuleList()
        fp_source_channel = skip_channel_list.pop()
        fp_target_channel = skip_channel_list.pop()
        for fp_index in range(len(fp_channels)):
            cur_fp_mlps = [fp_source_channel + fp_target_channel] + list(fp_channels[fp_index])
            self.FP_modules.append(PointFPModule(mlp_channels=cur_fp_mlps))
            if fp_index != len(fp_channels) - 1:
                fp_source_channel = cur_fp_mlps[-1]
                fp_target_channel = skip_channel_list.pop()

    def forward(self, points):
        """points (B, N, 3 + C) -> dict(fp_xyz, fp_features, fp_indices), lists over the FP
        stages; fp_indices index the input points."""
        xyz, features = self._split_point_feats(points)
        sa_xyz, sa_features, sa_indices = [xyz], [features], [_input_indices(xyz)]
        for i in range(self.num_sa):
            cur_xyz, cur_features, cur_indices = self.SA_modules[i](sa_xyz[i], sa_features[i])
            sa_xyz.append(cur_xyz)
            sa_features.append(cur_features)
            sa_indices.append(torch.gather(sa_indices[-1], 1, cur_indices.long()))
        fp_xyz, fp_features, fp_indices = [sa_xyz[-1]], [sa_features[-1]], [sa_indices[-1]]
        for i in range(self.num_fp):
            fp_features.append(self.FP_modules[i](
                sa_xyz[self.num_sa - i - 1], sa_xyz[self.num_sa - i],
                sa_features[self.num_sa - i - 1], fp_features[-1]))
            fp_xyz.append(sa_xyz[self.num_sa - i - 1])
            fp_indices.append(sa_indices[self.num_sa - i - 1])
        return dict(fp_xyz=fp_xyz, fp_features=fp_features, fp_indices=fp_indices)


@BACKBONES.register_module()
class PointNet2SAMSG(BasePointNet):
    """pointnet2_sa_msg.py:11-162."""

    def __init__(self, in_channels, num_points=(2048, 1024, 512, 256),
                 radii=((0.2, 0.4, 0.8), (0.4, 0.8, 1.6), (1.6, 3.2, 4.8)),
                 num_samples=((32, 32, 64), (32, 32, 64), (32, 32, 32)),
                 sa_channels=(((16, 16, 32), (16, 16, 32), (32, 32, 64)),
                              ((64, 64, 128), (64, 64, 128), (64, 96, 128)),
                              ((128, 128, 256), (128, 192, 256), (128, 256, 256))),
                 aggregation_channels=(64, 128, 256),
                 fps_mods=(("D-FPS"), ("FS"), ("F-FPS", "D-FPS")),
                 fps_sample_range_lists=((-1), (-1), (512, -1)),
                 dilated_group=(True, True, True), out_indices=(2, ),
                 norm_cfg=dict(type="BN2d"),
                 sa_cfg=dict(type="PointSAModuleMSG", pool_mod="max", use_xyz=True,
                             normalize_xyz=False)):
        super().__init__()
        self.num_sa = len(sa_channels)
        self.out_indices = out_indices
        assert max(out_indices) < self.num_sa
        assert len(num_points) == len(radii) == len(num_samples) == len(sa_channels) == \
            len(aggregation_channels)
        self.SA_modules = nn.ModuleList()
        self.aggregation_mlps = nn.ModuleList()
        sa_in_channel = in_channels - 3
        for sa_index in range(self.num_sa):
            cur_sa_mlps = list(sa_channels[sa_index])
            sa_out_channel = 0
            for radius_index in range(len(radii[sa_index])):
                cur_sa_mlps[radius_index] = [sa_in_channel] + list(cur_sa_mlps[radius_index])
                sa_out_channel += cur_sa_mlps[radius_index][-1]
            cur_fps_mod = list(fps_mods[sa_index]) if isinstance(fps_mods[sa_index], tuple) \
                else [fps_mods[sa_index]]
            cur_range = list(fps_sample_range_lists[sa_index]) \
                if isinstance(fps_sample_range_lists[sa_index], tuple) \
                else [fps_sample_range_lists[sa_index]]
            self.SA_modules.append(build_sa_module(
                num_point=num_points[sa_index], radii=radii[sa_index],
                sample_nums=num_samples[sa_index], mlp_channels=cur_sa_mlps,
                fps_mod=cur_fps_mod, fps_sample_range_list=cur_range,
                dilated_group=dilated_group[sa_index], norm_cfg=norm_cfg, cfg=sa_cfg, bias=True))
            self.aggregation_mlps.append(ConvModule(sa_out_channel,
                                                    aggregation_channels[sa_index], 1, bias=True,
                                                    conv="Conv1d", norm="BN1d"))
            sa_in_channel = aggregation_channels[sa_index]

    def forward(self, points):
        """points (B, N, 3 + C) -> dict(sa_xyz, sa_features, sa_indices), lists over
        out_indices; sa_indices index the input points."""
        xyz, features = self._split_point_feats(points)
        sa_xyz, sa_features, sa_indices = [xyz], [features], [_input_indices(xyz)]
        out_sa_xyz, out_sa_features, out_sa_indices = [], [], []
        for i in range(self.num_sa):
            cur_xyz, cur_features, cur_indices = self.SA_modules[i](sa_xyz[i], sa_features[i])
            cur_features = self.aggregation_mlps[i](cur_features)
            sa_xyz.append(cur_xyz)
            sa_features.append(cur_features)
            sa_indices.append(torch.gather(sa_indices[-1], 1, cur_indices.long()))
            if i in self.out_indices:
                out_sa_xyz.append(sa_xyz[-1])
                out_sa_features.append(sa_features[-1])
                out_sa_indices.append(sa_indices[-1])
        return dict(sa_xyz=out_sa_xyz, sa_features=out_sa_features, sa_indices=out_sa_indices)
