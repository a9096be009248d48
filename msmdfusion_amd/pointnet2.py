"""PointNet++ backbones: PointNet2SASSG (single-scale grouping, with feature propagation),
PointNet2SAMSG (multi-scale grouping) and H3DNet's MultiBackbone (several SSG streams and an
aggregation MLP), with the constructor arguments, output dict keys and index bookkeeping of
mmdet3d/models/backbones/{pointnet2_sa_ssg,pointnet2_sa_msg,multi_backbone}.py and
base_pointnet.py.  auto_fp16 of the reference is plain float32 here."""
import copy

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

    def forward(self, points, sa_indices=None, return_sa_indices=False):
        """points (B, N, 3 + C) -> dict(fp_xyz, fp_features, fp_indices), lists over the FP
        stages; fp_indices index the input points.  sa_indices (not in the reference): one
        (B, num_points[i]) int32 tensor per SA level, used instead of sampling there --
        MultiBackbone hands the first stream's samples to the others.  return_sa_indices adds
        the per-level samples this pass used to the dict (key `sa_level_indices`)."""
        xyz, features = self._split_point_feats(points)
        given = sa_indices
        assert given is None or len(given) == self.num_sa
        level_indices = []
        sa_xyz, sa_features, sa_indices = [xyz], [features], [_input_indices(xyz)]
        for i in range(self.num_sa):
            cur_xyz, cur_features, cur_indices = self.SA_modules[i](
                sa_xyz[i], sa_features[i], indices=None if given is None else given[i])
            level_indices.append(cur_indices)
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
        ret = dict(fp_xyz=fp_xyz, fp_features=fp_features, fp_indices=fp_indices)
        if return_sa_indices:
            ret["sa_level_indices"] = level_indices
        return ret

    def shares_sampling_with(self, other):
        """True when `other` samples what this backbone samples at every SA level: D-FPS reads
        only xyz, the levels' inputs are the previous levels' samples, so equal num_points on
        equal input points give equal indices."""
        def plan(net):
            return [(tuple(m.num_point), tuple(m.fps_mod_list), tuple(m.fps_sample_range_list))
                    for m in net.SA_modules]
        return type(other) is PointNet2SASSG and type(self) is PointNet2SASSG and \
            plan(self) == plan(other) and \
            all(mods == ("D-FPS",) and ranges == (-1,) for _, mods, ranges in plan(self))


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


@BACKBONES.register_module()
class MultiBackbone(nn.Module):
    """multi_backbone.py:10-124: `num_streams` backbones on the same points and an aggregation
    MLP over their last FP features (`hd_feature`); the streams' dict keys get the suffixes.

    share_sampling (not in the reference): all streams receive the same points and D-FPS reads
    only xyz, so streams with equal `num_points` compute the same sampling indices at every SA
    level.  Stream 0 samples; every later PointNet2SASSG stream that samples the same way takes
    its indices (`sa_indices=`) instead of running furthest-point sampling again.  The results
    are equal bit for bit; streams that do not qualify sample on their own."""

    def __init__(self, num_streams, backbones, aggregation_mlp_channels=None,
                 conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d", eps=1e-5, momentum=0.01),
                 act_cfg=dict(type="ReLU"), suffixes=("net0", "net1"), share_sampling=True,
                 **kwargs):
        super().__init__()
        assert isinstance(backbones, dict) or isinstance(backbones, list)
        if isinstance(backbones, dict):
            backbones = [copy.deepcopy(backbones) for _ in range(num_streams)]
        assert len(backbones) == num_streams
        assert len(suffixes) == num_streams
        assert conv_cfg["type"] == "Conv1d" and act_cfg["type"] == "ReLU"
        self.backbone_list = nn.ModuleList()
        self.suffixes = suffixes
        self.share_sampling = share_sampling
        out_channels = 0
        for backbone_cfg in backbones:
            out_channels += backbone_cfg["fp_channels"][-1][-1]
            self.backbone_list.append(BACKBONES.build(backbone_cfg))
        if aggregation_mlp_channels is None:
            aggregation_mlp_channels = [out_channels, out_channels // 2,
                                        out_channels // len(self.backbone_list)]
        else:
            aggregation_mlp_channels.insert(0, out_channels)    # in place, as the reference
        norm_kwargs = dict(norm_cfg)
        norm = norm_kwargs.pop("type")
        norm_kwargs.pop("requires_grad", None)
        self.aggregation_layers = nn.Sequential()
        for i in range(len(aggregation_mlp_channels) - 1):
            self.aggregation_layers.add_module(
                f"layer{i}", ConvModule(aggregation_mlp_channels[i],
                                        aggregation_mlp_channels[i + 1], 1, padding=0, bias=True,
                                        conv="Conv1d", norm=norm, norm_kwargs=norm_kwargs))

    def init_weights(self, pretrained=None):
        if isinstance(pretrained, str):
            state = torch.load(pretrained, map_location="cpu")
            self.load_state_dict(state.get("state_dict", state), strict=False)

    def forward(self, points):
        """points (B, N, 3 + C) -> the streams' dicts with suffixed keys (fp_xyz_net0, ...) and
        hd_feature (B, C_out, num_seeds)."""
        ret, fp_features, shared = {}, [], None
        first = self.backbone_list[0]
        for ind, backbone in enumerate(self.backbone_list):
            if not self.share_sampling or not isinstance(first, PointNet2SASSG) or \
                    not first.shares_sampling_with(backbone):
                cur_ret = backbone(points)
            elif ind == 0:
                cur_ret = backbone(points, return_sa_indices=True)
                shared = cur_ret.pop("sa_level_indices")
            else:
                cur_ret = backbone(points, sa_indices=shared)
            cur_suffix = self.suffixes[ind]
            fp_features.append(cur_ret["fp_features"][-1])
            if cur_suffix != "":
                cur_ret = {k + "_" + cur_suffix: v for k, v in cur_ret.items()}
            ret.update(cur_ret)
        ret["hd_feature"] = self.aggregation_layers(torch.cat(fp_features, dim=1))
        return ret
