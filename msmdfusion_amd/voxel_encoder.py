"""Voxel encoders: mmdet3d/models/voxel_encoders/voxel_encoder.py -- HardSimpleVFE (:14-46),
DynamicSimpleVFE (:49-89) and DynamicVFE (:92-286)."""
import torch
from torch import nn

from . import kernels as K
from .dynamic_scatter import DynamicScatter, gather_points, scatter_index, scatter_reduce
from .registry import VOXEL_ENCODERS


@VOXEL_ENCODERS.register_module()
class HardSimpleVFE(nn.Module):
    """Mean of the points of each voxel (sum over the slots / num_points)."""

    def __init__(self, num_features=4):
        super().__init__()
        self.num_features = num_features
        self.fp16_enabled = False

    def forward(self, features, num_points, coors):
        return K.voxel_mean(features, num_points, self.num_features)


@VOXEL_ENCODERS.register_module()
class DynamicSimpleVFE(nn.Module):
    """Mean of the points of each voxel under dynamic voxelization: (features[N, C],
    coors[N, 3 | 4]) -> (voxel means[M, C], voxel coors[M, 3 | 4]).  `index`: a ScatterIndex of
    `coors` computed before (TransFusionDetector.prepare does)."""

    def __init__(self, voxel_size=(0.2, 0.2, 4), point_cloud_range=(0, -40, -3, 70.4, 40, 1)):
        super().__init__()
        self.scatter = DynamicScatter(voxel_size, point_cloud_range, True)
        self.fp16_enabled = False

    @torch.no_grad()
    def forward(self, features, coors, index=None):
        return self.scatter(features.float(), coors, index=index)


def _norm_layer(norm_cfg, channels):
    cfg = dict(norm_cfg)
    kind = cfg.pop("type", "BN1d")
    if kind not in ("BN1d", "BN"):
        raise NotImplementedError("DynamicVFE: norm type %r is not built (BN1d only)" % kind)
    cfg.pop("requires_grad", None)
    return nn.BatchNorm1d(channels, **cfg)


@VOXEL_ENCODERS.register_module()
class DynamicVFE(nn.Module):
    """Dynamic voxel feature encoder (DV-SECOND): point decorations (cluster centre, voxel
    centre), then per layer Linear -> BN1d -> ReLU on the points, a max / mean scatter to the
    voxels and -- between layers -- the voxel result concatenated back onto its points.

    Same constructor arguments, attributes and state-dict keys as the reference
    (`vfe_layers.{i}.0.weight`, `vfe_layers.{i}.1.*`).  The index half of the scatters is
    computed once per forward (or taken from `index=`) and shared by the cluster scatter,
    every vfe scatter and every voxel -> point gather; no dense canvas is built.

    Semantic edge: with out-of-range points (a negative coordinate) present, the reference's
    map_voxel_center_to_point indexes its canvas with a negative id and reads a wrapped
    element; here such points get 0.  Voxel features are the same either way (invalid points
    never reach a voxel), but in training mode the BN1d batch statistics of the later layers
    include those rows, so parity is defined for in-range inputs -- what the reference
    pipelines feed after PointsRangeFilter.

    with_distance=True reproduces the reference's constructor arithmetic (in_channels + 3
    for the one distance channel appended), whose first Linear then cannot take the
    decorated features: forward raises instead.

    fusion_layer: the constructor refuses a config dict; registry.build_voxel_encoder builds
    the layer (PointFusion) and attaches it with set_fusion_layer.  With a layer set and
    img_feats given, the last vfe layer's point features pass through it before the last
    scatter (voxel_encoder.py:270-276)."""

    def __init__(self, in_channels=4, feat_channels=[], with_distance=False,
                 with_cluster_center=False, with_voxel_center=False, voxel_size=(0.2, 0.2, 4),
                 point_cloud_range=(0, -40, -3, 70.4, 40, 1),
                 norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01), mode="max",
                 fusion_layer=None, return_point_feats=False):
        super().__init__()
        assert mode in ["avg", "max"]
        assert len(feat_channels) > 0
        if fusion_layer is not None:
            raise NotImplementedError("DynamicVFE: a fusion_layer config is not built by the "
                                      "constructor; build the encoder with "
                                      "registry.build_voxel_encoder, which attaches the layer "
                                      "with set_fusion_layer")
        if with_cluster_center:
            in_channels += 3
        if with_voxel_center:
            in_channels += 3
        if with_distance:
            in_channels += 3        # (sic: one channel is appended, voxel_encoder.py:139-140)
        self.in_channels = in_channels
        self._with_distance = with_distance
        self._with_cluster_center = with_cluster_center
        self._with_voxel_center = with_voxel_center
        self.return_point_feats = return_point_feats
        self.fp16_enabled = False
        self.vx, self.vy, self.vz = voxel_size[0], voxel_size[1], voxel_size[2]
        self.x_offset = self.vx / 2 + point_cloud_range[0]
        self.y_offset = self.vy / 2 + point_cloud_range[1]
        self.z_offset = self.vz / 2 + point_cloud_range[2]
        self.point_cloud_range = point_cloud_range
        self.scatter = DynamicScatter(voxel_size, point_cloud_range, True)
        feat_channels = [self.in_channels] + list(feat_channels)
        vfe_layers = []
        for i in range(len(feat_channels) - 1):
            in_filters = feat_channels[i] * (2 if i > 0 else 1)
            out_filters = feat_channels[i + 1]
            vfe_layers.append(nn.Sequential(nn.Linear(in_filters, out_filters, bias=False),
                                            _norm_layer(norm_cfg, out_filters),
                                            nn.ReLU(inplace=True)))
        self.vfe_layers = nn.ModuleList(vfe_layers)
        self.num_vfe = len(vfe_layers)
        self.vfe_scatter = DynamicScatter(voxel_size, point_cloud_range, mode != "max")
        self.cluster_scatter = DynamicScatter(voxel_size, point_cloud_range, average_points=True)
        self.fusion_layer = None

    def set_fusion_layer(self, module):
        """Attach the point-image fusion layer (state-dict prefix `fusion_layer.*`)."""
        self.fusion_layer = module

    def map_voxel_center_to_point(self, voxel_feats, index):
        """voxel_feats[M, C] -> [N, C] through the shared index (0 for invalid points)."""
        return gather_points(voxel_feats, index)

    def forward(self, features, coors, points=None, img_feats=None, img_metas=None, index=None):
        """features[N, C], coors[N, 4] (batch, z, y, x) -> (voxel_feats[M, C'], voxel_coors[M, 4])
        or, return_point_feats, the last layer's point features."""
        features = raw = features.float()
        decorated = features.shape[1] + 3 * (self._with_cluster_center + self._with_voxel_center) \
            + int(self._with_distance)
        if decorated != self.vfe_layers[0][0].in_features:
            raise RuntimeError("DynamicVFE: the decorated features have %d channels, the first "
                               "layer takes %d (with_distance adds 3 to in_channels but appends "
                               "one channel, as in the reference)"
                               % (decorated, self.vfe_layers[0][0].in_features))
        if img_feats is not None and self.fusion_layer is None:
            raise NotImplementedError("DynamicVFE: img_feats given but no fusion layer is set "
                                      "(set_fusion_layer / registry.build_voxel_encoder)")
        if img_feats is not None and (points is None or img_metas is None):
            raise ValueError("DynamicVFE: fusing img_feats needs points and img_metas")
        if index is None:
            index = scatter_index(coors.contiguous())
        features_ls = [features]
        if self._with_cluster_center:
            # the mean of every column is independent: only the three the decoration reads
            voxel_mean = scatter_reduce(features[:, :3].contiguous(), index,
                                        self.cluster_scatter.reduce_type)
            points_mean = self.map_voxel_center_to_point(voxel_mean, index)
            features_ls.append(features[:, :3] - points_mean)
        if self._with_voxel_center:
            f_center = features.new_zeros(size=(features.size(0), 3))
            f_center[:, 0] = features[:, 0] - (coors[:, 3].type_as(features) * self.vx +
                                               self.x_offset)
            f_center[:, 1] = features[:, 1] - (coors[:, 2].type_as(features) * self.vy +
                                               self.y_offset)
            f_center[:, 2] = features[:, 2] - (coors[:, 1].type_as(features) * self.vz +
                                               self.z_offset)
            features_ls.append(f_center)
        if self._with_distance:
            features_ls.append(torch.norm(features[:, :3], 2, 1, keepdim=True))
        features = torch.cat(features_ls, dim=-1)
        reduce = self.vfe_scatter.reduce_type
        for i, vfe in enumerate(self.vfe_layers):
            point_feats = vfe(features)
            if i == len(self.vfe_layers) - 1 and self.fusion_layer is not None \
                    and img_feats is not None:
                # `features` are the clouds concatenated: the layer need not do it again
                point_feats = self.fusion_layer(img_feats, points, point_feats, img_metas,
                                                pts_cat=raw)
            voxel_feats = scatter_reduce(point_feats, index, reduce)
            if i != len(self.vfe_layers) - 1:
                features = torch.cat([point_feats,
                                      self.map_voxel_center_to_point(voxel_feats, index)], dim=1)
        if self.return_point_feats:
            return point_feats
        return voxel_feats, index.voxel_coors
