"""Minimal stand-in for the mmcv / mmdet3d registries the reference configs go
through (mmdet3d/models/registry.py:1-5, mmdet3d/models/builder.py:1-63,
mmcv.cnn.build_conv_layer / build_norm_layer as used by
mmdet3d/ops/sparse_block.py:159-187).

Only the registry *mechanics* are restated (type-string -> class, kwargs
pass-through) so `configs/MSMDFusion_nusc_voxel_LC.py`'s `model=` sub-dicts for
the hot path build unchanged: dict(type='SparseEncoder', ...),
dict(type='SubMConv3d', indice_key=...), dict(type='BN1d', eps=1e-3, momentum=0.01).
"""
import inspect

from torch import distributed as dist
from torch import nn


class Registry:
    def __init__(self, name):
        self.name = name
        self._modules = {}

    def get(self, key):
        if key not in self._modules:
            raise KeyError(f"{key} is not in the {self.name} registry")
        return self._modules[key]

    def __contains__(self, key):
        return key in self._modules

    def register_module(self, name=None, module=None, force=False):
        def _register(cls):
            key = name or cls.__name__
            if key in self._modules and not force:
                raise KeyError(f"{key} is already registered in {self.name}")
            self._modules[key] = cls
            return cls
        if module is not None:
            return _register(module)
        return _register

    def build(self, cfg, *args, **kwargs):
        if not isinstance(cfg, dict) or "type" not in cfg:
            raise TypeError(f"cfg must be a dict with a 'type' key, got {cfg!r}")
        cfg = dict(cfg)
        cls = cfg.pop("type")
        if isinstance(cls, str):
            cls = self.get(cls)
        elif not inspect.isclass(cls):
            raise TypeError(f"type must be a str or class, got {type(cls)}")
        return cls(*args, **kwargs, **cfg)


CONV_LAYERS = Registry("conv layer")
NORM_LAYERS = Registry("norm layer")
MIDDLE_ENCODERS = Registry("middle_encoder")
VOXEL_ENCODERS = Registry("voxel_encoder")
BACKBONES = Registry("backbone")
NECKS = Registry("neck")
DETECTORS = Registry("detector")
ROI_EXTRACTORS = Registry("roi_extractor")
HEADS = Registry("head")
FUSION_LAYERS = Registry("fusion_layer")
BBOX_SAMPLERS = Registry("bbox_sampler")

CONV_LAYERS.register_module("Conv1d", module=nn.Conv1d)
CONV_LAYERS.register_module("Conv2d", module=nn.Conv2d)
CONV_LAYERS.register_module("Conv3d", module=nn.Conv3d)
CONV_LAYERS.register_module("Conv", module=nn.Conv2d)
NORM_LAYERS.register_module("BN", module=nn.BatchNorm2d)
NORM_LAYERS.register_module("BN1d", module=nn.BatchNorm1d)
NORM_LAYERS.register_module("BN2d", module=nn.BatchNorm2d)
NORM_LAYERS.register_module("BN3d", module=nn.BatchNorm3d)



class _NaiveSyncMixin:
    """mmdet3d/ops/norm.py (NaiveSyncBatchNorm1d / 2d): in a single process -- no process
    group, or one of world size 1 -- and in eval mode the reference runs plain BatchNorm, and
    so does this.  Its multi-rank training branch all-reduces the batch mean and mean of
    squares; that exchange is not built, and normalising with per-rank statistics instead
    would be a silent deviation, so it is refused."""

    def plain_branch(self):
        """Whether forward would be plain BatchNorm (what the fused kernels may stand in for)."""
        return not (self.training and dist.is_available() and dist.is_initialized()
                    and dist.get_world_size() > 1)

    def check_single_process(self):
        if not self.plain_branch():
            raise NotImplementedError(
                "%s: training with a process group of world size %d needs the all-reduce of the "
                "batch statistics (mean and mean of squares) across ranks, which is not built; "
                "per-rank statistics would silently differ from the reference"
                % (type(self).__name__, dist.get_world_size()))

    def forward(self, input):
        self.check_single_process()
        return super().forward(input)


class NaiveSyncBatchNorm1d(_NaiveSyncMixin, nn.BatchNorm1d):
    pass


class NaiveSyncBatchNorm2d(_NaiveSyncMixin, nn.BatchNorm2d):
    pass


NORM_LAYERS.register_module("naiveSyncBN1d", module=NaiveSyncBatchNorm1d)
NORM_LAYERS.register_module("naiveSyncBN2d", module=NaiveSyncBatchNorm2d)

_NORM_ABBR = {"BN": "bn", "BN1d": "bn", "BN2d": "bn", "BN3d": "bn", "naiveSyncBN1d": "bn",
              "naiveSyncBN2d": "bn"}


def build_conv_layer(cfg, *args, **kwargs):
    """mmcv.cnn.build_conv_layer: cfg=None means Conv2d."""
    cfg = dict(type="Conv2d") if cfg is None else cfg
    return CONV_LAYERS.build(cfg, *args, **kwargs)


def build_norm_layer(cfg, num_features, postfix=""):
    """mmcv.cnn.build_norm_layer -> (name, layer); name = abbreviation +
    postfix, e.g. 'bn1' (the attribute name BasicBlock registers, which is what
    makes checkpoint keys '...bn1.weight')."""
    cfg = dict(cfg)
    layer_type = cfg.pop("type")
    requires_grad = cfg.pop("requires_grad", True)
    cfg.setdefault("eps", 1e-5)
    layer = NORM_LAYERS.get(layer_type)(num_features, **cfg)
    for p in layer.parameters():
        p.requires_grad = requires_grad
    return _NORM_ABBR.get(layer_type, "norm") + str(postfix), layer


def _register_hot_path():
    """Import the modules whose decorators fill the registries (mmdet3d does
    this from its package __init__)."""
    from . import (bev, hard_vfe, multimodal_encoder, pillar_encoder, pointnet2,  # noqa: F401
                   sparse_encoder, voxel_encoder)
    from .spconv import conv  # noqa: F401


def build_middle_encoder(cfg):
    _register_hot_path()
    return MIDDLE_ENCODERS.build(cfg)


def build_fusion_layer(cfg):
    """mmdet3d.models.builder.build_fusion_layer (PointFusion, fusion_layers.py)."""
    from . import fusion_layers  # noqa: F401
    return FUSION_LAYERS.build(cfg)


def build_voxel_encoder(cfg):
    """mmdet3d.models.builder.build_voxel_encoder.  A DynamicVFE config carrying a
    `fusion_layer` dict: the encoder is built without it, the layer by build_fusion_layer, and
    attached with set_fusion_layer (state-dict prefix `fusion_layer.*`, the reference's).  Any
    other type goes to its constructor unchanged (HardVFE refuses a fusion layer)."""
    _register_hot_path()
    if isinstance(cfg, dict) and cfg.get("type") == "DynamicVFE" and \
            isinstance(cfg.get("fusion_layer"), dict):
        encoder = VOXEL_ENCODERS.build({k: v for k, v in cfg.items() if k != "fusion_layer"})
        encoder.set_fusion_layer(build_fusion_layer(cfg["fusion_layer"]))
        return encoder
    return VOXEL_ENCODERS.build(cfg)


def build_backbone(cfg):
    """mmdet3d.models.builder.build_backbone for the BEV tail (SECOND)."""
    _register_hot_path()
    return BACKBONES.build(cfg)


def build_detector(cfg, train_cfg=None, test_cfg=None, **injected):
    """mmdet3d.models.build_detector (msmdfusion_amd/detector.py registers the classes)."""
    from . import detector
    return detector.build_detector(cfg, train_cfg=train_cfg, test_cfg=test_cfg, **injected)


def build_neck(cfg):
    """mmdet3d.models.builder.build_neck for the BEV tail (SECONDFPN)."""
    _register_hot_path()
    return NECKS.build(cfg)


def build_roi_extractor(cfg):
    """mmdet.models.builder.build_roi_extractor (Part-A2's Single3DRoIAwareExtractor)."""
    from . import roiaware_pool3d  # noqa: F401
    return ROI_EXTRACTORS.build(cfg)


def build_head(cfg, **kwargs):
    """mmdet3d.models.builder.build_head: CenterHead / SeparateHead (center_head.py),
    Anchor3DHead (anchor_head.py), FreeAnchor3DHead (free_anchor_head.py), VoteHead /
    BaseConvBboxHead (vote_head.py), SSD3DHead (ssd3d_head.py), PrimitiveHead
    (primitive_head.py), H3DBboxHead / H3DRoIHead (h3d_head.py), PointwiseSemanticHead
    (semantic_head.py), PartA2RPNHead (parta2_rpn_head.py), PartA2BboxHead
    (parta2_bbox_head.py), PartAggregationROIHead (parta2_roi_head.py), TransFusionHead (head.py) and,
    for a TransFusionHead config with fuse_img=True, TransFusionHeadLC (fusion_head.py): the
    reference has one class for both, so its config dicts build unchanged."""
    from . import (anchor_head, center_head, free_anchor_head, fusion_head, h3d_head,  # noqa: F401
                   head, parta2_bbox_head, parta2_roi_head, parta2_rpn_head, primitive_head,
                   semantic_head, ssd3d_head, vote_head)
    if isinstance(cfg, dict) and cfg.get("type") == "TransFusionHead" and cfg.get("fuse_img"):
        cfg = dict(cfg, type="TransFusionHeadLC")
    return HEADS.build(cfg, **kwargs)


def build_sampler(cfg):
    """mmdet.core.build_sampler for the RoI heads: IoUNegPiecewiseSampler (parta2_roi_head.py)."""
    from . import parta2_roi_head  # noqa: F401
    return cfg if not isinstance(cfg, dict) else BBOX_SAMPLERS.build(cfg)
