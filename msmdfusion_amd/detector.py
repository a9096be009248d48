"""The detectors the two target configs name, assembled from the hot-path modules.

    model = build_detector(MSMDFUSION_LC["model"], train_cfg=..., test_cfg=...)

`type='MSMDFusionDetector'` (configs/MSMDFusion_nusc_voxel_LC.py:141-268) and
`type='TransFusionDetector'` (configs/transfusion_nusc_voxel_L.py:150-169) resolve through the
DETECTORS registry, as mmdet3d.models.build_detector does; child modules are built from the
unchanged config sub-dicts by the registries of msmdfusion_amd.registry and carry the
reference's attribute names, so checkpoint keys (`pts_middle_encoder.*`,
`multimodal_middle_encoder.*`, `bev_fusion.*`, `pts_backbone.*`, `pts_neck.*`,
`pts_bbox_head.*`, `conv1x1_blocks.*`, `score_net.*`) load one to one.

Reference: mmdet3d/models/detectors/MSMDFusion.py (extract_img_feat :140-167,
extract_multiscale_voxel_feat :400-419, extract_pts_feat :421-452, forward_train :494-560,
forward_pts_train :562-590, simple_test :592-640), mmdet3d/models/detectors/transfusion.py
:61-101, mmdet3d/models/detectors/mvx_two_stage.py:38-120, tools/train.py:185-219
(freeze_lidar_components).

Out of scope: the image backbone and neck (frozen ResNet-50 + FPN).  They
are INJECTED: `img_backbone` / `img_neck` may be any nn.Module / callable producing the
multi-scale feature list the reference's FPN yields; without them the detector takes the
per-scale virtual points directly (`virtual_points=`), which is what bench.py feeds it.
"""
import logging
import warnings

import torch
from torch import nn

from . import spconv
from .fusion import SparseFusionPath
from . import sparse_unet  # noqa: F401,E402  (registers SparseUNet in MIDDLE_ENCODERS)
from .registry import (DETECTORS, build_backbone, build_middle_encoder, build_neck,
                       build_voxel_encoder)
from .voxelize import Voxelization


def build_detector(cfg, train_cfg=None, test_cfg=None, **injected):
    """mmdet3d.models.build_detector: cfg = the config's `model` dict (its own train_cfg /
    test_cfg keys win, as in mmdet3d).  injected: img_backbone / img_neck modules."""
    cfg = dict(cfg)
    if train_cfg is not None:
        cfg.setdefault("train_cfg", train_cfg)
    if test_cfg is not None:
        cfg.setdefault("test_cfg", test_cfg)
    cfg.update(injected)
    return DETECTORS.build(cfg)


def _build_head(cfg, train_cfg, test_cfg, rows):
    from .head import TransFusionHead
    if isinstance(cfg, nn.Module):
        return cfg
    args = {k: v for k, v in cfg.items() if k != "type"}
    pts = lambda c: (c or {}).get("pts", c) if isinstance(c, dict) else c
    kind = cfg.get("type", "TransFusionHead")
    if kind in ("CenterHead", "Anchor3DHead", "FreeAnchor3DHead"):
        from .registry import build_head
        return build_head(dict(cfg, train_cfg=pts(train_cfg), test_cfg=pts(test_cfg)))
    if kind not in ("TransFusionHead", "TransFusionHeadLC"):
        raise KeyError("pts_bbox_head type %r is not built here" % kind)
    if kind == "TransFusionHeadLC" or cfg.get("fuse_img"):
        from .fusion_head import TransFusionHeadLC
        return TransFusionHeadLC(train_cfg=pts(train_cfg), test_cfg=pts(test_cfg), rows=rows,
                                 **args)
    return TransFusionHead(train_cfg=pts(train_cfg), test_cfg=pts(test_cfg), rows=rows, **args)


@DETECTORS.register_module()
class TransFusionDetector(nn.Module):
    """LiDAR-only detector (configs/transfusion_nusc_voxel_L.py): voxelize -> HardSimpleVFE ->
    SparseEncoder -> SECOND -> SECONDFPN -> TransFusionHead; and the pillar form of
    configs/transfusion_nusc_pillar_L.py: voxelize -> PillarFeatureNet (on the padded pillar
    table) -> PointPillarsScatter -> the same tail.

    A `pts_voxel_layer` with max_num_points=-1 (or max_voxels=-1) selects dynamic
    voxelization (DynamicVoxelNet.voxelize, dynamic_voxelnet.py:46-71) with a dynamic voxel
    encoder (DynamicSimpleVFE / DynamicVFE): every point keeps its voxel coordinates, the
    encoder reduces them, and prepare() computes the scatters' index half up front."""

    def __init__(self, pts_voxel_layer=None, pts_voxel_encoder=None, pts_middle_encoder=None,
                 pts_backbone=None, pts_neck=None, pts_bbox_head=None, img_backbone=None,
                 img_neck=None, train_cfg=None, test_cfg=None, pretrained=None, freeze_img=True,
                 rows=True, **unused):
        super().__init__()
        self.pts_voxel_layer = Voxelization(**pts_voxel_layer)
        self.pts_voxel_encoder = build_voxel_encoder(pts_voxel_encoder)
        self.pts_middle_encoder = build_middle_encoder(pts_middle_encoder)
        self.rows = bool(rows)
        self.pts_backbone = self._dense(pts_backbone, build_backbone, "SECONDRows")
        self.pts_neck = self._dense(pts_neck, build_neck, "SECONDFPNRows")
        self.pts_bbox_head = None if pts_bbox_head is None else \
            _build_head(pts_bbox_head, train_cfg, test_cfg, self.rows)
        self.unused_cfg = dict(unused)      # keys of the config this path does not consume
        # the image branch is injected as modules; a config dict for it (the LC configs carry
        # the reference's ResNet / FPN dicts) is kept as a fact and builds nothing
        if isinstance(img_backbone, dict):
            self.unused_cfg["img_backbone"], img_backbone = img_backbone, None
        if isinstance(img_neck, dict):
            self.unused_cfg["img_neck"], img_neck = img_neck, None
        self.img_backbone, self.img_neck = img_backbone, img_neck
        self.freeze_img = freeze_img
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        if freeze_img:
            for m in (img_backbone, img_neck):
                if isinstance(m, nn.Module):
                    for p in m.parameters():
                        p.requires_grad = False

    def _dense(self, cfg, builder, rows_cls):
        """A dense BEV module from its config dict: the torch / MIOpen form, or (rows=True)
        the same parameters and state-dict keys computed on channels-last pixel rows by the
        sparse-conv kernels (grid_conv.py) -- for the type that has a row form (`rows_cls`
        without its suffix: SECOND, SECONDFPN); any other type is built by the registry."""
        if cfg is None or isinstance(cfg, nn.Module):
            return cfg
        if not self.rows or cfg.get("type", rows_cls[:-4]) != rows_cls[:-4]:
            return builder(cfg)      # (a type without a row form, e.g. FPN: the torch form)
        from . import grid_conv
        return getattr(grid_conv, rows_cls)(**{k: v for k, v in cfg.items() if k != "type"})

    # ---- mvx_two_stage.py properties ---------------------------------------------------
    with_pts_bbox = property(lambda self: self.pts_bbox_head is not None)
    with_pts_backbone = property(lambda self: self.pts_backbone is not None)
    with_pts_neck = property(lambda self: self.pts_neck is not None)
    with_img_backbone = property(lambda self: self.img_backbone is not None)
    with_img_neck = property(lambda self: self.img_neck is not None)

    @property
    def dynamic_voxelization(self):
        return self.pts_voxel_layer.max_num_points == -1 or -1 in self.pts_voxel_layer.max_voxels

    @property
    def voxel_table_encoder(self):
        """The voxel encoder reads the padded [N, max_points, C] table (PillarFeatureNet),
        not the per-voxel means: it says so itself (`takes_voxel_table`)."""
        return bool(getattr(self.pts_voxel_encoder, "takes_voxel_table", False))

    # ---- the path ----------------------------------------------------------------------
    @torch.no_grad()
    def voxelize_table(self, points):
        """mvx_two_stage.py:voxelize: hard voxelization per sample, batch id prepended, the
        table kept.  -> (voxels[N, max_points, C], num_points[N], coors[N, 4])"""
        voxels, nums, coors = [], [], []
        for b, (v, c, n) in enumerate(self.pts_voxel_layer.forward_batch(points, fused_mean=False)):
            voxels.append(v)
            nums.append(n)
            coors.append(nn.functional.pad(c, (1, 0), mode="constant", value=b))
        return torch.cat(voxels, 0), torch.cat(nums, 0), torch.cat(coors, 0)

    @torch.no_grad()
    def voxelize_dynamic(self, points):
        """dynamic_voxelnet.py:46-71: per-sample dynamic voxelization, batch id prepended.
        -> (points[N, C] concatenated, coors[N, 4] (b, z, y, x); -1 entries: out of range)"""
        coors = [nn.functional.pad(self.pts_voxel_layer(p), (1, 0), mode="constant", value=b)
                 for b, p in enumerate(points)]
        return torch.cat(points, dim=0), torch.cat(coors, dim=0)

    @torch.no_grad()
    def voxelize(self, points):
        """transfusion.py:76-101: hard voxelization per sample, batch id prepended; the
        HardSimpleVFE mean is fused into the gather (voxels are never materialised).
        -> (mean features [M,C], coors [M,4])"""
        feats, coors = [], []
        for b, (mean, c, _) in enumerate(self.pts_voxel_layer.forward_batch(points, fused_mean=True)):
            feats.append(mean)
            coors.append(nn.functional.pad(c, (1, 0), mode="constant", value=b))
        return torch.cat(feats, 0), torch.cat(coors, 0)

    def prepare(self, points):
        """The index-only part of a step (no weights, no previous step): voxelization and
        every rulebook / tiling / pair list of the encoder -- what IndexPrefetcher runs a
        step ahead.  Dynamic voxelization: the points, their coordinates and the scatter
        index (whose voxel rows the encoder's rulebooks are built on) take the place of the
        voxel features."""
        if not hasattr(self.pts_middle_encoder, "plan"):
            return self._prepare_pillars(points)
        if self.dynamic_voxelization:
            from .dynamic_scatter import scatter_index
            pts, coors = self.voxelize_dynamic(points)
            index = scatter_index(coors.contiguous())
            planned, _ = self.pts_middle_encoder.plan(index.voxel_coors, len(points))
            return (pts, coors, index), index.voxel_coors, planned
        feats, coors = self.voxelize(points)
        planned, _ = self.pts_middle_encoder.plan(coors, len(points))
        return feats, coors, planned

    def _prepare_pillars(self, points):
        """prepare() in front of a middle encoder with nothing to plan (PointPillarsScatter):
        the pillar table, or under dynamic voxelization the points and their scatter index."""
        if self.dynamic_voxelization:
            from .dynamic_scatter import scatter_index
            pts, coors = self.voxelize_dynamic(points)
            index = scatter_index(coors.contiguous())
            return (pts, coors, index), index.voxel_coors, None
        if not self.voxel_table_encoder:
            raise NotImplementedError("%s in front of %s is not built"
                                      % (type(self.pts_voxel_encoder).__name__,
                                         type(self.pts_middle_encoder).__name__))
        voxels, num_points, coors = self.voxelize_table(points)
        return (voxels, num_points), coors, None

    def extract_sparse_feat(self, points, prepared=None):
        feats, coors, planned = prepared if prepared is not None else self.prepare(points)
        if not hasattr(self.pts_middle_encoder, "plan"):
            if self.dynamic_voxelization:
                pts, pts_coors, index = feats
                feats, coors = self.pts_voxel_encoder(pts, pts_coors, index=index)
            else:
                voxels, num_points = feats
                feats = self.pts_voxel_encoder(voxels, num_points, coors)
            return self.pts_middle_encoder(feats, coors, len(points))
        if self.dynamic_voxelization:
            pts, pts_coors, index = feats
            feats, coors = self.pts_voxel_encoder(pts, pts_coors, index=index)
        bev, _ = self.pts_middle_encoder(feats, coors, len(points), planned=planned)
        return bev

    def extract_pts_feat(self, pts, img_feats=None, img_metas=None, prepared=None):
        """transfusion.py:61-74 -> list of BEV maps (the neck's output)."""
        x = self.extract_sparse_feat(pts, prepared=prepared)
        if self.with_pts_backbone:
            x = self.pts_backbone(x)
        if self.with_pts_neck:
            x = self.pts_neck(x)
        return x if isinstance(x, (list, tuple)) else [x]

    def extract_img_feat(self, img, img_metas):
        """MSMDFusion.py:140-167 around the injected image branch."""
        if self.img_backbone is None or img is None:
            return None
        input_shape = img.shape[-2:]
        for meta in img_metas:
            meta.update(input_shape=input_shape)
        if img.dim() == 5:
            img = img.view(-1, *img.shape[2:])
        feats = self.img_backbone(img.float())
        if self.img_neck is not None:
            feats = self.img_neck(feats)
        return feats

    def extract_feat(self, points, img=None, img_metas=None, **kw):
        img_feats = self.extract_img_feat(img, img_metas)
        return img_feats, self.extract_pts_feat(points, img_feats, img_metas, **kw)

    def forward_pts_train(self, pts_feats, img_feats, gt_bboxes_3d, gt_labels_3d, img_metas=None):
        """MSMDFusion.py:562-590 / transfusion.py:163-190 -> dict of losses."""
        outs = self.pts_bbox_head(pts_feats, img_feats, img_metas)
        return self.pts_bbox_head.loss(gt_bboxes_3d, gt_labels_3d, outs)

    def forward_train(self, points=None, img_metas=None, gt_bboxes_3d=None, gt_labels_3d=None,
                      img=None, **kw):
        """MSMDFusion.py:494-560: features, then the point branch's losses."""
        img_feats, pts_feats = self.extract_feat(points, img=img, img_metas=img_metas, **kw)
        return self.forward_pts_train(pts_feats, img_feats, gt_bboxes_3d, gt_labels_3d, img_metas)

    def simple_test(self, points, img_metas=None, img=None, **kw):
        """MSMDFusion.py:592-640 without NMS (nms_type=None in both configs): per sample a
        dict(boxes_3d, scores_3d, labels_3d)."""
        img_feats, pts_feats = self.extract_feat(points, img=img, img_metas=img_metas, **kw)
        outs = self.pts_bbox_head(pts_feats, img_feats, img_metas)
        # bbox3d2result's fields (mmdet3d/core/bbox/transforms.py)
        return [dict(boxes_3d=r["bboxes"], scores_3d=r["scores"], labels_3d=r["labels"])
                for r in self.pts_bbox_head.get_bboxes(outs)]

    def forward(self, points, *extra, return_loss=False, prepared=None, **kw):
        """return_loss=False (default): the BEV feature list of extract_pts_feat (what the
        throughput benchmark differentiates); True: forward_train's loss dict."""
        if return_loss:
            return self.forward_train(points=points, prepared=prepared, **kw)
        return self.extract_pts_feat(points, *extra, prepared=prepared, **kw)


@DETECTORS.register_module()
class CenterPoint(TransFusionDetector):
    """mmdet3d/models/detectors/centerpoint.py: the same voxelize -> encoder -> SECOND ->
    SECONDFPN path with CenterHead on the neck's maps (configs.CENTERPOINT_VOXEL_NUS /
    CENTERPOINT_PILLAR_NUS)."""

    def forward_pts_train(self, pts_feats, img_feats, gt_bboxes_3d, gt_labels_3d, img_metas=None):
        """centerpoint.py:52-76."""
        outs = self.pts_bbox_head(pts_feats)
        return self.pts_bbox_head.loss(gt_bboxes_3d, gt_labels_3d, outs)

    def simple_test(self, points, img_metas=None, img=None, **kw):
        """centerpoint.py:78-87 (simple_test_pts + bbox3d2result's fields)."""
        _, pts_feats = self.extract_feat(points, img=img, img_metas=img_metas, **kw)
        outs = self.pts_bbox_head(pts_feats)
        return [dict(boxes_3d=b, scores_3d=s, labels_3d=l)
                for b, s, l in self.pts_bbox_head.get_bboxes(outs, img_metas)]


@DETECTORS.register_module()
class VoxelNet(TransFusionDetector):
    """mmdet3d/models/detectors/voxelnet.py (SingleStage3DDetector): the same voxelize ->
    encoder -> SECOND -> SECONDFPN path under the reference's attribute names (`voxel_layer`,
    `voxel_encoder`, `middle_encoder`, `backbone`, `neck`, `bbox_head`, which are also its
    state-dict prefixes) with Anchor3DHead on the neck's maps (configs.POINTPILLARS_SECFPN_KITTI
    / SECOND_SECFPN_KITTI).  The path itself is TransFusionDetector's: its `pts_*` names
    resolve to these attributes."""

    _ALIAS = dict(pts_voxel_layer="voxel_layer", pts_voxel_encoder="voxel_encoder",
                  pts_middle_encoder="middle_encoder", pts_backbone="backbone", pts_neck="neck",
                  pts_bbox_head="bbox_head")

    def __init__(self, voxel_layer=None, voxel_encoder=None, middle_encoder=None, backbone=None,
                 neck=None, bbox_head=None, train_cfg=None, test_cfg=None, pretrained=None,
                 init_cfg=None, **kwargs):
        super().__init__(pts_voxel_layer=voxel_layer, pts_voxel_encoder=voxel_encoder,
                         pts_middle_encoder=middle_encoder, pts_backbone=backbone, pts_neck=neck,
                         pts_bbox_head=bbox_head, train_cfg=train_cfg, test_cfg=test_cfg,
                         pretrained=pretrained, **kwargs)

    def __setattr__(self, name, value):
        # the base constructor assigns the six pts_* names: they land under the reference's
        super().__setattr__(self._ALIAS.get(name, name), value)

    pts_voxel_layer = property(lambda self: self.voxel_layer)
    pts_voxel_encoder = property(lambda self: self.voxel_encoder)
    pts_middle_encoder = property(lambda self: self.middle_encoder)
    pts_backbone = property(lambda self: self.backbone)
    pts_neck = property(lambda self: self.neck)
    pts_bbox_head = property(lambda self: self.bbox_head)

    def forward_pts_train(self, pts_feats, img_feats, gt_bboxes_3d, gt_labels_3d, img_metas=None):
        """voxelnet.py:67-96."""
        outs = self.bbox_head(pts_feats)
        return self.bbox_head.loss(*outs, gt_bboxes_3d, gt_labels_3d, img_metas)

    def simple_test(self, points, img_metas=None, imgs=None, rescale=False, **kw):
        """voxelnet.py:98-108 (bbox3d2result's fields)."""
        _, pts_feats = self.extract_feat(points, img_metas=img_metas, **kw)
        outs = self.bbox_head(pts_feats)
        metas = img_metas if img_metas is not None else [None] * len(points)
        return [dict(boxes_3d=b, scores_3d=s, labels_3d=l)
                for b, s, l in self.bbox_head.get_bboxes(*outs, metas, rescale=rescale)]


@DETECTORS.register_module()
class MVXTwoStageDetector(TransFusionDetector):
    """mmdet3d/models/detectors/mvx_two_stage.py, the point branch: voxelize -> pts_voxel_encoder
    -> pts_middle_encoder -> pts_backbone -> pts_neck -> pts_bbox_head under the reference's
    `pts_*` attribute names (its state-dict prefixes), the head called as forward_pts_train
    (:261-289) and simple_test_pts (:386-396) call it.  The batch size is len(points), not the
    reference's host read of coors[-1, 0] + 1.  The image branch and pts_fusion_layer are out of
    scope.  With rows=True the backbone runs on pixel rows and hands the neck NCHW views of its
    channels-last buffers; an FPN neck (no row form) takes them as they are."""

    def __init__(self, pts_fusion_layer=None, img_rpn_head=None, img_roi_head=None, **kwargs):
        if pts_fusion_layer is not None or img_rpn_head is not None or img_roi_head is not None:
            raise NotImplementedError("%s: pts_fusion_layer and the image heads are not built"
                                      % type(self).__name__)
        super().__init__(**kwargs)

    def _check_norms(self):
        for m in self.modules():
            if hasattr(m, "check_single_process"):     # (the row-form layers bypass forward)
                m.check_single_process()

    def forward_train(self, *args, **kw):
        self._check_norms()
        return super().forward_train(*args, **kw)

    def forward_pts_train(self, pts_feats, img_feats, gt_bboxes_3d, gt_labels_3d, img_metas=None):
        """mvx_two_stage.py:261-289."""
        outs = self.pts_bbox_head(pts_feats)
        return self.pts_bbox_head.loss(*outs, gt_bboxes_3d, gt_labels_3d, img_metas)

    def simple_test(self, points, img_metas=None, img=None, rescale=False, **kw):
        """mvx_two_stage.py:386-396, 398-412 (bbox3d2result's fields)."""
        _, pts_feats = self.extract_feat(points, img=img, img_metas=img_metas, **kw)
        outs = self.pts_bbox_head(pts_feats)
        metas = img_metas if img_metas is not None else [None] * len(points)
        return [dict(boxes_3d=b, scores_3d=s, labels_3d=l)
                for b, s, l in self.pts_bbox_head.get_bboxes(*outs, metas, rescale=rescale)]


@DETECTORS.register_module()
class MVXFasterRCNN(MVXTwoStageDetector):
    """mmdet3d/models/detectors/mvx_faster_rcnn.py: MVXTwoStageDetector under the name the
    nuScenes PointPillars-FPN and free_anchor configs use."""


@DETECTORS.register_module()
class DynamicMVXFasterRCNN(MVXTwoStageDetector):
    """mmdet3d/models/detectors/mvx_faster_rcnn.py:17-61 (MVX-Net with dynamic voxelization,
    configs.MVXNET_DV_SECOND_KITTI): the voxel encoder (DynamicVFE) takes the clouds, the image
    features and the metas and fuses them into the point features through its fusion layer
    (PointFusion).  The image features come from the injected image branch (extract_img_feat
    records `input_shape` in the metas) or from an `img_feats=` keyword, whose metas then carry
    `input_shape` already.  The batch size is len(points)."""

    def extract_feat(self, points, img=None, img_metas=None, img_feats=None, **kw):
        if img_feats is None:
            img_feats = self.extract_img_feat(img, img_metas)
        return img_feats, self.extract_pts_feat(points, img_feats, img_metas, **kw)

    def extract_pts_feat(self, pts, img_feats=None, img_metas=None, prepared=None):
        """mvx_faster_rcnn.py:46-61 on the prepared scatter index."""
        if not self.dynamic_voxelization:
            raise NotImplementedError("DynamicMVXFasterRCNN needs dynamic voxelization "
                                      "(max_num_points=-1)")
        feats, coors, planned = prepared if prepared is not None else self.prepare(pts)
        cat, pts_coors, index = feats
        feats, coors = self.pts_voxel_encoder(cat, pts_coors, points=pts, img_feats=img_feats,
                                              img_metas=img_metas, index=index)
        if hasattr(self.pts_middle_encoder, "plan"):
            x, _ = self.pts_middle_encoder(feats, coors, len(pts), planned=planned)
        else:
            x = self.pts_middle_encoder(feats, coors, len(pts))
        if self.with_pts_backbone:
            x = self.pts_backbone(x)
        if self.with_pts_neck:
            x = self.pts_neck(x)
        return x if isinstance(x, (list, tuple)) else [x]


@DETECTORS.register_module()
class VoteNet(nn.Module):
    """mmdet3d/models/detectors/votenet.py on single_stage.py (SingleStage3DDetector): a
    PointNet++ backbone built from BACKBONES and VoteHead, under the reference's attribute
    names `backbone` and `bbox_head` (its state-dict prefixes).  Points arrive as a list of
    equally long [N, C] tensors and are stacked, as there."""

    def __init__(self, backbone, bbox_head=None, train_cfg=None, test_cfg=None, pretrained=None,
                 init_cfg=None):
        super().__init__()
        from .registry import build_head
        self.backbone = build_backbone(backbone)
        self.bbox_head = bbox_head if isinstance(bbox_head, nn.Module) or bbox_head is None else \
            build_head(dict(bbox_head, train_cfg=train_cfg, test_cfg=test_cfg))
        self.train_cfg, self.test_cfg = train_cfg, test_cfg

    @staticmethod
    def _stack(points):
        return points if torch.is_tensor(points) else torch.stack(list(points))

    def extract_feat(self, points, img_metas=None):
        """single_stage.py:52-59 (VoteNet has no neck)."""
        return self.backbone(points)

    def forward_train(self, points, img_metas=None, gt_bboxes_3d=None, gt_labels_3d=None,
                      pts_semantic_mask=None, pts_instance_mask=None, gt_bboxes_ignore=None):
        """votenet.py:26-62 -> the head's loss dict."""
        points_cat = self._stack(points)
        x = self.extract_feat(points_cat)
        bbox_preds = self.bbox_head(x, self.train_cfg["sample_mod"])
        return self.bbox_head.loss(bbox_preds, points_cat, gt_bboxes_3d, gt_labels_3d,
                                   pts_semantic_mask, pts_instance_mask, img_metas,
                                   gt_bboxes_ignore=gt_bboxes_ignore)

    def simple_test(self, points, img_metas=None, imgs=None, rescale=False):
        """votenet.py:64-84 (bbox3d2result's fields)."""
        points_cat = self._stack(points)
        x = self.extract_feat(points_cat)
        bbox_preds = self.bbox_head(x, self.test_cfg["sample_mod"])
        bbox_list = self.bbox_head.get_bboxes(points_cat, bbox_preds, img_metas, rescale=rescale)
        return [dict(boxes_3d=b, scores_3d=s, labels_3d=l) for b, s, l in bbox_list]

    def forward(self, points, img_metas=None, return_loss=False, **kw):
        if return_loss:
            return self.forward_train(points, img_metas, **kw)
        return self.simple_test(points, img_metas, **kw)


@DETECTORS.register_module()
class SSD3DNet(VoteNet):
    """mmdet3d/models/detectors/ssd3dnet.py: VoteNet's flow with a PointNet2SAMSG backbone and
    SSD3DHead."""


@DETECTORS.register_module()
class H3DNet(nn.Module):
    """mmdet3d/models/detectors/h3dnet.py on two_stage.py (TwoStage3DDetector): MultiBackbone,
    VoteHead as `rpn_head` (built with train_cfg.rpn / test_cfg.rpn) and H3DRoIHead as
    `roi_head` (train_cfg.rcnn / test_cfg.rcnn), under the reference's attribute names.
    aug_test is not built, as for the other detectors."""

    def __init__(self, backbone, neck=None, rpn_head=None, roi_head=None, train_cfg=None,
                 test_cfg=None, pretrained=None, init_cfg=None):
        super().__init__()
        from .registry import build_head
        if neck is not None:
            raise NotImplementedError("H3DNet has no neck")
        sub = lambda cfg, key: None if cfg is None else cfg[key]              # noqa: E731
        self.backbone = build_backbone(backbone)
        self.rpn_head = rpn_head if isinstance(rpn_head, nn.Module) else build_head(
            dict(rpn_head, train_cfg=sub(train_cfg, "rpn"), test_cfg=sub(test_cfg, "rpn")))
        self.roi_head = roi_head if isinstance(roi_head, nn.Module) else build_head(
            dict(roi_head, train_cfg=sub(train_cfg, "rcnn"), test_cfg=sub(test_cfg, "rcnn")))
        self.train_cfg, self.test_cfg = train_cfg, test_cfg

    _stack = staticmethod(VoteNet._stack)

    def extract_feat(self, points, img_metas=None):
        """h3dnet.py:59-62: the backbone's dictionary, with the names VoteHead reads aliased to
        the first stream's seeds and the fused feature."""
        feats_dict = self.backbone(points)
        feats_dict["fp_xyz"] = [feats_dict["fp_xyz_net0"][-1]]
        feats_dict["fp_features"] = [feats_dict["hd_feature"]]
        feats_dict["fp_indices"] = [feats_dict["fp_indices_net0"][-1]]
        return feats_dict

    def forward_train(self, points, img_metas=None, gt_bboxes_3d=None, gt_labels_3d=None,
                      pts_semantic_mask=None, pts_instance_mask=None, gt_bboxes_ignore=None):
        """h3dnet.py:32-96 -> the losses of the rpn head and of the RoI head."""
        points_cat = self._stack(points)
        feats_dict = self.extract_feat(points_cat)
        rpn_outs = self.rpn_head(feats_dict, self.train_cfg["rpn"]["sample_mod"])
        feats_dict.update(rpn_outs)
        losses = self.rpn_head.loss(rpn_outs, points_cat, gt_bboxes_3d, gt_labels_3d,
                                    pts_semantic_mask, pts_instance_mask, img_metas,
                                    gt_bboxes_ignore=gt_bboxes_ignore, ret_target=True)
        feats_dict["targets"] = losses.pop("targets")
        proposal_cfg = self.train_cfg.get("rpn_proposal", self.test_cfg["rpn"])
        feats_dict["proposal_list"] = self.rpn_head.get_bboxes(
            points_cat, rpn_outs, img_metas, use_nms=proposal_cfg["use_nms"])
        losses.update(self.roi_head.forward_train(
            feats_dict, img_metas, points_cat, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask,
            pts_instance_mask, gt_bboxes_ignore))
        return losses

    def simple_test(self, points, img_metas=None, imgs=None, rescale=False):
        """h3dnet.py:98-128."""
        points_cat = self._stack(points)
        feats_dict = self.extract_feat(points_cat)
        proposal_cfg = self.test_cfg["rpn"]
        rpn_outs = self.rpn_head(feats_dict, proposal_cfg["sample_mod"])
        feats_dict.update(rpn_outs)
        feats_dict["proposal_list"] = self.rpn_head.get_bboxes(
            points_cat, rpn_outs, img_metas, use_nms=proposal_cfg["use_nms"])
        return self.roi_head.simple_test(feats_dict, img_metas, points_cat, rescale=rescale)

    def forward(self, points, img_metas=None, return_loss=False, **kw):
        if return_loss:
            return self.forward_train(points, img_metas, **kw)
        return self.simple_test(points, img_metas, **kw)


@DETECTORS.register_module()
class PartA2(nn.Module):
    """mmdet3d/models/detectors/parta2.py on two_stage.py (TwoStage3DDetector): hard
    voxelization, HardSimpleVFE, SparseUNet, SECOND / SECONDFPN, PartA2RPNHead as `rpn_head`
    (built with train_cfg.rpn / test_cfg.rpn) and PartAggregationROIHead as `roi_head`
    (train_cfg.rcnn / test_cfg.rcnn), under the reference's attribute names (its state-dict
    prefixes).  The batch size is the length of the point list, where the reference reads
    `coors[-1, 0].item() + 1` (:47).  aug_test is not built, as for the other detectors."""

    def __init__(self, voxel_layer, voxel_encoder, middle_encoder, backbone, neck=None,
                 rpn_head=None, roi_head=None, train_cfg=None, test_cfg=None, pretrained=None,
                 init_cfg=None):
        super().__init__()
        from .registry import build_head
        sub = lambda cfg, key: None if cfg is None else cfg[key]              # noqa: E731
        self.backbone = build_backbone(backbone)
        self.neck = None if neck is None else build_neck(neck)
        self.rpn_head = rpn_head if isinstance(rpn_head, nn.Module) or rpn_head is None else \
            build_head(dict(rpn_head, train_cfg=sub(train_cfg, "rpn"),
                            test_cfg=sub(test_cfg, "rpn")))
        self.roi_head = roi_head if isinstance(roi_head, nn.Module) or roi_head is None else \
            build_head(dict(roi_head, train_cfg=sub(train_cfg, "rcnn"),
                            test_cfg=sub(test_cfg, "rcnn")))
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.voxel_layer = Voxelization(**voxel_layer)
        self.voxel_encoder = build_voxel_encoder(voxel_encoder)
        self.middle_encoder = build_middle_encoder(middle_encoder)

    with_neck = property(lambda self: self.neck is not None)
    with_rpn = property(lambda self: self.rpn_head is not None)
    with_roi_head = property(lambda self: self.roi_head is not None)

    @torch.no_grad()
    def voxelize(self, points):
        """parta2.py:56-85: hard voxelization per sample, the batch id prepended, and the voxel
        centres (semantic_head.voxel_centers)."""
        from .semantic_head import voxel_centers
        voxels, nums, coors = [], [], []
        for b, (v, c, n) in enumerate(self.voxel_layer.forward_batch(points, fused_mean=False)):
            voxels.append(v)
            nums.append(n)
            coors.append(nn.functional.pad(c, (1, 0), mode="constant", value=b))
        coors = torch.cat(coors, dim=0)
        return dict(voxels=torch.cat(voxels, dim=0), num_points=torch.cat(nums, dim=0),
                    coors=coors,
                    voxel_centers=voxel_centers(coors, self.voxel_layer.voxel_size,
                                                self.voxel_layer.point_cloud_range))

    def extract_feat(self, points, img_metas=None):
        """parta2.py:41-54 -> (feats_dict with spatial_features / seg_features / neck_feats,
        voxel_dict)."""
        voxel_dict = self.voxelize(points)
        voxel_features = self.voxel_encoder(voxel_dict["voxels"], voxel_dict["num_points"],
                                            voxel_dict["coors"])
        feats_dict = self.middle_encoder(voxel_features, voxel_dict["coors"], len(points))
        x = self.backbone(feats_dict["spatial_features"])
        if self.with_neck:
            feats_dict.update({"neck_feats": self.neck(x)})
        return feats_dict, voxel_dict

    def forward_train(self, points, img_metas=None, gt_bboxes_3d=None, gt_labels_3d=None,
                      gt_bboxes_ignore=None, proposals=None, generator=None):
        """parta2.py:87-134 -> the losses of the RPN head, the semantic head and the bbox head.
        generator: the torch.Generator of the RoI sampler's keys."""
        feats_dict, voxels_dict = self.extract_feat(points, img_metas)
        metas = img_metas if img_metas is not None else [None] * len(points)
        losses = dict()
        if self.with_rpn:
            rpn_outs = self.rpn_head(feats_dict["neck_feats"])
            losses.update(self.rpn_head.loss(*rpn_outs, gt_bboxes_3d, gt_labels_3d, metas,
                                             gt_bboxes_ignore=gt_bboxes_ignore))
            proposal_cfg = self.train_cfg.get("rpn_proposal", self.test_cfg["rpn"])
            with torch.no_grad():
                proposal_list = self.rpn_head.get_bboxes(*rpn_outs, metas, proposal_cfg)
        else:
            proposal_list = proposals
        losses.update(self.roi_head.forward_train(feats_dict, voxels_dict, metas, proposal_list,
                                                  gt_bboxes_3d, gt_labels_3d,
                                                  generator=generator))
        return losses

    def simple_test(self, points, img_metas=None, proposals=None, rescale=False):
        """parta2.py:136-149."""
        feats_dict, voxels_dict = self.extract_feat(points, img_metas)
        metas = img_metas if img_metas is not None else [None] * len(points)
        if self.with_rpn:
            rpn_outs = self.rpn_head(feats_dict["neck_feats"])
            proposal_list = self.rpn_head.get_bboxes(*rpn_outs, metas, self.test_cfg["rpn"])
        else:
            proposal_list = proposals
        return self.roi_head.simple_test(feats_dict, voxels_dict, metas, proposal_list)

    def forward(self, points, img_metas=None, return_loss=False, **kw):
        if return_loss:
            return self.forward_train(points, img_metas, **kw)
        return self.simple_test(points, img_metas, **kw)


class MLP(nn.Module):
    """mmdet3d/models/utils/mlp.py: (B, C, N) features through kernel-size-1 ConvModules with a
    conv bias under the norm, keys `mlp.layer{i}.conv.*` / `mlp.layer{i}.bn.*`."""

    def __init__(self, in_channel=18, conv_channels=(256, 256), conv_cfg=dict(type="Conv1d"),
                 norm_cfg=dict(type="BN1d"), act_cfg=dict(type="ReLU")):
        super().__init__()
        from .vote_head import _conv_module
        self.mlp = nn.Sequential()
        prev_channels = in_channel
        for i, conv_channel in enumerate(conv_channels):
            self.mlp.add_module("layer%d" % i, _conv_module(prev_channels, conv_channel, conv_cfg,
                                                            norm_cfg, act_cfg, bias=True))
            prev_channels = conv_channel

    def forward(self, img_features):
        return self.mlp(img_features)


def sample_valid_seeds(mask, num_sampled_seed=1024, generator=None):
    """imvotenet.py:12-49 for the whole batch, without its nonzero / unique / randperm per
    sample and their host reads.  mask bool [B, N] -> long [B, num_sampled_seed], per sample by
    the reference's two branches (chosen with torch.where on the valid count n):
      n >= num_sampled_seed: a uniformly random num_sampled_seed of the valid indices, in random
        order (the argsort of uniform keys over the valid entries);
      n < num_sampled_seed: every valid index in ascending order, then uniformly random distinct
        members of {0 .. num_sampled_seed - 1} minus {valid % num_sampled_seed}.
    The draws have the reference's law, not its randperm stream.  generator: a torch.Generator
    on mask's device."""
    b, n_all = mask.shape
    s, dev = int(num_sampled_seed), mask.device
    mask = mask.bool()
    count = mask.sum(dim=1, keepdim=True)                                    # [B, 1]
    take = min(n_all, s)
    pad = (lambda t: nn.functional.pad(t, (0, s - take))) if take < s else (lambda t: t)
    # n >= s: the valid entries in random order
    keys = torch.rand((b, n_all), generator=generator, device=dev)
    many = pad(torch.argsort(torch.where(mask, keys, keys.new_full((), 2.0)), dim=1)[:, :take])
    # n < s: the valid entries in ascending order ...
    pos = torch.arange(n_all, device=dev).expand(b, n_all)
    ascending = pad(torch.sort(torch.where(mask, pos, pos.new_full((), n_all)), dim=1)[0][:, :take])
    # ... then the difference set in random order
    present = torch.zeros((b, s), dtype=torch.int32, device=dev).scatter_add_(
        1, pos % s, mask.int()) > 0
    keys2 = torch.rand((b, s), generator=generator, device=dev)
    rest = torch.argsort(torch.where(present, keys2.new_full((), 2.0), keys2), dim=1)
    slot = torch.arange(s, device=dev).expand(b, s)
    few = torch.where(slot < count, ascending, rest.gather(1, (slot - count).clamp(min=0)))
    return torch.where(count >= s, many, few)


@DETECTORS.register_module()
class ImVoteNet(nn.Module):
    """mmdet3d/models/detectors/imvotenet.py, stage 2 (forward_train :445-523, simple_test
    :677-716): a PointNet++ backbone, VoteFusion lifting 2-D detections onto the seeds, and three
    VoteHead towers (joint / points only / image only) under the reference's attribute names
    `pts_backbone`, `pts_bbox_head_joint` / `_pts` / `_img`, `img_mlp`, `fusion_layer` (its
    state-dict prefixes).  The towers are built from pts_bbox_heads.common updated by joint, pts
    and img; their losses are combined by pts_bbox_heads.loss_weights, non-loss entries come
    from the joint tower.

    The image branch is INJECTED, as in the MVX detectors: the 2-D detections arrive as
    `bboxes_2d` (a list of [n, 6] = (l, t, r, b, conf, class) tensors in the rescaled image
    frame) or from `img_detector(img, img_metas)`, any callable returning that list; it runs
    under no_grad and its parameters are frozen.  In training half of each list is dropped
    (a sorted randperm over its length, :352-367).  The image-only pre-training branch
    (points=None) and aug_test are not built."""

    def __init__(self, pts_backbone=None, pts_bbox_heads=None, pts_neck=None, img_mlp=None,
                 fusion_layer=None, num_sampled_seed=None, freeze_img_branch=False,
                 img_detector=None, train_cfg=None, test_cfg=None, pretrained=None, **unused):
        super().__init__()
        from .registry import build_fusion_layer, build_head
        if pts_neck is not None:
            raise NotImplementedError("ImVoteNet: pts_neck is not built")
        self.pts_backbone = build_backbone(pts_backbone)
        pts = lambda c: (c or {}).get("pts", c) if isinstance(c, dict) else c     # noqa: E731
        heads = dict(pts_bbox_heads)
        common = dict(heads["common"], train_cfg=pts(train_cfg), test_cfg=pts(test_cfg))
        self.pts_bbox_head_joint = build_head(dict(common, **heads["joint"]))
        self.pts_bbox_head_pts = build_head(dict(common, **heads["pts"]))
        self.pts_bbox_head_img = build_head(dict(common, **heads["img"]))
        self.loss_weights = list(heads["loss_weights"])
        self.fusion_layer = build_fusion_layer(fusion_layer)
        self.max_imvote_per_pixel = self.fusion_layer.max_imvote_per_pixel
        self.img_mlp = MLP(**img_mlp)
        self.num_sampled_seed = num_sampled_seed
        self.freeze_img_branch = freeze_img_branch
        object.__setattr__(self, "img_detector", img_detector)    # (injected: no keys of ours)
        if isinstance(img_detector, nn.Module):
            for p in img_detector.parameters():
                p.requires_grad = False
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.unused_cfg = dict(unused)      # keys of the config this path does not consume

    @property
    def pts_bbox_heads(self):
        return [self.pts_bbox_head_joint, self.pts_bbox_head_pts, self.pts_bbox_head_img]

    def extract_pts_feat(self, pts):
        """:294-304 -> (seed_points, seed_features, seed_indices)."""
        x = self.pts_backbone(pts)
        return x["fp_xyz"][-1], x["fp_features"][-1], x["fp_indices"][-1]

    @torch.no_grad()
    def extract_bboxes_2d(self, img, img_metas, train=True, bboxes_2d=None, generator=None):
        """:311-368 around the injected detector: the lists as float tensors, in training with
        half of each dropped."""
        if bboxes_2d is None:
            if self.img_detector is None:
                raise ValueError("ImVoteNet needs bboxes_2d or an injected img_detector")
            bboxes_2d = self.img_detector(img, img_metas)
        out = []
        for ret in bboxes_2d:
            if len(ret) > 0 and train:
                keep = torch.randperm(len(ret), generator=generator)[:(len(ret) + 1) // 2]
                ret = ret[torch.sort(keep)[0].to(ret.device)]
            out.append(ret.float())
        return out

    def fuse_and_sample(self, img, bboxes_2d, seeds_3d, seed_3d_features, seed_indices, img_metas,
                        calib, generator=None):
        """:452-470: fuse, sample num_sampled_seed imvotes per sample, gather the seed points,
        features and indices they belong to, img_mlp.  No host read on the fused path.
        -> (seeds_3d, seed_3d_features, img_features, seed_indices)"""
        img_features, masks = self.fusion_layer(img, bboxes_2d, seeds_3d, img_metas, calib)
        inds = sample_valid_seeds(masks, self.num_sampled_seed, generator=generator)
        batch_size, img_feat_size = img_features.shape[:2]
        pts_feat_size = seed_3d_features.shape[1]
        img_features = img_features.gather(
            -1, inds.view(batch_size, 1, -1).expand(-1, img_feat_size, -1))
        inds = inds % inds.shape[1]
        seeds_3d = seeds_3d.gather(1, inds.view(batch_size, -1, 1).expand(-1, -1, 3))
        seed_3d_features = seed_3d_features.gather(
            -1, inds.view(batch_size, 1, -1).expand(-1, pts_feat_size, -1))
        seed_indices = seed_indices.gather(1, inds)
        return seeds_3d, seed_3d_features, self.img_mlp(img_features), seed_indices

    @staticmethod
    def _stack(points):
        return points if torch.is_tensor(points) else torch.stack(list(points))

    def tower_losses(self, points, img, img_metas, calib, bboxes_2d, gt_bboxes_3d, gt_labels_3d,
                     pts_semantic_mask=None, pts_instance_mask=None, gt_bboxes_ignore=None,
                     generator=None, drop_generator=None):
        """The three towers' own loss dicts (joint, pts, img), :445-508.  generator: for the
        seed sampling, on the points' device; drop_generator: for the half drop, on the CPU."""
        bboxes_2d = self.extract_bboxes_2d(img, img_metas, bboxes_2d=bboxes_2d,
                                           generator=drop_generator)
        points = self._stack(points)
        seeds_3d, seed_3d_features, seed_indices = self.extract_pts_feat(points)
        seeds_3d, seed_3d_features, img_features, seed_indices = self.fuse_and_sample(
            img, bboxes_2d, seeds_3d, seed_3d_features, seed_indices, img_metas, calib,
            generator=generator)
        fused_features = torch.cat([seed_3d_features, img_features], dim=1)
        feats = (fused_features, seed_3d_features, img_features)
        losses = []
        for head, f in zip(self.pts_bbox_heads, feats):
            feat_dict = dict(seed_points=seeds_3d, seed_features=f, seed_indices=seed_indices)
            preds = head(feat_dict, self.train_cfg["pts"]["sample_mod"])
            losses.append(head.loss(preds, points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask,
                                    pts_instance_mask, img_metas,
                                    gt_bboxes_ignore=gt_bboxes_ignore))
        return losses

    def combine_losses(self, losses_towers):
        """:509-523."""
        combined = dict()
        for term in losses_towers[0]:
            if "loss" in term:
                combined[term] = 0
                for i in range(len(losses_towers)):
                    combined[term] = combined[term] + losses_towers[i][term] * self.loss_weights[i]
            else:
                combined[term] = losses_towers[0][term]
        return combined

    def forward_train(self, points=None, img=None, img_metas=None, calib=None, bboxes_2d=None,
                      gt_bboxes_3d=None, gt_labels_3d=None, pts_semantic_mask=None,
                      pts_instance_mask=None, gt_bboxes_ignore=None, generator=None,
                      drop_generator=None, **kwargs):
        """:445-523 -> the combined loss dict."""
        if points is None:
            raise NotImplementedError("ImVoteNet: the image-only pre-training branch is not built")
        return self.combine_losses(self.tower_losses(
            points, img, img_metas, calib, bboxes_2d, gt_bboxes_3d, gt_labels_3d,
            pts_semantic_mask, pts_instance_mask, gt_bboxes_ignore, generator=generator,
            drop_generator=drop_generator))

    def simple_test(self, points=None, img_metas=None, img=None, calibs=None, bboxes_2d=None,
                    rescale=False, generator=None, **kwargs):
        """:677-716: the joint tower only (bbox3d2result's fields)."""
        bboxes_2d = self.extract_bboxes_2d(img, img_metas, train=False, bboxes_2d=bboxes_2d)
        points = self._stack(points)
        seeds_3d, seed_3d_features, seed_indices = self.extract_pts_feat(points)
        seeds_3d, seed_3d_features, img_features, seed_indices = self.fuse_and_sample(
            img, bboxes_2d, seeds_3d, seed_3d_features, seed_indices, img_metas, calibs,
            generator=generator)
        feat_dict = dict(seed_points=seeds_3d,
                         seed_features=torch.cat([seed_3d_features, img_features], dim=1),
                         seed_indices=seed_indices)
        bbox_preds = self.pts_bbox_head_joint(feat_dict, self.test_cfg["pts"]["sample_mod"])
        bbox_list = self.pts_bbox_head_joint.get_bboxes(points, bbox_preds, img_metas,
                                                        rescale=rescale)
        return [dict(boxes_3d=b, scores_3d=s, labels_3d=l) for b, s, l in bbox_list]

    def forward(self, points, img_metas=None, return_loss=False, **kw):
        if return_loss:
            return self.forward_train(points=points, img_metas=img_metas, **kw)
        return self.simple_test(points=points, img_metas=img_metas, **kw)


_WARNED = {}


def _notice_split_mode(reference_quirks):
    """One line per process and mode, when a detector is built from a config: which
    voxel_modality_split the unchanged reference config gets here (logger `msmdfusion_amd`,
    level INFO; the load-time warning above is the loud one)."""
    key = ("mode", bool(reference_quirks))
    if _WARNED.get(key):
        return
    _WARNED[key] = True
    logging.getLogger("msmdfusion_amd").info(
        "MSMDFusionDetector: reference_quirks=%s -- voxel_modality_split uses %s",
        bool(reference_quirks),
        "the reference's float32 keys and non-cumulative batch offsets (bit for bit the "
        "reference, MSMDFusion.py:251-325)" if reference_quirks else
        "exact integer keys and cumulative batch offsets (differs from the reference where "
        "its float32 keys alias: z >= 17 or x >= 1000 on the scale-1 grid; set "
        "reference_quirks=True in the model config to reproduce the reference)")


@DETECTORS.register_module()
class MSMDFusionDetector(TransFusionDetector):
    """LiDAR + camera detector (configs/MSMDFusion_nusc_voxel_LC.py): the LiDAR encoder's
    four scales meet virtual-point voxels from the image branch in the GMA-Conv stack."""

    def __init__(self, spatial_shapes=None, downscale_factors=None, fps_num_list=None,
                 radius_list=None, max_cluster_samples_list=None, dist_thresh_list=None,
                 multimodal_middle_encoder=None, reference_quirks=False, **kwargs):
        """reference_quirks (config key of the same name, default False): True reproduces
        the reference's float32-key voxel_modality_split and its batch-offset arithmetic bit
        for bit -- the mode that matches a checkpoint trained with the reference
        (fusion.SparseFusionPath)."""
        super().__init__(**kwargs)
        self.reference_quirks = bool(reference_quirks)
        _notice_split_mode(self.reference_quirks)
        from .bev import SPPModule
        from .image_glue import DepthAwareChannelCompression, ScoreNet
        self.spatial_shapes = [list(s) for s in spatial_shapes]
        self.downscale_factors = list(downscale_factors)
        self.fps_num_list = list(fps_num_list)
        self.radius_list = list(radius_list)
        self.max_cluster_samples_list = list(max_cluster_samples_list)
        self.dist_thresh_list = list(dist_thresh_list)
        self.multimodal_middle_encoder = build_middle_encoder(multimodal_middle_encoder)
        # channel compression for ResNet-50 (MSMDFusion.py:106-128): the ModuleList itself is
        # the attribute, as in the reference (keys `conv1x1_blocks.0.0.weight` ...)
        compress = DepthAwareChannelCompression()
        self.conv1x1_blocks = compress.conv1x1_blocks
        object.__setattr__(self, "_compress", compress)      # (unregistered: one set of keys)
        self.score_net = ScoreNet()
        if self.rows:
            from .grid_conv import SPPModuleRows
            self.bev_fusion = SPPModuleRows()
        else:
            self.bev_fusion = SPPModule()
        # one object owns the sparse section's schedule (index pass first, neighbour search on
        # side streams); it holds the SAME child modules, unregistered, to keep one set of keys
        object.__setattr__(self, "_path", SparseFusionPath(
            self.pts_voxel_layer, self.pts_middle_encoder, self.multimodal_middle_encoder,
            self.spatial_shapes, self.downscale_factors, self.fps_num_list, self.radius_list,
            self.max_cluster_samples_list, self.dist_thresh_list,
            base_voxel_size=self.pts_voxel_layer.voxel_size,
            reference_quirks=self.reference_quirks))

    def load_state_dict(self, state_dict, *args, **kwargs):
        """A checkpoint trained with the reference has seen the float32-key split's false
        'mixed' voxels on every frame (MSMDFusion.py:271-272); loading weights into a detector
        built with reference_quirks=False (the exact-key split) runs them on a different voxel
        partition than they were trained with.  Said once per process, at load time."""
        if not self.reference_quirks and not _WARNED.get("load"):
            _WARNED["load"] = True
            warnings.warn(
                "MSMDFusionDetector.load_state_dict: reference_quirks=False -- "
                "voxel_modality_split keys voxels exactly.  A checkpoint trained with the "
                "reference (float32 keys: false 'mixed' voxels wherever keys alias, on every "
                "nuScenes frame at the 0.075 m scale) was trained on a different partition; "
                "build the detector with reference_quirks=True to reproduce it "
                "(INTEGRATION.md, 'Which mode reproduces a published checkpoint').",
                stacklevel=2)
        return super().load_state_dict(state_dict, *args, **kwargs)

    # ---- image side --------------------------------------------------------------------
    def virtual_points_from_images(self, img_feats, img_metas):
        """depth_aware_channel_compression + get_foreground2D per scale
        (MSMDFusion.py:400-407, 169-238) -> 4 lists of B [n, 15 + 49] tensors."""
        from .image_glue import get_foreground2D, pack_foreground, raise_if_any_bad
        pack = pack_foreground(img_metas, img_feats[0].device)
        bad = []       # out-of-map pixel counters of the five kernels: ONE host read below
        comp = self._compress(img_feats, img_metas, pack=pack, check=bad)
        per_scale = [comp[0]] + list(comp)               # img_feat_list[0] twice, :404-405
        out = [get_foreground2D(f, img_metas, self.score_net, pack=pack, check=bad,
                                reference_quirks=self.reference_quirks) for f in per_scale[:4]]
        raise_if_any_bad(bad)
        return out

    # ---- the path ----------------------------------------------------------------------
    def prepare(self, points, virtual_points, nn_side_stream=True):
        vps = virtual_points if isinstance(virtual_points[0], (list, tuple)) else [virtual_points] * 4
        return self._path.prepare(points, vps, nn_side_stream=nn_side_stream)

    def extract_sparse_feat(self, points, virtual_points, prepared=None):
        """MSMDFusion.py:421-440 up to bev_fusion's input: cat([x, x_mm], 1) as ONE
        channels-last map both sparse tensors scatter into."""
        vps = virtual_points if isinstance(virtual_points[0], (list, tuple)) else [virtual_points] * 4
        return self._path(points, vps, prepared=prepared, joint_bev=True)

    def extract_pts_feat(self, pts, img_feats=None, img_metas=None, virtual_points=None,
                         prepared=None):
        """MSMDFusion.py:421-452.  virtual_points: the per-scale foreground points when the
        caller has them already (bench.py, tests); otherwise they come from img_feats."""
        if virtual_points is None:
            if img_feats is None:
                raise ValueError("MSMDFusionDetector needs img_feats + img_metas or virtual_points")
            virtual_points = self.virtual_points_from_images(img_feats, img_metas)
        x = self.bev_fusion(self.extract_sparse_feat(pts, virtual_points, prepared=prepared))
        if self.with_pts_backbone:
            x = self.pts_backbone(x)
        if self.with_pts_neck:
            x = self.pts_neck(x)
        return x if isinstance(x, (list, tuple)) else [x]

    def forward(self, points, virtual_points=None, return_loss=False, prepared=None, **kw):
        if return_loss:
            return self.forward_train(points=points, virtual_points=virtual_points,
                                      prepared=prepared, **kw)
        return self.extract_pts_feat(points, kw.get("img_feats"), kw.get("img_metas"),
                                     virtual_points=virtual_points, prepared=prepared)


def freeze_lidar_components(model):
    """tools/train.py:185-219 (`freeze_lidar_components=True` in the LC config): the voxel
    layer, voxel encoder and LiDAR middle encoder stop training, and their BatchNorms stop
    tracking running statistics (they keep normalising with batch statistics, as the
    reference's `fix_bn` leaves them).  Also freezes the multimodal encoder's two block
    lists its forward never calls (sparse_multimodal_encoder_painting.py:142-156 vs :413-428)
    so that DDP needs no find_unused_parameters.  -> names of the parameters still trained."""
    for name, p in model.named_parameters():
        if any(k in name for k in ("pts_middle_encoder", "pts_voxel_layer", "pts_voxel_encoder")):
            p.requires_grad = False
    for part in (model.pts_voxel_layer, model.pts_voxel_encoder, model.pts_middle_encoder):
        if isinstance(part, nn.Module):
            for m in part.modules():
                if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
                    m.track_running_stats = False
    mm = getattr(model, "multimodal_middle_encoder", None)
    if mm is not None:
        from .distributed import freeze_unused_fusion_blocks
        freeze_unused_fusion_blocks(mm)
    spconv.functional.invalidate_packed_weights()
    return [n for n, p in model.named_parameters() if p.requires_grad]
