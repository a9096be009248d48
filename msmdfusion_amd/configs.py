"""The hot-path sections of the two target model configs, restated.

Reference: configs/MSMDFusion_nusc_voxel_LC.py:141-190 and
configs/transfusion_nusc_voxel_L.py:150-169 (values are facts; equality with the
reference dicts is pinned by tests/golden/reference_configs.json).  Only the
keys this path consumes are kept (plus the dense BEV backbone/neck of row f1);
the image backbone and the detection head are not built here.

    from msmdfusion_amd.configs import MSMDFUSION_LC, build_hot_path
    vox, vfe, enc, mm = build_hot_path(MSMDFUSION_LC)
"""
POINT_CLOUD_RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
VOXEL_SIZE = [0.075, 0.075, 0.2]

_PTS_VOXEL_LAYER = dict(max_num_points=10, voxel_size=VOXEL_SIZE, max_voxels=(120000, 160000),
                        point_cloud_range=POINT_CLOUD_RANGE)
_PTS_VOXEL_ENCODER = dict(type="HardSimpleVFE", num_features=5)
_PTS_MIDDLE_ENCODER = dict(
    type="SparseEncoder", in_channels=5, sparse_shape=[41, 1440, 1440], output_channels=128,
    order=("conv", "norm", "act"),
    encoder_channels=((16, 16, 32), (32, 32, 64), (64, 64, 128), (128, 128)),
    encoder_paddings=((0, 0, 1), (0, 0, 1), (0, 0, [0, 1, 1]), (0, 0)),
    block_type="basicblock")

_BN2D = dict(type="BN", eps=0.001, momentum=0.01)
_PTS_BACKBONE = dict(type="SECOND", in_channels=256, out_channels=[128, 256], layer_nums=[5, 5],
                     layer_strides=[1, 2], norm_cfg=_BN2D,
                     conv_cfg=dict(type="Conv2d", bias=False))
_PTS_NECK = dict(type="SECONDFPN", in_channels=[128, 256], out_channels=[256, 256],
                 upsample_strides=[1, 2], norm_cfg=_BN2D,
                 upsample_cfg=dict(type="deconv", bias=False), use_conv_for_no_stride=True)

_OUT_SIZE_FACTOR = 8
_PTS_BBOX_HEAD = dict(
    type="TransFusionHead", num_proposals=200, auxiliary=True, in_channels=256 * 2,
    hidden_channel=128, num_classes=10, num_decoder_layers=1, num_heads=8,
    learnable_query_pos=False, initialize_by_heatmap=True, nms_kernel_size=3, ffn_channel=256,
    dropout=0.1, bn_momentum=0.1, activation="relu",
    common_heads=dict(center=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2)),
    bbox_coder=dict(type="TransFusionBBoxCoder", pc_range=POINT_CLOUD_RANGE[:2],
                    voxel_size=VOXEL_SIZE[:2], out_size_factor=_OUT_SIZE_FACTOR,
                    post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                    score_threshold=0.0, code_size=10),
    loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2, alpha=0.25, reduction="mean",
                  loss_weight=1.0),
    loss_bbox=dict(type="L1Loss", reduction="mean", loss_weight=0.25),
    loss_heatmap=dict(type="GaussianFocalLoss", reduction="mean", loss_weight=1.0))
# train_cfg.pts of configs/MSMDFusion_nusc_voxel_LC.py:242-259
_TRAIN_CFG_PTS = dict(
    dataset="nuScenes",
    assigner=dict(type="HungarianAssigner3D",
                  iou_calculator=dict(type="BboxOverlaps3D", coordinate="lidar"),
                  cls_cost=dict(type="FocalLossCost", gamma=2, alpha=0.25, weight=0.15),
                  reg_cost=dict(type="BBoxBEVL1Cost", weight=0.25),
                  iou_cost=dict(type="IoU3DCost", weight=0.25)),
    pos_weight=-1, gaussian_overlap=0.1, min_radius=2, grid_size=[1440, 1440, 40],
    voxel_size=VOXEL_SIZE, out_size_factor=_OUT_SIZE_FACTOR,
    code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2],
    point_cloud_range=POINT_CLOUD_RANGE)
_TEST_CFG_PTS = dict(dataset="nuScenes", grid_size=[1440, 1440, 40],
                     out_size_factor=_OUT_SIZE_FACTOR, pc_range=POINT_CLOUD_RANGE[0:2],
                     voxel_size=VOXEL_SIZE[:2], nms_type=None)

TRANSFUSION_L = dict(
    model=dict(type="TransFusionDetector", pts_voxel_layer=_PTS_VOXEL_LAYER,
               pts_voxel_encoder=_PTS_VOXEL_ENCODER, pts_middle_encoder=_PTS_MIDDLE_ENCODER,
               pts_backbone=_PTS_BACKBONE, pts_neck=_PTS_NECK),
    samples_per_gpu=4, point_cloud_range=POINT_CLOUD_RANGE, voxel_size=VOXEL_SIZE,
    optimizer=dict(type="AdamW", lr=0.0002, weight_decay=0.01),
    freeze_lidar_components=False)

MSMDFUSION_LC = dict(
    model=dict(
        type="MSMDFusionDetector",
        spatial_shapes=[[41, 1440, 1440], [21, 720, 720], [11, 360, 360], [5, 180, 180]],
        downscale_factors=[1, 2, 4, 8],
        fps_num_list=[2048] * 4,
        radius_list=[6, 3, 2, 1],
        max_cluster_samples_list=[200, 100, 50, 25],
        dist_thresh_list=[13.3, 6.6, 3.3, 1.6],
        pts_voxel_layer=_PTS_VOXEL_LAYER,
        pts_voxel_encoder=_PTS_VOXEL_ENCODER,
        pts_middle_encoder=_PTS_MIDDLE_ENCODER,
        multimodal_middle_encoder=dict(
            type="SparseMultiModalEncoderPaint", in_channels_3D=(16, 32, 64, 128),
            in_channels_2D=(64, 64, 64, 64), out_channels=(32, 64, 128, 128),
            padding=(1, 1, [0, 1, 1], 0), order=("conv", "norm", "act"),
            norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01)),
        pts_backbone=_PTS_BACKBONE, pts_neck=_PTS_NECK),
    samples_per_gpu=2, point_cloud_range=POINT_CLOUD_RANGE, voxel_size=VOXEL_SIZE,
    optimizer=dict(type="AdamW", lr=0.0001, betas=(0.9, 0.999), weight_decay=0.05,
                   paramwise_cfg=dict(custom_keys={
                       "absolute_pos_embed": dict(decay_mult=0.),
                       "relative_position_bias_table": dict(decay_mult=0.),
                       "norm": dict(decay_mult=0.)})),
    freeze_lidar_components=True)

# configs/transfusion_nusc_pillar_L.py:150-242: the whole `model` dict (head, train_cfg and
# test_cfg included; equality pinned by tests/golden/reference_pillar_config.json)
PILLAR_POINT_CLOUD_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
PILLAR_VOXEL_SIZE = [0.2, 0.2, 8]
_PILLAR_OUT_SIZE_FACTOR = 4
_PILLAR_BN = dict(type="BN", eps=0.001, momentum=0.01)

TRANSFUSION_PILLAR_L = dict(
    model=dict(
        type="TransFusionDetector",
        pts_voxel_layer=dict(max_num_points=20, voxel_size=PILLAR_VOXEL_SIZE,
                             max_voxels=(30000, 60000),
                             point_cloud_range=PILLAR_POINT_CLOUD_RANGE),
        pts_voxel_encoder=dict(type="PillarFeatureNet", in_channels=5, feat_channels=[64],
                               with_distance=False, voxel_size=PILLAR_VOXEL_SIZE,
                               norm_cfg=dict(type="BN1d", eps=0.001, momentum=0.01),
                               point_cloud_range=PILLAR_POINT_CLOUD_RANGE),
        pts_middle_encoder=dict(type="PointPillarsScatter", in_channels=64,
                                output_shape=(512, 512)),
        pts_backbone=dict(type="SECOND", in_channels=64, out_channels=[64, 128, 256],
                          layer_nums=[3, 5, 5], layer_strides=[2, 2, 2], norm_cfg=_PILLAR_BN,
                          conv_cfg=dict(type="Conv2d", bias=False)),
        pts_neck=dict(type="SECONDFPN", in_channels=[64, 128, 256], out_channels=[128, 128, 128],
                      upsample_strides=[0.5, 1, 2], norm_cfg=_PILLAR_BN,
                      upsample_cfg=dict(type="deconv", bias=False), use_conv_for_no_stride=True),
        pts_bbox_head=dict(
            type="TransFusionHead", num_proposals=200, auxiliary=True, in_channels=128 * 3,
            hidden_channel=128, num_classes=10, num_decoder_layers=1, num_heads=8,
            learnable_query_pos=False, initialize_by_heatmap=True, nms_kernel_size=3,
            ffn_channel=256, dropout=0.1, bn_momentum=0.1, activation="relu",
            common_heads=dict(center=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2)),
            bbox_coder=dict(type="TransFusionBBoxCoder", pc_range=PILLAR_POINT_CLOUD_RANGE[:2],
                            voxel_size=PILLAR_VOXEL_SIZE[:2],
                            out_size_factor=_PILLAR_OUT_SIZE_FACTOR,
                            post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                            score_threshold=0.0, code_size=10),
            loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2, alpha=0.25,
                          reduction="mean", loss_weight=1.0),
            loss_bbox=dict(type="L1Loss", reduction="mean", loss_weight=0.25),
            loss_heatmap=dict(type="GaussianFocalLoss", reduction="mean", loss_weight=1.0)),
        train_cfg=dict(pts=dict(
            dataset="nuScenes",
            assigner=dict(type="HungarianAssigner3D",
                          iou_calculator=dict(type="BboxOverlaps3D", coordinate="lidar"),
                          cls_cost=dict(type="FocalLossCost", gamma=2, alpha=0.25, weight=0.15),
                          reg_cost=dict(type="BBoxBEVL1Cost", weight=0.25),
                          iou_cost=dict(type="IoU3DCost", weight=0.25)),
            pos_weight=-1, gaussian_overlap=0.1, min_radius=2, grid_size=[512, 512, 1],
            voxel_size=PILLAR_VOXEL_SIZE, out_size_factor=_PILLAR_OUT_SIZE_FACTOR,
            code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2],
            point_cloud_range=PILLAR_POINT_CLOUD_RANGE)),
        test_cfg=dict(pts=dict(dataset="nuScenes", grid_size=[512, 512, 1],
                               out_size_factor=_PILLAR_OUT_SIZE_FACTOR,
                               pc_range=PILLAR_POINT_CLOUD_RANGE[0:2],
                               voxel_size=PILLAR_VOXEL_SIZE[:2], nms_type=None))),
    samples_per_gpu=2, point_cloud_range=PILLAR_POINT_CLOUD_RANGE, voxel_size=PILLAR_VOXEL_SIZE,
    optimizer=dict(type="AdamW", lr=0.0001, weight_decay=0.01),
    freeze_lidar_components=False)


# configs/transfusion_nusc_voxel_LC.py and transfusion_nusc_pillar_LC.py: the L models with the
# camera branch -- an image backbone and neck (injected here, their dicts kept as facts), and a
# head with fuse_img=True over num_views = 6 views (msmdfusion_amd/fusion_head.py).  Equality
# with the reference dicts is pinned by tests/golden/reference_transfusion_lc_configs.json.
_LC_IMG_BRANCH = dict(
    freeze_img=True,
    img_backbone=dict(type="ResNet", depth=50, num_stages=4, out_indices=(0, 1, 2, 3),
                      frozen_stages=1, norm_cfg=dict(type="BN", requires_grad=True),
                      norm_eval=True, style="pytorch"),
    img_neck=dict(type="FPN", in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5))
_LC_HEAD_IMG = dict(fuse_img=True, num_views=6, in_channels_img=256, out_size_factor_img=4)

TRANSFUSION_VOXEL_LC = dict(
    model=dict(TRANSFUSION_L["model"], **_LC_IMG_BRANCH,
               pts_bbox_head=dict(_PTS_BBOX_HEAD, **_LC_HEAD_IMG),
               train_cfg=dict(pts=_TRAIN_CFG_PTS), test_cfg=dict(pts=_TEST_CFG_PTS)),
    samples_per_gpu=2, point_cloud_range=POINT_CLOUD_RANGE, voxel_size=VOXEL_SIZE,
    optimizer=dict(type="AdamW", lr=0.0001, weight_decay=0.01),
    freeze_lidar_components=True)

TRANSFUSION_PILLAR_LC = dict(
    model=dict(TRANSFUSION_PILLAR_L["model"], **_LC_IMG_BRANCH,
               pts_bbox_head=dict(TRANSFUSION_PILLAR_L["model"]["pts_bbox_head"], **_LC_HEAD_IMG)),
    samples_per_gpu=2, point_cloud_range=PILLAR_POINT_CLOUD_RANGE, voxel_size=PILLAR_VOXEL_SIZE,
    optimizer=dict(type="AdamW", lr=0.0001, weight_decay=0.01),
    freeze_lidar_components=True)


# ---------------------------------------------------------------------------------------------
# CenterPoint (configs/_base_/models/centerpoint_{01voxel,02pillar}_second_secfpn_nus.py under
# configs/centerpoint/*): the `model` dicts after the `_base_` merge.  VOXEL: the 0.075 m
# voxel chain with circle NMS (centerpoint_0075voxel_second_secfpn_circlenms_4x8_cyclic_20e_nus
# .py); PILLAR: centerpoint_02pillar_second_secfpn_4x8_cyclic_20e_nus.py (rotated NMS).
# tests/golden/reference_centerpoint_configs.json holds the reference's values.
# NOTE: this fork's CenterHead.get_targets_single reads train_cfg['pc_range'], which these
# stock dicts do not carry (they carry point_cloud_range): add it before training, as the
# fork's own MSMD_centerpoint_* configs do.
_CENTERPOINT_TASKS = [
    dict(num_class=1, class_names=["car"]),
    dict(num_class=2, class_names=["truck", "construction_vehicle"]),
    dict(num_class=2, class_names=["bus", "trailer"]),
    dict(num_class=1, class_names=["barrier"]),
    dict(num_class=2, class_names=["motorcycle", "bicycle"]),
    dict(num_class=2, class_names=["pedestrian", "traffic_cone"])]
_CENTERPOINT_BN = dict(type="BN", eps=0.001, momentum=0.01)


def _centerpoint_head(in_channels, out_size_factor, voxel_size, pc_range):
    return dict(
        type="CenterHead", in_channels=in_channels, tasks=_CENTERPOINT_TASKS,
        common_heads=dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2)),
        share_conv_channel=64,
        bbox_coder=dict(type="CenterPointBBoxCoder",
                        post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_num=500,
                        score_threshold=0.1, out_size_factor=out_size_factor,
                        voxel_size=voxel_size[:2], pc_range=pc_range[:2], code_size=9),
        separate_head=dict(type="SeparateHead", init_bias=-2.19, final_kernel=3),
        loss_cls=dict(type="GaussianFocalLoss", reduction="mean"),
        loss_bbox=dict(type="L1Loss", reduction="mean", loss_weight=0.25), norm_bbox=True)


def _centerpoint_cfgs(grid_size, out_size_factor, voxel_size, pc_range, nms_type):
    train = dict(pts=dict(grid_size=grid_size, voxel_size=voxel_size,
                          out_size_factor=out_size_factor, dense_reg=1, gaussian_overlap=0.1,
                          max_objs=500, min_radius=2,
                          code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2],
                          point_cloud_range=pc_range))
    test = dict(pts=dict(post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                         max_per_img=500, max_pool_nms=False,
                         min_radius=[4, 12, 10, 1, 0.85, 0.175], score_threshold=0.1,
                         out_size_factor=out_size_factor, voxel_size=voxel_size[:2],
                         pc_range=pc_range[:2], nms_type=nms_type, pre_max_size=1000,
                         post_max_size=83, nms_thr=0.2))
    return train, test


_CP_VOXEL_SIZE, _CP_VOXEL_RANGE = [0.075, 0.075, 0.2], [-54, -54, -5.0, 54, 54, 3.0]
_CP_VOXEL_TRAIN, _CP_VOXEL_TEST = _centerpoint_cfgs([1440, 1440, 40], 8, _CP_VOXEL_SIZE,
                                                    _CP_VOXEL_RANGE, "circle")
CENTERPOINT_VOXEL_NUS = dict(model=dict(
    type="CenterPoint",
    pts_voxel_layer=dict(max_num_points=10, voxel_size=_CP_VOXEL_SIZE, max_voxels=(90000, 120000),
                         point_cloud_range=_CP_VOXEL_RANGE),
    pts_voxel_encoder=dict(type="HardSimpleVFE", num_features=5),
    pts_middle_encoder=dict(
        type="SparseEncoder", in_channels=5, sparse_shape=[41, 1440, 1440], output_channels=128,
        order=("conv", "norm", "act"),
        encoder_channels=((16, 16, 32), (32, 32, 64), (64, 64, 128), (128, 128)),
        encoder_paddings=((0, 0, 1), (0, 0, 1), (0, 0, [0, 1, 1]), (0, 0)),
        block_type="basicblock"),
    pts_backbone=dict(type="SECOND", in_channels=256, out_channels=[128, 256], layer_nums=[5, 5],
                      layer_strides=[1, 2], norm_cfg=_CENTERPOINT_BN,
                      conv_cfg=dict(type="Conv2d", bias=False)),
    pts_neck=dict(type="SECONDFPN", in_channels=[128, 256], out_channels=[256, 256],
                  upsample_strides=[1, 2], norm_cfg=_CENTERPOINT_BN,
                  upsample_cfg=dict(type="deconv", bias=False), use_conv_for_no_stride=True),
    pts_bbox_head=_centerpoint_head(512, 8, _CP_VOXEL_SIZE, _CP_VOXEL_RANGE),
    train_cfg=_CP_VOXEL_TRAIN, test_cfg=_CP_VOXEL_TEST))

_CP_PILLAR_TRAIN, _CP_PILLAR_TEST = _centerpoint_cfgs([512, 512, 1], 4, PILLAR_VOXEL_SIZE,
                                                      PILLAR_POINT_CLOUD_RANGE, "rotate")
CENTERPOINT_PILLAR_NUS = dict(model=dict(
    type="CenterPoint",
    pts_voxel_layer=dict(max_num_points=20, voxel_size=PILLAR_VOXEL_SIZE,
                         max_voxels=(30000, 40000), point_cloud_range=PILLAR_POINT_CLOUD_RANGE),
    pts_voxel_encoder=dict(type="PillarFeatureNet", in_channels=5, feat_channels=[64],
                           with_distance=False, voxel_size=(0.2, 0.2, 8),
                           norm_cfg=dict(type="BN1d", eps=0.001, momentum=0.01), legacy=False,
                           point_cloud_range=PILLAR_POINT_CLOUD_RANGE),
    pts_middle_encoder=dict(type="PointPillarsScatter", in_channels=64, output_shape=(512, 512)),
    pts_backbone=dict(type="SECOND", in_channels=64, out_channels=[64, 128, 256],
                      layer_nums=[3, 5, 5], layer_strides=[2, 2, 2], norm_cfg=_CENTERPOINT_BN,
                      conv_cfg=dict(type="Conv2d", bias=False)),
    pts_neck=dict(type="SECONDFPN", in_channels=[64, 128, 256], out_channels=[128, 128, 128],
                  upsample_strides=[0.5, 1, 2], norm_cfg=_CENTERPOINT_BN,
                  upsample_cfg=dict(type="deconv", bias=False), use_conv_for_no_stride=True),
    pts_bbox_head=_centerpoint_head(384, 4, PILLAR_VOXEL_SIZE, PILLAR_POINT_CLOUD_RANGE),
    train_cfg=_CP_PILLAR_TRAIN, test_cfg=_CP_PILLAR_TEST))


# ---------------------------------------------------------------------------------------------
# PointPillars and SECOND on KITTI (configs/_base_/models/hv_pointpillars_secfpn_kitti.py and
# hv_second_secfpn_kitti.py, the bases of every configs/pointpillars/*kitti* and
# configs/second/*kitti* file): VoxelNet with Anchor3DHead, three classes (Pedestrian, Cyclist,
# Car), one MaxIoUAssigner per anchor size.  tests/golden/reference_anchor_head_configs.json
# holds the reference's values.
def _kitti_assigner(pos_iou_thr, neg_iou_thr):
    return dict(type="MaxIoUAssigner", iou_calculator=dict(type="BboxOverlapsNearest3D"),
                pos_iou_thr=pos_iou_thr, neg_iou_thr=neg_iou_thr, min_pos_iou=neg_iou_thr,
                ignore_iof_thr=-1)


def _kitti_anchor_head(channels, y_range):
    return dict(
        type="Anchor3DHead", num_classes=3, in_channels=channels, feat_channels=channels,
        use_direction_classifier=True,
        anchor_generator=dict(
            type="Anchor3DRangeGenerator",
            ranges=[[0, -y_range, -0.6, 70.4, y_range, -0.6],
                    [0, -y_range, -0.6, 70.4, y_range, -0.6],
                    [0, -y_range, -1.78, 70.4, y_range, -1.78]],
            sizes=[[0.6, 0.8, 1.73], [0.6, 1.76, 1.73], [1.6, 3.9, 1.56]],
            rotations=[0, 1.57], reshape_out=False),
        diff_rad_by_sin=True, bbox_coder=dict(type="DeltaXYZWLHRBBoxCoder"),
        loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
        loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=2.0),
        loss_dir=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.2))


def _kitti_cfgs(small_pos, small_neg):
    train = dict(assigner=[_kitti_assigner(small_pos, small_neg),      # Pedestrian
                           _kitti_assigner(small_pos, small_neg),      # Cyclist
                           _kitti_assigner(0.6, 0.45)],                # Car
                 allowed_border=0, pos_weight=-1, debug=False)
    test = dict(use_rotate_nms=True, nms_across_levels=False, nms_thr=0.01, score_thr=0.1,
                min_bbox_size=0, nms_pre=100, max_num=50)
    return train, test


_KITTI_PILLAR_VOXEL, _KITTI_PILLAR_RANGE = [0.16, 0.16, 4], [0, -39.68, -3, 69.12, 39.68, 1]
_KITTI_PILLAR_TRAIN, _KITTI_PILLAR_TEST = _kitti_cfgs(0.5, 0.35)
POINTPILLARS_SECFPN_KITTI = dict(model=dict(
    type="VoxelNet",
    voxel_layer=dict(max_num_points=32, point_cloud_range=_KITTI_PILLAR_RANGE,
                     voxel_size=_KITTI_PILLAR_VOXEL, max_voxels=(16000, 40000)),
    voxel_encoder=dict(type="PillarFeatureNet", in_channels=4, feat_channels=[64],
                       with_distance=False, voxel_size=_KITTI_PILLAR_VOXEL,
                       point_cloud_range=_KITTI_PILLAR_RANGE),
    middle_encoder=dict(type="PointPillarsScatter", in_channels=64, output_shape=[496, 432]),
    backbone=dict(type="SECOND", in_channels=64, layer_nums=[3, 5, 5], layer_strides=[2, 2, 2],
                  out_channels=[64, 128, 256]),
    neck=dict(type="SECONDFPN", in_channels=[64, 128, 256], upsample_strides=[1, 2, 4],
              out_channels=[128, 128, 128]),
    bbox_head=_kitti_anchor_head(384, 39.68),
    train_cfg=_KITTI_PILLAR_TRAIN, test_cfg=_KITTI_PILLAR_TEST))

_KITTI_SECOND_TRAIN, _KITTI_SECOND_TEST = _kitti_cfgs(0.35, 0.2)
SECOND_SECFPN_KITTI = dict(model=dict(
    type="VoxelNet",
    voxel_layer=dict(max_num_points=5, point_cloud_range=[0, -40, -3, 70.4, 40, 1],
                     voxel_size=[0.05, 0.05, 0.1], max_voxels=(16000, 40000)),
    voxel_encoder=dict(type="HardSimpleVFE"),
    middle_encoder=dict(type="SparseEncoder", in_channels=4, sparse_shape=[41, 1600, 1408],
                        order=("conv", "norm", "act")),
    backbone=dict(type="SECOND", in_channels=256, layer_nums=[5, 5], layer_strides=[1, 2],
                  out_channels=[128, 256]),
    neck=dict(type="SECONDFPN", in_channels=[128, 256], upsample_strides=[1, 2],
              out_channels=[256, 256]),
    bbox_head=_kitti_anchor_head(512, 40.0),
    train_cfg=_KITTI_SECOND_TRAIN, test_cfg=_KITTI_SECOND_TEST))


# ---------------------------------------------------------------------------------------------
# VoteNet (configs/_base_/models/votenet.py under configs/votenet/votenet_16x8_sunrgbd-3d-10class.py
# and votenet_8x8_scannet-3d-18class.py): PointNet2SASSG + VoteHead.  SUN RGB-D boxes carry a
# yaw (12 direction bins, box-form vote targets); ScanNet boxes are axis-aligned (one bin,
# instance-mask vote targets).  tests/golden/reference_votenet_configs.json holds the reference's
# values.
_SUNRGBD_MEAN_SIZES = [
    [2.114256, 1.620300, 0.927272], [0.791118, 1.279516, 0.718182], [0.923508, 1.867419, 0.845495],
    [0.591958, 0.552978, 0.827272], [0.699104, 0.454178, 0.75625], [0.69519, 1.346299, 0.736364],
    [0.528526, 1.002642, 1.172878], [0.500618, 0.632163, 0.683424], [0.404671, 1.071108, 1.688889],
    [0.76584, 1.398258, 0.472728]]
_SCANNET_MEAN_SIZES = [
    [0.76966727, 0.8116021, 0.92573744], [1.876858, 1.8425595, 1.1931566],
    [0.61328, 0.6148609, 0.7182701], [1.3955007, 1.5121545, 0.83443564],
    [0.97949594, 1.0675149, 0.6329687], [0.531663, 0.5955577, 1.7500148],
    [0.9624706, 0.72462326, 1.1481868], [0.83221924, 1.0490936, 1.6875663],
    [0.21132214, 0.4206159, 0.5372846], [1.4440073, 1.8970833, 0.26985747],
    [1.0294262, 1.4040797, 0.87554324], [1.3766412, 0.65521795, 1.6813129],
    [0.6650819, 0.71111923, 1.298853], [0.41999173, 0.37906948, 1.7513971],
    [0.59359556, 0.5912492, 0.73919016], [0.50867593, 0.50656086, 0.30136237],
    [1.1511526, 1.0546296, 0.49706793], [0.47535285, 0.49249494, 0.5802117]]


def _votenet(num_classes, num_dir_bins, with_rot, mean_sizes):
    return dict(model=dict(
        type="VoteNet",
        backbone=dict(
            type="PointNet2SASSG", in_channels=4, num_points=(2048, 1024, 512, 256),
            radius=(0.2, 0.4, 0.8, 1.2), num_samples=(64, 32, 16, 16),
            sa_channels=((64, 64, 128), (128, 128, 256), (128, 128, 256), (128, 128, 256)),
            fp_channels=((256, 256), (256, 256)), norm_cfg=dict(type="BN2d"),
            sa_cfg=dict(type="PointSAModule", pool_mod="max", use_xyz=True, normalize_xyz=True)),
        bbox_head=dict(
            type="VoteHead",
            vote_module_cfg=dict(
                in_channels=256, vote_per_seed=1, gt_per_seed=3, conv_channels=(256, 256),
                conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d"), norm_feats=True,
                vote_loss=dict(type="ChamferDistance", mode="l1", reduction="none",
                               loss_dst_weight=10.0)),
            vote_aggregation_cfg=dict(
                type="PointSAModule", num_point=256, radius=0.3, num_sample=16,
                mlp_channels=[256, 128, 128, 128], use_xyz=True, normalize_xyz=True),
            pred_layer_cfg=dict(in_channels=128, shared_conv_channels=(128, 128), bias=True),
            conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d"),
            objectness_loss=dict(type="CrossEntropyLoss", class_weight=[0.2, 0.8],
                                 reduction="sum", loss_weight=5.0),
            center_loss=dict(type="ChamferDistance", mode="l2", reduction="sum",
                             loss_src_weight=10.0, loss_dst_weight=10.0),
            dir_class_loss=dict(type="CrossEntropyLoss", reduction="sum", loss_weight=1.0),
            dir_res_loss=dict(type="SmoothL1Loss", reduction="sum", loss_weight=10.0),
            size_class_loss=dict(type="CrossEntropyLoss", reduction="sum", loss_weight=1.0),
            size_res_loss=dict(type="SmoothL1Loss", reduction="sum", loss_weight=10.0 / 3.0),
            semantic_loss=dict(type="CrossEntropyLoss", reduction="sum", loss_weight=1.0),
            num_classes=num_classes,
            bbox_coder=dict(type="PartialBinBasedBBoxCoder", num_sizes=num_classes,
                            num_dir_bins=num_dir_bins, with_rot=with_rot, mean_sizes=mean_sizes)),
        train_cfg=dict(pos_distance_thr=0.3, neg_distance_thr=0.6, sample_mod="vote"),
        test_cfg=dict(sample_mod="seed", nms_thr=0.25, score_thr=0.05, per_class_proposal=True)))


VOTENET_SUNRGBD = _votenet(10, 12, True, _SUNRGBD_MEAN_SIZES)
VOTENET_SCANNET = _votenet(18, 1, False, _SCANNET_MEAN_SIZES)


# ---------------------------------------------------------------------------------------------
# configs/imvotenet/imvotenet_stage2_16x8_sunrgbd-3d-10class.py (type 'ImVoteNet' from its base
# configs/_base_/models/imvotenet_image.py): VoteNet's backbone, VoteFusion and three VoteHead
# towers.  The image branch keys of the base (img_backbone, img_neck, img_rpn_head,
# img_roi_head and their train / test settings) are left out: the 2-D detector is injected.
# tests/golden/reference_imvotenet_config.json holds the reference's values.
def _imvotenet_tower(in_channels, conv_channels):
    vote = _votenet(10, 12, True, _SUNRGBD_MEAN_SIZES)["model"]["bbox_head"]
    return dict(
        vote_module_cfg=dict(vote["vote_module_cfg"], in_channels=in_channels,
                             conv_channels=conv_channels),
        vote_aggregation_cfg=dict(vote["vote_aggregation_cfg"],
                                  mlp_channels=[in_channels, 128, 128, 128]))


def _imvotenet_stage2():
    vote = _votenet(10, 12, True, _SUNRGBD_MEAN_SIZES)["model"]
    common = {k: v for k, v in vote["bbox_head"].items()
              if k not in ("vote_module_cfg", "vote_aggregation_cfg")}
    return dict(model=dict(
        type="ImVoteNet",
        pts_backbone=vote["backbone"],
        pts_bbox_heads=dict(common=common, joint=_imvotenet_tower(512, (512, 256)),
                            pts=_imvotenet_tower(256, (256, 256)),
                            img=_imvotenet_tower(256, (256, 256)), loss_weights=[0.4, 0.3, 0.3]),
        img_mlp=dict(in_channel=18, conv_channels=(256, 256), conv_cfg=dict(type="Conv1d"),
                     norm_cfg=dict(type="BN1d"), act_cfg=dict(type="ReLU")),
        fusion_layer=dict(type="VoteFusion", num_classes=10, max_imvote_per_pixel=3),
        num_sampled_seed=1024, freeze_img_branch=True,
        train_cfg=dict(pts=dict(pos_distance_thr=0.3, neg_distance_thr=0.6, sample_mod="vote")),
        test_cfg=dict(pts=dict(sample_mod="seed", nms_thr=0.25, score_thr=0.05,
                               per_class_proposal=True))))


IMVOTENET_STAGE2_SUNRGBD = _imvotenet_stage2()


# ---------------------------------------------------------------------------------------------
# 3DSSD (configs/_base_/models/3dssd.py under configs/3dssd/3dssd_kitti-3d-car.py):
# PointNet2SAMSG + SSD3DHead, one class.  tests/golden/reference_3dssd_config.json holds the
# reference's values.
_SSD3D_BN1D = dict(type="BN1d", eps=1e-3, momentum=0.1)
_SSD3D_BN2D = dict(type="BN2d", eps=1e-3, momentum=0.1)
_SSD3D_SUM = dict(type="SmoothL1Loss", reduction="sum", loss_weight=1.0)
SSD3D_KITTI_CAR = dict(model=dict(
    type="SSD3DNet",
    backbone=dict(
        type="PointNet2SAMSG", in_channels=4, num_points=(4096, 512, (256, 256)),
        radii=((0.2, 0.4, 0.8), (0.4, 0.8, 1.6), (1.6, 3.2, 4.8)),
        num_samples=((32, 32, 64), (32, 32, 64), (32, 32, 32)),
        sa_channels=(((16, 16, 32), (16, 16, 32), (32, 32, 64)),
                     ((64, 64, 128), (64, 64, 128), (64, 96, 128)),
                     ((128, 128, 256), (128, 192, 256), (128, 256, 256))),
        aggregation_channels=(64, 128, 256),
        fps_mods=(("D-FPS"), ("FS"), ("F-FPS", "D-FPS")),
        fps_sample_range_lists=((-1), (-1), (512, -1)),
        norm_cfg=dict(_SSD3D_BN2D),
        sa_cfg=dict(type="PointSAModuleMSG", pool_mod="max", use_xyz=True, normalize_xyz=False)),
    bbox_head=dict(
        type="SSD3DHead", in_channels=256,
        vote_module_cfg=dict(
            in_channels=256, num_points=256, gt_per_seed=1, conv_channels=(128,),
            conv_cfg=dict(type="Conv1d"), norm_cfg=dict(_SSD3D_BN1D), with_res_feat=False,
            vote_xyz_range=(3.0, 3.0, 2.0)),
        vote_aggregation_cfg=dict(
            type="PointSAModuleMSG", num_point=256, radii=(4.8, 6.4), sample_nums=(16, 32),
            mlp_channels=((256, 256, 256, 512), (256, 256, 512, 1024)),
            norm_cfg=dict(_SSD3D_BN2D), use_xyz=True, normalize_xyz=False, bias=True),
        pred_layer_cfg=dict(
            in_channels=1536, shared_conv_channels=(512, 128), cls_conv_channels=(128,),
            reg_conv_channels=(128,), conv_cfg=dict(type="Conv1d"), norm_cfg=dict(_SSD3D_BN1D),
            bias=True),
        conv_cfg=dict(type="Conv1d"), norm_cfg=dict(_SSD3D_BN1D),
        objectness_loss=dict(type="CrossEntropyLoss", use_sigmoid=True, reduction="sum",
                             loss_weight=1.0),
        center_loss=dict(_SSD3D_SUM), dir_class_loss=dict(type="CrossEntropyLoss",
                                                          reduction="sum", loss_weight=1.0),
        dir_res_loss=dict(_SSD3D_SUM), size_res_loss=dict(_SSD3D_SUM),
        corner_loss=dict(_SSD3D_SUM), vote_loss=dict(_SSD3D_SUM),
        num_classes=1,
        bbox_coder=dict(type="AnchorFreeBBoxCoder", num_dir_bins=12, with_rot=True)),
    train_cfg=dict(sample_mod="spec", pos_distance_thr=10.0, expand_dims_length=0.05),
    test_cfg=dict(nms_cfg=dict(type="nms", iou_thr=0.1), sample_mod="spec", score_thr=0.0,
                  per_class_proposal=True, max_output_num=100)))


def build_hot_path(cfg):
    """(Voxelization, voxel encoder, SparseEncoder, multimodal encoder | None) from one of
    the dicts above -- what MSMDFusionDetector.__init__ / MVXTwoStageDetector.__init__ build
    for this path (mmdet3d/models/detectors/mvx_two_stage.py:38-60, MSMDFusion.py:92-104)."""
    from .registry import build_middle_encoder, build_voxel_encoder
    from .voxelize import Voxelization
    m = cfg["model"]
    vox = Voxelization(**m["pts_voxel_layer"])
    vfe = build_voxel_encoder(m["pts_voxel_encoder"])
    enc = build_middle_encoder(m["pts_middle_encoder"])
    mm = build_middle_encoder(m["multimodal_middle_encoder"]) \
        if "multimodal_middle_encoder" in m else None
    return vox, vfe, enc, mm


def build_bev_tail(cfg, compute_dtype=None, rows=True):
    """bev_fusion (SPPModule, built without a config: MSMDFusion.py:130) +
    pts_backbone + pts_neck of one of the dicts above.  rows=True (default): the same
    modules, same parameters and checkpoint keys, computed on channels-last pixel rows by
    the sparse-conv kernels (grid_conv.py: fp32-equivalent, 1.7x MIOpen's fp32 on the SPP
    block); rows=False: MIOpen, optionally under bf16 autocast (compute_dtype)."""
    from .bev import BevTail, SPPModule
    from .registry import build_backbone, build_neck
    m = cfg["model"]
    if not rows:
        return BevTail(SPPModule(), build_backbone(m["pts_backbone"]),
                       build_neck(m["pts_neck"]), compute_dtype=compute_dtype)
    from .grid_conv import SECONDFPNRows, SECONDRows, SPPModuleRows

    def args(d):
        return {k: v for k, v in d.items() if k != "type"}
    return BevTail(SPPModuleRows(), SECONDRows(**args(m["pts_backbone"])),
                   SECONDFPNRows(**args(m["pts_neck"])), compute_dtype=None)


def build_head(cfg=None, rows=False):
    """pts_bbox_head of configs/MSMDFusion_nusc_voxel_LC.py:207-241 with its test_cfg
    (:260-268) and train_cfg (:242-259): TransFusionHead, LiDAR branch (msmdfusion_amd/head.py,
    head_loss.py).  cfg: one of the dicts above; one whose model carries `pts_bbox_head`,
    `train_cfg` and `test_cfg` (TRANSFUSION_PILLAR_L) gets its own head, and a head dict with
    fuse_img=True (TRANSFUSION_VOXEL_LC, TRANSFUSION_PILLAR_LC) builds TransFusionHeadLC
    (msmdfusion_amd/fusion_head.py)."""
    from .head import TransFusionHead
    if cfg is not None and "pts_bbox_head" in cfg.get("model", {}):
        # a config that carries its own head (TRANSFUSION_PILLAR_L): its dicts, not the LC ones
        m = cfg["model"]
        args = {k: v for k, v in m["pts_bbox_head"].items() if k != "type"}
        if args.get("fuse_img"):
            from .fusion_head import TransFusionHeadLC
            return TransFusionHeadLC(test_cfg=dict(m["test_cfg"]["pts"]),
                                     train_cfg=dict(m["train_cfg"]["pts"]), rows=rows, **args)
        return TransFusionHead(test_cfg=dict(m["test_cfg"]["pts"]),
                               train_cfg=dict(m["train_cfg"]["pts"]), rows=rows, **args)
    args = {k: v for k, v in _PTS_BBOX_HEAD.items() if k != "type"}
    return TransFusionHead(test_cfg=dict(_TEST_CFG_PTS), train_cfg=dict(_TRAIN_CFG_PTS), rows=rows,
                           **args)


# ---------------------------------------------------------------------------------------------
# FreeAnchor (configs/free_anchor/hv_pointpillars_fpn_sbn-all_free-anchor_4x8_2x_nus-3d.py): the
# `pts_bbox_head` that file puts in place of the base model's (its `_delete_=True` is a merge
# directive, not a value) and the `train_cfg` it adds.  Ten classes, three FPN levels, eight
# anchors per cell, code size 9.  The model it is merged into is POINTPILLARS_FPN_NUS below
# (FREE_ANCHOR_POINTPILLARS_FPN_NUS is the merged result).
# tests/golden/reference_free_anchor_config.json holds the reference's values.
FREE_ANCHOR_HEAD_NUS = dict(
    type="FreeAnchor3DHead", num_classes=10, in_channels=256, feat_channels=256,
    use_direction_classifier=True, pre_anchor_topk=25, bbox_thr=0.5, gamma=2.0, alpha=0.5,
    anchor_generator=dict(
        type="AlignedAnchor3DRangeGenerator", ranges=[[-50, -50, -1.8, 50, 50, -1.8]],
        scales=[1, 2, 4],
        sizes=[[0.8660, 2.5981, 1.0], [0.5774, 1.7321, 1.0], [1.0, 1.0, 1.0], [0.4, 0.4, 1]],
        custom_values=[0, 0], rotations=[0, 1.57], reshape_out=True),
    assigner_per_size=False, diff_rad_by_sin=True, dir_offset=0.7854, dir_limit_offset=0,
    bbox_coder=dict(type="DeltaXYZWLHRBBoxCoder", code_size=9),
    loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
    loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=0.8),
    loss_dir=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.2))
FREE_ANCHOR_TRAIN_CFG_NUS = dict(
    pts=dict(code_weight=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.25, 0.25]))


# ---------------------------------------------------------------------------------------------
# nuScenes PointPillars with an FPN neck (configs/_base_/models/hv_pointpillars_fpn_nus.py):
# hard voxelization (64 points per 0.25 m pillar) -> HardVFE (two VFELayers, 64 wide) ->
# PointPillarsScatter -> SECOND -> FPN -> Anchor3DHead on three levels, as MVXFasterRCNN.
# tests/golden/reference_pointpillars_fpn_configs.json holds the reference's values.
_FPN_NUS_VOXEL_SIZE = [0.25, 0.25, 8]
_FPN_NUS_RANGE = [-50, -50, -5, 50, 50, 3]
POINTPILLARS_FPN_NUS = dict(
    type="MVXFasterRCNN",
    pts_voxel_layer=dict(max_num_points=64, point_cloud_range=_FPN_NUS_RANGE,
                         voxel_size=_FPN_NUS_VOXEL_SIZE, max_voxels=(30000, 40000)),
    pts_voxel_encoder=dict(
        type="HardVFE", in_channels=4, feat_channels=[64, 64], with_distance=False,
        voxel_size=_FPN_NUS_VOXEL_SIZE, with_cluster_center=True, with_voxel_center=True,
        point_cloud_range=_FPN_NUS_RANGE,
        norm_cfg=dict(type="naiveSyncBN1d", eps=1e-3, momentum=0.01)),
    pts_middle_encoder=dict(type="PointPillarsScatter", in_channels=64, output_shape=[400, 400]),
    pts_backbone=dict(
        type="SECOND", in_channels=64,
        norm_cfg=dict(type="naiveSyncBN2d", eps=1e-3, momentum=0.01), layer_nums=[3, 5, 5],
        layer_strides=[2, 2, 2], out_channels=[64, 128, 256]),
    pts_neck=dict(
        type="FPN", norm_cfg=dict(type="naiveSyncBN2d", eps=1e-3, momentum=0.01),
        act_cfg=dict(type="ReLU"), in_channels=[64, 128, 256], out_channels=256, start_level=0,
        num_outs=3),
    pts_bbox_head=dict(
        type="Anchor3DHead", num_classes=10, in_channels=256, feat_channels=256,
        use_direction_classifier=True,
        anchor_generator=dict(
            type="AlignedAnchor3DRangeGenerator", ranges=[[-50, -50, -1.8, 50, 50, -1.8]],
            scales=[1, 2, 4],
            sizes=[[0.8660, 2.5981, 1.0], [0.5774, 1.7321, 1.0], [1.0, 1.0, 1.0], [0.4, 0.4, 1]],
            custom_values=[0, 0], rotations=[0, 1.57], reshape_out=True),
        assigner_per_size=False, diff_rad_by_sin=True, dir_offset=0.7854, dir_limit_offset=0,
        bbox_coder=dict(type="DeltaXYZWLHRBBoxCoder", code_size=9),
        loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
        loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=1.0),
        loss_dir=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.2)),
    train_cfg=dict(pts=dict(
        assigner=dict(type="MaxIoUAssigner", iou_calculator=dict(type="BboxOverlapsNearest3D"),
                      pos_iou_thr=0.6, neg_iou_thr=0.3, min_pos_iou=0.3, ignore_iof_thr=-1),
        allowed_border=0, code_weight=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2],
        pos_weight=-1, debug=False)),
    test_cfg=dict(pts=dict(use_rotate_nms=True, nms_across_levels=False, nms_pre=1000,
                           nms_thr=0.2, score_thr=0.05, min_bbox_size=0, max_num=500)))

# configs/free_anchor/hv_pointpillars_fpn_sbn-all_free-anchor_4x8_2x_nus-3d.py merged over it as
# mmcv's Config does: `pts_bbox_head` replaced (`_delete_=True`), `train_cfg.pts` updated key
# by key.
FREE_ANCHOR_POINTPILLARS_FPN_NUS = dict(
    POINTPILLARS_FPN_NUS, pts_bbox_head=FREE_ANCHOR_HEAD_NUS,
    train_cfg=dict(pts=dict(POINTPILLARS_FPN_NUS["train_cfg"]["pts"],
                            **FREE_ANCHOR_TRAIN_CFG_NUS["pts"])))


# ---------------------------------------------------------------------------------------------
# MVX-Net on KITTI with dynamic voxelization
# (configs/mvxnet/dv_mvx-fpn_second_secfpn_adamw_2x8_80e_kitti-3d-3class.py): dynamic
# voxelization -> DynamicVFE with PointFusion over five image levels -> SparseEncoder -> SECOND
# -> SECONDFPN -> Anchor3DHead, as DynamicMVXFasterRCNN.  The image backbone and neck (ResNet-50
# + FPN with five outputs) are injected, as for MSMDFUSION_LC: their entries are left out.
# tests/golden/reference_mvxnet_config.json holds the reference's values.
_MVX_VOXEL_SIZE, _MVX_RANGE = [0.05, 0.05, 0.1], [0, -40, -3, 70.4, 40, 1]
_MVX_TRAIN, _MVX_TEST = _kitti_cfgs(0.35, 0.2)
MVXNET_DV_SECOND_KITTI = dict(
    type="DynamicMVXFasterRCNN",
    pts_voxel_layer=dict(max_num_points=-1, point_cloud_range=_MVX_RANGE,
                         voxel_size=_MVX_VOXEL_SIZE, max_voxels=(-1, -1)),
    pts_voxel_encoder=dict(
        type="DynamicVFE", in_channels=4, feat_channels=[64, 64], with_distance=False,
        voxel_size=_MVX_VOXEL_SIZE, with_cluster_center=True, with_voxel_center=True,
        point_cloud_range=_MVX_RANGE,
        fusion_layer=dict(type="PointFusion", img_channels=256, pts_channels=64,
                          mid_channels=128, out_channels=128, img_levels=[0, 1, 2, 3, 4],
                          align_corners=False, activate_out=True, fuse_out=False)),
    pts_middle_encoder=dict(type="SparseEncoder", in_channels=128, sparse_shape=[41, 1600, 1408],
                            order=("conv", "norm", "act")),
    pts_backbone=dict(type="SECOND", in_channels=256, layer_nums=[5, 5], layer_strides=[1, 2],
                      out_channels=[128, 256]),
    pts_neck=dict(type="SECONDFPN", in_channels=[128, 256], upsample_strides=[1, 2],
                  out_channels=[256, 256]),
    pts_bbox_head=dict(_kitti_anchor_head(512, 40.0), assigner_per_size=True,
                       assign_per_class=True),
    train_cfg=dict(pts=_MVX_TRAIN), test_cfg=dict(pts=_MVX_TEST))


# ------------------------------------------------------------------------------- H3DNet (front)
# configs/_base_/models/h3dnet.py: the four-stream backbone and the three primitive heads of
# the ScanNet model (H3DNET_SCANNET below is the whole model)
H3DNET_SCANNET_BACKBONE = dict(
    type="MultiBackbone", num_streams=4, suffixes=["net0", "net1", "net2", "net3"],
    conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d", eps=1e-5, momentum=0.01),
    act_cfg=dict(type="ReLU"),
    backbones=dict(
        type="PointNet2SASSG", in_channels=4, num_points=(2048, 1024, 512, 256),
        radius=(0.2, 0.4, 0.8, 1.2), num_samples=(64, 32, 16, 16),
        sa_channels=((64, 64, 128), (128, 128, 256), (128, 128, 256), (128, 128, 256)),
        fp_channels=((256, 256), (256, 256)), norm_cfg=dict(type="BN2d"),
        sa_cfg=dict(type="PointSAModule", pool_mod="max", use_xyz=True, normalize_xyz=True)))


def _h3dnet_primitive(mode, num_dims, side_weight, sem_weight):
    chamfer = dict(type="ChamferDistance", mode="l1", reduction="sum",
                   loss_src_weight=side_weight, loss_dst_weight=side_weight)
    return dict(
        type="PrimitiveHead", num_dims=num_dims, num_classes=18, primitive_mode=mode,
        upper_thresh=100.0, surface_thresh=0.5,
        vote_module_cfg=dict(
            in_channels=256, vote_per_seed=1, gt_per_seed=1, conv_channels=(256, 256),
            conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d"), norm_feats=True,
            vote_loss=dict(type="ChamferDistance", mode="l1", reduction="none",
                           loss_dst_weight=10.0)),
        vote_aggregation_cfg=dict(
            type="PointSAModule", num_point=1024, radius=0.3, num_sample=16,
            mlp_channels=[256, 128, 128, 128], use_xyz=True, normalize_xyz=True),
        feat_channels=(128, 128), conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d"),
        objectness_loss=dict(type="CrossEntropyLoss", class_weight=[0.4, 0.6], reduction="mean",
                             loss_weight=30.0),
        center_loss=dict(chamfer), semantic_reg_loss=dict(chamfer),
        semantic_cls_loss=dict(type="CrossEntropyLoss", reduction="sum", loss_weight=sem_weight),
        train_cfg=dict(dist_thresh=0.2, var_thresh=1e-2, lower_thresh=1e-6, num_point=100,
                       num_point_line=10, line_thresh=0.2))


H3DNET_PRIMITIVE_Z = _h3dnet_primitive("z", 2, 0.5, 1.0)
H3DNET_PRIMITIVE_XY = _h3dnet_primitive("xy", 1, 0.5, 1.0)
H3DNET_PRIMITIVE_LINE = _h3dnet_primitive("line", 0, 1.0, 2.0)


# ------------------------------------------------------------------------------ H3DNet (whole)
# configs/_base_/models/h3dnet.py merged with configs/h3dnet/h3dnet_3x8_scannet-3d-18class.py:
# the rpn VoteHead, H3DRoIHead with its H3DBboxHead and the two-stage train_cfg / test_cfg.
# tests/golden/reference_h3dnet_model_config.json holds the reference's values.
def _h3dnet_scannet():
    ce = lambda weight, **kw: dict(type="CrossEntropyLoss", reduction="sum",  # noqa: E731
                                   loss_weight=weight, **kw)
    coder = dict(type="PartialBinBasedBBoxCoder", num_sizes=18, num_dir_bins=24, with_rot=False,
                 mean_sizes=_SCANNET_MEAN_SIZES)
    center = dict(type="ChamferDistance", mode="l2", reduction="sum", loss_src_weight=10.0,
                  loss_dst_weight=10.0)
    smooth = dict(type="SmoothL1Loss", reduction="sum", loss_weight=10.0)
    matching = lambda rows: dict(                                             # noqa: E731
        type="PointSAModule", num_point=256 * rows, radius=0.5, num_sample=32,
        mlp_channels=[128 + rows, 128, 64, 32], use_xyz=True, normalize_xyz=True)
    cues = lambda weights, reduction: dict(type="CrossEntropyLoss",           # noqa: E731
                                           class_weight=weights, reduction=reduction,
                                           loss_weight=5.0)
    rpn_head = dict(
        type="VoteHead",
        vote_module_cfg=dict(
            in_channels=256, vote_per_seed=1, gt_per_seed=3, conv_channels=(256, 256),
            conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d"), norm_feats=True,
            vote_loss=dict(type="ChamferDistance", mode="l1", reduction="none",
                           loss_dst_weight=10.0)),
        vote_aggregation_cfg=dict(
            type="PointSAModule", num_point=256, radius=0.3, num_sample=16,
            mlp_channels=[256, 128, 128, 128], use_xyz=True, normalize_xyz=True),
        pred_layer_cfg=dict(in_channels=128, shared_conv_channels=(128, 128), bias=True),
        conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d"),
        objectness_loss=ce(5.0, class_weight=[0.2, 0.8]), center_loss=dict(center),
        dir_class_loss=ce(1.0), dir_res_loss=dict(smooth), size_class_loss=ce(1.0),
        size_res_loss=dict(smooth), semantic_loss=ce(1.0), num_classes=18,
        bbox_coder=dict(coder))
    bbox_head = dict(
        type="H3DBboxHead", gt_per_seed=3, num_proposal=256,
        suface_matching_cfg=matching(6), line_matching_cfg=matching(12),
        feat_channels=(128, 128), primitive_refine_channels=[128, 128, 128], upper_thresh=100.0,
        surface_thresh=0.5, line_thresh=0.5, conv_cfg=dict(type="Conv1d"),
        norm_cfg=dict(type="BN1d"),
        objectness_loss=ce(5.0, class_weight=[0.2, 0.8]), center_loss=dict(center),
        dir_class_loss=ce(0.1), dir_res_loss=dict(smooth), size_class_loss=ce(0.1),
        size_res_loss=dict(smooth), semantic_loss=ce(0.1),
        cues_objectness_loss=cues([0.3, 0.7], "mean"), cues_semantic_loss=cues([0.3, 0.7], "mean"),
        proposal_objectness_loss=cues([0.2, 0.8], "none"),
        primitive_center_loss=dict(type="MSELoss", reduction="none", loss_weight=1.0),
        num_classes=18, bbox_coder=dict(coder))
    nms = dict(sample_mod="seed", nms_thr=0.25, score_thr=0.05, per_class_proposal=True)
    return dict(model=dict(
        type="H3DNet", backbone=H3DNET_SCANNET_BACKBONE, rpn_head=rpn_head,
        roi_head=dict(type="H3DRoIHead",
                      primitive_list=[H3DNET_PRIMITIVE_Z, H3DNET_PRIMITIVE_XY,
                                      H3DNET_PRIMITIVE_LINE],
                      bbox_head=bbox_head),
        train_cfg=dict(
            rpn=dict(pos_distance_thr=0.3, neg_distance_thr=0.6, sample_mod="vote"),
            rpn_proposal=dict(use_nms=False),
            rcnn=dict(pos_distance_thr=0.3, neg_distance_thr=0.6, sample_mod="vote",
                      far_threshold=0.6, near_threshold=0.3, mask_surface_threshold=0.3,
                      label_surface_threshold=0.3, mask_line_threshold=0.3,
                      label_line_threshold=0.3)),
        test_cfg=dict(rpn=dict(nms, use_nms=False), rcnn=dict(nms))))


H3DNET_SCANNET = _h3dnet_scannet()


# ---------------------------------------------------------------------------------------------
# Part-A2 on KITTI (configs/parta2/hv_PartA2_secfpn_2x8_cyclic_80e_kitti-3d-3class.py and
# -car.py, the second with its _base_ merged): SparseUNet + SECOND / SECONDFPN + PartA2RPNHead,
# then PartAggregationROIHead with PointwiseSemanticHead.  The roi_head's extractors, its
# bbox_head and the rcnn entries are data here: PartAggregationROIHead, PartA2BboxHead and the
# PartA2 detector are not built.  tests/golden/reference_parta2_configs.json holds the
# reference's values.
def _parta2_rcnn_assigner():
    return dict(type="MaxIoUAssigner", iou_calculator=dict(type="BboxOverlaps3D",
                                                           coordinate="lidar"),
                pos_iou_thr=0.55, neg_iou_thr=0.55, min_pos_iou=0.55, ignore_iof_thr=-1)


def _parta2_roi_extractor(mode):
    return dict(type="Single3DRoIAwareExtractor",
                roi_layer=dict(type="RoIAwarePool3d", out_size=14, max_pts_per_voxel=128,
                               mode=mode))


def _parta2(num_classes, anchor_ranges, anchor_sizes, rpn_assigner, rcnn_assigner):
    return dict(model=dict(
        type="PartA2",
        voxel_layer=dict(max_num_points=5, point_cloud_range=[0, -40, -3, 70.4, 40, 1],
                         voxel_size=[0.05, 0.05, 0.1], max_voxels=(16000, 40000)),
        voxel_encoder=dict(type="HardSimpleVFE"),
        middle_encoder=dict(type="SparseUNet", in_channels=4, sparse_shape=[41, 1600, 1408],
                            order=("conv", "norm", "act")),
        backbone=dict(type="SECOND", in_channels=256, layer_nums=[5, 5], layer_strides=[1, 2],
                      out_channels=[128, 256]),
        neck=dict(type="SECONDFPN", in_channels=[128, 256], upsample_strides=[1, 2],
                  out_channels=[256, 256]),
        rpn_head=dict(
            type="PartA2RPNHead", num_classes=num_classes, in_channels=512, feat_channels=512,
            use_direction_classifier=True,
            anchor_generator=dict(type="Anchor3DRangeGenerator", ranges=anchor_ranges,
                                  sizes=anchor_sizes, rotations=[0, 1.57], reshape_out=False),
            diff_rad_by_sin=True, assigner_per_size=True, assign_per_class=True,
            bbox_coder=dict(type="DeltaXYZWLHRBBoxCoder"),
            loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25,
                          loss_weight=1.0),
            loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=2.0),
            loss_dir=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.2)),
        roi_head=dict(
            type="PartAggregationROIHead", num_classes=num_classes,
            semantic_head=dict(
                type="PointwiseSemanticHead", in_channels=16, extra_width=0.2, seg_score_thr=0.3,
                num_classes=num_classes,
                loss_seg=dict(type="FocalLoss", use_sigmoid=True, reduction="sum", gamma=2.0,
                              alpha=0.25, loss_weight=1.0),
                loss_part=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0)),
            seg_roi_extractor=_parta2_roi_extractor("max"),
            part_roi_extractor=_parta2_roi_extractor("avg"),
            bbox_head=dict(
                type="PartA2BboxHead", num_classes=num_classes, seg_in_channels=16,
                part_in_channels=4, seg_conv_channels=[64, 64], part_conv_channels=[64, 64],
                merge_conv_channels=[128, 128], down_conv_channels=[128, 256],
                bbox_coder=dict(type="DeltaXYZWLHRBBoxCoder"),
                shared_fc_channels=[256, 512, 512, 512], cls_channels=[256, 256],
                reg_channels=[256, 256], dropout_ratio=0.1, roi_feat_size=14,
                with_corner_loss=True,
                loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, reduction="sum",
                               loss_weight=1.0),
                loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, reduction="sum",
                              loss_weight=1.0))),
        train_cfg=dict(
            rpn=dict(assigner=rpn_assigner, allowed_border=0, pos_weight=-1, debug=False),
            rpn_proposal=dict(nms_pre=9000, nms_post=512, max_num=512, nms_thr=0.8, score_thr=0,
                              use_rotate_nms=False),
            rcnn=dict(assigner=rcnn_assigner,
                      sampler=dict(type="IoUNegPiecewiseSampler", num=128, pos_fraction=0.55,
                                   neg_piece_fractions=[0.8, 0.2], neg_iou_piece_thrs=[0.55, 0.1],
                                   neg_pos_ub=-1, add_gt_as_proposals=False, return_iou=True),
                      cls_pos_thr=0.75, cls_neg_thr=0.25)),
        test_cfg=dict(
            rpn=dict(nms_pre=1024, nms_post=100, max_num=100, nms_thr=0.7, score_thr=0,
                     use_rotate_nms=True),
            rcnn=dict(use_rotate_nms=True, use_raw_score=True, nms_thr=0.01, score_thr=0.1))))


PARTA2_SECFPN_KITTI_3CLASS = _parta2(
    3, [[0, -40.0, -0.6, 70.4, 40.0, -0.6], [0, -40.0, -0.6, 70.4, 40.0, -0.6],
        [0, -40.0, -1.78, 70.4, 40.0, -1.78]],
    [[0.6, 0.8, 1.73], [0.6, 1.76, 1.73], [1.6, 3.9, 1.56]],
    [_kitti_assigner(0.5, 0.35), _kitti_assigner(0.5, 0.35), _kitti_assigner(0.6, 0.45)],
    [_parta2_rcnn_assigner(), _parta2_rcnn_assigner(), _parta2_rcnn_assigner()])
PARTA2_SECFPN_KITTI_CAR = _parta2(
    1, [[0, -40.0, -1.78, 70.4, 40.0, -1.78]], [[1.6, 3.9, 1.56]], _kitti_assigner(0.6, 0.45),
    _parta2_rcnn_assigner())
