"""The iou3d / CenterHead surface without a GPU: the numpy restatements against the
reference's own literals, the registries and state-dict keys, and the C ABI's refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iou3d_ref as R  # noqa: E402

# tests/test_utils/test_nms.py::test_circle_nms of the reference, as data
CIRCLE_DETS = [[-11.1100, 2.1300, 0.8823], [-11.2810, 2.2422, 0.8914], [-10.3966, -0.3198, 0.8643],
               [-10.2906, -13.3159, 0.8401], [5.6518, 9.9791, 0.8271], [-11.2652, 13.3637, 0.8267],
               [4.7768, -13.0409, 0.7810], [5.6621, 9.0422, 0.7753], [-10.5561, 18.9627, 0.7518],
               [-10.5643, 13.2293, 0.7200]]
CIRCLE_KEEP = [1, 2, 3, 4, 5, 6, 7, 8, 9]


@pytest.fixture(autouse=True)
def _leave_the_global_rng_alone():
    """Building a head draws its initial weights: keep that out of the global generator."""
    import torch
    with torch.random.fork_rng(devices=[]):
        yield


def test_circle_restatement_matches_the_reference_literal():
    dets = np.asarray(CIRCLE_DETS, np.float32)
    assert R.circle_nms(dets, 0.175) == CIRCLE_KEEP
    order = R.stable_order(dets[:, 2])
    assert R.nms("circle", dets[:, :2], 0.175, order) == CIRCLE_KEEP
    assert R.circle_nms(dets, 0.175, post_max_size=3) == CIRCLE_KEEP[:3]


def test_greedy_and_iou_normal_restatements():
    # a chain: 0 suppresses 1, 1 would suppress 2, 0 does not reach 2
    hit = np.zeros((3, 3), bool)
    hit[0, 1] = hit[1, 2] = True
    assert R.greedy_nms(hit) == [0, 2]
    assert R.greedy_nms(np.zeros((0, 0), bool)) == []
    a = np.array([[0, 0, 2, 2], [1, 1, 3, 3], [5, 5, 5, 9]], np.float32)
    iou = R.iou_normal(a, a)
    assert iou[0, 1] == np.float32(1) / np.float32(7) and iou[0, 0] == 1 and iou[2, 2] == 0
    assert R.stable_order([0.5, 0.9, 0.5, 0.9]).tolist() == [1, 3, 0, 2]


def test_rotated_iou_restatement_on_known_answers():
    # unit squares: identical (1), half shifted (1/3), one turned by 45 degrees about the
    # shared centre (octagon: 2 (sqrt 2 - 1) over 2 - that)
    sq = np.array([[0, 0, 1, 1, 0], [0.5, 0, 1.5, 1, 0], [0, 0, 1, 1, np.pi / 4]], np.float32)
    iou = R.iou_bev(sq, sq)
    inter = 2 * (np.sqrt(2) - 1)
    assert abs(iou[0, 0] - 1) < 1e-5 and abs(iou[0, 1] - 1 / 3) < 1e-5
    assert abs(iou[0, 2] - inter / (2 - inter)) < 1e-5


def test_heads_registry_and_state_dict_keys():
    from msmdfusion_amd import registry
    from msmdfusion_amd.center_head import CenterHead, CenterPointBBoxCoder
    head = registry.build_head(dict(
        type="CenterHead", in_channels=32,
        tasks=[dict(num_class=1, class_names=["car"]),
               dict(num_class=2, class_names=["truck", "construction_vehicle"])],
        common_heads=dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2)),
        share_conv_channel=16,
        bbox_coder=dict(type="CenterPointBBoxCoder", post_center_range=[-10] * 3 + [10] * 3,
                        max_num=8, score_threshold=0.1, out_size_factor=4, voxel_size=[0.2, 0.2],
                        pc_range=[-8, -8], code_size=9),
        separate_head=dict(type="SeparateHead", init_bias=-2.19, final_kernel=3),
        loss_cls=dict(type="GaussianFocalLoss", reduction="mean"),
        loss_bbox=dict(type="L1Loss", reduction="mean", loss_weight=0.25), norm_bbox=True))
    assert isinstance(head, CenterHead) and isinstance(head.bbox_coder, CenterPointBBoxCoder)
    assert head.num_classes == [1, 2] and head.class_names[1] == ["truck", "construction_vehicle"]
    keys = set(head.state_dict())
    for k in ("shared_conv.conv.weight", "shared_conv.bn.running_mean",
              "task_heads.0.reg.0.conv.weight", "task_heads.0.reg.0.bn.weight",
              "task_heads.0.reg.1.weight", "task_heads.0.reg.1.bias",
              "task_heads.1.heatmap.1.bias", "task_heads.1.vel.1.weight"):
        assert k in keys, k
    assert "shared_conv.conv.bias" not in keys              # bias='auto' under a norm
    sd = head.state_dict()
    assert tuple(sd["task_heads.1.heatmap.1.weight"].shape) == (2, 64, 3, 3)
    assert float(sd["task_heads.1.heatmap.1.bias"][0]) == pytest.approx(-2.19)
    assert float(sd["task_heads.0.reg.1.bias"][0]) == 0.0
    for name in ("SeparateHead", "CenterHead", "TransFusionHead", "DCNSeparateHead"):
        assert name in registry.HEADS
    with pytest.raises(NotImplementedError, match="DCNSeparateHead"):
        registry.build_head(dict(type="DCNSeparateHead", in_channels=4, heads={}))


def test_nms_c_abi_refusals():
    """Bad arguments are refused on the host, before anything is enqueued."""
    from msmdfusion_amd._lib import lib
    p = ctypes.c_void_p(256)
    call = lambda **kw: lib.msmd_nms_batched_f32(*[{**dict(  # noqa: E731
        kind=0, boxes=p, ld=5, offsets=p, segments=1, total=100, max_segment=100, thresh=p,
        post_max=100, order=None, keep=p, stride=100, num_keep=p, ws=p, ws_bytes=1 << 20,
        stream=None), **kw}[k] for k in (
        "kind", "boxes", "ld", "offsets", "segments", "total", "max_segment", "thresh", "post_max",
        "order", "keep", "stride", "num_keep", "ws", "ws_bytes", "stream")])
    assert call(max_segment=16385, total=20000) == -1          # n > 16384
    assert call(kind=3) == -1 and call(kind=-1) == -1
    assert call(segments=-1) == -1 and call(total=-1) == -1 and call(post_max=-1) == -1
    assert call(stride=-1) == -1 and call(max_segment=-1) == -1
    assert call(boxes=None) == -1 and call(offsets=None) == -1 and call(thresh=None) == -1
    assert call(keep=None) == -1 and call(num_keep=None) == -1
    assert call(ld=4) == -1 and call(kind=2, ld=1) == -1 and call(kind=1, ld=3) == -1
    assert call(ws=None) == -2 and call(ws_bytes=8) == -2     # workspace missing / too small
    assert call(segments=0) == 0                                # nothing to do
    assert lib.msmd_nms_workspace_bytes(100, 100) == 1792     # 1600 rounded up to 256
    assert lib.msmd_nms_workspace_bytes(24000, 1000) == 24000 * 16 * 8
    assert lib.msmd_nms_workspace_bytes(10, 16385) == 0
    assert lib.msmd_boxes_iou_bev_f32(None, -1, None, 0, None, None) == -1
    assert lib.msmd_boxes_iou_bev_f32(None, 3, p, 3, p, None) == -1
    assert lib.msmd_boxes_iou_bev_f32(None, 0, None, 5, None, None) == 0


def test_wrappers_refuse_cpu_tensors_and_oversized_lists():
    import torch
    from msmdfusion_amd import iou3d
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        iou3d.nms_gpu(torch.zeros((4, 5)), torch.zeros(4), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        iou3d.boxes_iou_bev(torch.zeros((4, 5)), torch.zeros((4, 5)))
    with pytest.raises(ValueError, match="pre_max"):
        iou3d.nms_batched("rotate", torch.zeros((20000, 5)), torch.zeros(20000),
                          torch.tensor([0, 10000, 20000]), 0.5)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_circle_restatement_matches_the_reference_run():
    """tests/golden/center_head_vectors.npz holds keep lists of the reference's own circle_nms
    (distinct scores) and the detections its get_bboxes kept."""
    gold = np.load(os.path.join(GOLDEN, "center_head_vectors.npz"))
    dets = gold["circle_dets"]
    for th in (0.01, 0.2, 0.7):
        assert R.circle_nms(dets, th) == gold["circle_keep_%s" % th].tolist()
        order = R.stable_order(dets[:, 2])
        assert R.nms("circle", dets[:, :2], th, order)[:83] == gold["circle_keep_%s" % th].tolist()
    assert R.circle_nms(dets, 0.7, 5) == gold["circle_keep_0.7_post5"].tolist()
    assert len(gold["circle_keep_0.7"]) < len(gold["circle_keep_0.01"]) <= 83
    # get_bboxes (circle) of the golden = decode + the restatement per task, z to the bottom
    radius, first = [0.5, 1.5, 0.8], [0, 1, 3]
    for i in range(2):
        boxes, scores, labels = [], [], []
        for t in range(3):
            b, s, l = (gold["decode_t%d_s%d_%s" % (t, i, k)] for k in ("bboxes", "scores", "labels"))
            keep = R.circle_nms(np.concatenate([b[:, :2], s[:, None]], 1), radius[t], 12)
            boxes.append(b[keep]), scores.append(s[keep]), labels.append(l[keep] + first[t])
        boxes = np.concatenate(boxes)
        boxes[:, 2] = boxes[:, 2] - boxes[:, 5] * np.float32(0.5)
        np.testing.assert_array_equal(boxes, gold["bboxes_s%d_bboxes" % i])
        np.testing.assert_array_equal(np.concatenate(scores), gold["bboxes_s%d_scores" % i])
        np.testing.assert_array_equal(np.concatenate(labels).astype(np.int32),
                                      gold["bboxes_s%d_labels" % i])


def test_centerpoint_configs_match_the_reference_dicts_and_build():
    import copy
    import json
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.registry import DETECTORS, build_detector
    fx = json.load(open(os.path.join(GOLDEN, "reference_centerpoint_configs.json")))
    norm = lambda o: json.loads(json.dumps(o))   # noqa: E731  tuples -> lists
    assert norm(C.CENTERPOINT_VOXEL_NUS) == fx["centerpoint_0075voxel_second_secfpn_circlenms_nus"]
    assert norm(C.CENTERPOINT_PILLAR_NUS) == fx["centerpoint_02pillar_second_secfpn_nus"]
    assert C.CENTERPOINT_VOXEL_NUS["model"]["test_cfg"]["pts"]["nms_type"] == "circle"
    det = build_detector(copy.deepcopy(C.CENTERPOINT_PILLAR_NUS["model"]))
    assert "CenterPoint" in DETECTORS and type(det).__name__ == "CenterPoint"
    assert type(det.pts_bbox_head).__name__ == "CenterHead" and len(det.pts_bbox_head.task_heads) == 6
    keys = set(det.state_dict())
    for k in ("pts_bbox_head.shared_conv.conv.weight", "pts_bbox_head.task_heads.5.heatmap.1.bias",
              "pts_voxel_encoder.pfn_layers.0.linear.weight", "pts_backbone.blocks.0.0.weight",
              "pts_neck.deblocks.0.0.weight"):
        assert k in keys, k
    assert tuple(det.state_dict()["pts_bbox_head.shared_conv.conv.weight"].shape) == (64, 384, 3, 3)
    assert det.pts_bbox_head.test_cfg["nms_type"] == "rotate"
    voxel = build_detector(copy.deepcopy(C.CENTERPOINT_VOXEL_NUS["model"]))
    assert type(voxel.pts_middle_encoder).__name__ == "SparseEncoder"
    assert voxel.pts_bbox_head.test_cfg["min_radius"] == [4, 12, 10, 1, 0.85, 0.175]
