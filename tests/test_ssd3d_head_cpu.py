"""3DSSD without a GPU: the restatements of tests/ssd3d_ref.py and the torch-only parts of
msmdfusion_amd (AnchorFreeBBoxCoder, the LiDARBoxes members, the sigmoid cross-entropy) against
tests/golden/ssd3d_head_vectors.npz (the reference's own outputs, make_ssd3d_head_golden.py),
the reference's test literals, state-dict keys, registries, the config fixture and the host-side
refusals of the two new C-ABI entry points."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ssd3d_ref as S  # noqa: E402

BATCH, CANDIDATES, CLASSES, BINS = 3, 64, 3, 12
POS_THR, EXPAND = 1.0, 0.05


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "ssd3d_head_vectors.npz")))


def _coder():
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.vote_head import build_bbox_coder
    return build_bbox_coder(C.SSD3D_KITTI_CAR["model"]["bbox_head"]["bbox_coder"])


def _t(a):
    return torch.from_numpy(np.asarray(a))


def gold_scene(gold):
    """-> (box tensors, label tensors) of the golden's three samples."""
    boxes = [torch.zeros(0, 7), _t(gold["gt_boxes_1"]), _t(gold["gt_boxes_2"])]
    labels = [torch.zeros(0, dtype=torch.long), _t(gold["gt_labels_1"]), _t(gold["gt_labels_2"])]
    return boxes, labels


# ------------------------------------------------------------------------------------ coder
def test_coder_against_the_reference_literals_and_the_golden(gold):
    from msmdfusion_amd.head_loss import LiDARBoxes
    from msmdfusion_amd.vote_head import AnchorFreeBBoxCoder, PartialBinBasedBBoxCoder
    coder = _coder()
    assert isinstance(coder, AnchorFreeBBoxCoder) and isinstance(coder, PartialBinBasedBBoxCoder)
    assert coder.num_dir_bins == 12 and coder.num_sizes == 0 and coder.with_rot
    # the reference test's own expectations, with its tolerances ...
    enc = coder.encode(LiDARBoxes(_t(gold["coder_lit_gt_bboxes"])),
                       _t(gold["coder_lit_gt_labels"]).long())
    assert torch.allclose(enc[0], _t(gold["coder_lit_expected_center_target"]), atol=1e-4)
    assert torch.allclose(enc[1], _t(gold["coder_lit_expected_size_targets"]), atol=1e-4)
    assert torch.equal(enc[2], _t(gold["coder_lit_expected_dir_class_target"]))
    assert torch.allclose(enc[3], _t(gold["coder_lit_expected_dir_res_target"]), atol=1e-3)
    # ... and the reference's outputs exactly
    for k, v in zip(("center", "size", "dir_class", "dir_res"), enc):
        assert torch.equal(v, _t(gold["coder_lit_encode_" + k])), k
    out = dict(center=_t(gold["coder_lit_center"]), size=_t(gold["coder_lit_size_res"]),
               dir_class=_t(gold["coder_lit_dir_class"]), dir_res=_t(gold["coder_lit_dir_res"]))
    decoded = coder.decode(out)
    assert torch.allclose(decoded, _t(gold["coder_lit_expected_bbox3d"]), atol=1e-4)
    assert torch.equal(decoded, _t(gold["coder_lit_decoded"]))
    assert torch.equal(S.decode(out, 12), decoded)
    # the scene's boxes
    enc = coder.encode(LiDARBoxes(_t(gold["gt_boxes_1"])), _t(gold["gt_labels_1"]))
    for k, v in zip(("center", "size", "dir_class", "dir_res"), enc):
        assert torch.equal(v, _t(gold["encode_" + k])), k
    assert int(enc[2][4]) == int(_t(gold["encode_dir_class"])[4])     # yaw 7.0: beyond 2 pi


def test_split_pred_against_the_golden(gold):
    coder = _coder()
    res = coder.split_pred(_t(gold["cls_preds"]), _t(gold["reg_preds"]),
                           _t(gold["aggregated_points"]))
    assert sorted(res) == ["center", "center_offset", "dir_class", "dir_res", "dir_res_norm",
                           "obj_scores", "size"]
    for k, v in res.items():
        assert torch.equal(v, _t(gold["split_" + k])), k
    shapes = coder.split_pred(torch.rand(2, 1, 256), torch.rand(2, 30, 256), torch.rand(2, 256, 3))
    want = dict(obj_scores=(2, 1, 256), center=(2, 256, 3), center_offset=(2, 256, 3),
                dir_class=(2, 256, 12), dir_res_norm=(2, 256, 12), dir_res=(2, 256, 12),
                size=(2, 256, 3))
    assert {k: tuple(v.shape) for k, v in shapes.items()} == want


# ------------------------------------------------------------------------------------ boxes
def test_lidar_boxes_members_against_the_golden(gold):
    from msmdfusion_amd.head_loss import LiDARBoxes
    raw = _t(gold["gt_boxes_1"])
    boxes = LiDARBoxes(raw)
    assert boxes.tensor.data_ptr() == raw.data_ptr()          # unchanged: the default keeps it
    assert torch.equal(boxes.gravity_center, _t(gold["box_gravity_center"]))
    assert torch.equal(boxes.dims, _t(gold["box_dims"]))
    assert torch.equal(boxes.yaw, _t(gold["box_yaw"]))
    assert torch.equal(boxes.bottom_center, raw[:, :3])
    assert torch.equal(boxes.corners, _t(gold["box_corners"]))
    assert torch.equal(S.corners(raw), _t(gold["box_corners"]))
    big = boxes.enlarged_box(0.05)
    assert torch.equal(big.tensor, _t(gold["box_enlarged"]))
    assert torch.equal(boxes.tensor, raw) and big.tensor.data_ptr() != raw.data_ptr()
    for origin, key in (((0.5, 0.5, 0.5), "box_from_gravity_origin"),
                        ((0.5, 0.5, 1.0), "box_from_top_origin")):
        moved = LiDARBoxes(raw, origin=origin)
        assert torch.equal(moved.tensor, _t(gold[key])), key
        assert torch.equal(S.from_origin(raw, origin), moved.tensor)
    assert torch.equal(raw, _t(gold["gt_boxes_1"]))           # the shift works on a copy
    pick = _t(gold["gt_labels_1"]) != -1
    assert torch.equal(boxes[pick].tensor, _t(gold["box_getitem_mask"]))
    assert len(boxes[pick]) == 5 and tuple(boxes[2].tensor.shape) == (1, 7)
    assert torch.equal(boxes[2].tensor[0], raw[2])
    fresh = boxes.new_box(torch.zeros(1, 7))
    assert isinstance(fresh, LiDARBoxes) and torch.equal(fresh.tensor, _t(gold["box_new_box"]))
    assert len(LiDARBoxes(torch.zeros(0, 7))) == 0 and boxes.box_dim == 7 and boxes.with_yaw


def test_first_hit_restatement_against_the_golden(gold):
    first = S.first_box(_t(gold["aggregated_points"][1]), _t(gold["gt_boxes_1"]))
    assert np.array_equal(first.numpy(), gold["points_in_boxes_1"])
    assert first[:7].tolist() == [0, -1, -1, 2, 4, 3, 0]


def test_points_in_boxes_needs_a_gpu():
    from msmdfusion_amd.head_loss import LiDARBoxes
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LiDARBoxes(torch.rand(2, 7)).points_in_boxes(torch.rand(5, 3))


# ------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_sigmoid_cross_entropy_is_bce_with_logits(reduction):
    from msmdfusion_amd.losses import CrossEntropyLoss, build_loss
    g = torch.Generator().manual_seed(3)
    pred = torch.randn(2, 17, 3, generator=g, requires_grad=True)
    target = torch.rand(2, 17, 3, generator=g)
    weight = torch.rand(2, 17, 3, generator=g)
    loss = build_loss(dict(type="CrossEntropyLoss", use_sigmoid=True, reduction=reduction,
                           loss_weight=2.5))
    assert isinstance(loss, CrossEntropyLoss) and loss.use_sigmoid
    raw = F.binary_cross_entropy_with_logits(pred, target, reduction="none") * weight
    want = 2.5 * (raw if reduction == "none" else raw.sum() if reduction == "sum" else raw.mean())
    got = loss(pred, target, weight=weight)
    assert torch.equal(got, want)
    assert torch.equal(loss(pred, target), 2.5 * {
        "none": lambda x: x, "sum": torch.sum, "mean": torch.mean}[reduction](
        F.binary_cross_entropy_with_logits(pred, target, reduction="none")))
    if reduction == "mean":
        assert torch.equal(loss(pred, target, weight=weight, avg_factor=7.0), 2.5 * raw.sum() / 7.0)
    grad, = torch.autograd.grad(got.sum(), pred)
    assert torch.isfinite(grad).all() and grad.abs().sum() > 0


def test_softmax_form_is_unchanged_and_the_mask_form_still_raises():
    from msmdfusion_amd.losses import CrossEntropyLoss
    g = torch.Generator().manual_seed(4)
    score, label = torch.randn(6, 5, generator=g), torch.randint(0, 5, (6,), generator=g)
    loss = CrossEntropyLoss(reduction="sum", class_weight=[0.2, 0.8, 1.0, 1.0, 1.0])
    want = F.cross_entropy(score, label, weight=torch.tensor([0.2, 0.8, 1.0, 1.0, 1.0]),
                           reduction="none").sum()
    assert torch.equal(loss(score, label), want)
    with pytest.raises(NotImplementedError):
        CrossEntropyLoss(use_mask=True)
    with pytest.raises(NotImplementedError):
        CrossEntropyLoss(use_sigmoid=True)(score, label)      # class indices: not built


# ------------------------------------------------------------------------ restatement, targets
def test_restated_targets_equal_the_golden(gold):
    """The float32 restatement of the per-sample loop IS the reference: every output equal."""
    boxes, labels = gold_scene(gold)
    got = S.targets(boxes, labels, _t(gold["aggregated_points"]), _t(gold["seed_points"]),
                    CANDIDATES, CLASSES, BINS, POS_THR, EXPAND)
    for name, value in zip(S.ALL_TARGET_NAMES, got):
        want = _t(gold["targets_" + name])
        assert value.dtype == want.dtype and torch.equal(value, want), name
    t = dict(zip(S.ALL_TARGET_NAMES, got))
    # what the case was built for (asserted by its maker on the reference's outputs)
    assert t["negative_mask"][0].all() and t["negative_mask"][2].all()
    assert not t["positive_mask"][0].any() and not t["centerness_targets"][2].any()
    assert t["positive_mask"][1, :7].tolist() == [True, False, False, False, True, True, False]
    assert (t["vote_mask"] > 0)[1, :4].tolist() == [True, True, False, False]
    assert t["mask_targets"][1, 1:4].tolist() == [1, 1, 1]    # the last VALID box, label 1
    for b in range(BATCH):
        bx = boxes[b] if len(labels[b]) else torch.zeros(1, 7)
        lb = labels[b] if len(labels[b]) else torch.zeros(1, dtype=torch.long)
        assert S.distance_margin(bx, lb, _t(gold["aggregated_points"][b]), POS_THR) > 1e-4


def test_restated_losses_against_the_golden(gold):
    """Float32 sums of a few hundred terms in the same order as the reference's modules: the
    float64 restatement bounds what reordering could do."""
    boxes, labels = gold_scene(gold)
    preds32 = {k[len("split_"):]: _t(v) for k, v in gold.items() if k.startswith("split_")}
    preds32["vote_offset"] = _t(gold["vote_offset"])
    agg, seeds = _t(gold["aggregated_points"]), _t(gold["seed_points"])
    t32 = S.targets(boxes, labels, agg, seeds, CANDIDATES, CLASSES, BINS, POS_THR, EXPAND)
    t64 = S.targets(boxes, labels, agg, seeds, CANDIDATES, CLASSES, BINS, POS_THR, EXPAND,
                    dtype=torch.float64)
    l32 = S.losses(preds32, t32, BINS)
    l64 = S.losses({k: v.double() for k, v in preds32.items()}, t64, BINS)
    assert sorted(l32) == sorted(k[len("loss_"):] for k in gold if k.startswith("loss_"))
    for k in l32:
        ref_err = abs(float(gold["loss_" + k]) - float(l64[k]))
        own_err = abs(float(l32[k]) - float(l64[k]))
        ulp = float(np.spacing(np.float32(abs(float(l64[k])))))
        assert own_err <= 4 * ref_err + ulp, (k, own_err, ref_err)


# ---------------------------------------------------------------------------------- the NMS
def test_written_out_nms_on_hand_cases():
    boxes = np.asarray([[0, 0, 2, 2], [0.1, 0, 2.1, 2], [5, 5, 6, 6], [0, 0, 2, 2.05]], np.float32)
    scores = np.asarray([0.9, 0.8, 0.7, 0.95], np.float32)
    assert S.mmcv_nms(boxes, scores, 0.5).tolist() == [3, 2]
    assert S.mmcv_batched_nms(boxes, scores, np.asarray([0, 1, 0, 0]), 0.5).tolist() == [3, 1, 2]
    # two identical zero-area boxes: 0 > thr * 0 is false, neither goes (iou_normal's floored
    # quotient 0 / 1e-8 would agree here, but NOT for thr = 0: see the GPU test)
    flat = np.asarray([[1, 1, 1, 3], [1, 1, 1, 3]], np.float32)
    assert S.mmcv_nms(flat, np.asarray([0.5, 0.4], np.float32), 0.1).tolist() == [0, 1]
    # a NaN coordinate: fmaxf / fminf drop it, the NaN areas make the comparison false
    nan = np.asarray([[0, 0, 2, 2], [np.nan, 0, 2, 2], [0, 0, 2, 2]], np.float32)
    assert S.mmcv_nms(nan, np.asarray([0.9, 0.8, 0.7], np.float32), 0.5).tolist() == [0, 1]


def test_restated_get_bboxes_against_the_golden(gold):
    preds = {k[len("split_"):]: _t(v) for k, v in gold.items() if k.startswith("split_")}
    preds["center"], preds["obj_scores"] = _t(gold["boxes_in_center"]), _t(gold["boxes_in_obj_scores"])
    assert torch.equal(S.decode(preds, BINS), _t(gold["boxes_decoded"]))
    cfgs = dict(per_class=dict(nms_cfg=dict(type="nms", iou_thr=0.1), score_thr=0.0,
                               per_class_proposal=True, max_output_num=100),
                cut=dict(nms_cfg=dict(type="nms", iou_thr=0.1), score_thr=0.4,
                         per_class_proposal=False, max_output_num=8))
    for tag, cfg in cfgs.items():
        for b, (box, score, label) in enumerate(S.get_bboxes(preds, BINS, cfg)):
            assert torch.equal(box, _t(gold["boxes_%s_%d_tensor" % (tag, b)])), (tag, b)
            assert torch.equal(score, _t(gold["boxes_%s_%d_scores" % (tag, b)])), (tag, b)
            assert torch.equal(label, _t(gold["boxes_%s_%d_labels" % (tag, b)])), (tag, b)


# ------------------------------------------------------------- keys, registries, the config
def test_state_dict_keys_registries_and_config():
    from msmdfusion_amd import configs as C
    from msmdfusion_amd import registry
    from msmdfusion_amd.detector import SSD3DNet, VoteNet
    from msmdfusion_amd.ssd3d_head import SSD3DHead
    from msmdfusion_amd.vote_head import AnchorFreeBBoxCoder, VoteHead
    fx = json.load(open(os.path.join(HERE, "golden", "reference_3dssd_config.json")))
    norm = lambda o: json.loads(json.dumps(o))   # noqa: E731  (tuples -> lists)
    assert norm(C.SSD3D_KITTI_CAR) == fx["3dssd_kitti-3d-car"]

    cfg = C.SSD3D_KITTI_CAR["model"]
    before = norm(cfg)
    head = registry.build_head(dict(cfg["bbox_head"], train_cfg=cfg["train_cfg"],
                                    test_cfg=cfg["test_cfg"]))
    assert norm(cfg) == before                                # the config dicts are left intact
    assert isinstance(head, SSD3DHead) and isinstance(head, VoteHead)
    assert isinstance(head.bbox_coder, AnchorFreeBBoxCoder)
    assert head.num_candidates == 256 and head.num_classes == 1 and head.num_dir_bins == 12
    assert head.gt_per_seed == 1 and head.num_proposal == 256
    assert head._get_cls_out_channels() == 1 and head._get_reg_out_channels() == 30
    state = head.state_dict()
    for k in ("vote_module.vote_conv.0.conv.weight", "vote_module.vote_conv.0.bn.running_var",
              "vote_module.conv_out.weight", "vote_aggregation.mlps.0.layer0.conv.weight",
              "vote_aggregation.mlps.1.layer2.bn.weight", "vote_aggregation.mlps.1.layer0.conv.bias",
              "conv_pred.shared_convs.layer0.conv.weight", "conv_pred.shared_convs.layer1.bn.bias",
              "conv_pred.cls_convs.layer0.conv.weight", "conv_pred.reg_convs.layer0.bn.weight",
              "conv_pred.conv_cls.weight", "conv_pred.conv_reg.bias"):
        assert k in state, k
    assert tuple(state["conv_pred.conv_cls.weight"].shape) == (1, 128, 1)
    assert tuple(state["conv_pred.conv_reg.weight"].shape) == (30, 128, 1)
    assert tuple(state["vote_module.conv_out.weight"].shape) == (3, 128, 1)   # no feature residual
    assert tuple(state["conv_pred.shared_convs.layer0.conv.weight"].shape) == (512, 1536, 1)
    assert tuple(state["vote_aggregation.mlps.1.layer0.conv.weight"].shape) == (256, 259, 1, 1)
    assert not [k for k in state if "loss" in k]
    for name in ("objectness_loss", "center_loss", "dir_class_loss", "dir_res_loss",
                 "size_res_loss", "corner_loss", "vote_loss"):
        assert hasattr(head, name), name
    assert head.objectness_loss.use_sigmoid and not hasattr(head, "semantic_loss")
    assert "SSD3DHead" in registry.HEADS and "SSD3DNet" in registry.DETECTORS
    assert issubclass(SSD3DNet, VoteNet)


def test_depth_boxes_are_refused():
    from msmdfusion_amd import configs as C
    from msmdfusion_amd import registry
    from msmdfusion_amd.head_loss import DepthBoxes
    cfg = C.SSD3D_KITTI_CAR["model"]
    bbox_head = dict(cfg["bbox_head"], vote_module_cfg=dict(
        cfg["bbox_head"]["vote_module_cfg"], num_points=4))
    head = registry.build_head(dict(bbox_head, train_cfg=cfg["train_cfg"],
                                    test_cfg=cfg["test_cfg"]))
    preds = dict(aggregated_points=torch.zeros(1, 4, 3), seed_points=torch.zeros(1, 8, 3))
    with pytest.raises(NotImplementedError):
        head.get_targets(None, [DepthBoxes(torch.rand(2, 7))], [torch.zeros(2, dtype=torch.long)],
                         bbox_preds=preds)


# ---------------------------------------------------------------------------- C-ABI refusals
def test_new_entry_points_refuse_bad_arguments_on_the_host():
    """Nothing is enqueued: these calls return before the first launch (no GPU needed)."""
    from msmdfusion_amd._lib import lib
    p = ctypes.c_void_p(256)                            # a non-null, aligned, never-read address
    INVALID, WORKSPACE, RANGE = -1, -2, -5
    assert lib.msmd_ssd3d_gt_chunk() == 64
    fn = lib.msmd_ssd3d_targets_f32

    def call(**kw):
        a = dict(aggregated=p, seeds=p, seed_stride=24, gt=p, vote=p, labels=p, offsets=p, table=p,
                 width=33, dir_class=p, batch=2, n=8, total=4, classes=3, thr=1.0, out=[p] * 11)
        a.update(kw)
        return fn(a["aggregated"], a["seeds"], a["seed_stride"], a["gt"], a["vote"], a["labels"],
                  a["offsets"], a["table"], a["width"], a["dir_class"], a["batch"], a["n"],
                  a["total"], a["classes"], a["thr"], *a["out"], None)

    for name in ("aggregated", "seeds", "gt", "vote", "labels", "offsets", "table", "dir_class"):
        assert call(**{name: None}) == INVALID, name
    for k in range(11):
        assert call(out=[None if j == k else p for j in range(11)]) == INVALID, k
    assert call(width=32) == INVALID and call(width=34) == INVALID
    assert call(seed_stride=23) == INVALID                     # samples would overlap
    assert call(batch=-1) == INVALID and call(n=-1) == INVALID and call(total=-1) == INVALID
    assert call(classes=0) == INVALID and call(thr=float("nan")) == INVALID
    assert call(batch=70000) == RANGE
    assert call(batch=4096, n=1 << 20, seed_stride=3 << 20) == RANGE
    assert call(batch=0) == 0 and call(n=0, seed_stride=0) == 0     # nothing to do
    assert call(total=0, gt=None, vote=None, labels=None, table=None, dir_class=None,
                aggregated=None) == INVALID

    nms, need = lib.msmd_nms_mmcv_f32, lib.msmd_nms_workspace_bytes
    ok = (p, 4, p, 1, 100, 100, p, 100, None, p, 100, p)
    assert nms(*ok, None, 0, None) == WORKSPACE
    assert nms(*ok, p, need(100, 100) - 1, None) == WORKSPACE
    assert nms(*ok, ctypes.c_void_p(260), need(100, 100), None) == WORKSPACE
    assert nms(None, 4, p, 1, 100, 100, p, 100, None, p, 100, p, p, 1 << 20, None) == INVALID
    assert nms(p, 4, None, 1, 100, 100, p, 100, None, p, 100, p, p, 1 << 20, None) == INVALID
    assert nms(p, 4, p, 1, 100, 100, None, 100, None, p, 100, p, p, 1 << 20, None) == INVALID
    assert nms(p, 4, p, 1, 100, 100, p, 100, None, None, 100, p, p, 1 << 20, None) == INVALID
    assert nms(p, 4, p, 1, 100, 100, p, 100, None, p, 100, None, p, 1 << 20, None) == INVALID
    assert nms(p, 3, p, 1, 100, 100, p, 100, None, p, 100, p, p, 1 << 20, None) == INVALID
    assert nms(p, 4, p, -1, 100, 100, p, 100, None, p, 100, p, p, 1 << 20, None) == INVALID
    assert nms(p, 4, p, 1, 100, 100, p, -1, None, p, 100, p, p, 1 << 20, None) == INVALID
    assert nms(p, 4, p, 1, 100000, 16385, p, 100, None, p, 100, p, p, 1 << 30, None) == INVALID
    assert nms(p, 4, p, 70000, 100, 100, p, 100, None, p, 100, p, p, 1 << 20, None) == RANGE
    assert nms(p, 4, p, 0, 100, 100, p, 100, None, p, 100, p, None, 0, None) == 0
    # the batched entry point keeps its three kinds: the new one is not a kind code of it
    assert lib.msmd_nms_batched_f32(4, p, 4, p, 1, 100, 100, p, 100, None, p, 100, p, p, 1 << 20,
                                    None) == INVALID


def test_python_wrappers_refuse_cpu_tensors_and_oversized_segments():
    from msmdfusion_amd import kernels as K
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.ssd3d_targets(z(1, 4, 3), z(1, 8, 3), z(2, 7), z(2, 7), z(2, dtype=torch.long),
                        z(2, dtype=torch.int32), z(2, 33), z(2, dtype=torch.long), 3, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.nms_segments("mmcv", z(4, 4), z(2, dtype=torch.int32), z(1), 4)
    assert K.SSD3D_GT_CHUNK == 64 and K.SSD3D_TABLE_WIDTH == 33
    assert K.SSD3D_TARGET_NAMES == S.TARGET_NAMES
