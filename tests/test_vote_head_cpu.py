"""VoteNet without a GPU: the restatements of tests/vote_ref.py and the torch-only parts of
msmdfusion_amd/vote_head.py against tests/golden/vote_head_vectors.npz (the reference's own
outputs, make_vote_head_golden.py), the reference's test literals, state-dict keys, registries,
config fixtures and the host-side refusals of every new C-ABI entry point."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import roiaware_ref as RR  # noqa: E402
import vote_ref as V  # noqa: E402

MODES = ("l2", "l1", "smooth_l1")
# Conv1d here is a matrix product, the reference's a convolution: the same <= 16-term float32
# dot products in another order, then BatchNorm over 32 (64) values of O(1).  16 * 2^-24 * |x|
# per product, amplified by the normalisation's 1 / sigma ~ O(1..10): 1e-5 absolute on O(1)
# outputs leaves a decade of room and is a thousand times below any wiring mistake.
COMPOSE_ATOL = 1e-5


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "vote_head_vectors.npz")))


def _coder():
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.vote_head import build_bbox_coder
    return build_bbox_coder(C.VOTENET_SUNRGBD["model"]["bbox_head"]["bbox_coder"])


# ------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("mode", MODES)
def test_chamfer_restatement_equals_the_reference(gold, mode):
    """Indices exactly, distances bit for bit (the generator saw a largest difference of 0.0)."""
    for tag in "abc":
        src, dst = gold["chamfer_%s_src" % tag], gold["chamfer_%s_dst" % tag]
        d1, i1, d2, i2 = V.chamfer_forward(src, dst, mode)
        key = "chamfer_%s_%s_" % (tag, mode)
        assert np.array_equal(i1, gold[key + "i1"]) and np.array_equal(i2, gold[key + "i2"])
        assert d1.tobytes() == gold[key + "d1"].tobytes()
        assert d2.tobytes() == gold[key + "d2"].tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_chamfer_torch_path_equals_the_reference(gold, mode):
    """CPU tensors (and C != 3) take the expanded formulation: the reference's results."""
    from msmdfusion_amd import losses as L
    src, dst = torch.from_numpy(gold["chamfer_b_src"]), torch.from_numpy(gold["chamfer_b_dst"])
    ls, ld, i1, i2 = L.chamfer_distance(src, dst, criterion_mode=mode, reduction="none")
    key = "chamfer_b_%s_" % mode
    assert np.array_equal(i1.numpy(), gold[key + "i1"]) and np.array_equal(i2.numpy(), gold[key + "i2"])
    assert np.array_equal(ls.numpy(), gold[key + "d1"]) and np.array_equal(ld.numpy(), gold[key + "d2"])
    wide = L.chamfer_distance(torch.cat([src, src[..., :1]], -1), torch.cat([dst, dst[..., :1]], -1),
                              criterion_mode=mode, reduction="none")
    assert wide[0].shape == ls.shape and wide[2].dtype == torch.long


def test_chamfer_reference_test_shapes_and_relations():
    """tests/test_metrics/test_losses.py test_chamfer_disrance of the reference."""
    from msmdfusion_amd.losses import ChamferDistance, build_loss, chamfer_distance
    with pytest.raises(AssertionError):
        ChamferDistance(mode="smoothl1")
    with pytest.raises(AssertionError):
        ChamferDistance(mode="l2", reduction=None)
    module = build_loss(dict(type="ChamferDistance", mode="l2", reduction="sum",
                             loss_src_weight=1.0, loss_dst_weight=1.0))
    assert isinstance(module, ChamferDistance)
    source = torch.tensor(
        [[[-0.9888, 0.9683, -0.8494], [-6.4536, 4.5146, 1.6861], [2.0482, 5.6936, -1.4701],
          [-0.5173, 5.6472, 2.1748], [-2.8010, 5.4423, -1.2158], [2.4018, 2.4389, -0.2403],
          [-2.8811, 3.8486, 1.4750], [-0.2031, 3.8969, -1.5245], [1.3827, 4.9295, 1.1537],
          [-2.6961, 2.2621, -1.0976]],
         [[0.3692, 1.8409, -1.4983], [1.9995, 6.3602, 0.1798], [-2.1317, 4.6011, -0.7028],
          [2.4158, 3.1482, 0.3169], [-0.5836, 3.6250, -1.2650], [-1.9862, 1.6182, -1.4901],
          [2.5992, 1.2847, -0.8471], [-0.3467, 5.3681, -1.4755], [-0.8576, 3.3400, -1.7399],
          [2.7447, 4.6349, 0.1994]]])
    target = torch.tensor(
        [[[-0.4758, 1.0094, -0.8645], [-0.3130, 0.8564, -0.9061], [-0.1560, 2.0394, -0.8936],
          [-0.3685, 1.6467, -0.8271], [-0.2740, 2.2212, -0.7980]],
         [[1.4856, 2.5299, -1.0047], [2.3262, 3.3065, -0.9475], [2.4593, 2.5870, -0.9423],
          [0.0000, 0.0000, 0.0000], [0.0000, 0.0000, 0.0000]]])
    inds1 = [[0, 4, 4, 4, 4, 2, 4, 4, 4, 3], [0, 1, 0, 1, 0, 4, 2, 0, 0, 1]]
    inds1_alt = [[0, 4, 4, 4, 4, 2, 4, 4, 4, 3], [0, 1, 0, 1, 0, 3, 2, 0, 0, 1]]
    inds2 = [[0, 0, 0, 0, 0], [0, 3, 6, 0, 0]]
    for call in (lambda: module(source, target, return_indices=True),
                 lambda: chamfer_distance(source, target, reduction="sum")):
        loss_source, loss_target, indices1, indices2 = call()
        assert torch.allclose(loss_source, torch.tensor(219.5936))
        assert torch.allclose(loss_target, torch.tensor(22.3705))
        assert indices1.tolist() in (inds1, inds1_alt) and indices2.tolist() == inds2
    own = V.chamfer_forward(source.numpy(), target.numpy(), "l2")
    assert own[1].tolist() == inds1_alt and own[3].tolist() == inds2     # ties: the lowest index
    assert len(module(source, target)) == 2


def test_aligned_nms_restatement(gold):
    """The reference's test_aligned_3d_nms literal, and its aligned_3d_nms on the golden boxes."""
    T = V
    order = np.argsort(-np.float64(T.LITERAL_SCORES), kind="stable")
    assert V.aligned_nms(T.LITERAL_BOXES, T.LITERAL_CLASSES, 0.25, order) == T.LITERAL_PICK
    scores = gold["nms_scores"]
    assert len(set(scores.tolist())) == len(scores)                      # no ties: one order
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    assert V.aligned_nms(gold["nms_boxes"], gold["nms_classes"], 0.25, order) == \
        gold["nms_pick"].tolist()
    assert len(gold["nms_pick"]) < len(scores)


def test_vote_target_restatement_and_the_frame_conversion(gold):
    """DepthBoxes' conversion + the roiaware restatement reproduce the reference's inclusion
    table; the loop restatement over it reproduces the reference's vote targets."""
    from msmdfusion_amd.head_loss import DepthBoxes
    boxes = DepthBoxes(torch.from_numpy(gold["gt_boxes_1"]))
    points = torch.from_numpy(gold["points"][1])
    lidar_boxes = DepthBoxes.boxes_to_lidar(boxes.tensor)
    assert np.array_equal(lidar_boxes.numpy(), gold["gt_boxes_lidar_1"])
    inside = RR.points_in_boxes_all(DepthBoxes.points_to_lidar(points).numpy()[None],
                                    lidar_boxes.numpy()[None])[0]
    assert np.array_equal(inside, gold["points_in_boxes_1"])
    assert inside[:4].sum(1).tolist() == [1, 2, 3, 4]
    targets, mask = V.vote_targets_loop(points, torch.from_numpy(inside), boxes.gravity_center)
    assert np.array_equal(targets.numpy(), gold["targets_vote_targets"][1])
    assert np.array_equal(mask.numpy(), gold["targets_vote_target_masks"][1])
    # the point inside four boxes: slot 2 carries the fourth (last) box's vote
    want = boxes.gravity_center[[0, 1, 3]] - points[3, :3]
    assert torch.equal(targets[3].view(3, 3), want)


def test_depth_boxes(gold):
    from msmdfusion_amd.head_loss import DepthBoxes
    boxes = DepthBoxes(gold["gt_boxes_1"])
    assert len(boxes) == 5 and boxes.with_yaw and boxes.box_dim == 7
    assert np.array_equal(boxes.gravity_center.numpy(), gold["gt_gravity_center_1"])
    assert np.abs(boxes.corners.numpy() - gold["gt_corners_1"]).max() <= 1e-6
    shifted = DepthBoxes(torch.from_numpy(gold["gt_boxes_1"]), origin=(0.5, 0.5, 0.5))
    assert np.array_equal(shifted.tensor.numpy(), gold["gt_from_gravity_origin_1"])
    fake = boxes.new_box(boxes.tensor.new_zeros(1, 7))
    assert isinstance(fake, DepthBoxes) and len(fake) == 1 and fake.with_yaw
    six = DepthBoxes(torch.ones(2, 6), box_dim=6)
    assert six.tensor.shape == (2, 7) and not six.with_yaw and float(six.tensor[:, 6].abs().max()) == 0
    assert len(DepthBoxes(torch.zeros(0, 7))) == 0
    assert boxes.to("cpu").tensor.data_ptr() != boxes.tensor.data_ptr()


# ------------------------------------------------------------------------------------- coder
def test_coder_against_the_golden_and_the_reference_literals(gold):
    from msmdfusion_amd.head_loss import DepthBoxes
    coder = _coder()
    boxes = DepthBoxes(torch.from_numpy(gold["gt_boxes_1"]))
    got = coder.encode(boxes, torch.from_numpy(gold["gt_labels_1"]))
    for k, v in zip(("center", "size_class", "size_res", "dir_class", "dir_res"), got):
        assert np.array_equal(v.numpy(), gold["encode_" + k]), k
    assert got[1].dtype == torch.long and got[3].dtype == torch.long
    # the reference's test_partial_bin_based_box_coder: encode ...
    gt = DepthBoxes([[0.8308, 4.1168, -1.2035, 2.2493, 1.8444, 1.9245, 1.6486],
                     [2.3002, 4.8149, -1.2442, 0.5718, 0.8629, 0.9510, 1.6030],
                     [-1.1477, 1.8090, -1.1725, 0.6965, 1.5273, 2.0563, 0.0552]])
    center, size_class, size_res, dir_class, dir_res = coder.encode(gt, torch.tensor([0, 1, 2]))
    assert torch.allclose(center, torch.tensor([[0.8308, 4.1168, -0.2413], [2.3002, 4.8149, -0.7687],
                                                [-1.1477, 1.8090, -0.1444]]), atol=1e-4)
    assert size_class.tolist() == [0, 1, 2] and dir_class.tolist() == [3, 3, 0]
    assert torch.allclose(size_res, torch.tensor([[0.1350, 0.2241, 0.9972],
                                                  [-0.2193, -0.4166, 0.2328],
                                                  [-0.2270, -0.3401, 1.2108]]), atol=1e-4)
    assert torch.allclose(dir_res, torch.tensor([0.0778, 0.0322, 0.0552]), atol=1e-4)
    # ... decode, on the literals the generator read from the reference's test file ...
    bbox_out = {k: torch.from_numpy(gold["coder_lit_" + k])
                for k in ("center", "size_class", "size_res", "dir_class", "dir_res")}
    decoded = coder.decode(bbox_out)
    assert np.array_equal(decoded.numpy(), gold["coder_lit_decoded"])
    assert torch.allclose(decoded, torch.from_numpy(gold["coder_lit_expected_bbox3d"]), atol=1e-4)
    # ... and split_pred's shapes
    res = coder.split_pred(torch.rand(2, 12, 256), torch.rand(2, 67, 256), torch.rand(2, 256, 3))
    shapes = dict(obj_scores=(2, 256, 2), center=(2, 256, 3), dir_class=(2, 256, 12),
                  dir_res_norm=(2, 256, 12), dir_res=(2, 256, 12), size_class=(2, 256, 10),
                  size_res_norm=(2, 256, 10, 3), size_res=(2, 256, 10, 3), sem_scores=(2, 256, 10))
    assert {k: tuple(v.shape) for k, v in res.items()} == shapes
    # class2angle inverts angle2class
    angle = torch.tensor([-3.0, -0.2, 0.0, 0.26, 1.7, 3.1])
    cls, res = coder.angle2class(angle)
    assert torch.allclose(coder.class2angle(cls, res), angle, atol=1e-6)


def test_split_pred_decode_and_corners_against_the_golden(gold):
    coder = _coder()
    split = coder.split_pred(torch.from_numpy(gold["cls_predictions"]),
                             torch.from_numpy(gold["reg_predictions"]),
                             torch.from_numpy(gold["aggregated_points"]))
    for k, v in split.items():
        assert np.array_equal(v.numpy(), gold["split_" + k]), k
    preds = dict(split)
    for k in ("center", "size_class", "size_res"):
        preds[k] = torch.from_numpy(gold["boxes_in_" + k])
    assert np.array_equal(coder.decode(preds).numpy(), gold["boxes_decoded"])
    corners = coder.decode_corners(split["center"], split["size_res_norm"],
                                   torch.argmax(split["size_class"], -1))
    assert corners.shape == (2, 16, 6) and bool((corners[..., 3:] >= corners[..., :3]).all())


# --------------------------------------------------------------------------- torch-only modules
def _load(module, gold, prefix):
    state = {k[len(prefix):]: torch.from_numpy(v) for k, v in gold.items() if k.startswith(prefix)}
    assert set(state) == set(module.state_dict())
    module.load_state_dict(state)
    return module.train()


def _golden_cfgs():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_vote_head_golden as G
    return G


def test_vote_module_and_prediction_layers_against_the_golden(gold):
    from msmdfusion_amd.vote_head import BaseConvBboxHead, VoteModule
    G = _golden_cfgs()
    vote = _load(VoteModule(**G.VOTE_MODULE_CFG), gold, "weights_vote_module.")
    points, feats, offset = vote(torch.from_numpy(gold["seed_points"]),
                                 torch.from_numpy(gold["seed_features"]))
    for got, key in ((points, "vote_points"), (feats, "vote_features"), (offset, "vote_offset")):
        assert got.shape == gold[key].shape
        assert np.abs(got.detach().numpy() - gold[key]).max() <= COMPOSE_ATOL, key
    pred = _load(BaseConvBboxHead(**G.PRED_LAYER_CFG, num_cls_out_channels=12,
                                  num_reg_out_channels=67), gold, "weights_conv_pred.")
    cls, reg = pred(torch.from_numpy(gold["aggregated_features"]))
    assert np.abs(cls.detach().numpy() - gold["cls_predictions"]).max() <= COMPOSE_ATOL
    assert np.abs(reg.detach().numpy() - gold["reg_predictions"]).max() <= COMPOSE_ATOL
    # the vote loss from the golden targets (CPU tensors: the expanded formulation)
    loss = vote.get_loss(torch.from_numpy(gold["seed_points"]), torch.from_numpy(gold["vote_points"]),
                         torch.from_numpy(gold["seed_indices"]),
                         torch.from_numpy(gold["targets_vote_target_masks"]),
                         torch.from_numpy(gold["targets_vote_targets"]))
    assert abs(float(loss) - float(gold["loss_vote_loss"])) <= 1e-6 * float(gold["loss_vote_loss"])
    # vote_xyz_range clamps the offsets; without residual features the seeds' pass through
    clamped = VoteModule(8, conv_channels=(8,), vote_xyz_range=(0.01, 0.02, 0.03),
                         with_res_feat=False)
    sp, sf = torch.randn(2, 5, 3), torch.randn(2, 8, 5)
    vp, vf, _ = clamped(sp, sf)
    assert bool(((vp - sp).abs() <= torch.tensor([0.01, 0.02, 0.03]) + 1e-6).all()) and vf is sf


def test_state_dict_keys_registries_and_configs():
    from msmdfusion_amd import configs as C
    from msmdfusion_amd import registry
    from msmdfusion_amd.detector import VoteNet
    from msmdfusion_amd.vote_head import PartialBinBasedBBoxCoder, VoteHead
    fx = json.load(open(os.path.join(HERE, "golden", "reference_votenet_configs.json")))
    norm = lambda o: json.loads(json.dumps(o))   # noqa: E731  (tuples -> lists)
    assert norm(C.VOTENET_SUNRGBD) == fx["votenet_16x8_sunrgbd-3d-10class"]
    assert norm(C.VOTENET_SCANNET) == fx["votenet_8x8_scannet-3d-18class"]

    for cfg, classes, bins in ((C.VOTENET_SUNRGBD, 10, 12), (C.VOTENET_SCANNET, 18, 1)):
        model = registry.build_detector(cfg["model"])
        again = registry.build_detector(cfg["model"])          # the config dicts are left intact
        assert isinstance(model, VoteNet) and isinstance(model.bbox_head, VoteHead)
        assert isinstance(model.bbox_head.bbox_coder, PartialBinBasedBBoxCoder)
        keys = set(model.state_dict())
        assert keys == set(again.state_dict())
        for k in ("backbone.SA_modules.0.mlps.0.layer0.conv.weight",
                  "backbone.FP_modules.1.mlps.layer1.bn.running_var",
                  "bbox_head.vote_module.vote_conv.0.conv.weight",
                  "bbox_head.vote_module.vote_conv.0.conv.bias",
                  "bbox_head.vote_module.vote_conv.1.bn.running_mean",
                  "bbox_head.vote_module.conv_out.bias",
                  "bbox_head.vote_aggregation.mlps.0.layer2.bn.weight",
                  "bbox_head.conv_pred.shared_convs.layer1.conv.bias",
                  "bbox_head.conv_pred.conv_cls.weight", "bbox_head.conv_pred.conv_reg.bias"):
            assert k in keys, k
        state = model.state_dict()
        assert tuple(state["bbox_head.conv_pred.conv_cls.weight"].shape) == (classes + 2, 128, 1)
        assert tuple(state["bbox_head.conv_pred.conv_reg.weight"].shape) == \
            (3 + 2 * bins + 4 * classes, 128, 1)
        assert tuple(state["bbox_head.vote_module.conv_out.weight"].shape) == (259, 256, 1)
        assert tuple(state["bbox_head.vote_aggregation.mlps.0.layer0.conv.weight"].shape) == \
            (128, 259, 1, 1)
        assert not [k for k in keys if "loss" in k or "mean_size" in k]
    head = registry.build_head(dict(C.VOTENET_SUNRGBD["model"]["bbox_head"],
                                    train_cfg=C.VOTENET_SUNRGBD["model"]["train_cfg"],
                                    test_cfg=C.VOTENET_SUNRGBD["model"]["test_cfg"]))
    assert head.num_proposal == 256 and head.gt_per_seed == 3 and head.num_sizes == 10
    assert "VoteHead" in registry.HEADS and "BaseConvBboxHead" in registry.HEADS
    assert "VoteNet" in registry.DETECTORS


def test_iou_loss_is_refused():
    from msmdfusion_amd import configs as C
    from msmdfusion_amd import registry
    cfg = dict(C.VOTENET_SCANNET["model"]["bbox_head"],
               iou_loss=dict(type="AxisAlignedIoULoss", reduction="sum", loss_weight=10.0 / 3.0))
    with pytest.raises(NotImplementedError, match="iou_loss"):
        registry.build_head(cfg)


# ------------------------------------------------------------------------------ C-ABI refusals
def test_new_entry_points_refuse_bad_arguments_on_the_host():
    """Nothing is enqueued: these calls return before the first launch (no GPU needed)."""
    from msmdfusion_amd._lib import lib
    p = ctypes.c_void_p(256)                            # a non-null, aligned, never-read address
    INVALID, WORKSPACE, RANGE = -1, -2, -5
    fwd = lib.msmd_chamfer_fwd_f32
    assert fwd(None, p, 1, 4, 4, 3, 0, p, p, p, p, None) == INVALID          # null pointers
    assert fwd(p, p, 1, 4, 4, 3, 0, p, None, p, p, None) == INVALID
    assert fwd(p, p, 1, 4, 4, 4, 0, p, p, p, p, None) == INVALID             # C != 3
    assert fwd(p, p, 1, 0, 4, 3, 0, p, p, p, p, None) == INVALID             # N = 0
    assert fwd(p, p, 1, 4, 0, 3, 0, p, p, p, p, None) == INVALID             # M = 0
    assert fwd(p, p, -1, 4, 4, 3, 0, p, p, p, p, None) == INVALID            # negative counts
    assert fwd(p, p, 1, -4, 4, 3, 0, p, p, p, p, None) == INVALID
    assert fwd(p, p, 1, 4, 4, 3, 3, p, p, p, p, None) == INVALID             # no such mode
    assert fwd(p, p, 1 << 20, 1 << 12, 4, 3, 0, p, p, p, p, None) == RANGE
    assert fwd(p, p, 0, 4, 4, 3, 0, p, p, p, p, None) == 0                   # an empty batch
    bwd = lib.msmd_chamfer_bwd_f32
    assert bwd(p, p, p, p, p, None, 1, 4, 4, 3, 0, p, p, None) == INVALID
    assert bwd(p, p, p, p, p, p, 1, 4, 4, 3, 0, None, None, None) == INVALID  # no output at all
    assert bwd(p, p, p, p, p, p, 1, 4, 4, 2, 0, p, p, None) == INVALID
    assert bwd(p, p, p, p, p, p, 1, 0, 4, 3, 0, p, p, None) == INVALID
    assert bwd(p, p, p, p, p, p, 1, 4, -1, 3, 0, p, p, None) == INVALID
    vote = lib.msmd_vote_targets_f32
    assert vote(None, 3, p, p, p, p, 2, 8, 4, 8, 3, p, p, None) == INVALID
    assert vote(p, 3, p, None, p, p, 2, 8, 4, 8, 3, p, p, None) == INVALID   # boxes missing
    assert vote(p, 3, p, p, p, p, 2, 8, 4, 8, 3, p, None, None) == INVALID
    assert vote(p, 2, p, p, p, p, 2, 8, 4, 8, 3, p, p, None) == INVALID      # rows without z
    assert vote(p, 3, p, p, p, p, 2, 8, 4, 8, 2, p, p, None) == INVALID      # gt_per_seed != 3
    assert vote(p, 3, p, p, p, p, -1, 8, 4, 8, 3, p, p, None) == INVALID
    assert vote(p, 3, p, p, p, p, 2, -8, 4, 8, 3, p, p, None) == INVALID
    assert vote(p, 3, p, p, p, p, 2, 8, -4, 8, 3, p, p, None) == INVALID
    assert vote(p, 3, p, p, p, p, 70000, 8, 4, 8, 3, p, p, None) == RANGE
    count = lib.msmd_points_in_boxes_count_f32
    assert count(None, p, 3, 1, 4, 8, p, None) == INVALID
    assert count(p, None, 3, 1, 4, 8, p, None) == INVALID
    assert count(p, p, 3, 1, 4, 8, None, None) == INVALID
    assert count(p, p, 2, 1, 4, 8, p, None) == INVALID
    assert count(p, p, 3, -1, 4, 8, p, None) == INVALID
    assert count(p, p, 3, 1, -4, 8, p, None) == INVALID
    assert count(p, p, 3, 1, 4, -8, p, None) == INVALID
    assert count(p, p, 3, 70000, 4, 8, p, None) == RANGE
    nms, need = lib.msmd_nms_aligned3d_f32, lib.msmd_nms_aligned3d_workspace_bytes
    assert need(100, 100) == lib.msmd_nms_workspace_bytes(100, 100) >= 100 * 2 * 8
    assert need(100, 16385) == 0 and need(-1, 10) == 0
    ok = (p, 7, p, 1, 100, 100, p, 100, None, p, 100, p)
    assert nms(*ok, None, 0, None) == WORKSPACE                              # workspace missing
    assert nms(*ok, p, need(100, 100) - 1, None) == WORKSPACE                # ... too small
    assert nms(*ok, ctypes.c_void_p(260), need(100, 100), None) == WORKSPACE  # ... misaligned
    assert nms(None, 7, p, 1, 100, 100, p, 100, None, p, 100, p, p, 1 << 20, None) == INVALID
    assert nms(p, 7, None, 1, 100, 100, p, 100, None, p, 100, p, p, 1 << 20, None) == INVALID
    assert nms(p, 7, p, 1, 100, 100, None, 100, None, p, 100, p, p, 1 << 20, None) == INVALID
    assert nms(p, 7, p, 1, 100, 100, p, 100, None, None, 100, p, p, 1 << 20, None) == INVALID
    assert nms(p, 7, p, 1, 100, 100, p, 100, None, p, 100, None, p, 1 << 20, None) == INVALID
    assert nms(p, 6, p, 1, 100, 100, p, 100, None, p, 100, p, p, 1 << 20, None) == INVALID  # no class
    assert nms(p, 7, p, -1, 100, 100, p, 100, None, p, 100, p, p, 1 << 20, None) == INVALID
    assert nms(p, 7, p, 1, -100, 100, p, 100, None, p, 100, p, p, 1 << 20, None) == INVALID
    assert nms(p, 7, p, 1, 100, 100, p, -1, None, p, 100, p, p, 1 << 20, None) == INVALID
    assert nms(p, 7, p, 1, 100000, 16385, p, 100, None, p, 100, p, p, 1 << 30, None) == INVALID
    assert nms(p, 7, p, 70000, 100, 100, p, 100, None, p, 100, p, p, 1 << 20, None) == RANGE
    assert nms(p, 7, p, 0, 100, 100, p, 100, None, p, 100, p, None, 0, None) == 0   # no segments


def test_python_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from msmdfusion_amd import kernels as K
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.chamfer_forward(z(1, 4, 3), z(1, 5, 3), "l2")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.vote_targets(z(8, 3), z(2, dtype=torch.int32), z(1, 7), z(1, 3), z(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.points_in_boxes_count(z(1, 2, 7), z(1, 8, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.nms_segments("aligned3d", z(4, 7), z(2, dtype=torch.int32), z(1), 4)
