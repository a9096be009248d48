"""SSD3DHead and SSD3DNet on the GPU: targets, losses and boxes against the reference's outputs
(tests/golden/ssd3d_head_vectors.npz) and the per-sample restatement (tests/ssd3d_ref.py), no
host read in get_targets, loss gradients against float64 autograd, the reference's
test_ssd3d_head shapes and a training / inference step of the detector built from the config.

Tolerance for the float32 chains (centerness, the loss values): the head's error against the
float64 restatement may be at most 4 x the reference's (the golden's) error against it plus one
float32 ulp at 1.0 -- see tests/test_gpu_ssd3d_ops.py."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ssd3d_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

ULP1 = float(np.spacing(np.float32(1.0)))
BATCH, CANDIDATES, CLASSES, BINS = 3, 64, 3, 12
POS_THR, EXPAND = 1.0, 0.05
TEST_CFGS = dict(
    per_class=dict(nms_cfg=dict(type="nms", iou_thr=0.1), sample_mod="spec", score_thr=0.0,
                   per_class_proposal=True, max_output_num=100),
    cut=dict(nms_cfg=dict(type="nms", iou_thr=0.1), sample_mod="spec", score_thr=0.4,
             per_class_proposal=False, max_output_num=8))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "ssd3d_head_vectors.npz")))


def _t(a, dev=None):
    t = torch.from_numpy(np.asarray(a))
    return t if dev is None else t.to(dev)


def build_head(dev, num_classes=CLASSES, candidates=CANDIDATES, test_cfg=None, **train):
    """SSD3DHead from the KITTI config with the golden case's sizes."""
    from msmdfusion_amd import configs as C
    from msmdfusion_amd import registry
    cfg = copy.deepcopy(C.SSD3D_KITTI_CAR["model"])
    head = cfg["bbox_head"]
    head["num_classes"] = num_classes
    head["vote_module_cfg"]["num_points"] = candidates
    head["vote_aggregation_cfg"]["num_point"] = candidates
    train_cfg = dict(cfg["train_cfg"], pos_distance_thr=POS_THR, expand_dims_length=EXPAND)
    train_cfg.update(train)
    torch.manual_seed(0)
    return registry.build_head(dict(head, train_cfg=train_cfg,
                                    test_cfg=test_cfg or cfg["test_cfg"])).to(dev)


def gold_scene(gold, dev=None):
    from msmdfusion_amd.head_loss import LiDARBoxes
    boxes = [torch.zeros(0, 7), _t(gold["gt_boxes_1"]), _t(gold["gt_boxes_2"])]
    labels = [torch.zeros(0, dtype=torch.long), _t(gold["gt_labels_1"]), _t(gold["gt_labels_2"])]
    if dev is not None:
        boxes, labels = [b.to(dev) for b in boxes], [v.to(dev) for v in labels]
    return [LiDARBoxes(b) for b in boxes], labels


def gold_preds(gold, dev, dtype=torch.float32, grad=False):
    """The golden's random maps through the coder's split -> (prediction dict, the three leaf
    maps)."""
    from msmdfusion_amd.vote_head import AnchorFreeBBoxCoder
    leaves = [_t(gold[k], dev).to(dtype).requires_grad_(grad)
              for k in ("cls_preds", "reg_preds", "vote_offset")]
    agg = _t(gold["aggregated_points"], dev).to(dtype)
    preds = dict(seed_points=_t(gold["seed_points"], dev).to(dtype), aggregated_points=agg,
                 vote_offset=leaves[2])
    preds.update(AnchorFreeBBoxCoder(BINS).split_pred(leaves[0], leaves[1], agg))
    return preds, leaves


def f64_targets(gold):
    boxes = [torch.zeros(0, 7), _t(gold["gt_boxes_1"]), _t(gold["gt_boxes_2"])]
    labels = [torch.zeros(0, dtype=torch.long), _t(gold["gt_labels_1"]), _t(gold["gt_labels_2"])]
    return S.targets(boxes, labels, _t(gold["aggregated_points"]), _t(gold["seed_points"]),
                     CANDIDATES, CLASSES, BINS, POS_THR, EXPAND, dtype=torch.float64)


# ----------------------------------------------------------------------------------- targets
def test_get_targets_against_the_golden(dev, gold):
    head = build_head(dev)
    boxes, labels = gold_scene(gold)                       # on the host, as a loader leaves them
    preds, _ = gold_preds(gold, dev)
    before = [b.tensor.clone() for b in boxes]
    got = head.get_targets(None, boxes, labels, None, None, preds)
    assert len(got) == len(S.ALL_TARGET_NAMES) and len(boxes[0]) == 0     # the lists are left alone
    assert all(torch.equal(a.tensor, b) for a, b in zip(boxes, before))
    t64 = dict(zip(S.ALL_TARGET_NAMES, f64_targets(gold)))
    for name, value in zip(S.ALL_TARGET_NAMES, got):
        want = _t(gold["targets_" + name])
        assert value.dtype == want.dtype and value.shape == want.shape, name
        if name == "centerness_targets":
            ref_err = float((want.double() - t64[name]).abs().max())
            own_err = float((value.cpu().double() - t64[name]).abs().max())
            print("centerness error vs float64: head %.3g, reference %.3g" % (own_err, ref_err))
            assert own_err <= 4 * ref_err + ULP1, (own_err, ref_err)
        else:
            assert torch.equal(value.cpu(), want), name
    # ground truths that already live on the device: the same integers and masks
    boxes_dev, labels_dev = gold_scene(gold, dev)
    again = head.get_targets(None, boxes_dev, labels_dev, None, None, preds)
    for name, a, b in zip(S.ALL_TARGET_NAMES, got, again):
        if a.dtype in (torch.long, torch.bool) or name in ("vote_mask", "centerness_weights",
                                                           "box_loss_weights",
                                                           "heading_res_loss_weight"):
            assert torch.equal(a, b), name


def test_get_targets_reads_nothing_back(dev, gold):
    head = build_head(dev)
    preds, _ = gold_preds(gold, dev)
    for on in (None, dev):
        boxes, labels = gold_scene(gold, on)
        head.get_targets(None, boxes, labels, None, None, preds)        # warm: constants, caches
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = head.get_targets(None, boxes, labels, None, None, preds)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert got[10].shape == (BATCH, CANDIDATES)


def test_losses_against_the_golden(dev, gold):
    head = build_head(dev)
    boxes, labels = gold_scene(gold)
    preds, _ = gold_preds(gold, dev)
    losses = head.loss(preds, None, boxes, labels)
    assert list(losses) == ["centerness_loss", "center_loss", "dir_class_loss", "dir_res_loss",
                            "size_res_loss", "corner_loss", "vote_loss"]
    preds64, _ = gold_preds(gold, "cpu", torch.float64)
    l64 = S.losses(preds64, f64_targets(gold), BINS)
    for k, v in losses.items():
        ref_err = abs(float(gold["loss_" + k]) - float(l64[k]))
        own_err = abs(float(v) - float(l64[k]))
        print("%s: %.7g (reference %.7g, float64 %.9g): error %.3g against the reference's %.3g"
              % (k, float(v), float(gold["loss_" + k]), float(l64[k]), own_err, ref_err))
        assert own_err <= 4 * ref_err + ULP1, (k, own_err, ref_err)


def test_loss_gradients_against_float64_autograd(dev, gold):
    """Every gradient entry is a sum of at most 24 float32 products (the corner loss: 8 corners
    x 3 coordinates per box parameter), each no larger than the largest entry: 32 x 2^-23 of
    that as the absolute part, 1e-5 relative for the few operations of a single term."""
    head = build_head(dev)
    boxes, labels = gold_scene(gold)
    preds, leaves = gold_preds(gold, dev, grad=True)
    sum(head.loss(preds, None, boxes, labels).values()).backward()
    preds64, leaves64 = gold_preds(gold, "cpu", torch.float64, grad=True)
    sum(S.losses(preds64, f64_targets(gold), BINS).values()).backward()
    for name, a, b in zip(("cls_preds", "reg_preds", "vote_offset"), leaves, leaves64):
        got, want = a.grad.cpu().double(), b.grad
        assert float(want.abs().max()) > 0, name
        bound = 1e-5 * want.abs() + 32 * 2.0 ** -23 * float(want.abs().max())
        worst = float(((got - want).abs() - bound).max())
        print("%s: largest gradient %.3g, largest difference %.3g" % (
            name, float(want.abs().max()), float((got - want).abs().max())))
        assert worst <= 0, (name, worst)


# ------------------------------------------------------------------------------------- boxes
def box_preds(gold, dev):
    preds, _ = gold_preds(gold, dev)
    preds["center"] = _t(gold["boxes_in_center"], dev)
    preds["obj_scores"] = _t(gold["boxes_in_obj_scores"], dev)
    return preds


@pytest.mark.parametrize("tag", sorted(TEST_CFGS))
def test_get_bboxes_against_the_golden_and_the_loop(dev, gold, tag):
    from msmdfusion_amd.head_loss import LiDARBoxes
    head = build_head(dev, test_cfg=TEST_CFGS[tag])
    preds = box_preds(gold, dev)
    points = _t(gold["points"], dev)
    with torch.no_grad():
        results = head.get_bboxes(points, preds, None)
        loop = S.get_bboxes(preds, BINS, TEST_CFGS[tag])
    assert len(results) == BATCH
    for b, (boxes, scores, labels) in enumerate(results):
        assert isinstance(boxes, LiDARBoxes) and boxes.with_yaw
        # the loop on the same device: everything equal
        assert torch.equal(boxes.tensor, loop[b][0]), (tag, b)
        assert torch.equal(scores, loop[b][1]) and torch.equal(labels, loop[b][2]), (tag, b)
        # the reference's CPU run: the same selection; scores and boxes up to the device's
        # sigmoid and sine (one float32 ulp of O(1) values, and of coordinates below 256)
        want = _t(gold["boxes_%s_%d_tensor" % (tag, b)])
        assert boxes.tensor.shape == want.shape, (tag, b)
        assert torch.equal(labels.cpu(), _t(gold["boxes_%s_%d_labels" % (tag, b)])), (tag, b)
        assert float((boxes.tensor.cpu() - want).abs().max()) <= 2 ** -15, (tag, b)
        assert float((scores.cpu() - _t(gold["boxes_%s_%d_scores" % (tag, b)])).abs().max()) \
            <= 2 * ULP1, (tag, b)
        if tag == "cut":
            assert len(boxes) <= 8 and bool((scores >= 0.4).all())
        else:
            assert len(boxes) % CLASSES == 0 and len(boxes) > 0
            k = len(boxes) // CLASSES
            assert labels.tolist() == [c for c in range(CLASSES) for _ in range(k)]
            assert torch.equal(boxes.tensor[:k], boxes.tensor[k:2 * k])    # the same selection
            assert torch.equal(scores[:k], scores[2 * k:])


def test_a_box_far_from_every_point_is_still_returned(dev, gold):
    """The reference's non-empty mask is `box_indices >= 0`: true for every box."""
    from msmdfusion_amd.head_loss import LiDARBoxes
    head = build_head(dev, test_cfg=TEST_CFGS["per_class"])
    preds = box_preds(gold, dev)
    points = _t(gold["points"], dev)
    with torch.no_grad():
        boxes, scores, _ = head.get_bboxes(points, preds, None)[0]
    far = LiDARBoxes(_t(gold["boxes_decoded"][0, 7:8], dev), origin=(0.5, 0.5, 1.0))
    assert bool((far.points_in_boxes(points[0, :, :3]) == -1).all())     # it holds no point
    assert bool((boxes.tensor == far.tensor[0]).all(1).any())            # and is returned
    assert float(far.tensor[0, 0]) == 200.0


def test_oversized_samples_are_refused(dev):
    head = build_head(dev, num_classes=1)
    n = 10000
    with pytest.raises(NotImplementedError, match="10000"):
        head.nms_keep_mask(torch.zeros(1, n, 4, device=dev), torch.zeros(1, n, device=dev),
                           torch.zeros(1, n, dtype=torch.long, device=dev))


# ------------------------------------------------------------- the reference's own test shapes
def test_reference_head_test_shapes_and_signs(dev):
    """tests/test_models/test_heads/test_heads.py test_ssd3d_head: 2 x 128 seeds, 64 candidates,
    five random boxes of label 0 per sample."""
    from msmdfusion_amd.head_loss import LiDARBoxes
    head = build_head(dev, num_classes=1, pos_distance_thr=10.0)
    g = torch.Generator().manual_seed(0)
    feats = dict(sa_xyz=[torch.rand(2, 128, 3, generator=g).to(dev)],
                 sa_features=[torch.rand(2, 256, 128, generator=g).to(dev)],
                 sa_indices=[torch.randint(0, 64, (2, 128), generator=g).to(dev)])
    ret = head(feats, "spec")
    assert ret["center"].shape == (2, 64, 3) and ret["obj_scores"].shape == (2, 1, 64)
    assert ret["size"].shape == (2, 64, 3) and ret["dir_res"].shape == (2, 64, 12)
    points = [torch.rand(4000, 4, generator=g).to(dev) for _ in range(2)]
    boxes = [LiDARBoxes(torch.rand(5, 7, generator=g).to(dev)) for _ in range(2)]
    labels = [torch.zeros(5, dtype=torch.long, device=dev) for _ in range(2)]
    losses = head.loss(ret, points, boxes, labels)
    assert sorted(losses) == ["center_loss", "centerness_loss", "corner_loss", "dir_class_loss",
                              "dir_res_loss", "size_res_loss", "vote_loss"]
    for k, v in losses.items():
        assert bool(torch.isfinite(v)) and float(v) >= 0, k
    sum(losses.values()).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all())
               for p in head.parameters())
    with torch.no_grad():
        results = head.get_bboxes(torch.stack(points), ret, None)
    assert len(results) == 2
    for box, score, label in results:
        assert box.tensor.shape[1] == 7 and score.shape[0] == label.shape[0] == len(box) <= 100


# -------------------------------------------------------------------------------- the detector
def _reduced():
    from msmdfusion_amd import configs as C
    cfg = copy.deepcopy(C.SSD3D_KITTI_CAR["model"])
    cfg["backbone"].update(num_points=(256, 64, (32, 32)),
                           num_samples=((8, 8, 16), (8, 8, 16), (8, 8, 8)),
                           fps_sample_range_lists=((-1), (-1), (64, -1)))
    head = cfg["bbox_head"]
    head["vote_module_cfg"]["num_points"] = 32
    head["vote_aggregation_cfg"].update(num_point=32, sample_nums=(8, 16))
    return cfg


def _scene(dev, batch=2, n=512):
    from msmdfusion_amd.head_loss import LiDARBoxes
    rng = np.random.default_rng(5)
    points, boxes, labels = [], [], []
    for b in range(batch):
        g = 3 + b
        centre = np.concatenate([rng.uniform(2, 18, (g, 2)), rng.uniform(-1.2, -0.8, (g, 1))], 1)
        size = rng.uniform(1.5, 4.0, (g, 3))
        xyz = np.concatenate([rng.uniform(0, 20, (n, 2)), rng.uniform(-1.5, 1.0, (n, 1))], 1)
        at = rng.integers(0, g, n)
        near = rng.uniform(size=n) < 0.6
        xyz[near] = (centre[at] + [0, 0, 0.5] * size[at] +
                     rng.uniform(-0.4, 0.4, (n, 3)) * size[at])[near]
        points.append(_t(np.concatenate([xyz, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32), dev))
        row = np.concatenate([centre, size, rng.uniform(-3, 3, (g, 1))], 1).astype(np.float32)
        boxes.append(LiDARBoxes(_t(row, dev)))
        labels.append(torch.zeros(g, dtype=torch.long, device=dev))
    return points, boxes, labels


def test_training_step_of_the_detector(dev):
    from msmdfusion_amd.detector import SSD3DNet
    from msmdfusion_amd.registry import build_detector
    points, boxes, labels = _scene(dev)

    def step():
        torch.manual_seed(0)
        model = build_detector(_reduced()).to(dev).train()
        losses = model.forward_train(points, None, list(boxes), list(labels))
        total = sum(losses.values())
        total.backward()
        return model, losses, total

    model, losses, total = step()
    assert isinstance(model, SSD3DNet)
    assert sorted(losses) == ["center_loss", "centerness_loss", "corner_loss", "dir_class_loss",
                              "dir_res_loss", "size_res_loss", "vote_loss"]
    assert all(bool(torch.isfinite(v)) for v in losses.values()) and float(total) > 0
    missing = [k for k, p in model.named_parameters() if p.grad is None]
    assert not missing, missing
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    again, losses2, _ = step()
    for k in losses:
        assert torch.equal(losses[k], losses2[k]), k


def test_inference_step_of_the_detector(dev):
    from msmdfusion_amd.head_loss import LiDARBoxes
    from msmdfusion_amd.registry import build_detector
    points, _, _ = _scene(dev)
    torch.manual_seed(0)
    model = build_detector(_reduced()).to(dev).eval()
    with torch.no_grad():
        results = model.simple_test(points)
    assert len(results) == 2
    for res in results:
        boxes, scores, labels = res["boxes_3d"], res["scores_3d"], res["labels_3d"]
        assert isinstance(boxes, LiDARBoxes) and boxes.tensor.shape[1] == 7
        n = len(boxes)
        assert 0 < n <= 32 and scores.shape == (n,) and labels.shape == (n,)
        assert bool((labels == 0).all()) and bool(torch.isfinite(boxes.tensor).all())
        assert bool((scores >= 0).all()) and bool((scores <= 1).all())
