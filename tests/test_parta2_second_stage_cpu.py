"""Part-A2's second stage without a GPU: the composition paths (the reference's assign loop,
IoUNegPiecewiseSampler, _get_target_single, the loss) against vectors the reference's own classes
produced (tests/golden/make_parta2_second_stage_golden.py) and against independent numpy
restatements (tests/parta2_roi_cases.py), with the oracle's 3-D IoU standing in for the kernel;
constructor arithmetic and state-dict keys, registries, both configs, the sampler's law, the
refusals and the C ABI's host-side argument checks."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parta2_roi_cases as RC  # noqa: E402


class OracleOverlaps:
    """BboxOverlaps3D(coordinate='lidar') on the CPU oracle."""
    coordinate = "lidar"

    def __call__(self, bboxes1, bboxes2, mode="iou"):
        return torch.from_numpy(RC.iou3d(bboxes1.numpy(), bboxes2.numpy()))


def assigner(**kw):
    from msmdfusion_amd.parta2_roi_head import MaxIoUAssigner3D
    args = dict(pos_iou_thr=0.55, neg_iou_thr=0.55, min_pos_iou=0.55, ignore_iof_thr=-1,
                iou_calculator=OracleOverlaps())
    args.update(kw)
    return MaxIoUAssigner3D(**args)


def sampler(**kw):
    from msmdfusion_amd.parta2_roi_head import IoUNegPiecewiseSampler
    args = dict(num=16, pos_fraction=0.55, neg_piece_fractions=[0.8, 0.2],
                neg_iou_piece_thrs=[0.55, 0.1], neg_pos_ub=-1, add_gt_as_proposals=False,
                return_iou=True)
    args.update(kw)
    return IoUNegPiecewiseSampler(**args)


def roi_head(classes=3, single=False, **kw):
    """The RoI head's assignment machinery alone (no extractors, no bbox head), fused=False."""
    from msmdfusion_amd.parta2_roi_head import PartAggregationROIHead
    from msmdfusion_amd.semantic_head import PointwiseSemanticHead
    one = assigner()
    train_cfg = dict(assigner=one if single else [assigner() for _ in range(classes)],
                     sampler=sampler(**kw), cls_pos_thr=0.75, cls_neg_thr=0.25)
    return PartAggregationROIHead(PointwiseSemanticHead(in_channels=16, num_classes=classes),
                                  num_classes=classes, train_cfg=train_cfg, fused=False)


def lists(case):
    proposals = [dict(boxes_3d=torch.from_numpy(p), labels_3d=torch.from_numpy(l))
                 for p, l in zip(case["props"], case["prop_labels"])]
    return proposals, [torch.from_numpy(g) for g in case["gt"]], \
        [torch.from_numpy(l) for l in case["gt_labels"]]


# ------------------------------------------------------------------ composition paths
@pytest.mark.parametrize("single", [False, True])
def test_assign_loop_matches_the_restatement(single):
    case = RC.make_case(3, (40, 0, 25), (7, 3, 0), classes=3, single=single)
    case["gt_labels"][0][2] = -1                       # KITTI's ignored class
    head = roi_head(single=single)
    proposals, gts, gt_labels = lists(case)
    results = head._assign_and_sample(proposals, gts, gt_labels,
                                      generator=torch.Generator().manual_seed(0))
    assert len(results) == 3
    seen_pos = 0
    for b, res in enumerate(results):
        iou = RC.pair_iou(case["props"][b], case["gt"][b])
        mask = RC.class_mask(case["prop_labels"][b], case["gt_labels"][b], 3, single)
        ref_inds, ref_ov, ref_lab = RC.assign_ref(np.where(mask, iou, 0).astype(np.float32), mask,
                                                  case["prop_labels"][b], case["gt_labels"][b], 3,
                                                  single)
        a = res.assign_result
        assert np.array_equal(a.gt_inds.numpy(), ref_inds)
        assert np.array_equal(a.max_overlaps.numpy(), ref_ov)
        assert np.array_equal(a.labels.numpy(), ref_lab)
        seen_pos += int((ref_inds > 0).sum())
        # the sampled rows are positives ascending, then negatives ascending
        assert np.all(np.diff(res.pos_inds.numpy()) > 0) and np.all(np.diff(res.neg_inds.numpy()) > 0)
        assert tuple(res.pos_gt_bboxes.shape) == (res.pos_inds.numel(), 7)   # [0, 7] without gt
        assert torch.equal(res.iou, a.max_overlaps[torch.cat([res.pos_inds, res.neg_inds])])
    assert seen_pos >= 5


@pytest.mark.parametrize("index", range(len(RC.SAMPLER_LAWS)))
def test_sampler_law_over_many_keys(index):
    """Category counts, quotas incl. extend_num, the last-piece rule, neg_pos_ub and both early
    returns; and over many key draws every member of a category is drawn equally often."""
    from msmdfusion_amd.anchor_head import AssignResult
    law = RC.SAMPLER_LAWS[index]
    num, pos_fraction, fractions, thrs, ub, counts = law
    smp = sampler(num=num, pos_fraction=pos_fraction, neg_piece_fractions=fractions,
                  neg_iou_piece_thrs=thrs, neg_pos_ub=ub)
    gt_inds, overlaps = RC.law_inputs(law, 50 + index)
    n_pos_all, piece_counts, outside = RC.counts_of(gt_inds, overlaps, thrs)
    assert (n_pos_all, *piece_counts, outside) == counts
    n_pos, taken, taken_outside = RC.quotas_ref(n_pos_all, piece_counts, outside, num, pos_fraction,
                                                fractions, ub)
    assert n_pos + sum(taken) + taken_outside <= num
    bboxes = torch.zeros((len(gt_inds), 7))
    hits = np.zeros(len(gt_inds))
    rounds = 40
    gen = torch.Generator().manual_seed(index)
    for _ in range(rounds):
        a = AssignResult(1, torch.from_numpy(gt_inds), torch.from_numpy(overlaps),
                         torch.zeros(len(gt_inds), dtype=torch.long))
        res = smp.sample(a, bboxes, torch.zeros((1, 7)), torch.zeros(1, dtype=torch.long),
                         generator=gen)
        pos, neg = res.pos_inds.numpy(), res.neg_inds.numpy()
        assert len(pos) == n_pos and (gt_inds[pos] > 0).all()
        assert (gt_inds[neg] == 0).all() and len(neg) == sum(taken) + taken_outside
        got = RC.counts_of(np.where(np.isin(np.arange(len(gt_inds)), neg), 0, -1), overlaps, thrs)
        assert got[1] == taken and got[2] == taken_outside
        hits[pos] += 1
        hits[neg] += 1
    assert hits[gt_inds < 0].sum() == 0
    if 0 < n_pos < n_pos_all:                            # a strict subset is drawn, not a fixed one
        assert (hits[gt_inds > 0] > 0).sum() > n_pos


def test_random_choice_takes_the_smallest_keys_with_ties_to_the_lower_index():
    from msmdfusion_amd.parta2_roi_head import IoUNegPiecewiseSampler as S
    keys = torch.tensor([0.5, 0.25, 0.5, 0.25, 0.75, 0.0])
    gallery = torch.tensor([0, 1, 2, 3, 4])
    assert S.random_choice(gallery, 3, keys).tolist() == [1, 3, 0]
    assert S.random_choice(gallery, 0, keys).numel() == 0
    assert sorted(S.random_choice(torch.tensor([2, 4, 5]), 2, keys).tolist()) == [2, 5]


def bbox_head(**kw):
    from msmdfusion_amd.parta2_bbox_head import PartA2BboxHead
    args = dict(num_classes=3, seg_in_channels=16, part_in_channels=4, seg_conv_channels=[16, 16],
                part_conv_channels=[16, 16], merge_conv_channels=[32, 32],
                down_conv_channels=[32, 32], shared_fc_channels=[32, 48, 48], cls_channels=[32, 32],
                reg_channels=[32, 32], roi_feat_size=4,
                loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, reduction="sum",
                               loss_weight=1.0),
                loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, reduction="sum",
                              loss_weight=1.0))
    args.update(kw)
    return PartA2BboxHead(**args)


@pytest.fixture(scope="module")
def small_head():
    torch.manual_seed(0)
    return bbox_head()


def test_get_target_single_in_float64_matches_the_restatement(small_head):
    rng = np.random.RandomState(4)
    gt, _ = RC.make_gt(rng, 12, 3)
    rois = gt.astype(np.float64) + rng.uniform(-0.2, 0.2, gt.shape)
    rois[:, 6] = gt[:, 6] + np.tile([0.1, np.pi - 0.1, -0.3, 7.0, -np.pi + 0.2, -9.0], 2)
    ious = np.concatenate([rng.uniform(0.76, 0.9, 6), rng.uniform(0.26, 0.74, 6),
                           rng.uniform(0.0, 0.24, 8)])
    cfg = dict(cls_pos_thr=0.75, cls_neg_thr=0.25)
    out = small_head._get_target_single(torch.from_numpy(rois), torch.from_numpy(gt).double(),
                                        torch.from_numpy(ious), cfg)
    label, bbox_targets, pos_gt, reg_mask, label_weights, bbox_weights = out
    assert bbox_targets.dtype == torch.float64
    ref = RC.bbox_targets_ref(rois, gt)
    assert np.abs(bbox_targets.numpy() - ref).max() < 1e-12
    assert np.abs(ref[:, 6]).max() <= np.pi / 2 and ref[:, 6].min() < 0 < ref[:, 6].max()
    want = np.where(ious > 0.75, 1.0, np.where(ious < 0.25, 0.0, ious * 2 - 0.5))
    assert np.array_equal(label.numpy(), want)
    assert reg_mask.tolist() == [1] * 12 + [0] * 8 and bbox_weights.tolist() == [1.0] * 12 + [0.0] * 8
    assert label_weights.tolist() == [1.0] * 20
    # no positive: the reference's empty [0, 7]
    none = small_head._get_target_single(torch.zeros((0, 7)), torch.zeros((0, 7)),
                                         torch.from_numpy(ious[12:]).float(), cfg)
    assert tuple(none[1].shape) == (0, 7) and none[3].sum() == 0


def test_get_targets_concatenates_and_normalises(small_head):
    class Res:
        pass
    rng = np.random.RandomState(5)
    results = []
    for n_pos, n_all in ((3, 9), (0, 5)):
        r = Res()
        gt, _ = RC.make_gt(rng, n_pos, 3)
        r.pos_bboxes = torch.from_numpy(gt + 0.1)
        r.pos_gt_bboxes = torch.from_numpy(gt).reshape(-1, 7)
        r.iou = torch.from_numpy(rng.uniform(0, 1, n_all).astype(np.float32))
        results.append(r)
    label, bbox_targets, pos_gt, reg_mask, label_weights, bbox_weights = small_head.get_targets(
        results, dict(cls_pos_thr=0.75, cls_neg_thr=0.25))
    assert tuple(label.shape) == (14,) and tuple(bbox_targets.shape) == (3, 7)
    assert tuple(pos_gt.shape) == (3, 7) and reg_mask.tolist() == [1] * 3 + [0] * 11
    assert abs(float(bbox_weights.sum()) - 1) < 1e-6 and abs(float(label_weights.sum()) - 1) < 1e-6


def corners_np(boxes):
    unit = np.asarray([[-0.5, -0.5, 0], [-0.5, -0.5, 1], [-0.5, 0.5, 1], [-0.5, 0.5, 0],
                       [0.5, -0.5, 0], [0.5, -0.5, 1], [0.5, 0.5, 1], [0.5, 0.5, 0]])
    c = boxes[:, None, 3:6] * unit[None]
    cs, sn = np.cos(boxes[:, 6])[:, None], np.sin(boxes[:, 6])[:, None]
    x, y = c[..., 0] * cs + c[..., 1] * sn, -c[..., 0] * sn + c[..., 1] * cs
    return np.stack([x, y, c[..., 2]], -1) + boxes[:, None, :3]


def test_corner_loss_and_masked_loss_terms(small_head):
    rng = np.random.RandomState(6)
    gt, _ = RC.make_gt(rng, 6, 3)
    pred = (gt + rng.uniform(-0.5, 0.5, gt.shape)).astype(np.float32)
    got = small_head.get_corner_loss_lidar(torch.from_numpy(pred), torch.from_numpy(gt)).numpy()
    a, b = corners_np(pred.astype(np.float64)), corners_np(gt.astype(np.float64))
    flip = gt.astype(np.float64).copy()
    flip[:, 6] += np.pi
    d = np.minimum(np.linalg.norm(a - b, axis=2), np.linalg.norm(a - corners_np(flip), axis=2))
    q = np.minimum(d, 1.0)
    want = (0.5 * q**2 + (d - q)).mean(1)
    assert np.abs(got - want).max() < 1e-4
    # loss: rows 1, 3 positive; the masked sums equal the reference's gathered form
    rois = torch.from_numpy(np.concatenate([np.zeros((5, 1), np.float32), gt[:5]], 1))
    reg_mask = torch.tensor([0, 1, 0, 1, 0])
    cls_score = torch.randn(5, 1, generator=torch.Generator().manual_seed(1))
    bbox_pred = (torch.randn(5, 7, generator=torch.Generator().manual_seed(2)) * 0.1
                 ).requires_grad_(True)
    targets = torch.randn(2, 7, generator=torch.Generator().manual_seed(3)) * 0.1
    pos_gt = torch.from_numpy(gt[[1, 3]] + 0.05)
    label, lw, bw = torch.rand(5), torch.ones(5) / 5, reg_mask.float() / 2
    losses = small_head.loss(cls_score, bbox_pred, rois, label, targets, pos_gt, reg_mask, lw, bw)
    assert sorted(losses) == ["loss_bbox", "loss_cls", "loss_corner"]
    pos = reg_mask > 0
    diff = (bbox_pred[pos] - targets).abs()
    beta = 1.0 / 9.0
    want_bbox = (torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)
                 * bw[pos][:, None]).sum()
    assert abs(float(losses["loss_bbox"].detach()) - float(want_bbox.detach())) < 1e-6
    decoded = small_head.decode_rois(rois[pos], bbox_pred[pos].detach())
    want_corner = small_head.get_corner_loss_lidar(decoded, pos_gt).mean()
    assert abs(float(losses["loss_corner"].detach()) - float(want_corner)) < 1e-6
    (losses["loss_bbox"] + losses["loss_corner"]).backward()
    assert float(bbox_pred.grad[~pos].abs().sum()) == 0 and float(bbox_pred.grad[pos].abs().sum()) > 0
    # nothing positive: the fake zero, finite, with a zero gradient
    none = small_head.loss(cls_score, bbox_pred, rois, label, targets[:0], pos_gt[:0],
                           torch.zeros(5, dtype=torch.long), lw, torch.zeros(5))
    assert float(none["loss_bbox"]) == 0.0 and float(none["loss_corner"]) == 0.0


# ------------------------------------------------------------------ construction
def reference_keys(part, seg, merge, down, shared, cls, reg, dropout):
    """The state-dict keys the reference's constructor yields (parta2_bbox_head.py:81-221):
    SparseSequential children by position, ConvModule's conv / bn, and the Dropout insertions
    that shift the indices of shared_fc / conv_cls / conv_reg."""
    bn = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    keys = []
    for name, count in (("part_conv", len(part)), ("seg_conv", len(seg)),
                        ("conv_down.merge_conv", len(merge)), ("conv_down.down_conv", len(down))):
        for i in range(count):
            keys += ["%s.%d.0.weight" % (name, i)] + ["%s.%d.1.%s" % (name, i, b) for b in bn]
    pos = 0
    for k in range(1, len(shared)):
        keys += ["shared_fc.%d.conv.weight" % pos] + ["shared_fc.%d.bn.%s" % (pos, b) for b in bn]
        pos += 1
        if k != len(shared) - 1 and dropout > 0:
            pos += 1
    for name, chans in (("conv_cls", cls), ("conv_reg", reg)):
        slots = list(range(len(chans) + 1))
        if dropout >= 0:
            slots = [s if s < 1 else s + 1 for s in slots]
        for s in slots[:-1]:
            keys += ["%s.%d.conv.weight" % (name, s)] + ["%s.%d.bn.%s" % (name, s, b) for b in bn]
        keys += ["%s.%d.conv.weight" % (name, slots[-1]), "%s.%d.conv.bias" % (name, slots[-1])]
    return keys


@pytest.fixture(scope="module")
def built():
    """Both configs built ONCE (the 87808-input shared_fc is 180 MB), with the config copies."""
    from msmdfusion_amd import configs, registry
    out = {}
    for name in ("PARTA2_SECFPN_KITTI_3CLASS", "PARTA2_SECFPN_KITTI_CAR"):
        cfg = getattr(configs, name)["model"]
        before = copy.deepcopy(cfg)
        out[name] = (registry.build_detector(cfg), cfg, before)
    return out


@pytest.mark.parametrize("name", ["PARTA2_SECFPN_KITTI_3CLASS", "PARTA2_SECFPN_KITTI_CAR"])
def test_configs_build_the_detector_unmodified(built, name):
    from msmdfusion_amd import detector, parta2_bbox_head, parta2_roi_head, parta2_rpn_head
    det, cfg, before = built[name]
    assert cfg == before
    assert type(det) is detector.PartA2
    assert type(det.rpn_head) is parta2_rpn_head.PartA2RPNHead
    head = det.roi_head
    assert type(head) is parta2_roi_head.PartAggregationROIHead and head.fused
    assert type(head.bbox_head) is parta2_bbox_head.PartA2BboxHead
    classes = cfg["roi_head"]["num_classes"]
    if classes == 1:
        assert isinstance(head.bbox_assigner, parta2_roi_head.MaxIoUAssigner3D)
    else:
        assert [type(a) for a in head.bbox_assigner] == [parta2_roi_head.MaxIoUAssigner3D] * 3
    smp = head.bbox_sampler
    assert (smp.num, smp.pos_fraction, smp.neg_piece_fractions, smp.neg_iou_thr, smp.neg_pos_ub,
            smp.return_iou) == (128, 0.55, [0.8, 0.2], [0.55, 0.1], -1, True)
    assert head.train_cfg["cls_pos_thr"] == 0.75 and head.test_cfg["nms_thr"] == 0.01
    bh = cfg["roi_head"]["bbox_head"]
    state = head.bbox_head.state_dict()
    assert list(state) == reference_keys(bh["part_conv_channels"], bh["seg_conv_channels"],
                                         bh["merge_conv_channels"], bh["down_conv_channels"],
                                         bh["shared_fc_channels"], bh["cls_channels"],
                                         bh["reg_channels"], bh["dropout_ratio"])
    assert tuple(state["shared_fc.0.conv.weight"].shape) == (512, 256 * 7**3, 1)     # 87808
    assert tuple(state["conv_cls.3.conv.weight"].shape) == (1, 256, 1)
    assert tuple(state["conv_reg.3.conv.weight"].shape) == (7, 256, 1)
    assert tuple(state["conv_down.merge_conv.0.0.weight"].shape)[-1] == 128
    assert float(state["conv_reg.3.conv.weight"].std()) < 0.002                       # N(0, 0.001)
    assert float(state["conv_reg.3.conv.bias"].abs().sum()) == 0
    prefixes = {k.split(".")[0] for k in det.state_dict()}
    assert prefixes == {"backbone", "neck", "rpn_head", "roi_head", "middle_encoder"}
    assert {k.split(".")[1] for k in det.state_dict() if k.startswith("roi_head.")} == \
        {"semantic_head", "bbox_head"}
    # the kernels' caps hold the config's shape with room
    from msmdfusion_amd import kernels as K
    assert K.ROI_SAMPLE_MAX_PROPOSALS >= 2 * 512 and K.ROI_SAMPLE_MAX_NUM >= 2 * 128
    assert K.ROI_SAMPLE_MAX_PIECES >= 4 and K.ROI_ASSIGN_MAX_CLASSES >= 2 * 3


def test_constructor_defaults_and_dropout_indices():
    import inspect
    from msmdfusion_amd.parta2_bbox_head import PartA2BboxHead
    from msmdfusion_amd.parta2_roi_head import IoUNegPiecewiseSampler, PartAggregationROIHead
    sig = inspect.signature(PartA2BboxHead.__init__).parameters
    assert list(sig)[1:] == ["num_classes", "seg_in_channels", "part_in_channels",
                             "seg_conv_channels", "part_conv_channels", "merge_conv_channels",
                             "down_conv_channels", "shared_fc_channels", "cls_channels",
                             "reg_channels", "dropout_ratio", "roi_feat_size", "with_corner_loss",
                             "bbox_coder", "conv_cfg", "norm_cfg", "loss_bbox", "loss_cls"]
    assert (sig["dropout_ratio"].default, sig["roi_feat_size"].default,
            sig["with_corner_loss"].default) == (0.1, 14, True)
    assert sig["norm_cfg"].default == dict(type="BN1d", eps=1e-3, momentum=0.01)
    assert sig["loss_bbox"].default == dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=2.0)
    assert sig["loss_cls"].default == dict(type="CrossEntropyLoss", use_sigmoid=True,
                                           reduction="none", loss_weight=1.0)
    assert list(inspect.signature(PartAggregationROIHead.__init__).parameters)[1:8] == [
        "semantic_head", "num_classes", "seg_roi_extractor", "part_roi_extractor", "bbox_head",
        "train_cfg", "test_cfg"]
    assert list(inspect.signature(IoUNegPiecewiseSampler.__init__).parameters)[1:] == [
        "num", "pos_fraction", "neg_piece_fractions", "neg_iou_piece_thrs", "neg_pos_ub",
        "add_gt_as_proposals", "return_iou"]
    for dropout in (0.1, 0.0, -1.0):
        head = bbox_head(dropout_ratio=dropout)
        assert list(head.state_dict()) == reference_keys([16, 16], [16, 16], [32, 32], [32, 32],
                                                         [32, 48, 48], [32, 32], [32, 32], dropout)
    head = bbox_head()
    assert head.shared_fc[0].conv.in_channels == 32 * 2**3 and head.shared_fc[0].bn.eps == 1e-3
    assert head.conv_cls[-1].bn is None and head.conv_cls[-1].activate is None


def test_registries():
    from msmdfusion_amd import registry
    registry.build_head(dict(type="PointwiseSemanticHead", in_channels=16))     # fills HEADS
    assert "PartA2BboxHead" in registry.HEADS and "PartAggregationROIHead" in registry.HEADS
    smp = registry.build_sampler(dict(type="IoUNegPiecewiseSampler", num=8, pos_fraction=0.5,
                                      neg_piece_fractions=[1.0], neg_iou_piece_thrs=[0.5]))
    assert "IoUNegPiecewiseSampler" in registry.BBOX_SAMPLERS and smp.num == 8
    from msmdfusion_amd import detector  # noqa: F401
    assert "PartA2" in registry.DETECTORS


# ------------------------------------------------------------------ refusals
def test_refusals():
    from msmdfusion_amd import parta2_roi_head as R
    with pytest.raises(NotImplementedError):
        sampler(add_gt_as_proposals=True)
    for bad in (dict(ignore_iof_thr=0.5), dict(match_low_quality=False),
                dict(gt_max_assign_all=False), dict(neg_iou_thr=(0.1, 0.5)), dict(neg_iou_thr=0),
                dict(iou_calculator=dict(type="BboxOverlapsNearest3D")),
                dict(iou_calculator=dict(type="BboxOverlaps3D", coordinate="camera"))):
        with pytest.raises(NotImplementedError):
            assigner(**bad)
    with pytest.raises(NotImplementedError):
        R.build_assigner(dict(type="HungarianAssigner3D"))
    with pytest.raises(KeyError):
        R.build_sampler(dict(type="RandomSampler", num=4))
    assert not sampler(neg_piece_fractions=[0.8, 0.6, 0.1],
                       neg_iou_piece_thrs=[0.5, 0.3, 0.1]).fits_kernel()
    assert not sampler(neg_iou_piece_thrs=[0.1, 0.55]).fits_kernel()
    assert not sampler(pos_fraction=1.5).fits_kernel()        # more positives than `num` rows
    assert sampler().fits_kernel()


def test_empty_cells_raise_before_any_launch(small_head):
    """CPU tensors: a launch would be refused with another error, so the RuntimeError shows
    that the decision was taken on the host from the count."""
    seg = torch.zeros((3, 4, 4, 4, 16))
    part = torch.zeros((3, 4, 4, 4, 4))
    with pytest.raises(RuntimeError, match="no active cell"):
        small_head(seg, part)


def test_c_abi_refusals():
    from msmdfusion_amd._lib import float_arr, lib
    p = ctypes.c_void_p(256)                              # never dereferenced: every call is refused
    INVALID, WORKSPACE, RANGE = -1, -2, -5
    ints = lambda *v: (ctypes.c_int * len(v))(*v)         # noqa: E731
    thr = float_arr([0.55] * 8)
    big = 1 << 20
    assign = lib.msmd_roi_assign3d_f32

    def call(props=p, plab=p, poffs=ints(0, 10), gts=p, glab=p, goffs=ints(0, 4), batch=1,
             classes=3, single=0, pos=thr, out=p, ws=p, ws_bytes=big):
        return assign(props, plab, poffs, gts, glab, goffs, batch, classes, single, pos, thr, thr,
                      out, p, p, ws, ws_bytes, None)

    assert call(batch=0) == 0 and call(poffs=ints(0, 0)) == 0       # nothing to do
    assert call(batch=-1) == INVALID and call(classes=0) == INVALID and call(single=2) == INVALID
    assert call(batch=lib.msmd_roi_assign_max_samples() + 1) == RANGE
    assert call(classes=lib.msmd_roi_assign_max_classes() + 1) == RANGE
    assert call(poffs=ints(1, 10)) == INVALID and call(poffs=ints(0, -1)) == INVALID
    assert call(goffs=None) == INVALID and call(pos=None) == INVALID
    assert call(props=None) == INVALID and call(out=None) == INVALID
    assert call(plab=None) == INVALID and call(plab=None, single=1, ws_bytes=0) == WORKSPACE
    assert call(gts=None) == INVALID and call(glab=None) == INVALID
    assert call(ws=None) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    assert call(ws=ctypes.c_void_p(258)) == WORKSPACE
    assert lib.msmd_roi_assign3d_workspace_bytes(-1) == 0
    assert lib.msmd_roi_assign3d_workspace_bytes(1000) >= 4000

    sample = lib.msmd_roi_sample_targets_f32
    frac = (ctypes.c_double * 2)(0.8, 0.2)

    def draw(poffs=ints(0, 10), goffs=ints(0, 4), batch=1, num=16, expected=8, ub=-1.0, pieces=2,
             fractions=frac, thrs=float_arr([0.55, 0.1]), props=p, keys=p, out=p, counts=p):
        return sample(props, poffs, p, p, keys, p, goffs, batch, num, expected, ub, pieces,
                      fractions, thrs, 0.75, 0.25, out, p, p, p, p, p, p, p, p, counts, None)

    assert draw(batch=0) == 0
    assert draw(num=0) == INVALID and draw(expected=-1) == INVALID and draw(pieces=0) == INVALID
    assert draw(ub=float("nan")) == INVALID and draw(num=16, expected=17) == INVALID
    assert draw(num=lib.msmd_roi_sample_max_num() + 1) == RANGE
    assert draw(pieces=lib.msmd_roi_sample_max_pieces() + 1) == RANGE
    assert draw(poffs=ints(0, lib.msmd_roi_sample_max_proposals() + 1)) == RANGE
    assert draw(fractions=None) == INVALID and draw(thrs=None) == INVALID
    assert draw(fractions=(ctypes.c_double * 2)(1.5, 0.2)) == INVALID
    assert draw(pieces=3, fractions=(ctypes.c_double * 3)(0.8, 0.6, 0.1),
                thrs=float_arr([0.5, 0.3, 0.1])) == INVALID                 # they sum above 1
    assert draw(thrs=float_arr([0.1, 0.55])) == INVALID                     # ascending bounds
    assert draw(props=None) == INVALID and draw(keys=None) == INVALID
    assert draw(out=None) == INVALID and draw(counts=None) == INVALID
    assert draw(goffs=ints(0, -4)) == INVALID
    assert (lib.msmd_roi_sample_max_proposals(), lib.msmd_roi_assign_gt_chunk()) == (2048, 64)


# ------------------------------------------------------------------ the reference's own vectors
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "parta2_second_stage_vectors.npz")
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def golden_lists(gold, tag, to=lambda t: t):
    t = lambda k: to(torch.from_numpy(gold[k]))                              # noqa: E731
    proposals = [dict(boxes_3d=t("%s_props_%d" % (tag, b)), labels_3d=t("%s_prop_labels_%d" % (tag, b)))
                 for b in range(2)]
    return proposals, [t("%s_gt_%d" % (tag, b)) for b in range(2)], \
        [t("%s_gt_labels_%d" % (tag, b)) for b in range(2)], \
        torch.cat([t("%s_keys_%d" % (tag, b)) for b in range(2)])


def close_to_golden(got, gold, key, ref32=None, ref64=None):
    """Within 4 x the reference's own float32 error of its float64 run, which counts as one ulp
    of the tensor's largest entry at the least (the form of tests/test_gpu_h3d_head.py)."""
    ref32 = gold[key].astype(np.float64) if ref32 is None else np.asarray(ref32, np.float64)
    ref64 = gold[key + "64"] if ref64 is None else np.asarray(ref64, np.float64)
    got = got.detach().cpu().double().numpy()
    assert got.shape == ref64.shape, key
    if not ref64.size:
        return
    err, err_ref = np.abs(got - ref64).max(), np.abs(ref32 - ref64).max()
    bound = 4.0 * max(err_ref, EPS * np.abs(ref64).max())
    assert err <= bound, (key, err, err_ref, bound)


@pytest.mark.parametrize("tag", ["c3", "car"])
def test_composition_paths_match_the_reference(gold, small_head, tag):
    single = tag == "car"
    head = roi_head(classes=1 if single else 3, single=single, num=24)
    proposals, gts, gt_labels, keys = golden_lists(gold, tag)
    results = head._assign_and_sample(proposals, gts, gt_labels, keys=keys)
    for b, res in enumerate(results):
        g = lambda k: gold["%s_%s_%d" % (tag, k, b)]                         # noqa: E731
        a = res.assign_result
        assert np.array_equal(a.gt_inds.numpy(), g("gt_inds"))
        assert np.array_equal(a.max_overlaps.numpy(), g("max_overlaps"))
        assert np.array_equal(a.labels.numpy(), g("labels"))
        assert np.array_equal(res.pos_inds.numpy(), g("pos_inds"))
        assert np.array_equal(res.neg_inds.numpy(), g("neg_inds"))
        assert np.array_equal(res.iou.numpy(), g("iou"))
        wide = small_head._get_target_single(res.pos_bboxes.double(), res.pos_gt_bboxes.double(),
                                             res.iou.double(), dict(cls_pos_thr=0.75,
                                                                    cls_neg_thr=0.25))
        assert np.abs(wide[1].numpy() - g("single64_bbox_targets")).max() < 1e-12
    targets = small_head.get_targets(results, dict(cls_pos_thr=0.75, cls_neg_thr=0.25))
    names = ("label", "bbox_targets", "pos_gt_bboxes", "reg_mask", "label_weights", "bbox_weights")
    for name, got in zip(names, targets):
        want = gold["%s_targets_%s" % (tag, name)]
        if name == "bbox_targets":
            wide = np.concatenate([gold["%s_single64_bbox_targets_%d" % (tag, b)] for b in range(2)])
            close_to_golden(got, gold, name, ref32=want, ref64=wide)
        else:
            assert np.array_equal(got.numpy(), want), name
    # the loss, on the reference's targets
    from msmdfusion_amd.parta2_roi_head import bbox3d2roi
    rois = bbox3d2roi([r.bboxes for r in results])
    assert np.array_equal(rois.numpy(), gold[tag + "_rois"])
    cls_score = torch.from_numpy(gold[tag + "_cls_score"]).requires_grad_(True)
    bbox_pred = torch.from_numpy(gold[tag + "_bbox_pred"]).requires_grad_(True)
    losses = small_head.loss(cls_score, bbox_pred, rois, *targets)
    close_to_golden(losses["loss_cls"], gold, tag + "_loss_cls")
    close_to_golden(losses["loss_bbox"], gold, tag + "_loss_bbox")
    close_to_golden(losses["loss_corner"], gold, "loss_corner",
                    ref32=gold[tag + "_loss_corner_vector"].astype(np.float64).mean(),
                    ref64=gold[tag + "_loss_corner_vector64"].mean())
    sum(losses.values()).backward()
    close_to_golden(cls_score.grad, gold, tag + "_grad_cls_score")
    close_to_golden(bbox_pred.grad, gold, tag + "_grad_bbox_pred")


def golden_head_cfg():
    return dict(merge_conv_channels=[32], down_conv_channels=[16, 16], shared_fc_channels=[16, 48, 48],
                dropout_ratio=0.0)


def test_state_dict_keys_and_shapes_are_the_reference_constructors(gold):
    """The reference's own __init__ (on the generator's spconv stand-ins) against this head."""
    head = bbox_head(**golden_head_cfg())
    keys = [str(k) for k in gold["head_state_keys"]]
    state = head.state_dict()
    assert list(state) == keys
    for k in keys:
        assert tuple(state[k].shape) == gold["head_weight_" + k].shape, k
    head.load_state_dict({k: torch.from_numpy(gold["head_weight_" + k]) for k in keys})
    assert keys == reference_keys([16, 16], [16, 16], [32], [16, 16], [16, 48, 48], [32, 32],
                                  [32, 32], 0.0)
