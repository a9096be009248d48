"""msmd_roi_assign3d_f32 / msmd_roi_sample_targets_f32 (csrc/roi_targets.hip) against the
composition path -- the reference's per-sample, per-class loop on K.boxes_iou3d matrices with
the key-based random_choice, host reads included (PartAggregationROIHead with fused=False) -- on
every scheduling edge and on constructed situations.

Discrete results (gt_inds, labels, the sampled rows, counts, masks, weights, label) are compared
with torch.equal, max_overlaps bit for bit.  bbox_targets is float32 arithmetic: the kernel has
to be within 4 x the float32 composition's own error against the float64 composition, floored
at one float32 ulp at the value's scale.  Every case keeps its IoUs MARGIN away from every
threshold (tests/parta2_roi_cases.py asserts it), so nothing discrete hangs on a rounding.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parta2_roi_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)
CLS_CFG = dict(cls_pos_thr=0.75, cls_neg_thr=0.25)


def assigner_cfg():
    return dict(type="MaxIoUAssigner", iou_calculator=dict(type="BboxOverlaps3D",
                                                           coordinate="lidar"),
                pos_iou_thr=0.55, neg_iou_thr=0.55, min_pos_iou=0.55, ignore_iof_thr=-1)


def sampler_cfg(**kw):
    cfg = dict(type="IoUNegPiecewiseSampler", num=16, pos_fraction=0.55,
               neg_piece_fractions=[0.8, 0.2], neg_iou_piece_thrs=[0.55, 0.1], neg_pos_ub=-1,
               add_gt_as_proposals=False, return_iou=True)
    cfg.update(kw)
    return cfg


def roi_head(fused, classes=3, single=False, **sampler_kw):
    from msmdfusion_amd.parta2_roi_head import PartAggregationROIHead
    from msmdfusion_amd.semantic_head import PointwiseSemanticHead
    train_cfg = dict(assigner=assigner_cfg() if single else [assigner_cfg() for _ in range(classes)],
                     sampler=sampler_cfg(**sampler_kw), **CLS_CFG)
    return PartAggregationROIHead(PointwiseSemanticHead(in_channels=16, num_classes=classes),
                                  num_classes=classes, train_cfg=train_cfg, fused=fused)


@pytest.fixture(scope="module")
def bbox_head():
    from msmdfusion_amd.parta2_bbox_head import PartA2BboxHead
    return PartA2BboxHead(num_classes=3, seg_in_channels=16, part_in_channels=4,
                          seg_conv_channels=[16], part_conv_channels=[16],
                          merge_conv_channels=[32], down_conv_channels=[32],
                          shared_fc_channels=[32, 32], cls_channels=[32], reg_channels=[32],
                          roi_feat_size=4)


def lists(case, dev):
    proposals = [dict(boxes_3d=torch.from_numpy(p).to(dev), labels_3d=torch.from_numpy(l).to(dev))
                 for p, l in zip(case["props"], case["prop_labels"])]
    return proposals, [torch.from_numpy(g).to(dev) for g in case["gt"]], \
        [torch.from_numpy(l).to(dev) for l in case["gt_labels"]]


def assign_inputs(case, dev):
    """The case's flat lists on the device: the arguments of K.roi_assign3d, and the offsets."""
    single = case["single"]
    classes = 1 if single else case["classes"]
    poffs = np.cumsum([0] + [p.shape[0] for p in case["props"]]).tolist()
    goffs = np.cumsum([0] + [g.shape[0] for g in case["gt"]]).tolist()
    cat = lambda xs, dt: torch.from_numpy(np.concatenate(xs).astype(dt)).to(dev)   # noqa: E731
    args = (cat(case["props"], np.float32).reshape(-1, 7),
            None if single else cat(case["prop_labels"], np.int64), poffs,
            cat(case["gt"], np.float32).reshape(-1, 7), cat(case["gt_labels"], np.int64), goffs,
            [0.55] * classes, [0.55] * classes, [0.55] * classes)
    return args, dict(single=single), poffs


def fused_assign(case, dev, inputs=None):
    """K.roi_assign3d on the case's flat lists -> per sample (gt_inds, max_overlaps, labels)."""
    from msmdfusion_amd import kernels as K
    args, kw, poffs = inputs if inputs is not None else assign_inputs(case, dev)
    out = K.roi_assign3d(*args, **kw)
    return [tuple(t[poffs[b]:poffs[b + 1]] for t in out) for b in range(len(case["props"]))]


def loop_assign(case, dev):
    head = roi_head(False, case["classes"], case["single"])
    proposals, gts, gt_labels = lists(case, dev)
    out = []
    for p, g, l in zip(proposals, gts, gt_labels):
        a = head._assign_composed(p["boxes_3d"], p["labels_3d"], g, l)
        out.append((a.gt_inds, a.max_overlaps, a.labels))
    return out


def check_assign(case, dev):
    got, want = fused_assign(case, dev), loop_assign(case, dev)
    for b, ((gi, ov, lb), (gi_c, ov_c, lb_c)) in enumerate(zip(got, want)):
        assert gi.dtype == torch.int32 and lb.dtype == torch.long and ov.dtype == torch.float32
        assert torch.equal(gi.long(), gi_c), b
        assert torch.equal(ov.view(torch.int32), ov_c.view(torch.int32)), b       # bit for bit
        assert torch.equal(lb, lb_c), b
    return got


ASSIGN_SHAPES = [((1,), (1,)), ((63,), (0,)), ((64,), (63,)), ((65,), (64,)),
                 ((255, 0, 3), (65, 2, 4)), ((256, 7), (129, 0)), ((257,), (1,)),
                 ((257, 64, 65), (129, 63, 64))]


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("index", range(len(ASSIGN_SHAPES)))
def test_assignment_against_the_loop_on_every_edge(dev, index, single):
    props, gts = ASSIGN_SHAPES[index]
    case = RC.make_case(200 + index, props, gts, classes=3, single=single)
    got = check_assign(case, dev)
    if index >= 4:
        total = torch.cat([g[0] for g in got])
        assert int((total > 0).sum()) > 0 and int((total == 0).sum()) > 0


def test_assignment_on_constructed_situations(dev):
    rng = np.random.RandomState(7)
    gt, _ = RC.make_gt(rng, 6, 3)
    gt_labels = np.asarray([0, 0, 1, 1, -1, 2], np.int64)
    jitter = lambda g, s: (gt[g] + np.asarray([s, s, 0, 0, 0, 0, 0.02], np.float32))   # noqa: E731
    # class 0: proposals and ground truth; class 1: ground truth only ... (proposal 4 aside);
    # class 2: its only ground truth far from its proposals; the -1 box matches nobody
    props = np.stack([jitter(0, 0.05), jitter(0, 0.4), jitter(1, 0.1), jitter(4, 0.0),
                      jitter(2, 0.05), jitter(3, 0.05) + np.asarray([50, 0, 0, 0, 0, 0, 0],
                                                                    np.float32)])
    prop_labels = np.asarray([0, 0, 0, 0, 1, 2], np.int64)
    case = dict(props=[props], prop_labels=[prop_labels], gt=[gt], gt_labels=[gt_labels],
                classes=3, single=False)
    RC.assert_margins(props, prop_labels, gt, gt_labels, 3)
    (gi, ov, lb), = check_assign(case, dev)
    assert gi.tolist()[0] == 1 and gi.tolist()[2] == 2 and gi.tolist()[3] == 0
    assert float(ov[3]) == 0.0 and gi.tolist()[4] == 3 and gi.tolist()[5] == 0
    assert lb.tolist() == [0, lb.tolist()[1], 0, -1, 1, -1]
    # a class without ground truth, a sample without ground truth, an empty proposal list
    empty = dict(props=[props, props[:0], props], prop_labels=[prop_labels, prop_labels[:0],
                                                                np.full(6, 2, np.int64)],
                 gt=[gt[:2], gt, gt[:0]], gt_labels=[gt_labels[:2], gt_labels, gt_labels[:0]],
                 classes=3, single=False)
    got = check_assign(empty, dev)
    assert got[0][0].tolist()[4:] == [0, 0] and got[2][0].tolist() == [0] * 6
    assert got[1][0].numel() == 0


def test_twin_ground_truths_and_the_low_quality_override(dev):
    rng = np.random.RandomState(8)
    gt, _ = RC.make_gt(rng, 3, 1)
    gt = np.concatenate([gt, gt[1:2]])                         # 1 and 3 are twins
    gt_labels = np.zeros(4, np.int64)
    near = lambda g, s: (gt[g] + np.asarray([s * gt[g][3], 0, 0, 0, 0, 0, 0], np.float32))  # noqa: E731
    props = np.stack([near(1, 0.02), near(1, 0.1), near(0, 0.03), near(2, 0.3)])
    labels = np.zeros(4, np.int64)
    RC.assert_margins(props, labels, gt, gt_labels, 1, twins=True)
    for single in (False, True):
        case = dict(props=[props], prop_labels=[labels], gt=[gt], gt_labels=[gt_labels],
                    classes=1, single=single)
        (gi, ov, _), = check_assign(case, dev)
        # rule 3 gives the arg-max to the lowest index (1); rule 4 hands the twins' best proposal
        # to the last claimant (3)
        assert gi.tolist()[:2] == [4, 2]
    # a low-quality match overriding the arg-max: proposal 0 sits on box A, and is also the best
    # (the only) proposal of the later box B that overlaps A
    a = gt[0]
    b = a + np.asarray([0.18 * a[3] * np.cos(a[6]), 0.18 * a[3] * np.sin(a[6]), 0, 0, 0, 0, 0],
                       np.float32)
    pair = np.stack([a, b]).astype(np.float32)
    props = np.stack([near(0, 0.01)])
    RC.assert_margins(props, np.zeros(1, np.int64), pair, np.zeros(2, np.int64), 1)
    iou = RC.pair_iou(props, pair)[0]
    assert iou[0] > iou[1] >= 0.55 + RC.MARGIN
    case = dict(props=[props], prop_labels=[np.zeros(1, np.int64)], gt=[pair],
                gt_labels=[np.zeros(2, np.int64)], classes=1, single=False)
    (gi, ov, _), = check_assign(case, dev)
    assert gi.tolist() == [2] and abs(float(ov[0]) - float(iou[0])) < 1e-5


def test_nan_boxes_stay_in_their_own_rows(dev):
    case = RC.make_case(31, (70, 20), (9, 5), classes=3)
    clean = fused_assign(case, dev)
    dirty = dict(case, props=[p.copy() for p in case["props"]], gt=[g.copy() for g in case["gt"]],
                 prop_labels=list(case["prop_labels"]), gt_labels=list(case["gt_labels"]))
    nan_row = np.full((1, 7), np.nan, np.float32)
    half = dirty["props"][0][:1].copy()
    half[0, 4] = np.nan
    dirty["props"][0] = np.concatenate([dirty["props"][0], nan_row, half])
    dirty["prop_labels"][0] = np.concatenate([dirty["prop_labels"][0], [0, 1]])
    dirty["gt"][1] = np.concatenate([dirty["gt"][1], nan_row])          # last: indices stay
    dirty["gt_labels"][1] = np.concatenate([dirty["gt_labels"][1], [2]])
    got = fused_assign(dirty, dev)
    for b in range(2):
        n = case["props"][b].shape[0]
        for k in range(3):
            assert torch.equal(got[b][k][:n], clean[b][k]), (b, k)
    assert got[0][0][-2:].tolist() == [-1, -1] and bool(torch.isnan(got[0][1][-2:]).all())
    assert got[0][2][-2:].tolist() == [-1, -1]
    assert int((got[1][0] == 6).sum()) == 0                              # nobody gets the NaN box


def test_assignment_is_reproducible_waits_for_nothing_and_forms_no_matrix(dev):
    from msmdfusion_amd import kernels as K
    case = RC.make_case(32, (257, 64), (65, 3), classes=3)
    inputs = assign_inputs(case, dev)
    first = fused_assign(case, dev, inputs)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = fused_assign(case, dev, inputs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(first, second):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    # P x G = 2048 x 1024: the IoU matrix alone would be 8 MiB
    rng = np.random.RandomState(1)
    p, g = 2048, 1024
    boxes = lambda n: torch.from_numpy(np.concatenate(                     # noqa: E731
        [rng.uniform(0, 40, (n, 2)), rng.uniform(-1, 1, (n, 1)), rng.uniform(1.5, 4, (n, 3)),
         rng.uniform(-3, 3, (n, 1))], 1).astype(np.float32)).to(dev)
    props, gts = boxes(p), boxes(g)
    pl = torch.from_numpy(rng.randint(0, 3, p)).to(dev)
    gl = torch.from_numpy(rng.randint(0, 3, g)).to(dev)
    run = lambda: K.roi_assign3d(props, pl, [0, p], gts, gl, [0, g], [0.55] * 3, [0.55] * 3,   # noqa: E731
                                 [0.55] * 3)
    run()                                                                # the scratch buffer exists
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = run()
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before <= (1 << 20), "something of size P x G"
    want = K.boxes_iou3d(gts, props).t()
    want = torch.where(pl[:, None] == gl[None, :], want, torch.zeros_like(want)).max(1)[0]
    assert torch.equal(out[1].view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------ sampling + targets
def law_case(index, dev, equal_keys=False):
    """A sampler law (parta2_roi_cases.SAMPLER_LAWS) as kernel inputs: assignment results with
    the law's category counts, random RoIs about five ground truths, yaws on both sides of the
    orientation flip."""
    law = RC.SAMPLER_LAWS[index]
    gt_inds, overlaps = RC.law_inputs(law, 50 + index)
    rng = np.random.RandomState(90 + index)
    n = len(gt_inds)
    for attempt in range(20):
        gt, _ = RC.make_gt(rng, 5, 3)
        gt_inds = np.where(gt_inds > 0, rng.randint(1, 6, n), gt_inds)
        rois = gt[np.clip(gt_inds - 1, 0, None)].astype(np.float64)
        rois[:, :3] += rng.uniform(-0.3, 0.3, (n, 3))
        rois[:, 3:6] *= rng.uniform(0.8, 1.2, (n, 3))
        # every second positive faces the other way (the orientation flip), whole turns on top
        rank = np.cumsum(gt_inds > 0) - 1
        rois[:, 6] += rng.uniform(-0.6, 0.6, n) + np.where(rank % 2 == 1, np.pi, 0.0) \
            + 2 * np.pi * rng.randint(-2, 3, n)
        rois = rois.astype(np.float32)
        rel = RC.canonical_yaw(rois, gt)[np.arange(n), np.clip(gt_inds - 1, 0, None)]
        if min(np.abs(rel - np.pi / 2).min(), np.abs(rel - 3 * np.pi / 2).min()) >= RC.YAW_MARGIN:
            break
    else:
        raise AssertionError("no draw keeps the yaw margin")
    flipped = (rel > np.pi / 2) & (rel < 3 * np.pi / 2) & (gt_inds > 0)
    assert (gt_inds > 0).sum() < 2 or (flipped.any() and (~flipped & (gt_inds > 0)).any())
    for t in RC.CLS_THR:
        assert np.abs(overlaps.astype(np.float64) - t).min() > RC.MARGIN
    keys = RC.make_keys(index, n, equal=equal_keys)
    to = lambda a: torch.from_numpy(a).to(dev)                            # noqa: E731
    return law, to(rois), to(gt_inds), to(overlaps), to(keys), to(gt)


def sample_fused(law, rois, gt_inds, overlaps, keys, gt, batch=1):
    from msmdfusion_amd import kernels as K
    num, pos_fraction, fractions, thrs, ub, _ = law
    n, g = rois.shape[0], gt.shape[0]
    rep = lambda t: torch.cat([t] * batch).contiguous()                   # noqa: E731
    return K.roi_sample_targets(rep(rois), [n * b for b in range(batch + 1)],
                                rep(gt_inds).int(), rep(overlaps), rep(keys), rep(gt),
                                [g * b for b in range(batch + 1)], num, int(num * pos_fraction), ub,
                                fractions, thrs, 0.75, 0.25)


def sample_composed(law, rois, gt_inds, overlaps, keys, gt, bbox_head):
    from msmdfusion_amd.anchor_head import AssignResult
    from msmdfusion_amd.parta2_roi_head import IoUNegPiecewiseSampler
    num, pos_fraction, fractions, thrs, ub, _ = law
    smp = IoUNegPiecewiseSampler(num, pos_fraction, fractions, thrs, ub, return_iou=True)
    a = AssignResult(gt.shape[0], gt_inds, overlaps, torch.zeros_like(gt_inds))
    res = smp.sample(a, rois, gt, torch.zeros(gt.shape[0], dtype=torch.long, device=gt.device),
                     keys=keys)
    t32 = bbox_head._get_target_single(res.pos_bboxes, res.pos_gt_bboxes, res.iou, CLS_CFG)
    t64 = bbox_head._get_target_single(res.pos_bboxes.double(), res.pos_gt_bboxes.double(),
                                       res.iou.double(), CLS_CFG)
    return res, t32, t64


def check_sample(out, s, res, t32, t64, rois):
    n_pos, n_neg = res.pos_inds.numel(), res.neg_inds.numel()
    assert out["counts"][s].tolist() == [n_pos, n_neg]
    n = n_pos + n_neg
    inds = torch.cat([res.pos_inds, res.neg_inds])
    assert torch.equal(out["inds"][s, :n].long(), inds)
    assert bool((out["inds"][s, n:] == -1).all())
    assert bool((out["rois"][s, :n, 0] == s).all())
    assert torch.equal(out["rois"][s, :n, 1:], rois[inds])
    assert torch.equal(out["iou"][s, :n], res.iou)
    label, bbox_targets, pos_gt, reg_mask, label_weights, bbox_weights = t32
    assert torch.equal(out["label"][s, :n], label)
    assert torch.equal(out["label_weights"][s, :n], label_weights)
    assert torch.equal(out["reg_mask"][s, :n], reg_mask)
    assert torch.equal(out["bbox_weights"][s, :n], bbox_weights)
    assert torch.equal(out["pos_gt_bboxes"][s, :n_pos], pos_gt)
    for key in ("rois", "iou", "label", "label_weights", "reg_mask", "bbox_weights",
                "pos_gt_bboxes", "bbox_targets"):
        assert float(out[key][s, n:].abs().sum()) == 0, key                # padding rows
    assert float(out["bbox_targets"][s, n_pos:].abs().sum()) == 0
    if n_pos:
        ref = t64[1]
        scale = ref.abs().clamp(min=1.0)
        err_c = float(((bbox_targets.double() - ref).abs() / scale).max())
        err_k = float(((out["bbox_targets"][s, :n_pos].double() - ref).abs() / scale).max())
        print("bbox_targets error: kernel %.3e, composition %.3e" % (err_k, err_c))
        assert err_k <= 4.0 * err_c + EPS, (err_k, err_c)
        assert float(ref[:, 6].abs().max()) <= np.pi / 2
    return n_pos, n_neg


@pytest.mark.parametrize("index", range(len(RC.SAMPLER_LAWS)))
def test_sampling_and_targets_against_the_loop(dev, bbox_head, index):
    args = law_case(index, dev)
    out = sample_fused(*args, batch=2)
    res, t32, t64 = sample_composed(*args, bbox_head)
    law = args[0]
    n_pos_all, pieces, outside = law[5][0], list(law[5][1:-1]), law[5][-1]
    n_pos, taken, taken_out = RC.quotas_ref(n_pos_all, pieces, outside, law[0], law[1], law[2],
                                            law[4])
    for s in range(2):
        got = check_sample(out, s, res, t32, t64, args[1])
        assert got == (n_pos, sum(taken) + taken_out)


@pytest.mark.parametrize("index", [0, 2, 8])
def test_equal_keys_go_to_the_lower_index(dev, bbox_head, index):
    args = law_case(index, dev, equal_keys=True)
    assert len(torch.unique(args[4])) <= 4
    out = sample_fused(*args)
    check_sample(out, 0, *sample_composed(*args, bbox_head), args[1])
    again = sample_fused(*args)
    for key, value in out.items():
        assert torch.equal(value.view(torch.uint8) if value.is_floating_point() else value,
                           again[key].view(torch.uint8) if value.is_floating_point()
                           else again[key]), key


def test_head_fused_equals_composed_and_reads_the_host_once(dev, bbox_head):
    """PartAggregationROIHead._assign_and_sample + get_targets, fused against fused=False with
    one generator seed, on real assignments; under the sync-debug mode the fused path waits for
    the device exactly once (the counts)."""
    import warnings
    case = RC.make_case(33, (120, 0, 90), (9, 4, 0), classes=3)
    case["gt_labels"][0][1] = -1
    proposals, gts, gt_labels = lists(case, dev)
    fused, composed = roi_head(True, num=32), roi_head(False, num=32)
    gen = lambda: torch.Generator(device=dev).manual_seed(5)              # noqa: E731
    batch = fused._assign_and_sample(proposals, gts, gt_labels, generator=gen())
    results = composed._assign_and_sample(proposals, gts, gt_labels, generator=gen())
    from msmdfusion_amd.parta2_roi_head import RoISampleBatch, bbox3d2roi
    assert isinstance(batch, RoISampleBatch) and isinstance(results, list)
    assert batch.counts == [(r.pos_inds.numel(), r.neg_inds.numel()) for r in results]
    assert batch.counts[0][0] > 0 and batch.counts[0][1] > 0 and batch.counts[1] == (0, 0)
    assert torch.equal(batch.rois, bbox3d2roi([r.bboxes for r in results]))
    got = bbox_head.get_targets(batch, CLS_CFG)
    want = bbox_head.get_targets(results, CLS_CFG)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, k
        if k == 1:
            assert float((a - b).abs().max()) <= 1e-5
        else:
            assert torch.equal(a, b), k
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            keys = fused.draw_keys([p["boxes_3d"] for p in proposals], gen())
            bbox_head.get_targets(fused._assign_and_sample(proposals, gts, gt_labels, keys=keys),
                                  CLS_CFG)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchroniz" in str(w.message).lower()
             and "prototype" not in str(w.message)]
    assert len(syncs) <= 1, [str(w.message) for w in syncs]


def test_sizes_above_the_caps_take_the_composition_path(dev):
    from msmdfusion_amd import kernels as K
    head = roi_head(True, num=K.ROI_SAMPLE_MAX_NUM + 1)
    case = RC.make_case(34, (20,), (3,), classes=3)
    proposals, gts, gt_labels = lists(case, dev)
    assert isinstance(head._assign_and_sample(proposals, gts, gt_labels), list)
    assert not isinstance(roi_head(True)._assign_and_sample(proposals, gts, gt_labels), list)
