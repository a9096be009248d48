"""Part-A2's second stage on the GPU: PartA2BboxHead (forward, loss, gradients, get_bboxes),
PartAggregationROIHead (fused against fused=False, the shared RoI index) and the PartA2 detector
built from shrunken copies of the two configs.

The yardstick of forward / loss / gradients is the dense restatement of the head
(tests/parta2_roi_cases.DenseBboxHead: SubM as a dense conv3d at the active sites, BatchNorm over
the active rows, the max-pool over active inputs, the reference's loss with its boolean gathers)
run in float64; the head has to be within 4 x the restatement's own float32 error of it, which
counts as one float32 ulp of the tensor's largest entry at the least.  Shapes are small: roi_feat_size 4, 16-32 channels,
6-20 RoIs.
"""
import copy
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


def bbox_head_cfg(**kw):
    cfg = dict(type="PartA2BboxHead", num_classes=3, seg_in_channels=16, part_in_channels=4,
               seg_conv_channels=[16, 16], part_conv_channels=[16, 16],
               merge_conv_channels=[32, 32], down_conv_channels=[32, 32],
               bbox_coder=dict(type="DeltaXYZWLHRBBoxCoder"), shared_fc_channels=[32, 48, 48],
               cls_channels=[32, 32], reg_channels=[32, 32], dropout_ratio=0.0, roi_feat_size=4,
               with_corner_loss=True,
               loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, reduction="sum",
                              loss_weight=1.0),
               loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, reduction="sum",
                             loss_weight=1.0))
    cfg.update(kw)
    return cfg


def make_head(dev, seed=0, **kw):
    """The head with weights that give outputs of order one (the reference's init leaves the
    regression layer at N(0, 0.001))."""
    from msmdfusion_amd import registry
    torch.manual_seed(seed)
    head = registry.build_head(bbox_head_cfg(**kw))
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in head.named_parameters():
            if name.endswith(".conv.weight") and name.startswith(("conv_cls.3", "conv_reg.3")):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.2)
            elif p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=gen) * 0.5 + (0.75 if "weight" in name else -0.25))
        for name, b in head.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=gen) * 0.1)
            elif name.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=gen) * 0.5 + 0.5)
    return head.to(dev)


def within(got, ref32, ref64, what):
    """The 4 x criterion in the form the other head tests use (test_gpu_h3d_head.py): the error
    against the float64 run is at most four times the error of the float32 run, which counts as
    one ulp of the tensor's largest entry at the least."""
    got, ref32, ref64 = (t.detach().cpu().double() for t in (got, ref32, ref64))
    assert got.shape == ref64.shape, what
    if not ref64.numel():
        return
    err_ref = float((ref32 - ref64).abs().max())
    bound = 4.0 * max(err_ref, EPS * float(ref64.abs().max()))
    err = float((got - ref64).abs().max())
    print("%s: head %.3e, float32 reference %.3e, bound %.3e" % (what, err, err_ref, bound))
    assert err <= bound, (what, err, err_ref, bound)


def targets_for(rois_n, n_pos, seed, dev=None):
    """get_targets' six tensors for rois_n rows of which the first n_pos are positive, and the
    RoIs [rois_n, 8]."""
    rng = np.random.RandomState(seed)
    gt, _ = RC.make_gt(rng, rois_n, 3)
    rois = np.concatenate([np.zeros((rois_n, 1)), gt + rng.uniform(-0.2, 0.2, gt.shape)], 1)
    label = rng.uniform(0, 1, rois_n)
    reg_mask = (np.arange(rois_n) < n_pos).astype(np.int64)
    out = [rois.astype(np.float32), label.astype(np.float32),
           (rng.normal(size=(n_pos, 7)) * 0.2).astype(np.float32), gt[:n_pos],
           reg_mask, np.full(rois_n, 1.0 / rois_n, np.float32),
           (reg_mask / max(n_pos, 1)).astype(np.float32)]
    out = [torch.from_numpy(np.ascontiguousarray(t)) for t in out]
    return [t.to(dev) for t in out] if dev is not None else out


@pytest.mark.parametrize("train", [False, True])
def test_forward_loss_and_gradients_against_the_dense_restatement(dev, train):
    rois_n, n_pos = 8, 3
    head = make_head(dev, seed=3)
    head.train(train)
    seg, part = RC.pooled_features(21, rois_n, 4)
    twins = {d: RC.DenseBboxHead(head, d) for d in (torch.float32, torch.float64)}
    seg_d = torch.from_numpy(seg).to(dev).requires_grad_(True)
    cls_score, bbox_pred = head(seg_d, torch.from_numpy(part).to(dev))
    assert tuple(cls_score.shape) == (rois_n, 1) and tuple(bbox_pred.shape) == (rois_n, 7)
    outs = {d: t.forward(seg, part) for d, t in twins.items()}
    within(cls_score, outs[torch.float32][0], outs[torch.float64][0], "cls_score")
    within(bbox_pred, outs[torch.float32][1], outs[torch.float64][1], "bbox_pred")
    assert float(outs[torch.float64][1].abs().max()) > 0.05
    targets = targets_for(rois_n, n_pos, 22)
    losses = head.loss(cls_score, bbox_pred, *[t.to(dev) for t in targets])
    ref = {d: twins[d].loss(*outs[d], *targets) for d in twins}
    assert sorted(losses) == ["loss_bbox", "loss_cls", "loss_corner"]
    for k in losses:
        within(losses[k], ref[torch.float32][k], ref[torch.float64][k], k)
        assert float(ref[torch.float64][k]) > 0
    sum(losses.values()).backward()
    for d in twins:
        sum(ref[d].values()).backward()
    p32 = dict(twins[torch.float32].head.named_parameters())
    p64 = dict(twins[torch.float64].head.named_parameters())
    failed = []
    for name, p in head.named_parameters():
        assert p.grad is not None and float(p64[name].grad.abs().max()) > 0, name
        try:
            within(p.grad, p32[name].grad, p64[name].grad, "grad " + name)
        except AssertionError as e:                                  # (list them all)
            failed.append(e.args[0])
    assert not failed, failed
    assert float(seg_d.grad.abs().sum()) > 0


def test_forward_at_a_sparse_batch_of_twenty_rois_and_single_cells(dev):
    head = make_head(dev, seed=4).eval()
    seg, part = RC.pooled_features(23, 20, 4, fill=0.1)
    part[5], seg[5] = 0, 0                                  # RoI 5: one active cell, RoI 6: none
    part[5, 3, 2, 1], seg[5, 3, 2, 1] = 0.5, 1.0
    part[6], seg[6] = 0, 0
    with torch.no_grad():
        got = head(torch.from_numpy(seg).to(dev), torch.from_numpy(part).to(dev))
    t32, t64 = (RC.DenseBboxHead(head, d).forward(seg, part) for d in (torch.float32,
                                                                       torch.float64))
    within(got[0], t32[0], t64[0], "cls_score")
    within(got[1], t32[1], t64[1], "bbox_pred")
    with pytest.raises(RuntimeError, match="no active cell"):
        head(torch.zeros((3, 4, 4, 4, 16), device=dev), torch.zeros((3, 4, 4, 4, 4), device=dev))


def test_loss_waits_for_nothing_and_fakes_a_zero_without_positives(dev):
    head = make_head(dev, seed=5)
    cls_score = torch.randn((10, 1), device=dev, requires_grad=True)
    bbox_pred = (torch.randn((10, 7), device=dev) * 0.1).requires_grad_(True)
    for n_pos in (4, 0):
        targets = targets_for(10, n_pos, 24, dev)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            losses = head.loss(cls_score, bbox_pred, *targets)
            total = sum(losses.values())
            total.backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert all(bool(torch.isfinite(v)) for v in losses.values())
        if n_pos == 0:
            assert float(losses["loss_bbox"]) == 0 and float(losses["loss_corner"]) == 0
        else:
            assert float(losses["loss_bbox"]) > 0 and float(losses["loss_corner"]) > 0
        assert bool(torch.isfinite(bbox_pred.grad).all())


# ------------------------------------------------------------------ get_bboxes
def nms_inputs(dev, sizes, seed, classes=3):
    """RoIs, head outputs and RPN results for samples of the given sizes.  Scores are pairwise
    distinct; boxes come in tight clusters, so NMS removes some; several rows pass score_thr for
    two classes."""
    rng = np.random.RandomState(seed)
    rois, labels, preds = [], [], []
    for b, n in enumerate(sizes):
        centres, _ = RC.make_gt(rng, max(n // 3, 1), classes)
        box = centres[rng.randint(0, centres.shape[0], n)].astype(np.float64)
        box[:, :2] += rng.uniform(-0.6, 0.6, (n, 2))
        rois.append(np.concatenate([np.full((n, 1), b), box], 1).astype(np.float32))
        labels.append(torch.from_numpy(rng.randint(0, classes, n)).to(dev))
        scores = rng.permutation(n * classes).reshape(n, classes) / float(n * classes + 1)
        preds.append(torch.from_numpy(scores.astype(np.float32)).to(dev))
    total = sum(sizes)
    rois = torch.from_numpy(np.concatenate(rois)).to(dev)
    cls_score = torch.from_numpy(rng.normal(size=(total, 1)).astype(np.float32)).to(dev)
    bbox_pred = torch.from_numpy((rng.normal(size=(total, 7)) * 0.05).astype(np.float32)).to(dev)
    return rois, cls_score, bbox_pred, labels, preds


@pytest.mark.parametrize("rotate", [True, False])
def test_get_bboxes_equals_the_per_sample_per_class_loop(dev, rotate):
    from msmdfusion_amd.head_loss import LiDARBoxes
    head = make_head(dev, seed=6).eval()
    sizes = (17, 0, 6, 9)
    rois, cls_score, bbox_pred, labels, preds = nms_inputs(dev, sizes, 25)
    preds[2] = preds[2] * 0 + 0.01                         # a sample in which nothing passes
    cfg = dict(use_rotate_nms=rotate, use_raw_score=True, nms_thr=0.1, score_thr=[0.3, 0.4, 0.5])
    metas = [dict(box_type_3d=LiDARBoxes)] * len(sizes)
    import warnings
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            results = head.get_bboxes(rois, cls_score, bbox_pred, labels, preds, metas, cfg=cfg)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchroniz" in str(w.message).lower()
             and "prototype" not in str(w.message)]
    assert len(syncs) <= 1, [str(w.message) for w in syncs]
    decoded = head.decode_rois(rois, bbox_pred)
    first = np.cumsum([0] + list(sizes))
    for b in range(len(sizes)):                                      # the case is well defined
        if sizes[b]:
            RC.assert_nms_margins(decoded[first[b]:first[b + 1]].cpu().numpy(),
                                  preds[b].cpu().numpy(), cfg["score_thr"], cfg["nms_thr"], rotate)
    looped = head._get_bboxes_loop(decoded, cls_score, labels, preds, metas, cfg, first.tolist())
    for (b1, s1, l1), (b2, s2, l2) in zip(results, looped):          # the fallback above the cap
        assert torch.equal(b1.tensor, b2.tensor) and torch.equal(s1, s2) and torch.equal(l1, l2)
    twice = 0
    for b, (boxes, scores, label_preds) in enumerate(results):
        assert isinstance(boxes, LiDARBoxes)
        cur = decoded[first[b]:first[b + 1]]
        if sizes[b] == 0 or b == 2:
            assert tuple(boxes.tensor.shape) == (0, 7) and scores.numel() == 0
            assert label_preds.numel() == 0
            continue
        selected = head.multi_class_nms(preds[b], cur, cfg["score_thr"], cfg["nms_thr"], metas[b],
                                        rotate)
        assert selected.numel() > 0
        assert torch.equal(boxes.tensor, cur[selected])
        assert torch.equal(scores, cls_score[first[b]:first[b + 1]].view(-1)[selected])
        assert torch.equal(label_preds, labels[b][selected])        # the RPN's labels, as written
        twice += selected.numel() - len(set(selected.tolist()))
        kept_fraction = selected.numel() / float((preds[b] >= torch.tensor(
            cfg["score_thr"], device=dev)).sum())
        assert kept_fraction < 1.0                                   # NMS removed something
    assert twice > 0                                                 # a box kept for two classes


# ------------------------------------------------------------------ the RoI head
def roi_head_cfg(fused=True, classes=3, num=16):
    assigner = dict(type="MaxIoUAssigner", iou_calculator=dict(type="BboxOverlaps3D",
                                                               coordinate="lidar"),
                    pos_iou_thr=0.55, neg_iou_thr=0.55, min_pos_iou=0.55, ignore_iof_thr=-1)
    extractor = lambda mode: dict(type="Single3DRoIAwareExtractor",               # noqa: E731
                                  roi_layer=dict(type="RoIAwarePool3d", out_size=4,
                                                 max_pts_per_voxel=128, mode=mode))
    return dict(
        type="PartAggregationROIHead", num_classes=classes, fused=fused,
        semantic_head=dict(type="PointwiseSemanticHead", in_channels=16, extra_width=0.2,
                           seg_score_thr=0.3, num_classes=classes),
        seg_roi_extractor=extractor("max"), part_roi_extractor=extractor("avg"),
        bbox_head=bbox_head_cfg(num_classes=classes),
        train_cfg=dict(assigner=[copy.deepcopy(assigner) for _ in range(classes)]
                       if classes > 1 else assigner,
                       sampler=dict(type="IoUNegPiecewiseSampler", num=num, pos_fraction=0.55,
                                    neg_piece_fractions=[0.8, 0.2], neg_iou_piece_thrs=[0.55, 0.1],
                                    neg_pos_ub=-1, add_gt_as_proposals=False, return_iou=True),
                       **CLS_CFG),
        test_cfg=dict(use_rotate_nms=True, use_raw_score=True, nms_thr=0.01, score_thr=0.1))


def roi_inputs(dev, seed=41):
    """Two samples: ground truths, jittered proposals (margins asserted), voxel centres inside
    and about the boxes, seg features."""
    case = RC.make_case(seed, (30, 24), (5, 4), classes=3)
    rng = np.random.RandomState(seed)
    centres, ids = [], []
    for b, gt in enumerate(case["gt"]):
        pick = gt[rng.randint(0, gt.shape[0], 600)]
        centres.append(pick[:, :3] + rng.uniform(-0.6, 0.6, (600, 3)) * pick[:, 3:6]
                       + [0, 0, 0.5] * pick[:, 3:6])
        ids.append(np.full(600, b))
    centres = torch.from_numpy(np.concatenate(centres).astype(np.float32)).to(dev)
    coors = torch.zeros((centres.shape[0], 4), dtype=torch.int32, device=dev)
    coors[:, 0] = torch.from_numpy(np.concatenate(ids)).to(dev)
    seg = torch.from_numpy(rng.normal(size=(centres.shape[0], 16)).astype(np.float32)).to(dev)
    proposals = [dict(boxes_3d=torch.from_numpy(p).to(dev), labels_3d=torch.from_numpy(l).to(dev),
                      cls_preds=torch.from_numpy(rng.uniform(0, 1, (len(l), 3)).astype(
                          np.float32)).to(dev))
                 for p, l in zip(case["props"], case["prop_labels"])]
    gts = [torch.from_numpy(g).to(dev) for g in case["gt"]]
    gt_labels = [torch.from_numpy(l).to(dev) for l in case["gt_labels"]]
    return dict(feats=dict(seg_features=seg), voxels=dict(voxel_centers=centres, coors=coors),
                proposals=proposals, gts=gts, gt_labels=gt_labels)


def test_roi_head_fused_equals_composed_end_to_end(dev):
    from msmdfusion_amd import registry
    torch.manual_seed(7)
    fused = registry.build_head(roi_head_cfg(True)).to(dev)
    composed = registry.build_head(roi_head_cfg(False)).to(dev)
    composed.load_state_dict(fused.state_dict())
    data = roi_inputs(dev)
    out = {}
    for name, head in (("fused", fused), ("composed", composed)):
        feats = dict(seg_features=data["feats"]["seg_features"].clone().requires_grad_(True))
        losses = head.forward_train(feats, data["voxels"], [None, None], data["proposals"],
                                    data["gts"], data["gt_labels"],
                                    generator=torch.Generator(device=dev).manual_seed(11))
        sum(losses.values()).backward()
        out[name] = (losses, feats["seg_features"].grad)
    assert sorted(out["fused"][0]) == ["loss_bbox", "loss_cls", "loss_corner", "loss_part",
                                       "loss_seg"]
    for k, v in out["fused"][0].items():
        w = out["composed"][0][k]
        assert bool(torch.isfinite(v)) and abs(float(v) - float(w)) <= 1e-4 * max(1, abs(float(w))), k
    assert float(out["fused"][0]["loss_bbox"]) > 0 and float(out["fused"][0]["loss_corner"]) > 0
    scale = float(out["composed"][1].abs().max())
    assert scale > 0 and float((out["fused"][1] - out["composed"][1]).abs().max()) <= 1e-4 * scale
    for (n, p), (_, q) in zip(fused.named_parameters(), composed.named_parameters()):
        assert (p.grad is None) == (q.grad is None), n
        if p.grad is not None:
            s = max(float(q.grad.abs().max()), 1e-6)
            assert float((p.grad - q.grad).abs().max()) <= 2e-3 * s, n


def test_one_shared_index_equals_two_separate_ones(dev):
    from msmdfusion_amd import registry
    from msmdfusion_amd.parta2_roi_head import bbox3d2roi
    torch.manual_seed(8)
    head = registry.build_head(roi_head_cfg(True)).to(dev).eval()
    data = roi_inputs(dev, seed=42)
    rois = bbox3d2roi([p["boxes_3d"] for p in data["proposals"]])
    sem = head.semantic_head(data["feats"]["seg_features"])
    with torch.no_grad():
        res = head._bbox_forward(data["feats"]["seg_features"], sem["part_feats"], data["voxels"],
                                 rois)
        centres, ids = data["voxels"]["voxel_centers"], data["voxels"]["coors"][..., 0]
        seg = head.seg_roi_extractor(data["feats"]["seg_features"], centres, ids, rois)
        part = head.part_roi_extractor(sem["part_feats"], centres, ids, rois)
    assert torch.equal(res["pooled_seg_feats"], seg) and torch.equal(res["pooled_part_feats"], part)
    assert tuple(seg.shape) == (rois.shape[0], 4, 4, 4, 16) and float(part.abs().sum()) > 0
    results = head.simple_test(data["feats"], data["voxels"], [None, None], data["proposals"])
    assert len(results) == 2 and all(r["boxes_3d"].shape[1] == 7 for r in results)


# ------------------------------------------------------------------ the detector
def shrunken(name, dev):
    """A copy of the config at the small sparse shape of the first-stage tests ([25, 32, 32]
    voxels over a 16 m x 16 m x 6 m range), narrow BEV tail and RoI head."""
    from msmdfusion_amd import configs
    from msmdfusion_amd.sparse_unet import SparseUNet
    cfg = copy.deepcopy(getattr(configs, name)["model"])
    classes = cfg["roi_head"]["num_classes"]
    cfg["voxel_layer"].update(point_cloud_range=[0, -8, -3, 16, 8, 3], voxel_size=[0.5, 0.5, 0.25])
    cfg["middle_encoder"].update(sparse_shape=[25, 32, 32])
    with torch.no_grad():                                   # the BEV channels of this shape
        unet = SparseUNet(4, [25, 32, 32]).to(dev)
        coors = torch.tensor([[0, 3, 4, 5], [0, 10, 20, 9]], dtype=torch.int32, device=dev)
        channels = unet(torch.ones((2, 4), device=dev), coors, 1)["spatial_features"].shape[1]
    cfg["backbone"].update(in_channels=channels, layer_nums=[1, 1], out_channels=[32, 64])
    cfg["neck"].update(in_channels=[32, 64], out_channels=[32, 32])
    ranges = [[0, -8.0, r[2], 16.0, 8.0, r[5]] for r in cfg["rpn_head"]["anchor_generator"]["ranges"]]
    cfg["rpn_head"].update(in_channels=64, feat_channels=64)
    cfg["rpn_head"]["anchor_generator"].update(ranges=ranges)
    small = roi_head_cfg(True, classes)
    cfg["roi_head"]["seg_roi_extractor"] = small["seg_roi_extractor"]
    cfg["roi_head"]["part_roi_extractor"] = small["part_roi_extractor"]
    cfg["roi_head"]["bbox_head"].update({k: v for k, v in small["bbox_head"].items()
                                         if k.endswith("_channels") or k == "roi_feat_size"})
    cfg["train_cfg"]["rpn_proposal"].update(nms_pre=200, nms_post=24, max_num=24)
    cfg["train_cfg"]["rcnn"]["sampler"].update(num=16)
    cfg["test_cfg"]["rpn"].update(nms_pre=200, nms_post=12, max_num=12)
    return cfg, classes


def cloud(dev, gt, seed):
    rs = np.random.RandomState(seed)
    points = []
    for boxes in gt:
        p = rs.uniform(0, 1, (2500, 4)).astype(np.float32)
        p[:, 0], p[:, 1], p[:, 2] = p[:, 0] * 15.9, p[:, 1] * 15.9 - 7.95, p[:, 2] * 5.9 - 2.95
        inside = boxes[rs.randint(0, len(boxes), 500)]
        q = np.concatenate([inside[:, :3] + rs.uniform(-0.3, 0.3, (500, 3)) * [1, 1, 0]
                            + [0, 0, 0.5], rs.uniform(0, 1, (500, 1))], 1).astype(np.float32)
        points.append(torch.from_numpy(np.concatenate([p, q])).to(dev))
    return points


@pytest.mark.parametrize("name", ["PARTA2_SECFPN_KITTI_3CLASS", "PARTA2_SECFPN_KITTI_CAR"])
def test_detector_trains_a_step_and_infers(dev, name):
    from msmdfusion_amd import registry
    from msmdfusion_amd.head_loss import LiDARBoxes
    from msmdfusion_amd.parta2_roi_head import MaxIoUAssigner3D
    torch.manual_seed(0)
    cfg, classes = shrunken(name, dev)
    before = copy.deepcopy(cfg)
    det = registry.build_detector(cfg).to(dev)
    assert cfg == before
    assert isinstance(det.roi_head.bbox_assigner, MaxIoUAssigner3D) == (classes == 1)
    keys = list(det.state_dict())
    for prefix in ("middle_encoder.conv_input.0.weight", "backbone.blocks.0.0.weight",
                   "neck.deblocks.0.0.weight", "rpn_head.conv_cls.weight",
                   "roi_head.semantic_head.seg_cls_layer.weight",
                   "roi_head.bbox_head.part_conv.0.0.weight",
                   "roi_head.bbox_head.conv_down.merge_conv.0.0.weight",
                   "roi_head.bbox_head.shared_fc.0.conv.weight",
                   "roi_head.bbox_head.conv_reg.3.conv.bias"):
        assert prefix in keys, prefix
    gt = [np.asarray([[4.0, -3.0, -1.8, 1.6, 3.9, 1.56, 0.3], [10.0, 2.0, -1.7, 1.7, 4.1, 1.5, 1.2],
                      [12.0, -5.0, -0.6, 0.6, 0.8, 1.73, -0.4]], np.float32),
          np.asarray([[7.0, 4.0, -1.75, 1.6, 3.8, 1.6, -1.0]], np.float32)]
    gt_labels = [np.asarray([2, 2, 0]), np.asarray([2])] if classes == 3 else \
        [np.asarray([0, 0, 0]), np.asarray([0])]
    points = cloud(dev, gt, 2)
    boxes = [LiDARBoxes(torch.from_numpy(b).to(dev)) for b in gt]
    labels = [torch.from_numpy(l).long().to(dev) for l in gt_labels]
    opt = torch.optim.SGD(det.parameters(), lr=1e-3)
    losses = det(points, return_loss=True, gt_bboxes_3d=boxes, gt_labels_3d=labels,
                 generator=torch.Generator(device=dev).manual_seed(3))
    assert sorted(losses) == ["loss_bbox", "loss_cls", "loss_corner", "loss_part", "loss_rpn_bbox",
                              "loss_rpn_cls", "loss_rpn_dir", "loss_seg"]
    total = 0
    for k, v in losses.items():
        v = sum(v) if isinstance(v, list) else v
        assert bool(torch.isfinite(v)), k
        total = total + v
    opt.zero_grad()
    total.backward()
    parts = dict(middle_encoder=det.middle_encoder, backbone=det.backbone, neck=det.neck,
                 rpn_head=det.rpn_head, semantic_head=det.roi_head.semantic_head,
                 bbox_head=det.roi_head.bbox_head)
    for part, module in parts.items():
        grads = [p.grad for p in module.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(g).all()) for g in grads), part
        assert sum(float(g.abs().sum()) for g in grads) > 0, part
    params = list(det.parameters())
    old = [p.detach().clone() for p in params]
    opt.step()
    assert any(not torch.equal(a, b) for a, b in zip(old, params))
    det.eval()
    with torch.no_grad():
        results = det(points, [dict(box_type_3d=LiDARBoxes)] * 2)
    assert len(results) == 2
    for r in results:
        assert isinstance(r["boxes_3d"], LiDARBoxes) and r["boxes_3d"].tensor.shape[1] == 7
        assert r["scores_3d"].shape == r["labels_3d"].shape
        assert bool(torch.isfinite(r["boxes_3d"].tensor).all())


# ------------------------------------------------------------------ the reference's own vectors
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "parta2_second_stage_vectors.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("tag", ["c3", "car"])
def test_fused_targets_loss_and_boxes_match_the_reference(dev, gold, tag):
    """tests/golden/make_parta2_second_stage_golden.py: the reference's own _assign_and_sample,
    IoUNegPiecewiseSampler, get_targets, loss and get_bboxes, with the recorded keys."""
    from msmdfusion_amd import registry
    from msmdfusion_amd.head_loss import LiDARBoxes
    classes = 1 if tag == "car" else 3
    head = registry.build_head(roi_head_cfg(True, classes, num=24)).to(dev)
    t = lambda k: torch.from_numpy(gold[k]).to(dev)                          # noqa: E731
    proposals = [dict(boxes_3d=t("%s_props_%d" % (tag, b)), labels_3d=t("%s_prop_labels_%d" % (tag, b)))
                 for b in range(2)]
    gts = [t("%s_gt_%d" % (tag, b)) for b in range(2)]
    gt_labels = [t("%s_gt_labels_%d" % (tag, b)) for b in range(2)]
    keys = torch.cat([t("%s_keys_%d" % (tag, b)) for b in range(2)])
    batch = head._assign_and_sample(proposals, gts, gt_labels, keys=keys)
    first = 0
    for b in range(2):
        g = lambda k: gold["%s_%s_%d" % (tag, k, b)]                         # noqa: E731
        n = g("props").shape[0]
        lo = batch.assign["offsets"][b]
        assert np.array_equal(batch.assign["gt_inds"][lo:lo + n].cpu().numpy(), g("gt_inds"))
        # (the GPU's sinf / cosf / atan2f are not the host's: the IoU is the oracle's to an ulp or
        # two; everything discrete is exact, which the cases' margins are for)
        assert np.abs(batch.assign["max_overlaps"][lo:lo + n].cpu().numpy()
                      - g("max_overlaps")).max() <= 1e-5
        assert np.array_equal(batch.assign["labels"][lo:lo + n].cpu().numpy(), g("labels"))
        rows = np.concatenate([g("pos_inds"), g("neg_inds")])
        assert batch.counts[b] == (len(g("pos_inds")), len(g("neg_inds")))
        assert np.array_equal(batch.inds[first:first + len(rows)].cpu().numpy(), rows)
        first += len(rows)
    assert torch.equal(batch.rois, t(tag + "_rois"))
    targets = head.bbox_head.get_targets(batch, CLS_CFG)
    names = ("label", "bbox_targets", "pos_gt_bboxes", "reg_mask", "label_weights", "bbox_weights")
    wide = np.concatenate([gold["%s_single64_bbox_targets_%d" % (tag, b)] for b in range(2)])
    for name, got in zip(names, targets):
        want = gold["%s_targets_%s" % (tag, name)]
        if name == "bbox_targets":
            scale = np.maximum(np.abs(wide), 1.0)
            err_ref = (np.abs(want - wide) / scale).max()
            err = (np.abs(got.cpu().numpy() - wide) / scale).max()
            print("bbox_targets: kernel %.3e, the reference's float32 %.3e" % (err, err_ref))
            assert err <= 4.0 * err_ref + EPS
        elif name == "label":
            assert np.abs(got.cpu().numpy() - want).max() <= 2e-5          # iou * 2 - 0.5
            assert np.array_equal(got.cpu().numpy() == 1, want == 1)
            assert np.array_equal(got.cpu().numpy() == 0, want == 0)
        else:
            assert np.array_equal(got.cpu().numpy(), want), name
    # the loss on the reference's own targets (its IoUs, to the last bit)
    targets = [t("%s_targets_%s" % (tag, name)) for name in names]
    cls_score, bbox_pred = t(tag + "_cls_score").requires_grad_(True), \
        t(tag + "_bbox_pred").requires_grad_(True)
    losses = head.bbox_head.loss(cls_score, bbox_pred, batch.rois, *targets)
    for k in ("loss_cls", "loss_bbox"):
        within(losses[k], torch.from_numpy(gold["%s_%s" % (tag, k)]),
               torch.from_numpy(gold["%s_%s64" % (tag, k)]), k)
    within(losses["loss_corner"], torch.from_numpy(gold[tag + "_loss_corner_vector"]).mean(),
           torch.from_numpy(gold[tag + "_loss_corner_vector64"]).mean(), "loss_corner")
    sum(losses.values()).backward()
    within(cls_score.grad, t(tag + "_grad_cls_score"), t(tag + "_grad_cls_score64"), "grad cls")
    within(bbox_pred.grad, t(tag + "_grad_bbox_pred"), t(tag + "_grad_bbox_pred64"), "grad reg")
    class_labels = [t("%s_class_labels_%d" % (tag, b)) for b in range(2)]
    class_pred = [t("%s_class_pred_%d" % (tag, b)) for b in range(2)]
    for kind, cfg in (("rotate", dict(use_rotate_nms=True, nms_thr=0.1, score_thr=0.3)),
                      ("normal", dict(use_rotate_nms=False, nms_thr=0.1,
                                      score_thr=[0.3, 0.4, 0.5][:classes]))):
        got = head.bbox_head.get_bboxes(batch.rois, cls_score.detach(), bbox_pred.detach(),
                                        class_labels, class_pred,
                                        [dict(box_type_3d=LiDARBoxes)] * 2, cfg=cfg)
        for b, (boxes, scores, labels) in enumerate(got):
            want = gold["%s_%s_boxes_%d" % (tag, kind, b)]
            assert tuple(boxes.tensor.shape) == want.shape, (kind, b)
            assert np.array_equal(scores.cpu().numpy(), gold["%s_%s_scores_%d" % (tag, kind, b)])
            assert np.array_equal(labels.cpu().numpy(), gold["%s_%s_labels_%d" % (tag, kind, b)])
            assert np.abs(boxes.tensor.cpu().numpy() - want).max() <= 1e-5 * max(
                1.0, np.abs(want).max())


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_head_matches_the_references_forward_loss_and_gradients(dev, gold, mode):
    """The reference's own __init__ / forward / loss on the generator's dense stand-ins, in
    float32 and float64: this head on its weights is within 4 x the reference's own float32 error
    of its float64 run."""
    from msmdfusion_amd import registry
    head = registry.build_head(bbox_head_cfg(merge_conv_channels=[32], down_conv_channels=[16, 16],
                                             shared_fc_channels=[16, 48, 48]))
    keys = [str(k) for k in gold["head_state_keys"]]
    assert list(head.state_dict()) == keys
    head.load_state_dict({k: torch.from_numpy(gold["head_weight_" + k]) for k in keys})
    head = head.to(dev).train(mode == "train")
    t = lambda k: torch.from_numpy(gold[k])                                   # noqa: E731
    cls_score, bbox_pred = head(t("head_seg_feats").to(dev), t("head_part_feats").to(dev))
    q = "head_%s" % mode
    within(cls_score, t(q + "_cls_score"), t(q + "64_cls_score"), "cls_score")
    within(bbox_pred, t(q + "_bbox_pred"), t(q + "64_bbox_pred"), "bbox_pred")
    names = ("rois", "labels", "bbox_targets", "pos_gt_bboxes", "reg_mask", "label_weights",
             "bbox_weights")
    losses = head.loss(cls_score, bbox_pred, *[t("head_target_" + n).to(dev) for n in names])
    for k in ("loss_cls", "loss_bbox"):
        within(losses[k], t("%s_%s" % (q, k)), t("%s64_%s" % (q, k)), k)
    within(losses["loss_corner"], t(q + "_loss_corner_vector").mean(),
           t(q + "64_loss_corner_vector").mean(), "loss_corner")
    if mode == "train":
        sum(losses.values()).backward()
        worst = []
        for name, p in head.named_parameters():
            ref = gold["head_train64_grad_" + name].astype(np.float64)
            err_ref = float(gold["head_train_graderr_" + name])
            err = float(np.abs(p.grad.cpu().double().numpy() - ref).max())
            bound = 4.0 * max(err_ref, EPS * float(np.abs(ref).max()))
            print("grad %s: head %.3e, float32 reference %.3e, bound %.3e"
                  % (name, err, err_ref, bound))
            worst.append((name, err, err_ref, bound))
        failed = [w for w in worst if w[1] > w[3]]
        assert not failed, failed
