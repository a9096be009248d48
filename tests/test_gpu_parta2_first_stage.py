"""Part-A2's first stage on the GPU (COVERAGE n9): PointwiseSemanticHead fused against composed
and against the golden vectors, PartA2RPNHead.loss and get_bboxes against the golden vectors and
against a per-sample loop over the single-list NMS, host waits, and one training step of the
composed first stage.

Tolerances: 4 x the reference's own float32 error against its float64 run (both recorded in
tests/golden/parta2_first_stage_vectors.npz), floored at one float32 ulp at the values'
magnitude.  Discrete results (labels, the kept order, seg targets) are exact.
"""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parta2_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = float(np.finfo(np.float32).eps)
SEM_CASES = {"b2": 2, "b1": 1, "empty": 2, "nopos": 2}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "parta2_first_stage_vectors.npz")))


def close(got, ref32, ref64, what, unit=False):
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, np.float64)
    ref32, ref64 = np.asarray(ref32, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, what
    if not got.size:
        return
    scale = 1.0 if unit else max(1.0, float(np.abs(ref64).max()))
    limit = 4.0 * float(np.abs(ref32 - ref64).max()) + EPS * scale
    worst = float(np.abs(got - ref64).max())
    print("%s: error %.3e, bound %.3e" % (what, worst, limit))
    assert worst <= limit, "%s: %.3e > %.3e" % (what, worst, limit)


def semantic_head(gold, dev, fused=True):
    from msmdfusion_amd.semantic_head import PointwiseSemanticHead
    head = PointwiseSemanticHead(in_channels=16, num_classes=3, fused=fused)
    head.load_state_dict({k: torch.from_numpy(gold["sem_weight_" + k])
                          for k in gold["sem_state_keys"]})
    return head.to(dev)


def semantic_inputs(gold, tag, dev):
    from msmdfusion_amd.head_loss import LiDARBoxes
    p = "sem_%s_" % tag
    n = gold[p + "centres"].shape[0]
    coors = np.zeros((n, 4), np.int32)
    coors[:, 0] = gold[p + "ids"]
    voxels_dict = dict(coors=torch.from_numpy(coors).to(dev),
                       voxel_centers=torch.from_numpy(gold[p + "centres"]).to(dev))
    boxes = [LiDARBoxes(torch.from_numpy(gold[p + "boxes_%d" % b]).reshape(-1, 7).to(dev))
             for b in range(SEM_CASES[tag])]
    labels = [torch.from_numpy(gold[p + "labels_%d" % b]).to(dev) for b in range(SEM_CASES[tag])]
    return voxels_dict, boxes, labels


# ----------------------------------------------------------------------------- semantic head
@pytest.mark.parametrize("tag", sorted(SEM_CASES))
def test_semantic_head_fused_composed_and_golden(gold, dev, tag):
    p = "sem_%s_" % tag
    ref64 = np.concatenate([gold[p + "single64_part_%d" % b] for b in range(SEM_CASES[tag])])
    results = {}
    for fused in (True, False):
        head = semantic_head(gold, dev, fused)
        voxels_dict, boxes, labels = semantic_inputs(gold, tag, dev)
        kept = [b.tensor.clone() for b in boxes], [l.clone() for l in labels]
        res = head(torch.from_numpy(gold[p + "x"]).to(dev))
        for k in ("seg_preds", "part_preds", "part_feats"):
            close(res[k], gold[p + "fwd_" + k], gold[p + "fwd64_" + k], "%s %s" % (tag, k))
        targets = head.get_targets(voxels_dict, boxes, labels)
        for b, l, kb, kl in zip(boxes, labels, *kept):            # the lists are left untouched
            assert torch.equal(b.tensor, kb) and torch.equal(l, kl)
        assert np.array_equal(targets["seg_targets"].cpu().numpy(), gold[p + "seg_targets"])
        close(targets["part_targets"], gold[p + "part_targets"], ref64, tag + " part", unit=True)
        losses = head.loss(res, targets)
        (losses["loss_seg"] + losses["loss_part"]).backward()
        for k in ("loss_seg", "loss_part"):
            close(losses[k], gold[p + k], gold[p + k + "64"], "%s %s" % (tag, k))
        for k, prm in head.named_parameters():
            assert torch.isfinite(prm.grad).all()
            close(prm.grad, gold[p + "grad_" + k], gold[p + "grad64_" + k],
                  "%s grad %s" % (tag, k))
        results[fused] = (targets, losses)
    assert torch.equal(results[True][0]["seg_targets"], results[False][0]["seg_targets"])
    if tag == "nopos":
        assert float(results[True][1]["loss_part"].detach()) == 0.0


def test_semantic_targets_and_loss_do_not_wait_for_the_device(gold, dev):
    head = semantic_head(gold, dev)
    voxels_dict, boxes, labels = semantic_inputs(gold, "b2", dev)
    x = torch.from_numpy(gold["sem_b2_x"]).to(dev)

    def work():
        res = head(x)
        losses = head.loss(res, head.get_targets(voxels_dict, boxes, labels))
        (losses["loss_seg"] + losses["loss_part"]).backward()
        return losses

    work()                                               # warm: module load, allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = work()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(losses["loss_seg"]) and torch.isfinite(losses["loss_part"])


# ------------------------------------------------------------------------------------- RPN
def rpn_head(gold, dev, **kw):
    from msmdfusion_amd.parta2_rpn_head import PartA2RPNHead
    head = PartA2RPNHead(**dict(PC.rpn_head_cfg(), **kw))
    if not kw:
        head.load_state_dict({k: torch.from_numpy(gold["rpn_weight_" + k])
                              for k in gold["rpn_state_keys"]})
    return head.to(dev)


def test_rpn_loss_matches_the_reference(gold, dev):
    from msmdfusion_amd.head_loss import LiDARBoxes
    head = rpn_head(gold, dev)
    outs = head([torch.from_numpy(gold["rpn_feats"]).to(dev)])
    for got, name in zip(outs, ("cls", "bbox", "dir")):
        assert np.abs(got[0].detach().cpu().numpy() - gold["rpn_pred_" + name]).max() < 1e-4
    gts = [LiDARBoxes(torch.from_numpy(gold["rpn_gt_boxes_%d" % b]).to(dev)) for b in range(2)]
    labels = [torch.from_numpy(gold["rpn_gt_labels_%d" % b]).to(dev) for b in range(2)]
    losses = head.loss(*outs, gts, labels, [None, None])
    assert sorted(losses) == ["loss_rpn_bbox", "loss_rpn_cls", "loss_rpn_dir"]
    sum(sum(v) for v in losses.values()).backward()
    for k, per_level in losses.items():
        close(torch.stack(list(per_level)), gold["rpn_" + k].astype(np.float32),
              gold["rpn_" + k + "64"], k)
    for k, prm in head.named_parameters():
        close(prm.grad, gold["rpn_grad_" + k], gold["rpn_grad64_" + k], "grad " + k)


@pytest.mark.parametrize("tag", sorted(PC.RPN_CFGS))
def test_rpn_get_bboxes_matches_the_reference(gold, dev, tag):
    from msmdfusion_amd.head_loss import LiDARBoxes
    head = rpn_head(gold, dev).eval()
    cfg = PC.RPN_CFGS[tag]
    preds = [[torch.from_numpy(gold["rpn_pred_" + k]).to(dev).clone()]
             for k in ("cls", "bbox", "dir")]
    if tag == "none":
        preds[0][0][1] -= 30.0
    metas = [dict(box_type_3d=LiDARBoxes)] * 2
    with torch.no_grad():
        results = head.get_bboxes(*preds, metas, cfg)
        single = head.get_bboxes_single([preds[0][0][1]], [preds[1][0][1]],
                                        [preds[2][0][1]], None, metas[1], cfg)
    assert len(results) == 2
    for i, r in enumerate(results):
        p, p64 = "rpn_%s_s%d_" % (tag, i), "rpn_%s_s%d64_" % (tag, i)
        assert isinstance(r["boxes_3d"], LiDARBoxes)
        assert sorted(r) == ["boxes_3d", "cls_preds", "labels_3d", "scores_3d"]
        want = torch.from_numpy(gold[p + "labels_3d"])
        assert r["labels_3d"].dtype == want.dtype                  # float for the empty result
        assert torch.equal(r["labels_3d"].cpu(), want)             # kept rows and their order
        close(r["boxes_3d"].tensor, gold[p + "boxes_3d"], gold[p64 + "boxes_3d"],
              "%s %d boxes" % (tag, i))
        for k in ("scores_3d", "cls_preds"):
            close(r[k], gold[p + k], gold[p64 + k], "%s %d %s" % (tag, i, k))
    for k in ("scores_3d", "labels_3d", "cls_preds"):
        assert torch.equal(single[k], results[1][k])
    assert torch.equal(single["boxes_3d"].tensor, results[1]["boxes_3d"].tensor)
    if tag == "none":
        r = results[1]
        assert tuple(r["boxes_3d"].tensor.shape) == (0, 7) and tuple(r["scores_3d"].shape) == (0,)
        assert tuple(r["labels_3d"].shape) == (0,) and r["labels_3d"].dtype == torch.float32
        assert tuple(r["cls_preds"].shape) == (0, 3)
    if tag == "quirk":
        assert float(results[0]["cls_preds"].min()) < 0            # the raw logits


def _rpn_outs(dev, batch, size, seed):
    g = torch.Generator().manual_seed(seed)
    return [[(torch.randn((batch, 6 * c, *size), generator=g) * s).to(dev)]
            for c, s in ((3, 1.5), (7, 0.3), (2, 1.0))]


@pytest.mark.parametrize("tag", ["train", "test", "quirk"])
def test_rpn_get_bboxes_equals_the_per_sample_loop(dev, tag):
    """B = 3 on an 8 x 10 map (480 anchors) against parta2_rpn_head.py:126-311 restated per
    sample on the single-list nms_gpu / nms_normal_gpu."""
    from msmdfusion_amd import iou3d
    head = rpn_head(None, dev, test_cfg=PC.RPN_CFGS["test"]).eval()
    cfg = dict(PC.RPN_CFGS[tag])
    outs = _rpn_outs(dev, 3, (8, 10), 17)
    outs[0][0][2, :, 4:, :] -= 30.0                    # a sample with few candidates above thr

    def nms(kind, boxes, scores, thresh):
        if boxes.shape[0] == 0:
            return torch.zeros((0,), dtype=torch.long, device=boxes.device)
        fn = iou3d.nms_gpu if kind == "rotate" else iou3d.nms_normal_gpu
        return fn(boxes.contiguous(), scores.contiguous(), thresh)

    with torch.no_grad():
        got = head.get_bboxes(*outs, [None] * 3, cfg)
        want = PC.rpn_loop(head, *outs, cfg, nms=nms)
    kept = []
    for g, w in zip(got, want):
        for k in ("boxes_3d", "scores_3d", "labels_3d", "cls_preds"):
            assert g[k].dtype == w[k].dtype and torch.equal(g[k], w[k]), k
        kept.append(int(g["scores_3d"].numel()))
    print(tag, "kept", kept)
    assert all(0 < k <= cfg["nms_post"] for k in kept)
    if tag == "train":
        assert kept[0] == cfg["nms_post"]              # more survivors than nms_post: the cut
    one = head.class_agnostic_nms(
        want[0]["boxes_3d"], torch.cat([want[0]["boxes_3d"][:, [0, 1]] - 0.5,
                                        want[0]["boxes_3d"][:, [0, 1]] + 0.5,
                                        want[0]["boxes_3d"][:, 6:7]], 1),
        want[0]["scores_3d"], want[0]["labels_3d"], want[0]["cls_preds"],
        torch.zeros_like(want[0]["labels_3d"]), 0.0, 5, cfg, None)
    assert one["scores_3d"].numel() <= 5
    assert bool((one["scores_3d"][:-1] >= one["scores_3d"][1:]).all())


def test_rpn_get_bboxes_reads_the_host_once(dev):
    head = rpn_head(None, dev, test_cfg=PC.RPN_CFGS["test"]).eval()
    outs = _rpn_outs(dev, 3, (8, 10), 19)
    cfg = PC.RPN_CFGS["train"]
    with torch.no_grad():
        head.get_bboxes(*outs, [None] * 3, cfg)            # warm: the anchor cache, workspaces
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                head.get_bboxes(*outs, [None] * 3, cfg)
            finally:
                torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchroniz" in str(w.message).lower()
             and "prototype" not in str(w.message)]
    assert len(syncs) == 1, [str(w.message) for w in syncs]


# -------------------------------------------------------------------------- the first stage
def test_one_training_step_of_the_composed_first_stage(dev):
    """points -> Voxelization -> HardSimpleVFE -> SparseUNet -> SECOND -> SECONDFPN ->
    PartA2RPNHead.loss + proposals, PointwiseSemanticHead on seg_features with targets and loss,
    at the small sparse shape of tests/test_gpu_sparse_unet.py ([25, 32, 32])."""
    from msmdfusion_amd.bev import SECOND, SECONDFPN
    from msmdfusion_amd.head_loss import LiDARBoxes
    from msmdfusion_amd.parta2_rpn_head import PartA2RPNHead
    from msmdfusion_amd.semantic_head import PointwiseSemanticHead, voxel_centers
    from msmdfusion_amd.sparse_unet import SparseUNet
    from msmdfusion_amd.voxel_encoder import HardSimpleVFE
    from msmdfusion_amd.voxelize import Voxelization
    torch.manual_seed(0)
    rs = np.random.RandomState(2)
    voxel_size, pc_range = [0.5, 0.5, 0.25], [0, -8, -3, 16, 8, 3]
    gt = [np.asarray([[4.0, -3.0, -1.8, 1.6, 3.9, 1.56, 0.3], [10.0, 2.0, -1.7, 1.7, 4.1, 1.5, 1.2],
                      [12.0, -5.0, -0.6, 0.6, 0.8, 1.73, -0.4]], np.float32),
          np.asarray([[7.0, 4.0, -1.75, 1.6, 3.8, 1.6, -1.0]], np.float32)]
    gt_labels = [np.asarray([2, 2, 0]), np.asarray([2])]
    points = []
    for b in range(2):
        p = rs.uniform(0, 1, (2500, 4)).astype(np.float32)
        p[:, 0], p[:, 1], p[:, 2] = p[:, 0] * 15.9, p[:, 1] * 15.9 - 7.95, p[:, 2] * 5.9 - 2.95
        inside = gt[b][rs.randint(0, len(gt[b]), 500)]
        q = np.concatenate([inside[:, :3] + rs.uniform(-0.3, 0.3, (500, 3)) * [1, 1, 0]
                            + [0, 0, 0.5], rs.uniform(0, 1, (500, 1))], 1).astype(np.float32)
        points.append(torch.from_numpy(np.concatenate([p, q])).to(dev))
    boxes = [LiDARBoxes(torch.from_numpy(b).to(dev)) for b in gt]
    labels = [torch.from_numpy(l).long().to(dev) for l in gt_labels]

    voxel_layer = Voxelization(voxel_size, pc_range, 5, (16000, 40000))
    vfe = HardSimpleVFE(4)
    unet = SparseUNet(4, [25, 32, 32]).to(dev)

    def encode():
        voxels, nums, coors = [], [], []
        for b, (v, c, n) in enumerate(voxel_layer.forward_batch(points, fused_mean=False)):
            voxels.append(v), nums.append(n)
            coors.append(torch.nn.functional.pad(c, (1, 0), mode="constant", value=b))
        coors = torch.cat(coors)
        feats = vfe(torch.cat(voxels), torch.cat(nums), coors)
        return unet(feats, coors, 2), coors

    with torch.no_grad():
        channels = encode()[0]["spatial_features"].shape[1]
    backbone = SECOND(in_channels=channels, out_channels=[32, 64], layer_nums=[1, 1],
                      layer_strides=[1, 2]).to(dev)
    neck = SECONDFPN(in_channels=[32, 64], out_channels=[32, 32], upsample_strides=[1, 2]).to(dev)
    rpn = PartA2RPNHead(**dict(PC.rpn_head_cfg(), in_channels=64, feat_channels=64)).to(dev)
    sem = PointwiseSemanticHead(in_channels=16, num_classes=3).to(dev)
    parts = dict(unet=unet, backbone=backbone, neck=neck, rpn=rpn, sem=sem)
    params = [p for m in parts.values() for p in m.parameters()]
    opt = torch.optim.SGD(params, lr=1e-3)
    proposal_cfg = dict(nms_pre=100, nms_post=20, max_num=20, nms_thr=0.8, score_thr=0,
                        use_rotate_nms=False)

    def step(train):
        feats, coors = encode()
        outs = rpn(neck(backbone(feats["spatial_features"])))
        assert feats["seg_features"].shape == (coors.shape[0], 16)
        voxels_dict = dict(coors=coors, voxel_centers=voxel_centers(coors, voxel_size, pc_range))
        sem_res = sem(feats["seg_features"])
        assert sem_res["part_feats"].shape == (coors.shape[0], 4)
        with torch.no_grad():
            proposals = rpn.get_bboxes(*outs, [dict(box_type_3d=LiDARBoxes)] * 2, proposal_cfg)
        if not train:
            return proposals, None
        losses = rpn.loss(*outs, boxes, labels, [None, None])
        targets = sem.get_targets(voxels_dict, boxes, labels)
        pos = (targets["seg_targets"] >= 0) & (targets["seg_targets"] < 3)
        assert int(pos.sum()) > 20                     # voxels inside the boxes exist
        losses.update(sem.loss(sem_res, targets))
        return proposals, losses

    proposals, losses = step(True)
    assert sorted(losses) == ["loss_part", "loss_rpn_bbox", "loss_rpn_cls", "loss_rpn_dir",
                              "loss_seg"]
    total = 0
    for k, v in losses.items():
        v = sum(v) if isinstance(v, list) else v
        assert torch.isfinite(v), k
        total = total + v
    opt.zero_grad()
    total.backward()
    for name, m in parts.items():
        grads = [p.grad for p in m.parameters() if p.grad is not None]
        assert grads and all(torch.isfinite(g).all() for g in grads), name
        assert sum(float(g.abs().sum()) for g in grads) > 0, name
    before = [p.detach().clone() for p in params]
    opt.step()
    assert any(not torch.equal(a, b) for a, b in zip(before, params))
    for p in proposals:
        assert 0 < p["scores_3d"].numel() <= 20 and tuple(p["cls_preds"].shape[1:]) == (3,)
    for m in parts.values():
        m.eval()
    voxel_layer.eval()
    with torch.no_grad():
        proposals, _ = step(False)
    for p in proposals:
        assert isinstance(p["boxes_3d"], LiDARBoxes) and p["boxes_3d"].tensor.shape[1] == 7
        assert torch.isfinite(p["boxes_3d"].tensor).all() and p["scores_3d"].numel() > 0
