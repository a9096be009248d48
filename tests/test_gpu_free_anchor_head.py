"""FreeAnchor3DHead on the device (msmdfusion_amd/free_anchor_head.py): the loss and its
gradients against the reference's own float32 and float64 outputs
(tests/golden/free_anchor_vectors.npz) and against float64 autograd of the functional
restatement (tests/free_anchor_ref.py) where bags overlap; no host wait; a VoxelNet with the
head swapped in; get_bboxes unchanged from Anchor3DHead."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import free_anchor_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "free_anchor_vectors.npz")
KEYS = ("positive_bag_loss", "negative_bag_loss")


@pytest.fixture(autouse=True)
def _leave_the_global_rng_alone(dev):
    with torch.random.fork_rng(devices=[dev]):
        yield


@pytest.fixture(scope="module")
def gold():
    """The reference's own FreeAnchor3DHead.loss outputs (tests/golden/
    make_free_anchor_golden.py); read-only."""
    return np.load(GOLD)


def _head(dev, kind, **kw):
    from msmdfusion_amd.registry import build_head
    cfg, sizes = R.head_cfg(kind, **kw)
    torch.manual_seed(0)
    head = build_head(cfg).to(dev)
    head.init_weights()
    return head, sizes


def _flat_anchors(head, sizes, dev):
    return torch.cat([a.reshape(-1, head.box_code_size)
                      for a in head.anchor_generator.grid_anchors(sizes, dev)])


def _run(head, preds, boxes, labels, record=None):
    """loss + backward on fresh leaves -> (losses, leaves); record: a dict that receives the
    bags and the box probability the head computed."""
    from msmdfusion_amd import free_anchor_head as FH
    leaves = [[v.clone().requires_grad_() for v in lv] for lv in preds]
    topk, prob = FH.K.free_anchor_topk, FH.K.free_anchor_box_prob
    if record is not None:
        def rec_topk(*a):
            record["matched"] = topk(*a)
            return record["matched"]

        def rec_prob(*a):
            record["box_prob"] = prob(*a)
            return record["box_prob"]
        FH.K.free_anchor_topk, FH.K.free_anchor_box_prob = rec_topk, rec_prob
    try:
        losses = head.loss(*leaves, boxes, labels, None)
    finally:
        FH.K.free_anchor_topk, FH.K.free_anchor_box_prob = topk, prob
    assert sorted(losses) == sorted(KEYS)
    (losses["positive_bag_loss"] + losses["negative_bag_loss"]).backward()
    return losses, leaves


# ---------------------------------------------------------------- against the reference's outputs
@pytest.mark.parametrize("tag", ["k05", "k15", "n05", "n15"])
def test_loss_equals_the_reference(gold, dev, tag):
    """Bags exactly; box_prob, both losses and all gradients with
    |ours - ref64| <= 4 max(|ref32 - ref64|, eps scale): the margin is the reference's own float32
    error, recorded in the fixture."""
    head, sizes = _head(dev, tag[0])
    assert head.pre_anchor_topk == int(gold["topk"]) and head.bbox_thr == float(gold["bbox_thr"])
    preds, boxes, labels = R.gold_inputs(gold, tag, len(sizes), dev)
    seen = {}
    losses, leaves = _run(head, preds, boxes, labels, seen)
    counts = [b.shape[0] for b in boxes]
    matched = seen["matched"].cpu().numpy()
    np.testing.assert_array_equal(matched[:counts[0]], gold[tag + "_matched_0"])
    np.testing.assert_array_equal(matched[counts[0]:], gold[tag + "_matched_1"])
    box_prob = seen["box_prob"].reshape(gold[tag + "_box_prob32"].shape).cpu().numpy()
    ok, err, margin = R.within_reference_error(box_prob, gold[tag + "_box_prob32"],
                                               gold[tag + "_box_prob64"])
    print(tag, "box_prob", err, margin)
    assert ok, ("box_prob", err, margin)
    assert ((box_prob > 0) == (gold[tag + "_box_prob32"] > 0)).all()
    for key in KEYS:
        ok, err, margin = R.within_reference_error(
            float(losses[key].detach()), gold["%s_%s32" % (tag, key)], gold["%s_%s64" % (tag, key)])
        print(tag, key, err, margin)
        assert ok, (key, err, margin)
    for name, per_level in zip(("cls", "bbox", "dir"), leaves):
        for lvl, v in enumerate(per_level):
            ok, err, margin = R.within_reference_error(
                v.grad.cpu().numpy(), gold["%s_grad32_%s_l%d" % (tag, name, lvl)],
                gold["%s_grad64_%s_l%d" % (tag, name, lvl)])
            print(tag, name, lvl, err, margin)
            assert ok, (name, lvl, err, margin)


# ---------------------------------------------------------------- against float64 autograd
def ground_truth(anchors, n, seed, twins=False):
    """n boxes near randomly chosen anchors; twins: the second is the first moved by 5 cm, so
    the two bags share their anchors."""
    rs = np.random.RandomState(seed)
    flat = anchors.cpu().numpy()
    pick = flat[rs.randint(0, flat.shape[0], n)].copy()
    box = pick.copy()
    box[:, :2] += rs.uniform(-0.4, 0.4, (n, 2))
    box[:, 3:6] *= rs.uniform(0.85, 1.2, (n, 3))
    box[:, 6] = rs.uniform(-3.0, 3.0, n)
    if box.shape[1] > 7:
        box[:, 7:] = rs.normal(size=(n, box.shape[1] - 7))
    if twins and n > 1:
        box[1] = box[0]
        box[1, 0] += 0.05
    return torch.from_numpy(box.astype(np.float32)), torch.from_numpy(rs.randint(0, 3, n))


def predictions(head, sizes, batch, seed, dev):
    g = torch.Generator().manual_seed(seed)
    a, c = head.num_anchors, head.box_code_size
    return [[(torch.randn((batch, a * w, *s), generator=g) * scale).to(dev) for s in sizes]
            for w, scale in ((head.num_classes, 1.0), (c, 0.1), (2, 1.0))]


def _against_float64(dev, kind, counts, topk, seed, twins=False):
    head, sizes = _head(dev, kind, topk=topk, bbox_thr=0.3)     # random predictions reach 0.3
    anchors = _flat_anchors(head, sizes, dev)
    preds = predictions(head, sizes, len(counts), seed, dev)
    gt = [ground_truth(anchors, n, seed + 7 * b, twins) for b, n in enumerate(counts)]
    boxes, labels = [g[0].to(dev) for g in gt], [g[1].to(dev) for g in gt]
    seen = {}
    losses, leaves = _run(head, preds, boxes, labels, seen)
    starts = np.cumsum([0] + list(counts))
    matched = [seen["matched"][starts[b]:starts[b + 1]].long() for b in range(len(counts))]
    runs = {}
    for dtype in (torch.float32, torch.float64):
        lv = [[v.detach().to(dtype).requires_grad_() for v in per] for per in preds]
        rl, prob, bags = R.loss_restatement(head, anchors, *lv, boxes, labels,
                                            matched=matched if dtype == torch.float64 else None)
        (rl["positive_bag_loss"] + rl["negative_bag_loss"]).backward()
        runs[dtype] = (rl, lv, prob, bags)
    for b in range(len(counts)):                  # the kernel's bags are the sorted matrix's
        assert torch.equal(matched[b], runs[torch.float32][3][b])
    (l32, g32, p32, _), (l64, g64, p64, _) = runs[torch.float32], runs[torch.float64]
    ok, err, margin = R.within_reference_error(seen["box_prob"].reshape(p32.shape).cpu().numpy(),
                                               p32.cpu().numpy(), p64.cpu().numpy())
    print(kind, counts, "box_prob", err, margin, int((p32 > 0).sum()))
    assert ok, ("box_prob", err, margin)
    for key in KEYS:
        ok, err, margin = R.within_reference_error(float(losses[key].detach()),
                                                   float(l32[key].detach()), float(l64[key].detach()))
        print(kind, counts, key, err, margin)
        assert ok, (key, err, margin)
    zero = lambda v: torch.zeros_like(v) if v.grad is None else v.grad
    for name, ours, r32, r64 in zip(("cls", "bbox", "dir"), leaves, g32, g64):
        for lvl, (v, a, b) in enumerate(zip(ours, r32, r64)):
            assert v.grad is not None, name          # zeros, not None, without ground truth
            ok, err, margin = R.within_reference_error(v.grad.cpu().numpy(), zero(a).cpu().numpy(),
                                                       zero(b).cpu().numpy())
            print(kind, counts, name, lvl, err, margin)
            assert ok, (name, lvl, err, margin)
    return head, matched, losses, leaves


@pytest.mark.parametrize("kind,counts", [("n", (0, 1, 7)), ("k", (0, 0))])
def test_loss_and_gradients_against_float64_autograd(dev, kind, counts):
    """k = 50, bags that overlap, an empty sample and an empty batch: loss and gradients within
    4 x the float32 restatement's own error of float64 autograd through the functional
    restatement (on the kernel's bags)."""
    head, matched, losses, leaves = _against_float64(dev, kind, counts, 50, 11)
    if sum(counts):
        rows = matched[2].reshape(-1).tolist()
        assert len(set(rows)) < len(rows)                         # an anchor sits in two bags
        assert float(losses["positive_bag_loss"]) > 0
    else:
        assert float(losses["positive_bag_loss"]) == 0.0
        for per_level in leaves[1:]:
            assert all(float(v.grad.abs().max()) == 0.0 for v in per_level)
        assert float(leaves[0][0].grad.abs().max()) > 0
    assert float(losses["negative_bag_loss"]) > 0


def test_an_anchor_in_two_bags_uses_its_own_encoding_in_each(dev):
    """The deviation: two ground truths 5 cm apart share their whole bags; every (ground truth,
    anchor) pair carries its own sin-difference encoding, as the functional restatement has it
    (the reference's in-place write would leave one of the two for both)."""
    head, matched, _, _ = _against_float64(dev, "k", (3,), 6, 23, twins=True)
    assert torch.equal(matched[0][0], matched[0][1])


# ---------------------------------------------------------------- no host wait
def test_loss_does_not_wait_for_the_device(dev):
    """The whole loss and its backward under torch's sync debug mode (after one warm call: the
    anchors come from the host once)."""
    head, sizes = _head(dev, "n", topk=25)
    anchors = _flat_anchors(head, sizes, dev)
    preds = predictions(head, sizes, 3, 5, dev)
    gt = [ground_truth(anchors, n, 40 + b) for b, n in enumerate((4, 0, 6))]
    boxes, labels = [g[0].to(dev) for g in gt], [g[1].to(dev) for g in gt]
    first, _ = _run(head, preds, boxes, labels)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second, leaves = _run(head, preds, boxes, labels)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for key in KEYS:
        assert torch.equal(first[key].detach(), second[key].detach())
    assert all(v.grad is not None for per_level in leaves for v in per_level)


# ---------------------------------------------------------------- detector, inference
def test_voxelnet_with_the_head_swapped_trains_and_infers(dev):
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.registry import build_detector
    model = copy.deepcopy(C.POINTPILLARS_SECFPN_KITTI["model"])
    rng_ = [0, -6.4, -3, 12.8, 6.4, 1]
    model["voxel_layer"].update(point_cloud_range=rng_, max_voxels=(6400, 6400))
    model["voxel_encoder"].update(point_cloud_range=rng_)
    model["middle_encoder"].update(output_shape=[80, 80])
    for r in model["bbox_head"]["anchor_generator"]["ranges"]:
        r[0:2], r[3:5] = [0, -6.4], [12.8, 6.4]
    model["bbox_head"].update(type="FreeAnchor3DHead", pre_anchor_topk=25, bbox_thr=0.5)
    torch.manual_seed(3)
    det = build_detector(model).to(dev)
    assert type(det).__name__ == "VoxelNet" and type(det.bbox_head).__name__ == "FreeAnchor3DHead"
    rs = np.random.RandomState(4)
    points = []
    for _ in range(2):
        p = rs.uniform(0, 1, (3000, 4)).astype(np.float32)
        p[:, 0] = rng_[0] + p[:, 0] * (rng_[3] - rng_[0]) * 0.999
        p[:, 1] = rng_[1] + p[:, 1] * (rng_[4] - rng_[1]) * 0.999
        p[:, 2] = rs.uniform(-2.5, 0.5, 3000)
        points.append(torch.from_numpy(p).to(dev))
    gt = [torch.tensor([[4.0, 1.0, -1.6, 1.6, 3.9, 1.56, 0.3],
                        [3.0, -2.0, -0.6, 0.6, 0.8, 1.73, 1.0]], device=dev),
          torch.zeros((0, 7), device=dev)]
    labels = [torch.tensor([2, 0], device=dev), torch.zeros((0,), dtype=torch.long, device=dev)]
    det.train()
    losses = det(points, return_loss=True, gt_bboxes_3d=gt, gt_labels_3d=labels)
    assert sorted(losses) == sorted(KEYS)
    total = sum(losses.values())
    assert torch.isfinite(total) and float(losses["positive_bag_loss"]) > 0
    total.backward()
    grads = [p.grad for p in det.parameters() if p.requires_grad]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    assert float(det.bbox_head.conv_reg.weight.grad.abs().sum()) > 0
    assert float(det.bbox_head.conv_dir_cls.weight.grad.abs().sum()) > 0
    assert float(det.voxel_encoder.pfn_layers[0].linear.weight.grad.abs().sum()) > 0
    det.eval()
    with torch.no_grad():
        out = det.simple_test(points)
    assert len(out) == 2
    for r in out:
        n = r["scores_3d"].shape[0]
        assert r["boxes_3d"].shape == (n, 7) and r["labels_3d"].shape == (n,) and n <= 50


def test_get_bboxes_equals_anchor3d_head(dev):
    from msmdfusion_amd.registry import build_head
    head, sizes = _head(dev, "n")
    cfg, _ = R.head_cfg("n")
    plain = build_head(dict({k: v for k, v in cfg.items() if k not in (
        "pre_anchor_topk", "bbox_thr", "gamma", "alpha")}, type="Anchor3DHead")).to(dev)
    plain.load_state_dict(head.state_dict())
    feats = [torch.randn((2, 16, *s), generator=torch.Generator().manual_seed(9)).to(dev)
             for s in sizes]
    with torch.no_grad():
        ours = head.get_bboxes(*head(feats), [None, None], cfg=dict(cfg["test_cfg"], score_thr=0.0))
        want = plain.get_bboxes(*plain(feats), [None, None],
                                cfg=dict(cfg["test_cfg"], score_thr=0.0))
    assert sum(r[1].numel() for r in want) > 0
    for a, b in zip(ours, want):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
