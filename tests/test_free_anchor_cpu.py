"""FreeAnchor3DHead without a GPU: the torch restatements of tests/free_anchor_ref.py against
the reference's own outputs (tests/golden/free_anchor_vectors.npz), the constructor, state-dict
keys, registry and config fixture, the C ABI's host-side refusals, and reduction_override=None
leaving the two loss classes as they were."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import free_anchor_ref as R  # noqa: E402

GOLD = os.path.join(HERE, "golden", "free_anchor_vectors.npz")
TAGS = ["k05", "k15", "n05", "n15"]


@pytest.fixture(scope="module")
def gold():
    """The reference's own outputs (tests/golden/make_free_anchor_golden.py); read-only."""
    return np.load(GOLD)


def _head(kind, **kw):
    from msmdfusion_amd.registry import build_head
    cfg, sizes = R.head_cfg(kind, **kw)
    torch.manual_seed(0)
    return build_head(cfg), sizes


@pytest.fixture(scope="module")
def restated(gold):
    """The whole-loss restatement on every golden case, once: float32 and float64 (on the
    float32 bags), with gradients."""
    out = {}
    for tag in TAGS:
        head, sizes = _head(tag[0])
        anchors = torch.cat([a.reshape(-1, head.box_code_size) for a in
                             head.anchor_generator.grid_anchors(sizes, "cpu")])
        runs = {}
        for dtype in (torch.float32, torch.float64):
            preds, boxes, labels = R.gold_inputs(gold, tag, len(sizes), "cpu", dtype)
            leaves = [[v.clone().requires_grad_() for v in lv] for lv in preds]
            matched = runs[torch.float32][2] if dtype == torch.float64 else None
            losses, box_prob, bags = R.loss_restatement(head, anchors, *leaves, boxes, labels,
                                                        matched=matched)
            (losses["positive_bag_loss"] + losses["negative_bag_loss"]).backward()
            runs[dtype] = (losses, box_prob, bags, leaves)
        out[tag] = runs
    return out


@pytest.mark.parametrize("tag", TAGS)
def test_restatements_equal_the_reference(gold, restated, tag):
    """Bags exactly; box_prob, both losses and every gradient: the float32 restatement within
    4 x the reference's own float32 error of the reference's float64, the float64 one close to
    it: the reference's box type keeps the ground truths, and with them the IoUs and the
    z-centre of encode, in float32 even in its float64 run, hence 1e-6 on the positive side and
    1e-5 on what goes through box_prob."""
    r32, r64 = restated[tag][torch.float32], restated[tag][torch.float64]
    for b in range(2):
        np.testing.assert_array_equal(r32[2][b].numpy(), gold["%s_matched_%d" % (tag, b)])
    ok, err, margin = R.within_reference_error(r32[1].numpy(), gold[tag + "_box_prob32"],
                                               gold[tag + "_box_prob64"])
    print(tag, "box_prob", err, margin)
    assert ok, (err, margin)
    assert (gold[tag + "_box_prob32"] > 0).sum() > 0
    for key in ("positive_bag_loss", "negative_bag_loss"):
        ref32, ref64 = gold["%s_%s32" % (tag, key)], gold["%s_%s64" % (tag, key)]
        ok, err, margin = R.within_reference_error(float(r32[0][key].detach()), ref32, ref64)
        print(tag, key, err, margin)
        assert ok, (key, err, margin)
        assert float(r64[0][key].detach()) == pytest.approx(
            float(ref64), rel=1e-6 if key == "positive_bag_loss" else 1e-5)
    for name, l32, l64 in zip(("cls", "bbox", "dir"), r32[3], r64[3]):
        for lvl, (v32, v64) in enumerate(zip(l32, l64)):
            ref32 = gold["%s_grad32_%s_l%d" % (tag, name, lvl)]
            ref64 = gold["%s_grad64_%s_l%d" % (tag, name, lvl)]
            ok, err, margin = R.within_reference_error(v32.grad.numpy(), ref32, ref64)
            print(tag, name, lvl, err, margin)
            assert ok, (name, lvl, err, margin)
            # (box_prob, which enters the class gradient linearly, carries the float32 IoUs'
            # error, about 1e-6 absolute, in the reference's float64 run)
            np.testing.assert_allclose(v64.grad.numpy(), ref64, rtol=1e-5,
                                       atol=1e-5 * float(np.abs(ref64).max()))


def test_topk_restatement_order():
    """Ties keep anchor order, NaN sorts first, rows come back ascending."""
    anchors = torch.tensor([[0.0, 0, 1, 1], [5.0, 5, 6, 6], [0.0, 0, 1, 1], [0.0, 0, 2, 2],
                            [0.0, 0, 1, 1]])
    gt = torch.tensor([[0.0, 0, 1, 1], [float("nan")] * 4, [9.0, 9, 10, 10]])
    got = R.topk_restatement(anchors, gt, 2)
    assert got.tolist() == [[0, 2], [0, 1], [0, 1]]
    assert R.topk_restatement(anchors, gt, 4)[0].tolist() == [0, 2, 3, 4]


def test_constructor_state_dict_registry():
    import inspect
    from msmdfusion_amd.anchor_head import Anchor3DHead
    from msmdfusion_amd.free_anchor_head import FreeAnchor3DHead
    from msmdfusion_amd.registry import HEADS, build_head
    sig = inspect.signature(FreeAnchor3DHead.__init__).parameters
    assert [(k, sig[k].default) for k in ("pre_anchor_topk", "bbox_thr", "gamma", "alpha")] == \
        [("pre_anchor_topk", 50), ("bbox_thr", 0.6), ("gamma", 2.0), ("alpha", 0.5)]
    cfg, _ = R.head_cfg("n")
    head = build_head(cfg)
    assert "FreeAnchor3DHead" in HEADS and type(head) is FreeAnchor3DHead
    assert isinstance(head, Anchor3DHead)
    plain = build_head(dict({k: v for k, v in cfg.items() if k not in (
        "pre_anchor_topk", "bbox_thr", "gamma", "alpha")}, type="Anchor3DHead"))
    assert sorted(head.state_dict()) == sorted(plain.state_dict())
    assert [tuple(v.shape) for v in head.state_dict().values()] == \
        [tuple(v.shape) for v in plain.state_dict().values()]
    assert (head.pre_anchor_topk, head.bbox_thr, head.gamma, head.alpha) == (6, 0.6, 2.0, 0.5)
    assert FreeAnchor3DHead.forward is Anchor3DHead.forward
    assert FreeAnchor3DHead.get_bboxes is Anchor3DHead.get_bboxes


def test_config_equals_the_reference_dicts():
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.registry import build_head
    fx = json.load(open(os.path.join(HERE, "golden", "reference_free_anchor_config.json")))
    norm = lambda o: json.loads(json.dumps(o))   # tuples -> lists
    assert norm(C.FREE_ANCHOR_HEAD_NUS) == fx["pts_bbox_head"]
    assert norm(C.FREE_ANCHOR_TRAIN_CFG_NUS) == fx["train_cfg"]
    head = build_head(dict(C.FREE_ANCHOR_HEAD_NUS, train_cfg=C.FREE_ANCHOR_TRAIN_CFG_NUS["pts"],
                           test_cfg=None))
    assert head.num_anchors == 8 and head.box_code_size == 9 and head.pre_anchor_topk == 25
    assert tuple(head.conv_cls.weight.shape) == (80, 256, 1, 1)


def test_c_abi_argument_validation():
    """k = 0, k above the cap, k above the anchors, gamma < 1, a code size below 7, null
    pointers, a missing or short workspace: refused before anything is enqueued."""
    from msmdfusion_amd._lib import lib
    p = ctypes.c_void_p(256)
    cap = lib.msmd_free_anchor_max_topk()
    assert cap >= 64
    ws = lib.msmd_free_anchor_topk_workspace_bytes(1000, 7)
    assert ws >= 7 * 4 * 256 * 4 and lib.msmd_free_anchor_topk_workspace_bytes(-1, 7) == 0

    def topk(anchors=p, a=1000, gt=p, g=7, k=25, out=p, work=p, nbytes=ws):
        return lib.msmd_free_anchor_topk(anchors, a, gt, g, k, out, work, nbytes, None)
    assert topk(k=0) == -1 and topk(k=-3) == -1 and topk(k=cap + 1) == -1
    assert topk(a=20, k=25) == -1                            # the reference's topk raises too
    assert topk(anchors=None) == -1 and topk(gt=None) == -1 and topk(out=None) == -1
    assert topk(a=-1) == -1 and topk(g=-1) == -1
    assert topk(work=None) == -2 and topk(nbytes=ws - 256) == -2
    assert topk(g=0) == 0                                    # nothing to do, nothing launched

    decode = lambda code=7, anchors=p, deltas=p, out=p, a=8, b=2: \
        lib.msmd_decode_nearest_bev_f32(anchors, a, code, deltas, b, out, None)
    assert decode(code=6) == -1 and decode(anchors=None) == -1 and decode(deltas=None) == -1
    assert decode(out=None) == -1 and decode(a=-1) == -1 and decode(b=-1) == -1
    assert decode(b=0) == 0

    wsb = lib.msmd_free_anchor_box_prob_workspace_bytes(5)
    assert wsb >= 20 and lib.msmd_free_anchor_box_prob_workspace_bytes(-1) == 0

    def prob(pred=p, b=2, a=8, gt=p, labels=p, g=5, offs=p, c=3, out=p, work=p, nbytes=wsb):
        return lib.msmd_free_anchor_box_prob_f32(pred, b, a, gt, labels, g, offs, c, 0.6, out,
                                                 work, nbytes, None)
    assert prob(pred=None) == -1 and prob(gt=None) == -1 and prob(labels=None) == -1
    assert prob(offs=None) == -1 and prob(out=None) == -1 and prob(c=0) == -1
    assert prob(b=-1) == -1 and prob(g=-1) == -1
    assert prob(work=None) == -2 and prob(nbytes=0) == -2

    assert lib.msmd_free_anchor_negative_workspace_bytes(4099, 10) >= 8 * 21
    assert lib.msmd_free_anchor_negative_workspace_bytes(-1, 3) == 0
    neg = lambda n=4, c=3, x=p, q=p, out=p, work=p, nbytes=256, gamma=2.0: \
        lib.msmd_free_anchor_negative_f32(x, q, n, c, gamma, 0.5, None, out, work, nbytes, None)
    assert neg(gamma=0.5) == -1 and neg(gamma=float("nan")) == -1
    assert neg(n=-1) == -1 and neg(c=0) == -1 and neg(x=None) == -1 and neg(q=None) == -1
    assert neg(out=None) == -1 and neg(work=None) == -2 and neg(nbytes=0) == -2


def test_python_wrappers_refuse_before_the_library():
    from msmdfusion_amd import kernels as K
    with pytest.raises(RuntimeError, match="CUDA"):
        K.free_anchor_topk(torch.zeros(8, 4), torch.zeros(1, 4), 2)
    with pytest.raises(RuntimeError, match="CUDA"):
        K.free_anchor_negative(torch.zeros(8, 3), torch.zeros(8, 3))


def test_reduction_override_none_changes_nothing():
    """With the default the two loss classes compute bit for bit what they did; 'none' returns
    the weighted elements times loss_weight."""
    from msmdfusion_amd import anchor_head as A
    g = torch.Generator().manual_seed(5)
    pred, target = torch.randn((40, 7), generator=g), torch.randn((40, 7), generator=g)
    weight = torch.rand((40, 7), generator=g)
    l1 = A.SmoothL1Loss(beta=1.0 / 9.0, loss_weight=2.0)
    diff = (pred - target).abs()
    each = torch.where(diff < l1.beta, 0.5 * diff * diff / l1.beta, diff - 0.5 * l1.beta)
    for avg in (None, 13.0):
        want = 2.0 * A._weighted_mean(each, weight, avg)
        assert torch.equal(l1(pred, target, weight, avg_factor=avg), want)
        assert torch.equal(l1(pred, target, weight, avg_factor=avg, reduction_override=None), want)
        assert torch.equal(l1(pred, target, weight, avg_factor=avg, reduction_override="mean"),
                           want)
    assert torch.equal(l1(pred, target, weight, reduction_override="none"), 2.0 * (each * weight))
    assert torch.equal(l1(pred, target, reduction_override="none"), 2.0 * each)
    ce = A.CrossEntropyLoss(loss_weight=0.2)
    score, label = torch.randn((40, 2), generator=g), torch.randint(0, 2, (40,), generator=g)
    w = torch.rand((40,), generator=g)
    raw = torch.nn.functional.cross_entropy(score, label, reduction="none")
    for avg in (None, 13.0):
        want = 0.2 * A._weighted_mean(raw, w, avg)
        assert torch.equal(ce(score, label, w, avg_factor=avg), want)
        assert torch.equal(ce(score, label, w, avg_factor=avg, reduction_override=None), want)
    assert torch.equal(ce(score, label, reduction_override="none"), 0.2 * raw)
    assert torch.equal(ce(score, label, w, reduction_override="none"), 0.2 * (raw * w))
    with pytest.raises(NotImplementedError):
        l1(pred, target, reduction_override="sum")
