"""The four native pieces of FreeAnchor3DHead's loss on the GPU (csrc/free_anchor.hip) against
the matrix restatements of tests/free_anchor_ref.py on the same device: the exact top-k with its
tie rule, the box probability, decode + nearest BEV, the negative bag loss; and that none of them
allocates a [G, A] matrix or waits for the device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import free_anchor_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ULP = float(np.finfo(np.float32).eps)


@pytest.fixture(autouse=True)
def _leave_the_global_rng_alone(dev):
    with torch.random.fork_rng(devices=[dev]):
        yield


# ---------------------------------------------------------------- top-k
def grid_anchors(n, seed):
    """n axis-aligned boxes with centres on an integer grid and sides 1 or 2 -- every corner is
    exact in float32, so equal geometry gives bitwise equal IoUs: ties everywhere."""
    g = torch.Generator().manual_seed(seed)
    side = int(np.ceil(np.sqrt(n / 2))) + 1
    c = torch.stack(torch.meshgrid(torch.arange(side), torch.arange(side), indexing="ij"), -1)
    c = c.reshape(-1, 2).float().repeat_interleave(2, 0)[:n]
    half = torch.tensor([0.5, 1.0]).repeat(c.shape[0] // 2 + 1)[:n, None]
    order = torch.randperm(n, generator=g)
    return torch.cat([c - half, c + half], 1)[order].contiguous(), side


def grid_truth(n, side, seed):
    """n boxes with corners on the quarter grid: some large (they hold many anchors of one size:
    equal IoUs), some small, one outside everything."""
    g = torch.Generator().manual_seed(seed)
    lo = torch.randint(0, 4 * side, (n, 2), generator=g).float() / 4 - 0.5
    size = torch.randint(1, 4 * max(side // 2, 2), (n, 2), generator=g).float() / 4
    box = torch.cat([lo, lo + size], 1)
    if n > 2:
        box[2] = torch.tensor([1e4, 1e4, 1e4 + 3, 1e4 + 3])          # touches nothing
    return box.contiguous()


@pytest.mark.parametrize("num_anchors", [64, 255, 256, 257, 4099])
def test_topk_equals_the_sorted_matrix(dev, num_anchors):
    """Exactly the restatement's bags for every G across the LDS chunks and every admissible k;
    rows ascending; two runs bitwise equal."""
    from msmdfusion_amd import kernels as K
    cap = K.FREE_ANCHOR_MAX_TOPK
    assert cap >= 64
    anchors, side = grid_anchors(num_anchors, num_anchors)
    anchors = anchors.to(dev)
    ties = 0
    for G in (0, 1, 127, 128, 129):
        gt = grid_truth(G, side, 10 * num_anchors + G).to(dev)
        for k in sorted({1, 25, 50, cap, num_anchors}):
            if k > min(cap, num_anchors):
                with pytest.raises(ValueError):
                    K.free_anchor_topk(anchors, gt, k)
                continue
            got = K.free_anchor_topk(anchors, gt, k)
            again = K.free_anchor_topk(anchors, gt, k)
            assert got.dtype == torch.int32 and tuple(got.shape) == (G, k)
            assert torch.equal(got, again)
            want = R.topk_restatement(anchors, gt, k)
            assert torch.equal(got.long(), want), (G, k)
            if k > 1 and G:
                assert bool((got[:, 1:] > got[:, :-1]).all())
            if G and k < num_anchors:
                val = torch.sort(R.A.bbox_overlaps(gt, anchors), dim=1, descending=True)[0]
                ties += int((val[:, k - 1] == val[:, k]).sum())
    assert ties > 0                                   # the cut went through equal IoUs


def test_topk_on_constructed_ties(dev):
    from msmdfusion_amd import kernels as K
    same = torch.tensor([[0.0, 0.0, 2.0, 2.0]]).repeat(600, 1).to(dev)
    gt = torch.tensor([[0.5, 0.5, 2.5, 2.5], [50.0, 50.0, 51.0, 51.0],
                       [float("nan")] * 4]).to(dev)
    for k in (1, 25, 256):
        # all anchors identical (and, for the second box, all IoUs zero; for the third, all NaN):
        # the first k by index
        got = K.free_anchor_topk(same, gt, k)
        assert torch.equal(got.long(), torch.arange(k, device=dev)[None].expand(3, -1))
        assert torch.equal(got.long(), R.topk_restatement(same, gt, k))
    # a box touching fewer than k anchors: they, then the lowest-index zeros
    anchors, side = grid_anchors(700, 3)
    anchors = anchors.to(dev)
    small = anchors[[411]].clone()
    iou = R.A.bbox_overlaps(small, anchors)[0]
    touched = int((iou > 0).sum())
    assert 0 < touched < 25
    got = K.free_anchor_topk(anchors, small, 25)
    assert torch.equal(got.long(), R.topk_restatement(anchors, small, 25))
    zeros = torch.nonzero(iou == 0)[:25 - touched, 0]
    assert set(got[0].tolist()) == set(torch.nonzero(iou > 0)[:, 0].tolist()) | set(zeros.tolist())
    # equal IoUs on both sides of the 256-lane workgroup boundary and of the cut: 13 identical
    # anchors at 250 .. 262, five better ones elsewhere, k = 5 + 7
    far = torch.tensor([[90.0, 90.0, 91.0, 91.0]]).repeat(600, 1)
    far[250:263] = torch.tensor([0.0, 0.0, 2.0, 4.0])
    for i in (3, 255, 256, 400, 599):
        far[i] = torch.tensor([0.0, 0.0, 2.0, 2.5])
    far = far.to(dev)
    box = torch.tensor([[0.0, 0.0, 2.0, 2.0]]).to(dev)
    got = K.free_anchor_topk(far, box, 12)
    assert got[0].tolist() == [3, 250, 251, 252, 253, 254, 255, 256, 257, 258, 400, 599]
    assert torch.equal(got.long(), R.topk_restatement(far, box, 12))
    # a NaN anchor sorts first for every ground truth
    far[77] = float("nan")
    got = K.free_anchor_topk(far, box, 3)
    assert got[0].tolist() == [3, 77, 255]
    assert torch.equal(got.long(), R.topk_restatement(far, box, 3))
    # a NaN ground truth (in one coordinate, in all) against anchors of DIFFERING sizes: every IoU
    # is NaN, as in torch, so the bag is the first k by index -- not the largest anchors, which
    # is what fmaxf / fminf dropping the NaN would select
    g = torch.Generator().manual_seed(8)
    centre, half = torch.rand((700, 2), generator=g) * 30, torch.rand((700, 2), generator=g) * 3 + 0.2
    mixed = torch.cat([centre - half, centre + half], 1).to(dev)
    nan = float("nan")
    bad = torch.tensor([[nan] * 4, [1.0, 1.0, nan, 9.0], [3.0, 3.0, 9.0, 9.0], [nan, 0.0, 5.0, 5.0]])
    bad = bad.to(dev)
    for k in (1, 25, 256):
        got = K.free_anchor_topk(mixed, bad, k)
        want = R.topk_restatement(mixed, bad, k)
        assert torch.equal(got.long(), want)
        for row in (0, 1, 3):
            assert got[row].tolist() == list(range(k))
    assert K.free_anchor_topk(mixed, bad, 25)[2].tolist() != list(range(25))
    area = (mixed[:, 2] - mixed[:, 0]) * (mixed[:, 3] - mixed[:, 1])
    assert torch.sort(area, descending=True)[1][:25].sort()[0].tolist() != list(range(25))
    # ... and two NaN anchors of differing finite remainder among them: both in every bag
    mixed[5, 2], mixed[300] = nan, nan
    got = K.free_anchor_topk(mixed, bad, 4)
    assert torch.equal(got.long(), R.topk_restatement(mixed, bad, 4))
    assert 5 in got[2].tolist() and 300 in got[2].tolist()


# ---------------------------------------------------------------- box probability
def _prob_case(dev, counts, num_anchors, num_classes, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(counts)
    centre = torch.rand((B * num_anchors, 2), generator=g) * 40
    half = torch.rand((B * num_anchors, 2), generator=g) * 1.5 + 0.5
    pred = torch.cat([centre - half, centre + half], 1)
    # every odd row is a near copy of the row before it: a box close to one is close to both
    pred[1::2] = pred[0::2] + (torch.rand((B * num_anchors // 2, 4), generator=g) - 0.5) * 0.3
    boxes, labels = [], []
    for b, n in enumerate(counts):
        pick = torch.randint(0, num_anchors, (n,), generator=g) + b * num_anchors
        box = pred[pick] + torch.randn((n, 4), generator=g) * 0.05
        lab = torch.randint(0, num_classes, (n,), generator=g)
        if n > 1:                                     # two boxes of one class on one anchor
            box[1] = box[0] + 0.02
            lab[1] = lab[0]
        if n > 2:
            box[2] = torch.tensor([500.0, 500.0, 501.0, 501.0])      # t2 = 0 <= t1
        if n > 4:
            lab[3], lab[4] = num_classes, -1                        # labels out of range
        boxes.append(box)
        labels.append(lab)
    return (pred.to(dev), torch.cat(boxes).to(dev), torch.cat(labels).to(dev),
            torch.tensor(np.cumsum([0] + list(counts)), dtype=torch.int32).to(dev))


@pytest.mark.parametrize("num_classes", [1, 3, 10])
@pytest.mark.parametrize("counts", [(130,), (0,), (0, 130, 5), (7, 0, 129), (128, 3, 0)])
def test_box_prob_equals_the_matrix_restatement(dev, counts, num_classes):
    """torch.equal on the same pred_bev: empty samples first, in the middle and last, ground
    truths across the LDS chunk of 128, 600 anchors (three workgroups, the last one ragged)."""
    from msmdfusion_amd import kernels as K
    pred, gt, labels, offsets = _prob_case(dev, counts, 600, num_classes, sum(counts) + num_classes)
    got = K.free_anchor_box_prob(pred, gt, labels, offsets, num_classes, 0.6)
    again = K.free_anchor_box_prob(pred, gt, labels, offsets, num_classes, 0.6)
    want = R.box_prob_restatement(pred, gt, labels, list(counts), num_classes, 0.6)
    assert tuple(got.shape) == (len(counts) * 600, num_classes)
    assert torch.equal(got, again) and torch.equal(got, want)
    assert bool(((got >= 0) & (got <= 1)).all())
    if sum(counts):
        assert int((got > 0).sum()) > 0 and float(got.max()) == 1.0
        mixed = (got > 0) & (got < 1)
        assert int(mixed.sum()) > 0


def test_box_prob_with_nan_boxes(dev):
    """A NaN coordinate in either box makes the pair's IoU NaN: a NaN ground truth is ignored, a
    NaN prediction keeps a zero row and stays out of every t2 (here the kernel departs from the
    matrix form, whose row maximum would turn t2 into NaN): the result equals the restatement
    on the inputs with the NaN boxes moved out of reach."""
    from msmdfusion_amd import kernels as K
    counts, C = (9, 6), 3
    pred, gt, labels, offsets = _prob_case(dev, counts, 600, C, 77)
    clean = R.box_prob_restatement(pred, gt, labels, list(counts), C, 0.6)
    hit = torch.nonzero((clean == 1.0).any(1))[:, 0]          # rows that set some t2
    assert hit.numel() >= 4
    nan = float("nan")
    bad_pred, bad_gt = pred.clone(), gt.clone()
    bad_pred[hit[0]] = nan
    bad_pred[hit[1], 2] = nan
    bad_gt[5, 0] = nan
    bad_gt[10] = nan
    away_pred, away_gt = pred.clone(), gt.clone()
    away_pred[hit[:2]] = torch.tensor([900.0, 900.0, 901.0, 901.0], device=dev)
    away_gt[[5, 10]] = torch.tensor([-900.0, -900.0, -899.0, -899.0], device=dev)
    got = K.free_anchor_box_prob(bad_pred, bad_gt, labels, offsets, C, 0.6)
    want = R.box_prob_restatement(away_pred, away_gt, labels, list(counts), C, 0.6)
    assert torch.equal(got, want)
    assert float(got[hit[:2]].abs().max()) == 0.0 and not torch.equal(want, clean)
    assert bool(torch.isfinite(got).all()) and float(got.max()) == 1.0


# ---------------------------------------------------------------- decode + nearest BEV
@pytest.mark.parametrize("code", [7, 9])
def test_decode_nearest_bev_against_float64(dev, code):
    """Within 4 x the error of the float32 torch form against the float64 torch form, floored
    at float32 eps of the scale; rotations stay 1e-3 away from the pi/4 swap."""
    from msmdfusion_amd import kernels as K
    g = torch.Generator().manual_seed(code)
    A_, B = 1000, 3
    anchors = torch.rand((A_, code), generator=g)
    anchors[:, :2] = anchors[:, :2] * 100 - 50
    anchors[:, 3:6] = anchors[:, 3:6] * 3 + 0.4
    anchors[:, 6] = torch.tensor([0.0, 1.57]).repeat(A_ // 2)
    deltas = torch.randn((B * A_, code), generator=g) * 0.4
    rot = (deltas[:, 6] + anchors[:, 6].repeat(B)).double()
    normed = (rot - torch.floor(rot / np.pi + 0.5) * np.pi).abs()
    deltas[(normed - np.pi / 4).abs() < 1e-3, 6] += 0.01
    anchors, deltas = anchors.to(dev), deltas.to(dev)
    want = R.decode_bev_restatement(anchors.double(), deltas.double())
    own = R.decode_bev_restatement(anchors, deltas)
    got = K.decode_nearest_bev(anchors, deltas)
    assert torch.equal(got, K.decode_nearest_bev(anchors, deltas))
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    ref = float((own.double() - want).abs().max())
    print(code, "decode", err / scale, ref / scale)
    assert err <= 4 * max(ref, ULP * scale)
    swapped = (want[:, 2] - want[:, 0]) > (want[:, 3] - want[:, 1])
    assert 0 < int(swapped.sum()) < swapped.numel()


# ---------------------------------------------------------------- negative bag loss
@pytest.mark.parametrize("c", [1, 3, 10])
@pytest.mark.parametrize("n", [1, 63, 4099])
def test_negative_bag_value_and_gradient(dev, n, c):
    """Value and gradient against float64 autograd of the restatement within 4 x the error the
    float32 torch restatement shows (floored at float32 eps of the scale): logits of +-30, box
    probabilities of exactly 0 and 1, gamma 1 and 2; two runs bitwise equal."""
    from msmdfusion_amd import kernels as K
    g = torch.Generator(device="cpu").manual_seed(n * 31 + c)
    x = (torch.randn((n, c), generator=g) * 3).to(dev)
    x.view(-1)[::7] = 30.0
    x.view(-1)[3::11] = -30.0
    q = torch.rand((n, c), generator=g).to(dev)
    q.view(-1)[::3] = 0.0
    q.view(-1)[1::5] = 1.0
    for gamma in (1.0, 2.0):
        x64 = x.double().requires_grad_()
        want = R.negative_restatement(x64, q.double(), gamma, 0.5)
        want.backward()
        x32 = x.clone().requires_grad_()
        own = R.negative_restatement(x32, q, gamma, 0.5)
        own.backward()
        total, grad = K.free_anchor_negative(x, q, gamma, 0.5)
        again, grad2 = K.free_anchor_negative(x, q, gamma, 0.5)
        assert torch.equal(total, again) and torch.equal(grad, grad2)
        assert K.free_anchor_negative(x, q, gamma, 0.5, want_grad=False)[1] is None
        vscale = max(abs(float(want.detach())), 1e-30)
        verr = abs(float(total) - float(want.detach()))
        vown = abs(float(own.detach()) - float(want.detach()))
        gscale = max(float(x64.grad.abs().max()), 1e-30)
        gerr = float((grad.double() - x64.grad).abs().max())
        gown = float((x32.grad.double() - x64.grad).abs().max())
        print(n, c, gamma, "value", verr / vscale, vown / vscale, "grad", gerr / gscale,
              gown / gscale)
        assert verr <= 4 * max(vown, ULP * vscale)
        assert gerr <= 4 * max(gown, ULP * gscale)
    with pytest.raises(ValueError):
        K.free_anchor_negative(x, q, 0.5, 0.5)


# ---------------------------------------------------------------- memory and waiting
def test_no_matrix_is_allocated_and_nothing_waits(dev):
    """A = 65 536, G = 256, C = 3: the top-k and the box probability together raise the peak by
    less than one [G, A] float matrix; all four calls run under the sync debug mode."""
    from msmdfusion_amd import kernels as K
    A_, G, C = 65536, 256, 3
    anchors, side = grid_anchors(A_, 1)
    gt = grid_truth(G, side, 2)
    anchors, gt = anchors.to(dev), gt.to(dev)
    labels = torch.randint(0, C, (G,), generator=torch.Generator().manual_seed(0)).to(dev)
    offsets = torch.tensor([0, G], dtype=torch.int32).to(dev)
    deltas = torch.zeros((A_, 7), device=dev)
    boxes7 = torch.zeros((A_, 7), device=dev)
    boxes7[:, 0:2] = (anchors[:, :2] + anchors[:, 2:]) / 2
    boxes7[:, 3:5] = anchors[:, 2:] - anchors[:, :2]
    logits = torch.zeros((A_, C), device=dev)

    def work():
        matched = K.free_anchor_topk(anchors, gt, 25)
        pred = K.decode_nearest_bev(boxes7, deltas)
        prob = K.free_anchor_box_prob(pred, gt, labels, offsets, C, 0.5)
        total, grad = K.free_anchor_negative(logits, prob, 2.0, 0.5)
        return matched, pred, prob, total, grad

    small = K.free_anchor_topk(anchors[:64], gt[:2], 2)          # warm: module load
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    matched = K.free_anchor_topk(anchors, gt, 25)
    prob = K.free_anchor_box_prob(anchors, gt, labels, offsets, C, 0.5)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - before
    print("peak delta %d bytes, matrix %d" % (delta, G * A_ * 4))
    assert delta < G * A_ * 4
    assert torch.equal(matched.long(), R.topk_restatement(anchors, gt, 25))
    assert torch.equal(prob, R.box_prob_restatement(anchors, gt, labels, [G], C, 0.5))
    first = work()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = work()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert small.shape == (2, 2)
