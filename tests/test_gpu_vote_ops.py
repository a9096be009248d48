"""The VoteNet kernels (csrc/vote.hip, the aligned3d entry of csrc/nms.hip) against the
restatements of tests/vote_ref.py: Chamfer forward and backward bit for bit, vote targets and
point counts exactly, aligned 3-D NMS keep lists exactly."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vote_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("l2", "l1", "smooth_l1")
ULP = float(np.finfo(np.float32).eps)
NAN, INF = float("nan"), float("inf")


@pytest.fixture(autouse=True)
def _leave_the_global_rng_alone(dev):
    with torch.random.fork_rng(devices=[dev]):
        yield


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, want):
    """Bit for bit, except that any NaN equals any NaN (its payload is not part of the contract)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    both_nan = np.isnan(got) & np.isnan(want)
    return got.shape == want.shape and bool(((_bits(got) == _bits(want)) | both_nan).all())


def _forward(src, dst, mode, dev):
    from msmdfusion_amd import kernels as K
    out = K.chamfer_forward(torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev), mode)
    assert out[1].dtype == torch.long and out[3].dtype == torch.long
    return [o.cpu().numpy() for o in out]


def _check_forward(src, dst, mode, dev):
    d1, i1, d2, i2 = _forward(src, dst, mode, dev)
    w1, wi1, w2, wi2 = V.chamfer_forward(src, dst, mode)
    assert np.array_equal(i1, wi1) and np.array_equal(i2, wi2), (mode, src.shape, dst.shape)
    assert _same_bits(d1, w1) and _same_bits(d2, w2), (mode, src.shape, dst.shape)


# ------------------------------------------------------------------------------ Chamfer forward
@pytest.mark.parametrize("mode", MODES)
def test_chamfer_forward_bitwise_over_the_shape_grid(dev, mode):
    """Both kernel shapes and their boundaries: fewer than 64 query points per batch (flat), 64 and
    more (tiled), the other set below, at and past one 256-point LDS tile, odd sizes; values
    around |d| = 1, where smooth_l1 changes branch."""
    rng = np.random.default_rng(17)
    for b in (1, 3):
        for n in (1, 63, 64, 65, 257, 1000):
            for m in (1, 3, 64, 65, 300):
                src = rng.normal(0, 1.2, (b, n, 3)).astype(np.float32)
                dst = rng.normal(0, 1.2, (b, m, 3)).astype(np.float32)
                _check_forward(src, dst, mode, dev)


@pytest.mark.parametrize("mode", MODES)
def test_chamfer_forward_vote_shape(dev, mode):
    """The vote loss: thousands of batches of 1 x 3 (and the 3 x 1 direction)."""
    rng = np.random.default_rng(23)
    src = rng.normal(0, 1, (4096, 1, 3)).astype(np.float32)
    dst = rng.normal(0, 1, (4096, 3, 3)).astype(np.float32)
    dst[::5, 2] = dst[::5, 0]                      # two of the three targets equal
    _check_forward(src, dst, mode, dev)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,m", [(5, 9), (70, 300)])
def test_chamfer_forward_ties_nan_and_inf(dev, mode, n, m):
    """torch.min's rules: equal distances -> the lowest index; a NaN distance is the minimum and
    the first NaN is reported; +-inf coordinates (inf - inf = NaN included)."""
    rng = np.random.default_rng(n * 100 + m)
    src = rng.normal(0, 1, (2, n, 3)).astype(np.float32)
    dst = rng.normal(0, 1, (2, m, 3)).astype(np.float32)
    dst[:, m - 1] = dst[:, 1]                      # duplicates: index 1 must win over m - 1
    dst[:, 4] = dst[:, 1]
    src[0, 2, 1] = NAN                             # a NaN on each side
    dst[0, 3, 0] = NAN
    dst[0, 7, 2] = NAN                             # a later NaN: the first one is reported
    src[1, 0, 0] = INF
    dst[1, 2, 0] = INF                             # inf - inf
    dst[1, 5, 1] = -INF
    src[1, 3] = INF                                # every distance of this point is inf or NaN
    _check_forward(src, dst, mode, dev)
    d1, i1, d2, i2 = _forward(src, dst, mode, dev)
    # the first NaN wins: destination 3 for every source but the NaN source itself, whose every
    # distance is NaN (index 0); source 2 for every destination but the two NaN ones
    assert i1[0].tolist() == [0 if k == 2 else 3 for k in range(n)] and np.isnan(d1[0]).all()
    assert i2[0].tolist() == [0 if k in (3, 7) else 2 for k in range(m)] and np.isnan(d2[0]).all()
    clean = np.ones(n, bool)
    clean[[0, 3]] = False
    assert not np.isin(i1[1][clean], (4, m - 1)).any()       # never the later duplicate


def test_chamfer_forward_refuses_what_it_does_not_handle(dev):
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd._lib import MsmdError
    ok = torch.zeros((2, 4, 3), device=dev)
    for src, dst in ((torch.zeros((2, 4, 4), device=dev), torch.zeros((2, 5, 4), device=dev)),
                     (torch.zeros((2, 0, 3), device=dev), ok), (ok, torch.zeros((2, 0, 3), device=dev))):
        with pytest.raises(MsmdError, match="msmd_chamfer_fwd_f32"):
            K.chamfer_forward(src, dst, "l2")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.chamfer_forward(ok.cpu(), ok.cpu(), "l2")


def test_chamfer_allocates_no_matrix(dev):
    """N = M = 4096: forward and backward together stay far below one [N, M] float matrix."""
    from msmdfusion_amd import losses as L
    n = 4096
    g = torch.Generator().manual_seed(3)
    src = torch.randn((1, n, 3), generator=g).to(dev).requires_grad_()
    dst = torch.randn((1, n, 3), generator=g).to(dev).requires_grad_()
    L.chamfer_distance(src[:, :8], dst[:, :8])                # warm: module load
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss_src, loss_dst, _, _ = L.chamfer_distance(src, dst, reduction="sum")
    (loss_src + loss_dst).backward()
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - before
    print("peak delta %d bytes, matrix %d" % (delta, n * n * 4))
    assert delta < n * n * 4
    assert src.grad.shape == src.shape and bool(torch.isfinite(dst.grad).all())


# ----------------------------------------------------------------------------- Chamfer backward
def _backward_case(name):
    rng = np.random.default_rng(41)
    if name == "crowd":
        # 1000 sources whose nearest is destination 0; destinations 1.. are nobody's nearest;
        # exact |d| = 1 and d = 0 coordinates for the l1 / smooth_l1 kinks
        src = rng.normal(0, 0.1, (2, 1000, 3)).astype(np.float32)
        dst = (rng.normal(0, 0.5, (2, 7, 3)) + 8).astype(np.float32)
        dst[:, 0] = np.float32([0.0625, 0, 0])
        src[:, 0] = dst[:, 0] + np.float32([1, 0, -1])
        src[:, 1] = dst[:, 0]
        src[:, 2] = dst[:, 0] + np.float32([0, 1, 0.5])
    elif name == "tiled":
        src = rng.normal(0, 1.5, (3, 257, 3)).astype(np.float32)
        dst = rng.normal(0, 1.5, (3, 300, 3)).astype(np.float32)
    else:                                            # the vote shape, both directions flat
        src = rng.normal(0, 1.5, (512, 1, 3)).astype(np.float32)
        dst = rng.normal(0, 1.5, (512, 3, 3)).astype(np.float32)
    w1 = rng.uniform(0.1, 2, src.shape[:2]).astype(np.float32)
    w2 = rng.uniform(0.1, 2, dst.shape[:2]).astype(np.float32)
    w2[:, ::3] = 0                                   # zero upstream gradients
    return src, dst, w1, w2


def _weighted(fn, src, dst, w1, w2, mode):
    a, b = fn(src, dst, mode)[:2]
    return (a * w1).sum() + (b * w2).sum()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ("crowd", "tiled", "vote"))
def test_chamfer_backward_bitwise_and_against_float64_autograd(dev, case, mode):
    from msmdfusion_amd import losses as L
    src, dst, w1, w2 = _backward_case(case)
    _, i1, _, i2 = V.chamfer_forward(src, dst, mode)
    if case == "crowd":
        assert (i1 == 0).all() and not np.isin(np.arange(1, 7), i1).any()
    want_src, want_dst = V.chamfer_backward(src, dst, w1, w2, i1, i2, mode)

    t = [torch.from_numpy(a).to(dev) for a in (src, dst, w1, w2)]
    s, d = t[0].clone().requires_grad_(), t[1].clone().requires_grad_()
    _weighted(L.chamfer_min, s, d, t[2], t[3], mode).backward()
    assert _same_bits(s.grad.cpu().numpy(), want_src), (case, mode)
    assert _same_bits(d.grad.cpu().numpy(), want_dst), (case, mode)

    # float64 autograd over the expanded formulation; torch's own float32 run of it is the yardstick
    s64, d64 = t[0].double().requires_grad_(), t[1].double().requires_grad_()
    _weighted(L.chamfer_distance_expanded, s64, d64, t[2].double(), t[3].double(), mode).backward()
    s32, d32 = t[0].clone().requires_grad_(), t[1].clone().requires_grad_()
    _weighted(L.chamfer_distance_expanded, s32, d32, t[2], t[3], mode).backward()
    for got, own, ref in ((s.grad, s32.grad, s64.grad), (d.grad, d32.grad, d64.grad)):
        scale = max(float(ref.abs().max()), 1e-30)
        err = float((got.double() - ref).abs().max())
        own_err = float((own.double() - ref).abs().max())
        print(case, mode, "grad err %.3g own %.3g scale %.3g" % (err, own_err, scale))
        assert err <= 4 * max(own_err, ULP * scale)


def test_chamfer_only_one_side_needs_a_gradient(dev):
    from msmdfusion_amd import losses as L
    src, dst, w1, w2 = _backward_case("tiled")
    t = [torch.from_numpy(a).to(dev) for a in (src, dst, w1, w2)]
    both_s, both_d = t[0].clone().requires_grad_(), t[1].clone().requires_grad_()
    _weighted(L.chamfer_min, both_s, both_d, t[2], t[3], "l2").backward()
    only = t[1].clone().requires_grad_()
    _weighted(L.chamfer_min, t[0], only, t[2], t[3], "l2").backward()
    assert torch.equal(only.grad, both_d.grad)
    # a loss on one direction only: the other upstream gradient is absent
    one = t[0].clone().requires_grad_()
    (L.chamfer_min(one, t[1], "l1")[0] * t[2]).sum().backward()
    _, i1, _, i2 = V.chamfer_forward(src, dst, "l1")
    want, _ = V.chamfer_backward(src, dst, w1, np.zeros_like(w2), i1, i2, "l1")
    assert _same_bits(one.grad.cpu().numpy(), want)


@pytest.mark.parametrize("mode", MODES)
def test_chamfer_bitwise_reproducible(dev, mode):
    from msmdfusion_amd import kernels as K
    g = torch.Generator().manual_seed(5)
    src = torch.randn((8, 1024, 3), generator=g).to(dev)
    dst = torch.randn((8, 64, 3), generator=g).to(dev)
    g1, g2 = torch.rand((8, 1024), generator=g).to(dev), torch.rand((8, 64), generator=g).to(dev)
    runs = []
    for _ in range(2):
        d1, i1, d2, i2 = K.chamfer_forward(src, dst, mode)
        gs, gd = K.chamfer_backward(src, dst, g1, g2, i1, i2, mode)
        runs.append((d1, i1, d2, i2, gs, gd))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)


# --------------------------------------------------------------------------------- vote targets
ROTATIONS = (0.0, np.pi / 2, -np.pi / 2)


def _boxes(rng, t, lo=-4.0, hi=4.0):
    """[t, 7] (x, y, z bottom, w, l, h, rz) crowded enough that points fall inside several."""
    xy = rng.uniform(lo, hi, (t, 2))
    zb = rng.uniform(-1, 0, (t, 1))
    size = rng.uniform(1.0, 5.0, (t, 3))
    rz = np.array([ROTATIONS[i % 4] if i % 4 < 3 else rng.uniform(-np.pi, np.pi) for i in range(t)])
    return np.concatenate([xy, zb, size, rz[:, None]], 1).astype(np.float32)


@pytest.fixture(scope="module")
def vote_case():
    """Four samples of unequal length, points [N, 4]: (1 point, the all-zero fake box), (255, 2
    nested boxes), (256, 65), (4099, 130) -- 65 and 130 cross the 64-box LDS chunk."""
    rng = np.random.default_rng(77)
    sizes, gts = (1, 255, 256, 4099), (1, 2, 65, 130)
    points, boxes = [], []
    for n, t in zip(sizes, gts):
        p = np.concatenate([rng.uniform(-5, 5, (n, 2)), rng.uniform(-1.5, 4, (n, 1)),
                            rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
        b = _boxes(rng, t)
        if t == 1:
            b[:] = 0                                 # the reference's fake box of an empty sample
        if t == 2:                                   # nested, rotated by +-pi/2
            b[0] = [0, 0, -1, 8, 6, 4, np.pi / 2]
            b[1] = [0, 0, -1, 4, 3, 2, -np.pi / 2]
        if t == 65:                                  # five nested boxes (0, +-pi/2, arbitrary) ...
            for k in range(5):
                b[k] = [1, -1, 0, 2 + k, 2 + k, 2, (0.0, np.pi / 2, -np.pi / 2, 0.7, 0.0)[k]]
            p[0, :3] = [1, -1, 1]                    # ... and a point at their centre
            p[1, :3] = [1, -1, 2]                    # on the top face: |z - cz| > h / 2 is false
            p[2, :3] = [1, -1, np.nextafter(np.float32(2), np.float32(3))]   # just above it
        points.append(p)
        boxes.append(b)
    return points, boxes


def test_vote_targets_exact_against_the_reference_loop(dev, vote_case):
    from msmdfusion_amd import kernels as K
    points, boxes = vote_case
    pts = torch.from_numpy(np.concatenate(points)).to(dev)
    bxs = torch.from_numpy(np.concatenate(boxes)).to(dev)
    centers = bxs[:, :3].clone()
    centers[:, 2] += bxs[:, 5] * 0.5
    p_off = torch.tensor(np.concatenate([[0], np.cumsum([len(p) for p in points])]),
                         dtype=torch.int32, device=dev)
    b_off = torch.tensor(np.concatenate([[0], np.cumsum([len(b) for b in boxes])]),
                         dtype=torch.int32, device=dev)
    targets, mask = K.vote_targets(pts, p_off, bxs, centers, b_off, max_points=4099)
    assert targets.shape == (pts.shape[0], 9) and mask.dtype == torch.long
    small_grid = K.vote_targets(pts, p_off, bxs, centers, b_off, max_points=256)   # strides
    assert torch.equal(small_grid[0], targets) and torch.equal(small_grid[1], mask)

    seen, at, bt = set(), 0, 0
    for p, b in zip(points, boxes):
        n, t = len(p), len(b)
        sample = pts[at:at + n]
        inside = K.points_in_boxes(bxs[bt:bt + t][None].contiguous(),
                                   sample[None, :, :3].contiguous(), True)[0]
        want_t, want_m = V.vote_targets_loop(sample.cpu(), inside.cpu(), centers[bt:bt + t].cpu())
        assert torch.equal(targets[at:at + n].cpu(), want_t), (n, t)
        assert torch.equal(mask[at:at + n].cpu(), want_m), (n, t)
        per_point = inside.sum(1).cpu().numpy()
        seen |= set(per_point.tolist())
        if t == 65:
            assert per_point[0] >= 5 and per_point[1] >= 5 and int(mask[at + 1]) == 1
            assert per_point[2] < per_point[1]
            # slot 2 holds the LAST box's vote, not the third's
            last = int(np.nonzero(inside[0].cpu().numpy())[0][-1])
            assert torch.equal(targets[at, 6:9], centers[bt + last] - sample[0, :3])
        if t == 1:
            assert int(mask[at]) == 0 and float(targets[at].abs().max()) == 0
        at, bt = at + n, bt + t
    assert {0, 1, 2, 3, 5} <= seen, seen


def test_points_per_box_equal_the_table_sum(dev):
    from msmdfusion_amd import kernels as K
    rng = np.random.default_rng(9)
    for b, m, t, ld in ((1, 1, 1, 3), (2, 255, 7, 3), (3, 1000, 65, 4), (2, 4099, 16, 6)):
        pts = np.concatenate([rng.uniform(-5, 5, (b, m, 2)), rng.uniform(-1.5, 4, (b, m, 1)),
                              rng.uniform(0, 1, (b, m, ld - 2))], 2)[..., :ld].astype(np.float32)
        boxes = np.stack([_boxes(rng, t) for _ in range(b)])
        d_pts, d_boxes = torch.from_numpy(pts).to(dev), torch.from_numpy(boxes).to(dev)
        count = K.points_in_boxes_count(d_boxes, d_pts)
        table = K.points_in_boxes(d_boxes, d_pts[..., :3].contiguous(), True)
        assert count.dtype == torch.int32 and count.shape == (b, t)
        assert torch.equal(count, table.sum(1).to(torch.int32))
        assert m < 100 or int(count.max()) > 5
    empty = K.points_in_boxes_count(d_boxes, d_pts[:, :0].contiguous())
    assert empty.shape == (2, 16) and int(empty.abs().max()) == 0


# ----------------------------------------------------------------------------------- aligned NMS
LITERAL_BOXES, LITERAL_SCORES = V.LITERAL_BOXES, V.LITERAL_SCORES
LITERAL_CLASSES, LITERAL_PICK = V.LITERAL_CLASSES, V.LITERAL_PICK


def _aligned(boxes, scores, classes, thresh, dev):
    from msmdfusion_amd import iou3d
    return iou3d.aligned_3d_nms(torch.tensor(boxes, dtype=torch.float32, device=dev),
                                torch.tensor(scores, dtype=torch.float32, device=dev),
                                torch.tensor(classes, device=dev), thresh).tolist()


def test_aligned_nms_reference_literal(dev):
    """tests/test_utils/test_nms.py test_aligned_3d_nms of the reference: 30 boxes, 0.25."""
    assert _aligned(LITERAL_BOXES, LITERAL_SCORES, LITERAL_CLASSES, 0.25, dev) == LITERAL_PICK


@pytest.fixture(scope="module")
def nms_pool():
    rng = np.random.default_rng(13)
    n = 1200
    centre = rng.uniform(0, 14, (n, 3))
    size = rng.uniform(1, 5, (n, 3))
    boxes = np.concatenate([centre - size / 2, centre + size / 2], 1).astype(np.float32)
    classes = rng.integers(0, 4, n)
    scores = (rng.permutation(n).astype(np.float32) + 1) / n
    scores[5::40] = scores[4::40]                    # score ties: the lower index goes first
    return boxes, scores, classes


def _run_batched(boxes, scores, classes, sizes, thresh, dev, pre_max=None, post_max=None):
    from msmdfusion_amd import iou3d
    total = int(sum(sizes))
    rows = np.concatenate([boxes[:total], classes[:total, None].astype(np.float32)], 1)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
    keep, num = iou3d.nms_batched("aligned3d", torch.from_numpy(rows).to(dev),
                                  torch.from_numpy(scores[:total]).to(dev), offsets, thresh,
                                  pre_max, post_max)
    keep, num = keep.cpu().numpy(), num.cpu().numpy()
    got = []
    for s in range(len(sizes)):
        assert (keep[s, num[s]:] == -1).all()
        got.append(keep[s, :num[s]].tolist())
    return got


def _want_batched(boxes, scores, classes, sizes, thresh, pre_max=None, post_max=None):
    out, at = [], 0
    for n in sizes:
        order = np.argsort(-scores[at:at + n].astype(np.float64), kind="stable")[:pre_max] + at
        out.append(V.aligned_nms(boxes, classes, thresh, order)[:post_max])
        at += n
    return out


@pytest.mark.parametrize("thresh", (0.1, 0.25, 0.7))
def test_aligned_nms_exact_keep_lists(dev, nms_pool, thresh):
    """Every operation of the pair test is a correctly rounded float32 one on both sides, so the
    lists are equal without a margin around the threshold."""
    boxes, scores, classes = nms_pool
    for sizes in ([0], [1], [63], [64], [65], [1000], [65, 0, 63, 1000, 1, 64]):
        got = _run_batched(boxes, scores, classes, sizes, thresh, dev)
        want = _want_batched(boxes, scores, classes, sizes, thresh)
        assert got == want, (thresh, sizes)
    assert 1 < len(want[3]) < 1000 or thresh == 0.7


def test_aligned_nms_hand_cases(dev):
    box = [0, 0, 0, 2, 2, 2]
    # the same box in two classes: both kept; in one class: only the better
    assert _aligned([box, box], [0.5, 0.9], [1, 2], 0.25, dev) == [1, 0]
    assert _aligned([box, box, box], [0.5, 0.9, 0.7], [3, 3, 3], 0.25, dev) == [1]
    # equal scores: the lower index is visited first
    assert _aligned([box, box], [0.5, 0.5], [3, 3], 0.25, dev) == [0]
    # IoU exactly at the threshold stays (iou <= thresh): [0,2]^3 and [0,2]x[0,2]x[0,1] -> 0.5
    half = [0, 0, 0, 2, 2, 1]
    assert _aligned([box, half], [0.9, 0.5], [0, 0], 0.5, dev) == [0, 1]
    assert _aligned([box, half], [0.9, 0.5], [0, 0], 0.49, dev) == [0]
    # two disjoint zero-volume boxes: inter 0, union 0, IoU NaN -> `NaN <= thresh` is false and the
    # later one goes, in ANOTHER class too (NaN * 0 = NaN); a proper box next to them stays
    flat_a, flat_b = [0, 0, 0, 1, 1, 0], [5, 5, 5, 6, 5, 6]
    assert _aligned([flat_a, flat_b, box], [0.9, 0.8, 0.7], [0, 1, 1], 0.25, dev) == [0, 2]
    want = V.aligned_nms(np.float32([flat_a, flat_b, box]), np.array([0, 1, 1]), 0.25, [0, 1, 2])
    assert want == [0, 2]


def test_aligned_nms_cuts_and_order(dev, nms_pool):
    from msmdfusion_amd import kernels as K
    boxes, scores, classes = nms_pool
    sizes = [65, 0, 300]
    full = _want_batched(boxes, scores, classes, sizes, 0.25)
    assert _run_batched(boxes, scores, classes, sizes, 0.25, dev, post_max=9) == [k[:9] for k in full]
    assert _run_batched(boxes, scores, classes, sizes, 0.25, dev, pre_max=40, post_max=9) == \
        _want_batched(boxes, scores, classes, sizes, 0.25, pre_max=40, post_max=9)
    # without `order` the call reports positions in the (already sorted) segment; with it, order[row]
    n = 200
    order = np.argsort(-scores[:n].astype(np.float64), kind="stable")
    rows = np.concatenate([boxes[:n], classes[:n, None].astype(np.float32)], 1)[order]
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    offsets = torch.tensor([0, n], dtype=torch.int32, device=dev)
    th = torch.full((1,), 0.25, device=dev)
    pos, num = K.nms_segments("aligned3d", d_rows, offsets, th, n)
    want = V.aligned_nms(boxes[:n], classes[:n], 0.25, order)
    assert order[pos[0, :int(num[0])].cpu().numpy()].tolist() == want
    mapped, num2 = K.nms_segments("aligned3d", d_rows, offsets, th, n,
                                  order=torch.from_numpy(order).to(dev))
    assert mapped[0, :int(num2[0])].tolist() == want
    with pytest.raises(Exception):
        K.nms_segments("aligned3d", d_rows[:, :6].contiguous(), offsets, th, n)    # no class column


def test_aligned_nms_no_allocation_no_host_wait_and_reproducible(dev, nms_pool):
    from msmdfusion_amd import kernels as K
    segs, n = 24, 1000
    boxes, _, classes = nms_pool
    rows = np.concatenate([boxes[:n], classes[:n, None].astype(np.float32)], 1)
    d_rows = torch.from_numpy(np.concatenate([rows] * segs)).to(dev)
    offsets = torch.arange(segs + 1, dtype=torch.int32, device=dev) * n
    th = torch.full((segs,), 0.25, device=dev)
    nbytes = K.lib.msmd_nms_aligned3d_workspace_bytes(segs * n, n)
    assert nbytes == segs * n * 16 * 8
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    keep = torch.empty((segs, 83), dtype=torch.long, device=dev)
    num = torch.empty((segs,), dtype=torch.int32, device=dev)
    call = lambda: K.nms_segments("aligned3d", d_rows, offsets, th, n, post_max=83, keep=keep,  # noqa
                                  num_keep=num, workspace=ws)
    call()                                              # warm: module load
    first = (keep.clone(), num.clone())
    big = torch.randn((8192, 8192), device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    stream = torch.cuda.current_stream()
    for _ in range(8):
        big = big @ big * 1e-4                          # tens of milliseconds of queued work
    mid = torch.cuda.max_memory_allocated()
    call()
    assert not stream.query(), "the NMS call synchronised with the device"
    assert torch.cuda.max_memory_allocated() == mid and torch.cuda.memory_allocated() <= mid
    torch.cuda.synchronize()
    assert torch.equal(keep, first[0]) and torch.equal(num, first[1])
    assert (num.cpu() == num.cpu()[0]).all() and 0 < int(num[0]) <= 83
