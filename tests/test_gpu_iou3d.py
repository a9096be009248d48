"""Device-side rotated / normal / circle NMS (csrc/nms.hip, msmdfusion_amd/iou3d.py) against
the numpy restatements of tests/iou3d_ref.py: exact keep lists."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iou3d_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.01, 0.2, 0.7)
MARGIN = 1e-4
KINDS = ("rotate", "normal", "circle")
SIZES = (0, 1, 2, 63, 64, 65, 129, 1000)
LAYOUTS = ([65, 0, 129], [1, 64, 1000])
POOL = 1065


@pytest.fixture(autouse=True)
def _leave_the_global_rng_alone(dev):
    """Seeds and draws of these tests stay inside them: later test files draw unseeded inputs
    and must see the generator state they would see without this file."""
    with torch.random.fork_rng(devices=[dev]):
        yield


def _draw(rng, n):
    xy = rng.uniform(0, 40, (n, 2))
    wl = rng.uniform(1.0, 5.0, (n, 2))
    r = rng.uniform(-np.pi, np.pi, (n, 1))
    return np.concatenate([xy - wl / 2, xy + wl / 2, r], 1).astype(np.float32)


def _near(boxes):
    """Pairs whose float64 IoU (rotated or axis-aligned) lies within MARGIN of a threshold."""
    bad = np.zeros((boxes.shape[0],) * 2, bool)
    for iou in (R.iou_bev(boxes, boxes, np.float64),
                R.iou_normal(boxes[:, :4].astype(np.float64), boxes[:, :4].astype(np.float64))):
        for t in THRESHOLDS:
            bad |= np.abs(iou.astype(np.float64) - t) < MARGIN
    return np.triu(bad, 1)


@pytest.fixture(scope="module")
def pool():
    """POOL boxes + distinct scores; rejection-sampled so that no pair sits within MARGIN of a
    threshold (device sin / cos / atan2 differ from the host's in the last bits)."""
    rng = np.random.default_rng(7)
    boxes = _draw(rng, POOL)
    for _ in range(50):
        cols = np.unique(np.nonzero(_near(boxes))[1])
        if cols.size == 0:
            break
        boxes[cols] = _draw(rng, cols.size)
    scores = rng.permutation(POOL).astype(np.float32) / POOL
    return boxes, scores


@pytest.fixture(scope="module")
def pool_iou(pool):
    """The float32 IoU matrices of the pool, computed once: every list of the tests below is a
    slice of the pool."""
    return {"rotate": R.iou_bev(pool[0], pool[0]), "normal": R.iou_normal(pool[0], pool[0])}


def test_threshold_margin_holds_for_the_final_set(pool):
    assert not _near(pool[0]).any()


def _columns(kind, boxes):
    if kind == "circle":      # centres
        return np.ascontiguousarray((boxes[:, :2] + boxes[:, 2:4]) / np.float32(2))
    return boxes


def _expected(kind, boxes, scores, sizes, thresh, pre_max=None, post_max=None, iou=None):
    out, at = [], 0
    for n in sizes:
        order = R.stable_order(scores[at:at + n])[:pre_max] + at
        if kind == "circle" or iou is None:
            keep = R.nms(kind, boxes, thresh, order) if n else []
        else:
            with np.errstate(invalid="ignore"):
                hit = iou[kind][np.ix_(order, order)] > np.float32(thresh)
            keep = [int(order[i]) for i in R.greedy_nms(hit)]
        out.append(keep[:post_max])
        at += n
    return out


def _run(kind, boxes, scores, sizes, thresh, dev, pre_max=None, post_max=None):
    from msmdfusion_amd import iou3d
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
    total = int(sum(sizes))
    keep, num = iou3d.nms_batched(kind, torch.from_numpy(boxes[:total]).to(dev),
                                  torch.from_numpy(scores[:total]).to(dev), offsets, thresh,
                                  pre_max, post_max)
    keep, num = keep.cpu().numpy(), num.cpu().numpy()
    got = []
    for s in range(len(sizes)):
        assert (keep[s, num[s]:] == -1).all()
        got.append(keep[s, :num[s]].tolist())
    return got


@pytest.mark.parametrize("thresh", THRESHOLDS)
@pytest.mark.parametrize("kind", KINDS)
def test_exact_keep_lists(pool, pool_iou, dev, kind, thresh):
    boxes, scores = _columns(kind, pool[0]), pool[1]
    for sizes in [[n] for n in SIZES] + list(LAYOUTS):
        want = _expected(kind, boxes, scores, sizes, thresh, iou=pool_iou)
        got = _run(kind, boxes, scores, sizes, thresh, dev)
        assert got == want, (kind, thresh, sizes)
    if thresh == 0.2:
        assert 1 < len(want[-1]) < 1000       # the case suppresses, and not everything


def test_single_list_functions_and_cuts(pool, dev):
    from msmdfusion_amd import iou3d
    boxes, scores = pool
    b, s = torch.from_numpy(boxes[:300]).to(dev), torch.from_numpy(scores[:300]).to(dev)
    order = R.stable_order(scores[:300])
    want = R.nms("rotate", boxes[:300], 0.2, order)
    assert iou3d.nms_gpu(b, s, 0.2).tolist() == want
    cut = R.nms("rotate", boxes[:300], 0.2, order[:100])
    assert iou3d.nms_gpu(b, s, 0.2, pre_maxsize=100).tolist() == cut
    assert iou3d.nms_gpu(b, s, 0.2, pre_maxsize=100, post_max_size=7).tolist() == cut[:7]
    assert iou3d.nms_gpu(b, s, 0.2, post_max_size=0).tolist() == []
    assert iou3d.nms_normal_gpu(b, s, 0.2).tolist() == R.nms("normal", boxes[:300], 0.2, order)
    dets = torch.cat([torch.from_numpy(_columns("circle", boxes[:300])).to(dev), s[:, None]], 1)
    got = iou3d.circle_nms(dets, 0.7)
    assert got.dtype == torch.long and got.is_cuda
    assert got.tolist() == R.circle_nms(dets.cpu().numpy(), 0.7)
    assert iou3d.circle_nms(dets, 0.7, post_max_size=5).tolist() == got.tolist()[:5]
    # batched cuts: pre_max / post_max apply to every list
    sizes = [65, 0, 129]
    assert _run("rotate", boxes, scores, sizes, 0.2, dev, pre_max=40, post_max=9) == \
        _expected("rotate", boxes, scores, sizes, 0.2, pre_max=40, post_max=9)
    iou = iou3d.boxes_iou_bev(b[:50], b[50:120]).cpu().numpy()
    assert np.abs(iou - R.iou_bev(boxes[:50], boxes[50:120])).max() < 1e-4


def _xyxyr(cx, cy, w, h, r=0.0):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, r]


def test_hand_cases(dev):
    from msmdfusion_amd import iou3d

    def rot(boxes, scores, thresh=0.3, kind="rotate"):
        f = iou3d.nms_gpu if kind == "rotate" else iou3d.nms_normal_gpu
        return f(torch.tensor(boxes, dtype=torch.float32, device=dev),
                 torch.tensor(scores, dtype=torch.float32, device=dev), thresh).tolist()

    for kind in ("rotate", "normal"):
        # a chain: A suppresses B (IoU 0.64), B would suppress C (0.64), A and C: 0.36 < 0.5
        chain = [_xyxyr(0, 0, 10, 10), _xyxyr(0, 0, 8, 8), _xyxyr(0, 0, 6, 6)]
        assert rot(chain, [0.9, 0.8, 0.7], 0.5, kind) == [0, 2]
        assert rot([_xyxyr(1, 2, 3, 4)] * 5, [0.1, 0.5, 0.3, 0.2, 0.4], 0.5, kind) == [1]
        # zero-area boxes: IoU 0 / 1e-8 = 0 with everything, themselves included
        zero = [_xyxyr(0, 0, 0, 4), _xyxyr(0, 0, 0, 4), _xyxyr(0, 0, 2, 4)]
        assert rot(zero, [0.3, 0.2, 0.1], 0.1, kind) == [0, 1, 2]
        # score ties: lower index first
        assert rot([_xyxyr(0, 0, 4, 4), _xyxyr(0.1, 0, 4, 4), _xyxyr(50, 0, 4, 4)], [0.5] * 3,
                   0.5, kind) == [0, 2]
        # NaN follows the comparisons as written.  Rotated (and circle, below): every test is
        # false -- the box is kept and suppresses nothing.  iou_normal as the reference wrote it
        # drops the NaN in fmaxf / fminf and divides by fmaxf(NaN, 1e-8) = 1e-8: the pair counts
        # as overlapping, which the restatement (np.fmax / np.fmin) reproduces.
        nan = float("nan")
        boxes = [_xyxyr(0, 0, 4, 4), [nan, -2, 2, 2, 0.0], _xyxyr(0, 0, 4, 4)]
        if kind == "rotate":
            assert rot(boxes, [0.2, 0.9, 0.8], 0.5, kind) == [1, 2]
        else:
            want = R.nms("normal", np.asarray(boxes, np.float32), 0.5, np.array([1, 2, 0]))
            assert rot(boxes, [0.2, 0.9, 0.8], 0.5, kind) == want == [1]
    # pairs across the 64 boundary in row and column: disjoint boxes on a unit grid (small
    # coordinates: the reference's inside-test margin of 1e-5 is below one float32 ulp past 128)
    # except 60 = 70 (one word apart) = 130 (two words apart) and 3 = 199
    n = 200
    boxes = np.array([_xyxyr(i % 16, i // 16, 0.5, 0.5, 0.3) for i in range(n)], np.float32)
    boxes[70] = boxes[60]
    boxes[130] = boxes[70]
    boxes[199] = boxes[3]
    scores = np.linspace(1, 0.1, n).astype(np.float32)
    want = [i for i in range(n) if i not in (70, 130, 199)]
    for kind in ("rotate", "normal"):
        assert rot(boxes.tolist(), scores.tolist(), 0.5, kind) == want
    dets = torch.tensor(np.concatenate([boxes[:, :2], scores[:, None]], 1), device=dev)
    assert iou3d.circle_nms(dets, 0.25, post_max_size=500).tolist() == want
    nan_dets = torch.tensor([[0, 0, 0.2], [float("nan"), 0, 0.9], [0, 0, 0.8]], device=dev)
    assert iou3d.circle_nms(nan_dets, 4.0).tolist() == [1, 2]


def test_circle_distance_equal_to_the_threshold_suppresses(dev):
    """`<=` and the float32 evaluation: 0.1f, 0.3f are not exact, so a fused multiply-add or a
    float64 evaluation gives another distance than numpy's float32 expression."""
    from msmdfusion_amd import iou3d
    rng = np.random.default_rng(3)
    xy = rng.uniform(-50, 50, (64, 2)).astype(np.float32)
    sc = np.linspace(1, 0, 64).astype(np.float32)
    for j, step in ((1, (0.1, 0.3)), (17, (-0.7, 0.2)), (40, (0.3, -0.9))):
        xy = xy.copy()
        xy[j] = xy[0] + np.asarray(step, np.float32)
        d = (xy[0, 0] - xy[j, 0]) ** 2 + (xy[0, 1] - xy[j, 1]) ** 2       # float32, :176
        assert d.dtype == np.float32
        dets = np.concatenate([xy, sc[:, None]], 1)
        for th, hit in ((d, True), (np.nextafter(d, np.float32(0)), False)):
            got = iou3d.circle_nms(torch.from_numpy(dets).to(dev), float(th), 64).tolist()
            assert got == R.circle_nms(dets, th, 64)
            assert (j not in got) == hit
    # 3-4-5: exact in float32
    dets = torch.tensor([[0, 0, 0.9], [3, 4, 0.8], [3, 4.000001, 0.7]], device=dev)
    assert iou3d.circle_nms(dets, 25.0).tolist() == [0, 2]


def test_shim_keeps_on_the_cpu(pool, dev):
    from msmdfusion_amd.integration import iou3d_cuda
    boxes, scores = pool
    order = R.stable_order(scores[:200])
    b = torch.from_numpy(boxes[:200][order]).to(dev)
    for fn, kind in ((iou3d_cuda.nms_gpu, "rotate"), (iou3d_cuda.nms_normal_gpu, "normal")):
        keep = torch.zeros(200, dtype=torch.long)
        num_out = fn(b, keep, 0.2, dev.index)
        want = R.nms(kind, boxes[:200][order], 0.2, np.arange(200))
        assert isinstance(num_out, int) and not keep.is_cuda
        assert keep[:num_out].tolist() == want
    out = torch.zeros((20, 30), device=dev)
    assert iou3d_cuda.boxes_iou_bev_gpu(b[:20], b[20:50], out) == 1
    assert np.abs(out.cpu().numpy() - R.iou_bev(boxes[:200][order][:20],
                                                boxes[:200][order][20:50])).max() < 1e-4
    ov = torch.zeros((20, 30), device=dev)
    iou3d_cuda.boxes_overlap_bev_gpu(b[:20], b[20:50], ov)
    assert (ov >= out).all()
    with pytest.raises(RuntimeError):
        fn(b, keep.to(dev), 0.2, dev.index)


def test_no_allocation_beyond_the_workspace_and_no_host_sync(pool, dev):
    from msmdfusion_amd import kernels as K
    segs, n = 24, 1000
    rng = np.random.default_rng(5)
    boxes = torch.from_numpy(np.concatenate([_draw(rng, n)] * segs)).to(dev)
    offsets = torch.arange(segs + 1, dtype=torch.int32, device=dev) * n
    th = torch.full((segs,), 0.2, device=dev)
    nbytes = K.nms_workspace_bytes(segs * n, n)
    assert nbytes == segs * n * 16 * 8
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    keep = torch.empty((segs, 83), dtype=torch.long, device=dev)
    num = torch.empty((segs,), dtype=torch.int32, device=dev)
    call = lambda: K.nms_segments("rotate", boxes, offsets, th, n, post_max=83, keep=keep,  # noqa
                                  num_keep=num, workspace=ws)
    call()                                              # warm: module load
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
    assert (num.cpu() == num.cpu()[0]).all() and 0 < int(num[0]) <= 83


@pytest.mark.parametrize("kind", ("rotate", "circle"))
def test_bitwise_reproducible(dev, kind):
    from msmdfusion_amd import iou3d
    segs, n = 24, 1000
    rng = np.random.default_rng(11)
    boxes = torch.from_numpy(_columns(kind, _draw(rng, segs * n))).to(dev)
    scores = torch.from_numpy(rng.random(segs * n).astype(np.float32)).to(dev)
    offsets = torch.arange(segs + 1, dtype=torch.int32, device=dev) * n
    runs = [iou3d.nms_batched(kind, boxes, scores, offsets, 0.2, 1000, 83) for _ in range(5)]
    for keep, num in runs[1:]:
        assert torch.equal(keep, runs[0][0]) and torch.equal(num, runs[0][1])
    assert int(runs[0][1].min()) > 0
