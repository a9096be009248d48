"""msmd_semantic_targets_f32 (csrc/parta2.hip) against the composition path -- the reference's
per-sample, per-box loop restated on LiDARBoxes.points_in_boxes
(PointwiseSemanticHead.get_targets_single) -- on every scheduling edge, on constructed
situations, against the golden vectors, for reproducibility, host waits and memory.

Discrete results (seg targets and the masks derived from them) are compared with torch.equal.
The part targets are float32 arithmetic whose rotation the composition takes through an einsum:
the kernel has to be within 4 x the composition's own error against the float64 restatement
(tests/parta2_cases.targets_ref) measured in the same test, floored at one float32 ulp at 1.0.
Every random case keeps its centres MARGIN away from every face (parta2_cases.make_case asserts
it), so the discrete results do not hang on a rounding.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parta2_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = float(np.finfo(np.float32).eps)
CLASSES = 3


def _head(fused=True, classes=CLASSES):
    from msmdfusion_amd.semantic_head import PointwiseSemanticHead
    return PointwiseSemanticHead(in_channels=4, num_classes=classes, fused=fused)


def _lists(case, dev):
    from msmdfusion_amd.head_loss import LiDARBoxes
    boxes = [LiDARBoxes(torch.from_numpy(np.asarray(b, np.float32)).reshape(-1, 7).to(dev))
             for b in case["boxes"]]
    labels = [torch.from_numpy(np.asarray(l, np.int64)).to(dev) for l in case["labels"]]
    return boxes, labels


def _voxels(case, dev):
    n = case["centres"].shape[0]
    coors = np.zeros((n, 4), np.int32)
    coors[:, 0] = case["ids"]
    return dict(coors=torch.from_numpy(coors).to(dev),
                voxel_centers=torch.from_numpy(case["centres"]).to(dev))


def fused(case, dev, classes=CLASSES):
    boxes, labels = _lists(case, dev)
    out = _head(True, classes).get_targets(_voxels(case, dev), boxes, labels)
    return out["seg_targets"], out["part_targets"]


def composed(case, dev, classes=CLASSES):
    """The composition path per sample, scattered back to input row order; a row whose id is
    outside [0, B) gets the documented seg = -1, part = 0."""
    head = _head(False, classes)
    boxes, labels = _lists(case, dev)
    n = case["centres"].shape[0]
    seg = torch.full((n,), -1, dtype=torch.long, device=dev)
    part = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    centres = torch.from_numpy(case["centres"]).to(dev)
    for b in range(len(boxes)):
        rows = torch.from_numpy(np.nonzero(case["ids"] == b)[0]).to(dev)
        s, p = head.get_targets_single(centres[rows], boxes[b], labels[b])
        seg[rows], part[rows] = s, p
    return seg, part


def check(case, dev, classes=CLASSES):
    seg, part = fused(case, dev, classes)
    seg_c, part_c = composed(case, dev, classes)
    n = case["centres"].shape[0]
    assert seg.dtype == torch.long and tuple(seg.shape) == (n,)
    assert part.dtype == torch.float32 and tuple(part.shape) == (n, 3)
    assert torch.equal(seg, seg_c)
    for mask in (lambda s: (s > -1) & (s < classes), lambda s: s == -1, lambda s: s == classes):
        assert torch.equal(mask(seg), mask(seg_c))
    seg_r, part_r = PC.batch_targets_ref(case["centres"], case["ids"], case["boxes"],
                                         case["labels"], classes)
    assert np.array_equal(seg.cpu().numpy(), seg_r)
    finite = np.isfinite(part_r).all(1)
    err_c = np.abs(part_c.cpu().numpy().astype(np.float64) - part_r)[finite].max(initial=0.0)
    err_k = np.abs(part.cpu().numpy().astype(np.float64) - part_r)[finite].max(initial=0.0)
    print("part error: kernel %.3e, composition %.3e" % (err_k, err_c))
    assert err_k <= 4.0 * err_c + EPS, (err_k, err_c)
    bg = torch.from_numpy(~((seg_r > -1) & (seg_r < classes)) & (seg_r != -1)).to(dev)
    assert bool((part[bg] == 0).all())
    return seg, part


def _split(n, batch):
    """Rows per sample: uneven, so that sample boundaries fall inside a wave and a workgroup."""
    if batch == 1:
        return (n,)
    if batch == 2:
        return (n * 3 // 8, n - n * 3 // 8)
    a, b = n * 3 // 8, n // 5
    return (a, b, n - a - b)


def shape_cases():
    from msmdfusion_amd import kernels as K
    c = K.SEMANTIC_GT_CHUNK
    return [(1, (1,)), (63, (0,)), (64, (c - 1,)), (65, (c,)), (255, (c + 1, 0, 3)),
            (256, (2 * c + 3, 1)), (257, (c, 0, c + 1)), (1025, (2 * c + 3, 0, c - 1)),
            (1025, (0, 0)), (257, (1, 2 * c + 3, c))]


@pytest.mark.parametrize("index", range(10))
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_kernel_against_the_composition_on_every_edge(dev, index, order):
    n, counts = shape_cases()[index]
    case = PC.make_case(100 + index, counts, _split(n, len(counts)), CLASSES, order)
    if len(counts) == 3:
        assert counts[1] == 0 or index == 9                      # the empty middle sample
    seg, _ = check(case, dev)
    if max(counts) > 1 and n >= 255:
        s = seg.cpu().numpy()
        assert (s == -1).any() and (s == CLASSES).any() and ((s >= 0) & (s < CLASSES)).any()


def test_the_first_box_may_lie_in_the_second_chunk(dev):
    from msmdfusion_amd import kernels as K
    c = K.SEMANTIC_GT_CHUNK
    case = PC.make_case(7, (c + 9,), (600,), CLASSES)
    _, _, box_idx, _ = PC.targets_ref(case["centres"], case["boxes"][0], case["labels"][0], CLASSES)
    assert (box_idx >= c).any() and ((box_idx >= 0) & (box_idx < c)).any()
    check(case, dev)


def test_an_out_of_range_batch_id(dev):
    case = PC.make_case(8, (5, 4), (150, 170), CLASSES, "shuffled")
    case["ids"] = case["ids"].copy()
    case["ids"][[3, 100, 319]] = [2, -1, 77]
    seg, part = check(case, dev)
    assert seg[[3, 100, 319]].tolist() == [-1, -1, -1]
    assert float(part[[3, 100, 319]].abs().max()) == 0.0


def constructed():
    """One sample of boxes built for their situations.  -> (boxes, labels, points, expectation)"""
    e = PC.EXTRA_WIDTH
    half_pi = math.pi / 2
    boxes = [[0.0, 0.0, 0.0, 2.0, 4.0, 2.0, 0.3],          # 0  A
             [0.5, 0.0, 0.0, 2.0, 4.0, 2.0, 0.3],          # 1  overlaps A
             [20.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0],         # 2  x 19 .. 21
             [22.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0],         # 3  x 21 .. 23, touches 2
             [40.0, 0.0, 0.0, 1.6, 3.9, 1.5, half_pi],     # 4
             [50.0, 0.0, 0.0, 1.6, 3.9, 1.5, -half_pi],    # 5
             [60.0, 0.0, 0.0, 1.6, 3.9, 1.5, math.pi],     # 6
             [70.0, 0.0, 0.0, 1.6, 3.9, 1.5, 7.0],         # 7
             [80.0, 0.0, 0.0, 1.6, 3.9, 1.5, -7.0],        # 8
             [90.0, 0.0, 0.0, 1.6, 3.9, 1.5, 0.0],         # 9
             [100.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.4]]        # 10 label -1
    labels = [1, 2, 0, 2, 0, 1, 2, 0, 1, 2, -1]
    points = [[0.2, 0.0, 1.0],             # 0 in boxes 0 and 1: the first wins
              [18.9, 0.0, 1.0],            # 1 only in box 2's margin: -1
              [21.1, 0.0, 1.0],            # 2 in box 3 and in box 2's margin: box 3's label
              [20.0, 0.0, -e / 2],         # 3 below box 2's bottom within extra_width: -1
              [20.0, 0.0, 2.0 + 2 * e],    # 4 above the top by more than extra_width: background
              [40.3, 0.2, 0.4], [50.3, 0.2, 0.4], [60.3, 0.2, 0.4], [70.3, 0.2, 0.4],
              [80.3, 0.2, 0.4], [90.3, 0.2, 0.4],        # 5 .. 10 the yaws
              [100.1, 0.1, 0.5],           # 11 in the box labelled -1
              [200.0, 50.0, 0.7]]          # 12 far from everything
    seg = [1, -1, 2, -1, CLASSES, 0, 1, 2, 0, 1, 2, -1, CLASSES]
    first = [0, -1, 3, -1, -1, 4, 5, 6, 7, 8, 9, 10, -1]
    return (np.asarray(boxes, np.float32), np.asarray(labels, np.int64),
            np.asarray(points, np.float32), np.asarray(seg, np.int64), np.asarray(first))


def test_constructed_situations(dev):
    boxes, labels, points, want_seg, want_first = constructed()
    case = dict(centres=points, ids=np.zeros(len(points), np.int32), boxes=[boxes],
                labels=[labels])
    PC.assert_margins(points, case["ids"], [boxes])
    _, part_r, first, _ = PC.targets_ref(points, boxes, labels, CLASSES)
    assert np.array_equal(first, want_first)                     # the construction holds
    seg, part = check(case, dev)
    assert seg.tolist() == want_seg.tolist()
    part = part.cpu().numpy()
    # the first of two overlapping boxes gives the part target: box 0's frame, not box 1's
    other = PC.targets_ref(points[:1], boxes[1:2], labels[1:2], CLASSES)[1]
    assert np.abs(part[0] - part_r[0]).max() < 1e-6 < np.abs(part[0] - other[0]).max()
    assert (part[[1, 3, 4, 12]] == 0).all() and (part[11] > 0).all()
    assert (part[5:11] > 0).all() and (part[5:11] < 1).all()


def test_nan_centre_and_nan_box_stay_isolated(dev):
    boxes, labels, points, want_seg, _ = constructed()
    ids = np.zeros(len(points) + 1, np.int32)
    with_nan = np.concatenate([points[:6], [[np.nan, 0.0, 1.0]], points[6:]]).astype(np.float32)
    case = dict(centres=with_nan, ids=ids, boxes=[boxes], labels=[labels])
    seg, part = fused(case, dev)
    base_seg, base_part = fused(dict(centres=points, ids=ids[:-1], boxes=[boxes],
                                     labels=[labels]), dev)
    keep = [i for i in range(len(with_nan)) if i != 6]
    assert int(seg[6]) == CLASSES and float(part[6].abs().max()) == 0.0       # background
    assert torch.equal(seg[keep], base_seg) and torch.equal(part[keep], base_part)
    seg_c, part_c = composed(case, dev)
    assert torch.equal(seg, seg_c)
    # a NaN box (second in the table) holds nothing and disturbs no other box
    nan_boxes = np.concatenate([boxes[:1], np.full((1, 7), np.nan, np.float32), boxes[1:]])
    nan_labels = np.concatenate([labels[:1], [0], labels[1:]])
    seg2, part2 = fused(dict(centres=points, ids=ids[:-1], boxes=[nan_boxes],
                             labels=[nan_labels]), dev)
    assert torch.equal(seg2, base_seg) and torch.equal(part2, base_part)
    for k in (3, 4, 5, 6):                                       # NaN in one field at a time
        one = boxes.copy()
        one[2, k] = np.nan
        seg3, _ = fused(dict(centres=points, ids=ids[:-1], boxes=[one], labels=[labels]), dev)
        seg3_c, _ = composed(dict(centres=points, ids=ids[:-1], boxes=[one], labels=[labels]), dev)
        assert torch.equal(seg3, seg3_c)


def test_int32_labels_and_class_counts(dev):
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd.semantic_head import pad_ground_truths
    from msmdfusion_amd.head_loss import LiDARBoxes
    case = PC.make_case(21, (6, 3), (120, 90), 5)
    boxes, labels = _lists(case, dev)
    table, lab, counts = pad_ground_truths(boxes, labels, dev)
    big = LiDARBoxes(table.view(-1, 7)).enlarged_box(PC.EXTRA_WIDTH).tensor.view(table.shape)
    v = _voxels(case, dev)
    args = (v["voxel_centers"], v["coors"][:, 0].contiguous(), table, big.contiguous())
    s64, p64 = K.semantic_targets(*args, lab, counts, 5)
    s32, p32 = K.semantic_targets(*args, lab.int(), counts, 5)
    assert torch.equal(s64, s32) and torch.equal(p64, p32)
    seg_r, _ = PC.batch_targets_ref(case["centres"], case["ids"], case["boxes"], case["labels"], 5)
    assert np.array_equal(s64.cpu().numpy(), seg_r)
    # counts beyond the table are clipped to it; negative counts mean no box
    s_clip, _ = K.semantic_targets(*args, lab, counts + 1000, 5)
    full = [np.concatenate([b, np.zeros((6 - len(b), 7), np.float32)]) for b in case["boxes"]]
    full_l = [np.concatenate([l, np.zeros(6 - len(l), np.int64)]) for l in case["labels"]]
    assert np.array_equal(s_clip.cpu().numpy(), PC.batch_targets_ref(
        case["centres"], case["ids"], full, full_l, 5)[0])
    s_none, p_none = K.semantic_targets(*args, lab, counts * 0 - 3, 5)
    assert bool((s_none == 5).all()) and float(p_none.abs().max()) == 0.0
    with pytest.raises(RuntimeError):
        K.semantic_targets(*args, lab, counts, 0)


def test_kernel_against_the_golden(dev):
    gold = dict(np.load(os.path.join(GOLDEN, "parta2_first_stage_vectors.npz")))
    for tag, batch in (("b2", 2), ("b1", 1), ("empty", 2), ("nopos", 2)):
        p = "sem_%s_" % tag
        case = dict(centres=gold[p + "centres"], ids=gold[p + "ids"],
                    boxes=[gold[p + "boxes_%d" % b] for b in range(batch)],
                    labels=[gold[p + "labels_%d" % b] for b in range(batch)])
        seg, part = fused(case, dev)
        assert np.array_equal(seg.cpu().numpy(), gold[p + "seg_targets"]), tag
        ref64 = np.concatenate([gold[p + "single64_part_%d" % b] for b in range(batch)])
        err_ref = np.abs(gold[p + "part_targets"].astype(np.float64) - ref64).max()
        err = np.abs(part.cpu().numpy().astype(np.float64) - ref64).max()
        print(tag, "part error: kernel %.3e, reference float32 %.3e" % (err, err_ref))
        assert err <= 4.0 * err_ref + EPS, (tag, err, err_ref)


def _config_shape(dev, rows=16000, boxes=30):
    rng = np.random.default_rng(5)
    tables = [PC.make_boxes(rng, boxes, cell=3.0 * b) for b in range(2)]
    centres = np.concatenate([PC.draw_centres(rng, rows, t) for t in tables])
    ids = np.repeat(np.arange(2, dtype=np.int32), rows)
    return dict(centres=centres, ids=ids, boxes=tables,
                labels=[rng.integers(0, CLASSES, size=boxes).astype(np.int64) for _ in range(2)])


def test_targets_are_bitwise_reproducible(dev):
    case = _config_shape(dev)
    head = _head()
    boxes, labels = _lists(case, dev)
    v = _voxels(case, dev)
    a = head.get_targets(v, boxes, labels)
    b = head.get_targets(v, boxes, labels)
    assert torch.equal(a["seg_targets"], b["seg_targets"])
    assert torch.equal(a["part_targets"].view(torch.int32), b["part_targets"].view(torch.int32))
    s = a["seg_targets"]
    assert int(((s > -1) & (s < CLASSES)).sum()) > 1000 and int((s == -1).sum()) > 1000


def test_get_targets_does_not_wait_and_builds_no_row_by_box_tensor(dev):
    """Under torch's sync debug mode, and with the peak memory growth bounded by the outputs, the
    int32 id column and the padded box tables: an [N, G] tensor of even one byte per entry
    (1 MiB here) does not fit the bound."""
    from msmdfusion_amd import kernels as K
    rows, g = 8192, 64
    case = _config_shape(dev, rows=rows, boxes=g)
    head = _head()
    boxes, labels = _lists(case, dev)
    v = _voxels(case, dev)
    head.get_targets(v, boxes, labels)                              # warm: module load, caches
    torch.cuda.synchronize()
    n = 2 * rows
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = head.get_targets(v, boxes, labels)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated(dev) - before
    outputs = n * 8 + n * 12
    tables = 2 * g * 7 * 4
    bound = outputs + n * 4 + 8 * tables + 2 * g * 8 + 32 * 512    # 512 B allocator granules
    print("peak growth %d bytes, bound %d, [N, G] bytes %d" % (growth, bound, n * g))
    assert growth <= bound < n * g
    assert out["seg_targets"].numel() == n
    assert K.SEMANTIC_GT_CHUNK == 64
