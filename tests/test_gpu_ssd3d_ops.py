"""3DSSD's two native pieces on the GPU: msmd_ssd3d_targets_f32 (the candidate targets of a
whole batch in one launch) against the reference's outputs and the per-sample loop of
tests/ssd3d_ref.py, and the 'mmcv' NMS kind against the written-out mmcv nms / batched_nms.

What is copied or decided by a comparison is compared exactly.  Centerness is a float32 chain
whose rounding differs from torch's einsum / pow: the kernel and the float32 restatement are
both measured against the float64 restatement, and the kernel's largest error over a case may
be at most 4 x the float32 restatement's on the same case plus one float32 ulp at 1.0 (the
project's standing margin for reordered float32 arithmetic; the floor covers a case where torch
happens to be exact)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ssd3d_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

ULP1 = float(np.spacing(np.float32(1.0)))
BINS, POS_THR, EXPAND = 12, 1.0, 0.05
YAWS = (0.0, math.pi / 2, -math.pi / 2, math.pi, 0.37, -2.2, 7.0, -9.5)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "ssd3d_head_vectors.npz")))


def _t(a, dev=None):
    t = torch.from_numpy(np.asarray(a))
    return t if dev is None else t.to(dev)


def run_kernel(boxes, labels, aggregated, seed_points, classes, dev, pos_thr=POS_THR):
    """boxes / labels: per-sample CPU tensors (at least one row each).  -> (the kernel's eleven
    outputs, its per-box table, box offsets): the tables are made on the device."""
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd.head_loss import LiDARBoxes
    from msmdfusion_amd.ssd3d_head import box_tables
    from msmdfusion_amd.vote_head import AnchorFreeBBoxCoder
    flat_labels = torch.cat(labels).to(dev)
    gt, vote, table, dir_class = box_tables(
        AnchorFreeBBoxCoder(BINS), LiDARBoxes(torch.cat(boxes).to(dev)), flat_labels, EXPAND)
    counts = [len(v) for v in labels]
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).to(dev)
    out = K.ssd3d_targets(aggregated.to(dev), seed_points.to(dev), gt, vote, flat_labels, offsets,
                          table, dir_class, classes, pos_thr)
    return out, table, dir_class, offsets


def centerness_errors(got, boxes, labels, aggregated, seeds, classes):
    """-> (kernel error, float32 restatement error) against the float64 restatement, the largest
    over the case; NaN must sit in the same places in all three."""
    worst_kernel = worst_f32 = 0.0
    for b in range(len(boxes)):
        args = (boxes[b], labels[b], aggregated[b], seeds[b, :aggregated.shape[1]], classes, BINS,
                POS_THR, EXPAND)
        c32 = S.targets_single(*args)[6]
        c64 = S.targets_single(*args, dtype=torch.float64)[6]
        mine = got[b].cpu()
        assert torch.equal(torch.isnan(mine), torch.isnan(c64)), b
        assert torch.equal(torch.isnan(c32), torch.isnan(c64)), b
        ok = ~torch.isnan(c64)
        if ok.any():
            worst_kernel = max(worst_kernel, float((mine.double() - c64)[ok].abs().max()))
            worst_f32 = max(worst_f32, float((c32.double() - c64)[ok].abs().max()))
    return worst_kernel, worst_f32


# ------------------------------------------------------------------------------ the golden
def test_targets_kernel_against_the_golden(dev, gold):
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd.head_loss import LiDARBoxes
    from msmdfusion_amd.ssd3d_head import box_tables
    from msmdfusion_amd.vote_head import AnchorFreeBBoxCoder
    boxes = [torch.zeros(1, 7), _t(gold["gt_boxes_1"]), _t(gold["gt_boxes_2"])]     # the fake box
    labels = [torch.zeros(1, dtype=torch.long), _t(gold["gt_labels_1"]), _t(gold["gt_labels_2"])]
    agg, seeds = _t(gold["aggregated_points"]), _t(gold["seed_points"])
    # the per-box tables on the host, as the head makes them for ground truths a loader left
    # there: the reference's CPU values bit for bit
    flat_labels = torch.cat(labels)
    tables = box_tables(AnchorFreeBBoxCoder(BINS), LiDARBoxes(torch.cat(boxes)), flat_labels, EXPAND)
    gt, vote, table, dir_class = [t.to(dev) for t in tables]
    offsets = torch.tensor([0, 1, 7, 11], dtype=torch.int32).to(dev)
    got = K.ssd3d_targets(agg.to(dev), seeds.to(dev), gt, vote, flat_labels.to(dev), offsets,
                          table, dir_class, 3, POS_THR)
    got = dict(zip(S.TARGET_NAMES, got))
    want = {k: _t(gold["targets_" + k]) for k in S.TARGET_NAMES}
    want["center_targets"] = want["center_targets"] + agg          # the kernel's are absolute
    want["vote_mask"] = want["vote_mask"] > 0
    for k in S.TARGET_NAMES:
        assert got[k].dtype == (torch.bool if "mask" in k and k != "mask_targets"
                                else want[k].dtype), k
    for k in ("vote_targets", "size_res_targets", "dir_class_targets", "dir_res_targets",
              "mask_targets", "corner3d_targets", "vote_mask", "positive_mask", "negative_mask"):
        assert torch.equal(got[k].cpu(), want[k]), k
    # (the golden's relative centre + the point is not the stored centre bit for bit; the stored
    # one is the table's)
    rel = got["center_targets"].cpu() - agg
    assert torch.equal(rel, _t(gold["targets_center_targets"]))
    kernel_err, f32_err = centerness_errors(got["centerness_targets"], boxes, labels, agg, seeds, 3)
    ref_err = float((_t(gold["targets_centerness_targets"]).double() - torch.stack(
        [S.targets_single(boxes[b], labels[b], agg[b], seeds[b, :64], 3, BINS, POS_THR, EXPAND,
                          dtype=torch.float64)[6] for b in range(3)])).abs().max())
    print("centerness error vs float64: kernel %.3g, float32 restatement %.3g, golden %.3g"
          % (kernel_err, f32_err, ref_err))
    assert kernel_err <= 4 * ref_err + ULP1, (kernel_err, ref_err)


# ------------------------------------------------------------------- the kernel's boundaries
def make_case(seed, counts, n, classes):
    """-> boxes, labels (per-sample CPU tensors), aggregated [B, n, 3], seeds [B, n + 5, 3].
    Box rows on a 1/16 grid (so face points are exact), yaws from YAWS; in a sample of three or
    more boxes rows 1 and 2 share row 0's centre, height and yaw (a point in three boxes) and
    labels -1 sit at the first, a middle and the last row in turn; a sample of zero boxes gets
    the fake box."""
    rs = np.random.RandomState(seed)
    boxes, labels = [], []
    agg = np.empty((len(counts), n, 3), np.float32)
    for b, t in enumerate(counts):
        if t == 0:
            bx, lb = np.zeros((1, 7), np.float32), np.zeros((1,), np.int64)
        else:
            bx = np.empty((t, 7), np.float32)
            bx[:, :2] = np.round(rs.uniform(0, 40, (t, 2)) * 16) / 16
            bx[:, 2] = np.round(rs.uniform(-2, 0, t) * 16) / 16
            bx[:, 3:6] = np.round(rs.uniform(0.5, 4.5, (t, 3)) * 16) / 16
            bx[:, 6] = np.asarray(YAWS, np.float32)[(np.arange(t) + b) % len(YAWS)]
            lb = rs.randint(0, classes, t).astype(np.int64)
            if t >= 3:
                bx[1, :3], bx[2, :3] = bx[0, :3], bx[0, :3]
                bx[1, 5:], bx[2, 5:] = bx[0, 5:], bx[0, 5:]       # same height and yaw
                lb[[0, t // 2, t - 1][(b + seed) % 3]] = -1
                if t > 3 and b % 2:
                    lb[t - 1] = -1
                    lb[t - 2] = -1                        # the fallback must skip two rows
        boxes.append(torch.from_numpy(bx))
        labels.append(torch.from_numpy(lb))
        # candidates: about half inside some box (centre + a fraction of the half sizes along
        # the box axes), the rest anywhere
        pick = bx[rs.randint(0, len(bx), n)]
        frac = rs.uniform(-0.9, 0.9, (n, 3)).astype(np.float32)
        c, s = np.cos(pick[:, 6] + np.pi / 2), np.sin(pick[:, 6] + np.pi / 2)
        lx, ly = frac[:, 0] * pick[:, 4] / 2, frac[:, 1] * pick[:, 3] / 2
        inside = np.stack([pick[:, 0] + lx * c - ly * s, pick[:, 1] + lx * s + ly * c,
                           pick[:, 2] + pick[:, 5] * (0.5 + 0.45 * frac[:, 2])], 1)
        anywhere = np.concatenate([rs.uniform(-3, 43, (n, 2)), rs.uniform(-3, 4, (n, 1))], 1)
        agg[b] = np.where((rs.uniform(size=n) < 0.5)[:, None], inside, anywhere)
        if n >= 4:
            agg[b, 0] = bx[0, :3] + [0, 0, bx[0, 5] / 2]          # the shared centre
            agg[b, 1] = bx[0, :3] + [0, 0, bx[0, 5]]              # exactly on the top face: inside
            agg[b, 2] = bx[0, :3]                                 # exactly on the bottom face
            agg[b, 3] = bx[0, :3] + [0, 0, bx[0, 5] + 1.0 / 16]   # one grid step above: outside
    agg_t = torch.from_numpy(agg)
    seeds = torch.cat([agg_t + torch.from_numpy(rs.normal(0, 0.2, agg.shape).astype(np.float32)),
                       torch.from_numpy(rs.uniform(0, 40, (len(counts), 5, 3)).astype(np.float32))], 1)
    if n >= 4:
        seeds[:, :4] = agg_t[:, :4]
        seeds[:, 3, 2] = agg_t[:, 2, 2] - 0.08                    # below box 0, in its vote box
    return boxes, labels, agg_t, seeds


CHUNK = 64
# off the 1/16 grid of the boxes: the shared-centre candidate lies at half a height from the
# top centre, which a threshold on the grid would meet exactly
SWEEP_THR = 1.03
CASES = [
    # (counts per sample, candidates, classes)
    ((0,), 1, 1), ((1,), 63, 3), ((CHUNK - 1, 0), 64, 3), ((CHUNK, 1, CHUNK + 1), 65, 1),
    ((2 * CHUNK + 3, 0, CHUNK, 3), 256, 3), ((CHUNK + 1, 2 * CHUNK + 3), 257, 3),
    ((3, CHUNK - 1, 1, 0), 64, 1),
]


@pytest.mark.parametrize("counts,n,classes", CASES)
def test_targets_kernel_against_the_loop(dev, counts, n, classes):
    from msmdfusion_amd import kernels as K
    assert K.SSD3D_GT_CHUNK == CHUNK
    boxes, labels, agg, seeds = make_case(len(counts) * 1000 + n + 7, counts, n, classes)
    # no candidate sits within 1e-4 (relative) of the positive distance in float64, so the
    # positive mask is compared exactly with nothing left out
    margin = min(S.distance_margin(boxes[b], labels[b], agg[b], SWEEP_THR) for b in range(len(counts)))
    assert margin > 1e-4, margin
    got, table, dir_class, offsets = run_kernel(boxes, labels, agg, seeds, classes, dev, pos_thr=SWEEP_THR)
    got = dict(zip(S.TARGET_NAMES, got))
    table, dir_class = table.cpu(), dir_class.cpu()
    seen = dict(inside=0, fallback=0, triple=0, empty=0, voted_only=0)
    for b in range(len(counts)):
        want = dict(zip(S.TARGET_NAMES, S.targets_single(
            boxes[b], labels[b], agg[b], seeds[b, :n], classes, BINS, SWEEP_THR, EXPAND)))
        mine = {k: v[b].cpu() for k, v in got.items()}
        for k in ("dir_class_targets", "mask_targets", "vote_mask", "positive_mask",
                  "negative_mask"):
            assert torch.equal(mine[k], want[k]), (b, k)
        valid = torch.nonzero(labels[b] != -1).flatten()
        if len(valid) == 0:
            seen["empty"] += 1
            for k in S.TARGET_NAMES:
                assert torch.equal(mine[k], want[k]), (b, k)            # zeros, negative = 1
            continue
        # floats copied from a box: the kernel's own table at the row the loop assigns
        base = int(offsets[b])
        inside, assignment = S.assign_by_points_inside(boxes[b][valid], agg[b])
        rows = table[base + valid[assignment]]
        assert torch.equal(mine["center_targets"], rows[:, 0:3]), b
        assert torch.equal(mine["size_res_targets"], rows[:, 3:6]), b
        assert torch.equal(mine["dir_res_targets"], rows[:, 6]), b
        assert torch.equal(mine["corner3d_targets"].reshape(n, 24), rows[:, 9:33]), b
        assert torch.equal(mine["dir_class_targets"], dir_class[base + valid[assignment]]), b
        vote32 = S.enlarged(boxes[b][valid], EXPAND)
        vote32[:, 2] -= EXPAND
        voted, vote_assignment = S.assign_by_points_inside(vote32, seeds[b, :n])
        assert torch.equal(mine["vote_targets"],
                           table[base + valid[vote_assignment], 0:3] - seeds[b, :n]), b
        # ... and those table rows are the loop's values up to the device's sin / cos / einsum
        for k, tol in (("center_targets", 0.0), ("size_res_targets", 0.0), ("vote_targets", 0.0),
                       ("dir_res_targets", 0.0), ("corner3d_targets", 1e-5)):
            # (corners: coordinates below 64, so one float32 ulp is 3.8e-6, plus a half size of
            # at most 2.25 times one ulp of a sine: under 1e-5)
            assert float((mine[k] - want[k]).abs().max()) <= tol, (b, k)
        seen["inside"] += int(inside.sum())
        seen["fallback"] += int((~inside).sum())
        seen["voted_only"] += int((voted & ~inside).sum())
        if n >= 4 and len(labels[b]) >= 3:
            hits = S.RR.points_in_boxes_all(agg[b, :1].numpy()[None], boxes[b].numpy()[None])[0, 0]
            assert hits[:3].tolist() == [1, 1, 1]
            seen["triple"] += 1
            first_valid = int(valid[0])
            assert int(mine["mask_targets"][0]) == int(labels[b][first_valid])
            assert not bool(mine["negative_mask"][1]) and not bool(mine["negative_mask"][2])
    kernel_err, f32_err = centerness_errors(got["centerness_targets"], boxes, labels, agg, seeds,
                                            classes)
    print("counts %s n %d: centerness error vs float64: kernel %.3g, float32 restatement %.3g; %s"
          % (counts, n, kernel_err, f32_err, seen))
    assert kernel_err <= 4 * f32_err + ULP1, (kernel_err, f32_err)
    if max(counts) >= 3 and n >= 63:
        assert seen["inside"] and seen["fallback"]


def test_nan_follows_the_expressions(dev):
    """The fake box (all zeros) with a candidate on its centre planes: 0 / 0 in the ratios, and
    the one-hot product spreads the NaN over every class column (NaN * 0)."""
    boxes, labels = [torch.zeros(1, 7)], [torch.zeros(1, dtype=torch.long)]
    agg = torch.tensor([[[0.0, 1.0, 0.5], [1.0, 2.0, 0.0], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0]]])
    got, _, _, _ = run_kernel(boxes, labels, agg, agg.clone(), 3, dev)
    got = dict(zip(S.TARGET_NAMES, got))
    want = S.targets_single(boxes[0], labels[0], agg[0], agg[0], 3, BINS, POS_THR, EXPAND)[6]
    mine = got["centerness_targets"][0].cpu()
    assert torch.isnan(want[0]).all() and torch.isnan(want[1]).all() and torch.isnan(want[3]).all()
    assert torch.equal(torch.isnan(mine), torch.isnan(want))
    assert torch.equal(mine[2], want[2]) and not torch.isnan(mine[2]).any()
    assert got["negative_mask"].all() and not got["positive_mask"].any()


def test_seed_rows_are_read_through_a_sample_stride(dev):
    """The head hands over seed_points [B, num_seed, 3] and only the first N of a sample are
    candidates' seeds: a view is taken as it is, a strided one is copied."""
    boxes, labels, agg, seeds = make_case(5, (5, 7), 64, 3)
    wide = torch.cat([seeds, torch.full((2, 40, 3), 1e6)], 1)
    a, _, _, _ = run_kernel(boxes, labels, agg, seeds[:, :64].contiguous(), 3, dev)
    b, _, _, _ = run_kernel(boxes, labels, agg, wide, 3, dev)
    strided = wide.transpose(1, 2).contiguous().transpose(1, 2)      # coordinates not adjacent
    assert not strided.is_contiguous()
    c, _, _, _ = run_kernel(boxes, labels, agg, strided, 3, dev)
    for name, x, y, z in zip(S.TARGET_NAMES, a, b, c):
        want = x.cpu().numpy().tobytes()
        assert y.cpu().numpy().tobytes() == want and z.cpu().numpy().tobytes() == want, name


def test_targets_are_bitwise_reproducible(dev):
    boxes, labels, agg, seeds = make_case(11, (131, 40, 131, 7), 256, 3)
    first, _, _, _ = run_kernel(boxes, labels, agg, seeds, 3, dev)
    again, _, _, _ = run_kernel(boxes, labels, agg, seeds, 3, dev)
    for name, x, y in zip(S.TARGET_NAMES, first, again):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), name


# -------------------------------------------------------------------------------- the NMS
def nms_case(seed, sizes, classes, nan=False):
    """Segments of the given sizes: clustered boxes with distinct scores, one zero-area box, a
    duplicate and, when asked, one NaN coordinate.  -> boxes [total, 4], scores, class ids,
    offsets."""
    rs = np.random.RandomState(seed)
    total = sum(sizes)
    centre = rs.uniform(0, 12, (total, 2))
    half = rs.uniform(0.4, 1.6, (total, 2))
    boxes = np.concatenate([centre - half, centre + half], 1).astype(np.float32)
    scores = rs.permutation(total).astype(np.float32) / total        # distinct
    idxs = rs.randint(0, classes, total)
    if total >= 8:
        boxes[3, 2] = boxes[3, 0]                                    # zero area
        boxes[5] = boxes[4]                                          # a duplicate
        idxs[5] = idxs[4]
        if nan:
            boxes[6, 1] = np.nan
    return boxes, scores, idxs, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


@pytest.mark.parametrize("sizes,classes", [((1,), 1), ((64,), 3), ((65,), 1), ((256,), 3),
                                           ((1, 64, 65, 256), 3), ((65, 64), 1)])
@pytest.mark.parametrize("post_max", [None, 8])
def test_mmcv_nms_kind_against_the_written_out_batched_nms(dev, sizes, classes, post_max):
    from msmdfusion_amd import iou3d
    boxes, scores, idxs, offsets = nms_case(sum(sizes) + classes, sizes, classes)
    thr = 0.1
    shifted = np.concatenate([S.class_shift(boxes[a:b], idxs[a:b])
                              for a, b in zip(offsets[:-1], offsets[1:])])
    keep, num = iou3d.nms_batched("mmcv", _t(shifted, dev), _t(scores, dev), _t(offsets, dev), thr,
                                  post_max=post_max)
    keep, num = keep.cpu().numpy(), num.cpu().numpy()
    for s, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        want = S.mmcv_batched_nms(boxes[a:b], scores[a:b], idxs[a:b], thr) + a
        assert np.array_equal(want, S.mmcv_nms(shifted[a:b], scores[a:b], thr) + a)
        if post_max is not None:
            want = want[:post_max]                                   # the max_output_num cut
        assert num[s] == len(want), (s, num[s], len(want))
        assert keep[s, :num[s]].tolist() == want.tolist(), s
        assert (keep[s, num[s]:] == -1).all()
        if b - a >= 64 and post_max is None:
            assert len(want) < b - a                                 # something was suppressed


def test_mmcv_nms_kind_with_a_nan_coordinate(dev):
    """Rows as given (one class): fmaxf / fminf drop the NaN, its area is NaN and every
    comparison with it false -- the row neither suppresses nor is suppressed.  Through
    batched_nms's class shift the NaN is the maximum (torch.max), so EVERY row becomes NaN and
    nothing is suppressed at all."""
    from msmdfusion_amd import iou3d
    boxes, scores, idxs, offsets = nms_case(77, (70,), 3, nan=True)
    want = S.mmcv_nms(boxes, scores, 0.1)
    assert 6 in want.tolist() and len(want) < 70
    keep, num = iou3d.nms_batched("mmcv", _t(boxes, dev), _t(scores, dev), _t(offsets, dev), 0.1)
    assert keep[0, :int(num[0])].tolist() == want.tolist()
    shifted = S.class_shift(boxes, idxs)
    assert np.isnan(shifted).all()
    want = S.mmcv_batched_nms(boxes, scores, idxs, 0.1)
    assert len(want) == 70
    keep, num = iou3d.nms_batched("mmcv", _t(shifted, dev), _t(scores, dev), _t(offsets, dev), 0.1)
    assert int(num[0]) == 70 and keep[0].tolist() == want.tolist()


def test_mmcv_kind_differs_from_the_normal_kind_on_degenerate_boxes(dev):
    """Two identical zero-area boxes at threshold 0: mmcv's 0 > 0 * 0 keeps both, iou_normal's
    0 / max(0, 1e-8) > 0 would too -- but two zero-area boxes inside a real one: inter 0 there as
    well.  The forms part where the union underflows the floor: tiny boxes."""
    from msmdfusion_amd import iou3d
    tiny = np.asarray([[0, 0, 1e-5, 1e-5], [0, 0, 1e-5, 1e-5]], np.float32)   # area 1e-10 < 1e-8
    scores = np.asarray([0.9, 0.8], np.float32)
    offsets = _t(np.asarray([0, 2], np.int32), dev)
    assert S.mmcv_nms(tiny, scores, 0.5).tolist() == [0]
    keep, num = iou3d.nms_batched("mmcv", _t(tiny, dev), _t(scores, dev), offsets, 0.5)
    assert int(num[0]) == 1 and keep[0, :1].tolist() == [0]
    keep, num = iou3d.nms_batched("normal", _t(tiny, dev), _t(scores, dev), offsets, 0.5)
    assert int(num[0]) == 2                                           # 1e-10 / 1e-8 = 0.01 <= 0.5


def test_mmcv_nms_call_allocates_nothing_and_does_not_wait(dev):
    from msmdfusion_amd import kernels as K
    boxes, scores, idxs, offsets = nms_case(9, (65, 64), 3)
    order = np.concatenate([np.argsort(-scores[a:b], kind="stable") + a
                            for a, b in zip(offsets[:-1], offsets[1:])])
    rows = _t(S.class_shift(boxes, idxs)[order], dev).contiguous()
    off, thr = _t(offsets, dev), torch.full((2,), 0.1, device=dev)
    keep = torch.empty((2, 65), dtype=torch.long, device=dev)
    num = torch.empty((2,), dtype=torch.int32, device=dev)
    ws = torch.empty(K.nms_workspace_bytes(129, 65), dtype=torch.uint8, device=dev)
    K.nms_segments("mmcv", rows, off, thr, 65, keep=keep, num_keep=num, workspace=ws)   # warm
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        K.nms_segments("mmcv", rows, off, thr, 65, keep=keep, num_keep=num, workspace=ws)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before
    assert int(num.sum()) > 0
