"""Anchor3DHead on the device (msmdfusion_amd/anchor_head.py, csrc/anchor.hip): the matrix-free
assigner and the target kernel against a torch restatement of the reference's matrix-and-loop
algorithm (mmdet MaxIoUAssigner.assign_wrt_overlaps, train_mixins.py:101-314) on the same
device, the focal loss against float64 autograd, loss against a float64 restatement,
get_bboxes against a per-sample, per-class loop over the single-list NMS, and VoxelNet built
from the two KITTI configs."""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ULP = float(np.finfo(np.float32).eps)


@pytest.fixture(autouse=True)
def _leave_the_global_rng_alone(dev):
    with torch.random.fork_rng(devices=[dev]):
        yield


# ---------------------------------------------------------------- the restatement
def assign_restatement(anchor_bev, gt_bev, pos, neg, min_pos):
    """MaxIoUAssigner.assign_wrt_overlaps (match_low_quality, gt_max_assign_all) on the
    [num_gt, num_anchors] matrix, with the loop over the ground truths; argmax ties to the
    lowest index (what torch on the CPU does)."""
    from msmdfusion_amd import anchor_head as A
    n, g = anchor_bev.shape[0], gt_bev.shape[0]
    if g == 0:
        return anchor_bev.new_zeros(n, dtype=torch.int32), anchor_bev.new_zeros(n)
    ov = A.bbox_overlaps(gt_bev, anchor_bev)
    mx = ov.max(0)[0]
    idx = torch.arange(g, device=ov.device)[:, None].expand(g, n)
    arg = torch.where(ov == mx[None], idx, torch.full_like(idx, g)).min(0)[0]
    assigned = torch.full((n,), -1, dtype=torch.int32, device=ov.device)
    assigned[(mx >= 0) & (mx < neg)] = 0
    p = mx >= pos
    assigned[p] = (arg[p] + 1).int()
    gmax = ov.max(1)[0]
    for i in range(g):
        if gmax[i] >= min_pos:
            assigned[ov[i] == gmax[i]] = i + 1
    return assigned, mx


def kitti_generator():
    from msmdfusion_amd import anchor_head as A
    return A.Anchor3DRangeGenerator(
        ranges=[[0, -8.0, -0.6, 20.0, 8.0, -0.6], [0, -8.0, -0.6, 20.0, 8.0, -0.6],
                [0, -8.0, -1.78, 20.0, 8.0, -1.78]],
        sizes=[[0.6, 0.8, 1.73], [0.6, 1.76, 1.73], [1.6, 3.9, 1.56]], rotations=[0, 1.57],
        reshape_out=False)


def ground_truth(anchors, n, seed, code=7, dir_offset=0.0):
    """n boxes near randomly chosen anchors: some exactly on an anchor, one duplicated, one
    midway between two neighbouring anchors, one far from everything; yaw kept 1e-2 away from
    the direction bins' edges."""
    rs = np.random.RandomState(seed)
    flat = anchors.reshape(-1, anchors.shape[-1]).cpu().numpy()
    pick = flat[rs.randint(0, flat.shape[0], n)].copy()
    box = pick.copy()
    box[:, :2] += rs.uniform(-0.6, 0.6, (n, 2))
    box[:, 3:6] *= rs.uniform(0.8, 1.25, (n, 3))
    box[:, 6] = rs.uniform(-3.1, 3.1, n)
    if n > 1:
        box[1] = pick[1]                                   # exactly an anchor: IoU 1
    if n > 3:
        box[3] = box[2]                                    # two identical ground truths
    if n > 4:                                              # midway between two anchors in x
        xs = np.unique(flat[:, 0])
        box[4, :] = pick[4]
        box[4, 0] = (xs[3] + xs[4]) / 2
    if n > 5:
        box[5, :2] = [300.0, 300.0]                        # below min_pos_iou everywhere
    if n > 6:
        box[-1] = pick[-1]                                 # the last one always gets its anchor
    bad = np.abs(np.sin(box[:, 6] - dir_offset)) < 1e-2
    box[bad, 6] += 0.1
    if code > 7:
        box = np.concatenate([box[:, :7], rs.normal(size=(n, code - 7))], 1)
    return torch.from_numpy(box.astype(np.float32)), torch.from_numpy(rs.randint(0, 3, n))


# ---------------------------------------------------------------- the assigner alone
def _segments_case(dev, counts, rows_per_segment, seed=0):
    """One call: len(counts) segments over anchor rows of unequal length."""
    from msmdfusion_amd import anchor_head as A
    anchors = kitti_generator().grid_anchors([(16, 20)], dev)[0].reshape(-1, 7)     # 1920 rows
    assert anchors.shape[0] == 1920
    offs, bev_rows = [0], []
    for k, r in enumerate(rows_per_segment):
        bev_rows.append(torch.cat([anchors, anchors])[(k * 37) % 200:][:r])   # wraps round
        offs.append(offs[-1] + r)
    seg_anchors = torch.cat(bev_rows)
    gts = [ground_truth(anchors, c, seed + k)[0].to(dev) for k, c in enumerate(counts)]
    gt_all = torch.cat(gts)
    gt_offsets = torch.tensor(np.cumsum([0] + list(counts)), dtype=torch.int32).to(dev)
    return seg_anchors, A.nearest_bev(seg_anchors), offs, gts, gt_all, gt_offsets


def test_assigner_equals_the_matrix_and_loop_restatement(dev):
    """Exact (assigned_gt, max_overlaps bitwise, num_pos) at shapes that cross every internal
    boundary: 1920 anchors (several workgroups per ground-truth maximum), ground-truth counts
    0, 1, 5 and chunk + 2, segments of unequal length, lengths that are no multiple of 64."""
    from msmdfusion_amd import anchor_head as A
    from msmdfusion_amd import kernels as K
    chunk = K.ANCHOR_GT_CHUNK
    assert chunk == 128
    counts = [0, 1, 5, chunk + 2, 7]
    rows = [1920, 1000, 1920, 1920, 77]
    anchors, bev, offs, gts, gt_all, gt_offsets = _segments_case(dev, counts, rows)
    thr = [(0.6, 0.45, 0.45), (0.5, 0.35, 0.35), (0.5, 0.35, 0.35), (0.6, 0.45, 0.45),
           (0.35, 0.2, 0.2)]
    assigned, overlaps, num_pos = K.anchor_assign(
        bev, offs, A.nearest_bev(gt_all), gt_offsets, [t[0] for t in thr], [t[1] for t in thr],
        [t[2] for t in thr])
    seen = set()
    for s, (c, r) in enumerate(zip(counts, rows)):
        want, mx = assign_restatement(bev[offs[s]:offs[s + 1]], A.nearest_bev(gts[s]) if c else
                                      bev.new_zeros((0, 4)), *thr[s])
        got = assigned[offs[s]:offs[s + 1]]
        assert torch.equal(got, want), s
        assert torch.equal(overlaps[offs[s]:offs[s + 1]].view(torch.int32), mx.view(torch.int32)), s
        assert int(num_pos[s]) == int((want > 0).sum())
        seen |= set(want.unique().tolist())
    assert -1 in seen and 0 in seen and max(seen) > chunk        # every kind, past the LDS chunk
    assert int(num_pos[0]) == 0 and int(num_pos[3]) > 0


def test_assigner_rules_on_constructed_situations(dev):
    """A tie between two anchors (both assigned), identical ground truths (rule 3 the lower
    index, rule 4 the higher), a ground truth below min_pos_iou, an anchor left at -1."""
    from msmdfusion_amd import kernels as K
    bev = torch.tensor([[0, 0, 2, 2], [2, 0, 4, 2], [10, 10, 12, 12], [20, 20, 22, 22],
                        [30, 30, 32, 33]], dtype=torch.float32, device=dev)
    gt = torch.tensor([[1, 0, 3, 2],            # midway: IoU 1/3 with anchors 0 and 1
                       [10, 10, 12, 12], [10, 10, 12, 12],     # identical, IoU 1 with anchor 2
                       [21.5, 21.5, 30, 30],    # best IoU tiny (< min_pos_iou): no anchor
                       [30, 30, 32, 32.2]],     # IoU 0.733 with anchor 4: neither pos nor neg
                      dtype=torch.float32, device=dev)
    off = torch.tensor([0, 5], dtype=torch.int32).to(dev)
    a, mx, n = K.anchor_assign(bev, [0, 5], gt, off, [0.9], [0.3], [0.3])
    assert a.tolist() == [1, 1, 3, 0, 5]         # rule 4 took 0, 1 (tie), 2 (higher twin), 4
    a, mx, n = K.anchor_assign(bev, [0, 5], gt, off, [0.9], [0.3], [0.8])
    assert a.tolist() == [-1, -1, 3, 0, -1] and int(n[0]) == 1
    a, mx, n = K.anchor_assign(bev, [0, 5], gt[:1], off.clamp(max=1), [0.9], [0.3], [0.8])
    assert a.tolist() == [-1, -1, 0, 0, 0]
    # rule 3 alone picks the LOWER twin: raise min_pos_iou above every IoU
    a, mx, n = K.anchor_assign(bev, [0, 5], gt, off, [0.9], [0.3], [1.5])
    assert a.tolist() == [-1, -1, 2, 0, -1]


def test_assigner_is_bitwise_reproducible(dev):
    from msmdfusion_amd import anchor_head as A
    from msmdfusion_amd import kernels as K
    anchors, bev, offs, gts, gt_all, gt_offsets = _segments_case(dev, [130], [1920], seed=5)
    gb = A.nearest_bev(gt_all)
    one = K.anchor_assign(bev, offs, gb, gt_offsets, [0.5], [0.35], [0.35])
    two = K.anchor_assign(bev, offs, gb, gt_offsets, [0.5], [0.35], [0.35])
    for x, y in zip(one, two):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert int(one[2][0]) > 0                  # positives exist: the comparison says something


# ---------------------------------------------------------------- head-level targets
def _head(dev, kind="kitti", assign_per_class=False, dir_offset=0.7854, test_cfg=None,
          num_classes=3, feat=16):
    from msmdfusion_amd.registry import build_head
    assigner = lambda p, n: dict(type="MaxIoUAssigner",
                                 iou_calculator=dict(type="BboxOverlapsNearest3D"), pos_iou_thr=p,
                                 neg_iou_thr=n, min_pos_iou=n, ignore_iof_thr=-1)
    test_cfg = test_cfg or dict(use_rotate_nms=True, nms_across_levels=False, nms_thr=0.01,
                                score_thr=0.1, min_bbox_size=0, nms_pre=100, max_num=50)
    common = dict(type="Anchor3DHead", num_classes=num_classes, in_channels=feat,
                  feat_channels=feat, use_direction_classifier=True, diff_rad_by_sin=True,
                  dir_offset=dir_offset, dir_limit_offset=0,
                  loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25,
                                loss_weight=1.0),
                  loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=2.0),
                  loss_dir=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.2),
                  test_cfg=test_cfg)
    if kind == "kitti":
        g = kitti_generator()
        cfg = dict(common, anchor_generator=dict(
            type="Anchor3DRangeGenerator", ranges=g.ranges, sizes=g.sizes, rotations=g.rotations,
            reshape_out=False), assigner_per_size=True, assign_per_class=assign_per_class,
            bbox_coder=dict(type="DeltaXYZWLHRBBoxCoder"),
            train_cfg=dict(assigner=[assigner(0.5, 0.35), assigner(0.5, 0.35),
                                     assigner(0.6, 0.45)], allowed_border=0, pos_weight=-1,
                           debug=False))
    else:       # nuScenes style: one assigner, aligned generator, two levels, code size 9
        cfg = dict(common, anchor_generator=dict(
            type="AlignedAnchor3DRangeGenerator", ranges=[[0, -8.0, -1.8, 20.0, 8.0, -1.8]],
            scales=[1, 2], sizes=[[0.866, 2.5981, 1.0], [0.5774, 1.7321, 1.0], [1.0, 1.0, 1.0]],
            custom_values=[0, 0], rotations=[0, 1.57], reshape_out=True),
            bbox_coder=dict(type="DeltaXYZWLHRBBoxCoder", code_size=9),
            train_cfg=dict(assigner=assigner(0.6, 0.3), allowed_border=0, pos_weight=2.0,
                           code_weight=[1.0] * 7 + [0.2, 0.2], debug=False))
    torch.manual_seed(0)
    head = build_head(cfg).to(dev)
    head.init_weights()
    return head


def targets_restatement(head, levels, boxes, labels):
    """anchor_target_3d_single / anchor_target_single_assigner for ONE sample in torch, with
    the reference's reshapes and concatenations.  -> the six tensors, flat over the sample's
    anchors, plus the number of positives."""
    from msmdfusion_amd import anchor_head as A
    code = head.box_code_size

    def single(assigner, anchors, gt, gt_labels):
        n = anchors.shape[0]
        bt, bw = torch.zeros_like(anchors), torch.zeros_like(anchors)
        dt = anchors.new_zeros(n, dtype=torch.long)
        dw, lw = anchors.new_zeros(n), anchors.new_zeros(n)
        lab = anchors.new_full((n,), head.num_classes, dtype=torch.long)
        a, _ = assign_restatement(A.nearest_bev(anchors), A.nearest_bev(gt) if len(gt) else
                                  anchors.new_zeros((0, 4)), assigner.pos_iou_thr,
                                  assigner.neg_iou_thr, assigner.min_pos_iou)
        pos = torch.nonzero(a > 0).squeeze(-1)
        if len(pos):
            tg = gt[(a[pos] - 1).long()]
            enc = A.DeltaXYZWLHRBBoxCoder.encode(anchors[pos], tg)
            rot_gt = enc[..., 6] + anchors[pos][..., 6]
            off = rot_gt - head.dir_offset
            two_pi = off.new_tensor(2 * np.pi)
            off = off - torch.floor(off / two_pi) * two_pi
            dt[pos] = torch.clamp(torch.floor(off / off.new_tensor(np.pi)).long(), 0, 1)
            bt[pos], bw[pos], dw[pos] = enc, 1.0, 1.0
            lab[pos] = gt_labels[(a[pos] - 1).long()]
            pw = head.train_cfg["pos_weight"]
            lw[pos] = 1.0 if pw <= 0 else pw
        lw[a == 0] = 1.0
        return lab, lw, bt, bw, dt, dw, int(len(pos)), (enc.double() if len(pos) else None, pos)

    if isinstance(head.bbox_assigner, list):
        anchors = levels[0]
        feat, rots = anchors.size(0) * anchors.size(1) * anchors.size(2), anchors.size(-2)
        parts, npos = [], 0
        for i, assigner in enumerate(head.bbox_assigner):
            cur = anchors[..., i, :, :].reshape(-1, code)
            m = labels == i if head.assign_per_class else torch.ones_like(labels, dtype=torch.bool)
            r = single(assigner, cur, boxes[m], labels[m])
            npos += r[6]
            parts.append([t.reshape(feat, 1, rots, *t.shape[1:]) for t in r[:6]])
        return [torch.cat(ts, dim=1).reshape(-1, *ts[0].shape[3:]) for ts in zip(*parts)], npos
    flat = torch.cat([a.reshape(-1, code) for a in levels])
    r = single(head.bbox_assigner, flat, boxes, labels)
    return list(r[:6]), r[6]


def encode_bound(anchors, gt):
    """|float32 torch encode - float64 encode| on the same inputs: the yardstick for the
    kernel's log / sqrt / divisions (4 x this, floored at one ulp of the value's scale)."""
    from msmdfusion_amd import anchor_head as A
    e32 = A.DeltaXYZWLHRBBoxCoder.encode(anchors, gt).double()
    e64 = A.DeltaXYZWLHRBBoxCoder.encode(anchors.double(), gt.double())
    scale = e64.abs().clamp(min=1.0)
    return e64, float(((e32 - e64).abs() / scale).max())


CASES = [("kitti", False, (0, 1, 7)), ("kitti", True, (7, 0, 1)), ("nus", False, (1, 7, 0))]


@pytest.mark.parametrize("kind,per_class,counts", CASES)
def test_anchor_target_3d_equals_the_per_sample_restatement(dev, kind, per_class, counts):
    """labels, all weights and dir_targets exact, in the reference's interleaved order (the map
    is 8 x 6, H != W); bbox_targets within 4 x the error torch's own float32 encode shows
    against float64; num_total_pos with max(., 1) per sample."""
    head = _head(dev, kind, per_class)
    sizes = [(8, 6)] if kind == "kitti" else [(8, 6), (4, 3)]
    levels = head.anchor_generator.grid_anchors(sizes, dev)
    code = head.box_code_size
    gt = [ground_truth(levels[0], c, 11 + k, code, head.dir_offset) for k, c in enumerate(counts)]
    boxes, labels = [g[0].to(dev) for g in gt], [g[1].to(dev) for g in gt]
    if per_class:
        labels[0][labels[0] == 1] = 2                      # a class without any ground truth
    got = head.anchor_target_3d([levels] * len(counts), boxes, [None] * len(counts),
                                gt_labels_list=labels, num_classes=head.num_classes,
                                sampling=False)
    flat = [torch.cat([lv.reshape(len(counts), -1, *lv.shape[2:]) for lv in t], dim=1)
            for t in got[:6]]
    total, seen_pos = 0, 0
    for b in range(len(counts)):
        want, npos = targets_restatement(head, levels, boxes[b], labels[b])
        total += max(npos, 1)
        seen_pos += npos
        for k in (0, 1, 3, 4, 5):
            assert torch.equal(flat[k][b], want[k]), (b, k)
        pos = want[3][:, 0] > 0
        if pos.any():
            # float64 of the same (anchor, gt) pairs; the float32 torch encode's distance to it
            # is the yardstick
            a_flat = _flat_anchors(head, levels)[pos]
            g_rows = _gt_rows(head, levels, boxes[b], labels[b])[pos]
            e64, err_own = encode_bound(a_flat, g_rows)
            scale = e64.abs().clamp(min=1.0)
            err = float(((flat[2][b][pos].double() - e64).abs() / scale).max())
            bound = 4 * max(err_own, ULP)
            print(kind, per_class, b, "encode err", err, "bound", bound)
            assert err <= bound, (err, bound)
            assert torch.equal(flat[2][b][~pos], want[2][~pos])
    assert seen_pos > 0 and int(got[6]) == total
    assert all(t[0].shape[0] == len(counts) for t in got[:6])
    assert [t.shape[1] for t in got[0]] == [lv.reshape(-1, code).shape[0] for lv in levels]


def _flat_anchors(head, levels):
    code = head.box_code_size
    return torch.cat([a.reshape(-1, code) for a in levels])       # the reference's output order


def _gt_rows(head, levels, boxes, labels):
    """The ground-truth box each anchor was assigned (rows of zeros elsewhere), in output
    order, from the restatement's assignment."""
    from msmdfusion_amd import anchor_head as A
    code = head.box_code_size
    flat = _flat_anchors(head, levels)
    out = torch.zeros_like(flat)
    if isinstance(head.bbox_assigner, list):
        anchors = levels[0]
        view = out.view(*anchors.shape)
        for i, assigner in enumerate(head.bbox_assigner):
            cur = anchors[..., i, :, :].reshape(-1, code)
            m = labels == i if head.assign_per_class else torch.ones_like(labels, dtype=torch.bool)
            gt = boxes[m]
            a, _ = assign_restatement(A.nearest_bev(cur), A.nearest_bev(gt) if len(gt) else
                                      cur.new_zeros((0, 4)), assigner.pos_iou_thr,
                                      assigner.neg_iou_thr, assigner.min_pos_iou)
            rows = torch.zeros_like(cur)
            if len(gt):
                rows[a > 0] = gt[(a[a > 0] - 1).long()]
            view[..., i, :, :] = rows.view(*anchors.shape[:3], anchors.shape[4], code)
        return out
    a, _ = assign_restatement(A.nearest_bev(flat), A.nearest_bev(boxes) if len(boxes) else
                              flat.new_zeros((0, 4)), head.bbox_assigner.pos_iou_thr,
                              head.bbox_assigner.neg_iou_thr, head.bbox_assigner.min_pos_iou)
    if len(boxes):
        out[a > 0] = boxes[(a[a > 0] - 1).long()]
    return out


# ---------------------------------------------------------------- focal loss
def focal_restatement(x, labels, weights, gamma, alpha):
    """mmdet py_sigmoid_focal_loss, weighted and summed."""
    c = x.shape[1]
    t = F.one_hot(labels, c + 1)[:, :c].to(x.dtype)
    p = x.sigmoid()
    pt = (1 - p) * t + p * (1 - t)
    fw = (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma)
    loss = F.binary_cross_entropy_with_logits(x, t, reduction="none") * fw
    return (loss * weights[:, None]).sum()


@pytest.mark.parametrize("c", [1, 3, 10])
@pytest.mark.parametrize("n", [1, 63, 4099])
def test_sigmoid_focal_value_and_gradient(dev, n, c):
    """Value and gradient against float64 autograd within 4 x the error the float32 torch
    restatement shows (floored at float32 eps of the scale); all-background labels,
    all-ignored weights and logits of +-30 included; two runs bitwise equal."""
    from msmdfusion_amd import kernels as K
    g = torch.Generator(device="cpu").manual_seed(n * 31 + c)
    x = (torch.randn((n, c), generator=g) * 3).to(dev)
    x.view(-1)[::7] = 30.0
    x.view(-1)[3::11] = -30.0
    labels = torch.randint(0, c + 1, (n,), generator=g).to(dev)
    weights = torch.rand((n,), generator=g).to(dev)
    weights[::5] = 0.0
    for mode in ("mixed", "background", "ignored"):
        lab = torch.full_like(labels, c) if mode == "background" else labels
        w = torch.zeros_like(weights) if mode == "ignored" else weights
        x64 = x.double().requires_grad_()
        want = focal_restatement(x64, lab, w.double(), 2.0, 0.25)
        want.backward()
        x32 = x.clone().requires_grad_()
        own = focal_restatement(x32, lab, w, 2.0, 0.25)
        own.backward()
        total, grad = K.sigmoid_focal(x, lab, w, 2.0, 0.25)
        again, grad2 = K.sigmoid_focal(x, lab, w, 2.0, 0.25)
        assert torch.equal(total, again) and torch.equal(grad, grad2)
        vscale = max(abs(float(want.detach())), 1e-30)
        verr = abs(float(total) - float(want.detach()))
        vown = abs(float(own.detach()) - float(want.detach()))
        gscale = max(float(x64.grad.abs().max()), 1e-30)
        gerr = float((grad.double() - x64.grad).abs().max())
        gown = float((x32.grad.double() - x64.grad).abs().max())
        print(n, c, mode, "value", verr / vscale, vown / vscale, "grad", gerr / gscale,
              gown / gscale)
        assert verr <= 4 * max(vown, ULP * vscale)
        assert gerr <= 4 * max(gown, ULP * gscale)
        if mode == "ignored":
            assert float(total) == 0.0 and float(grad.abs().max()) == 0.0


# ---------------------------------------------------------------- loss
def loss_restatement(head, outs, targets, dtype=torch.float64):
    """anchor3d_head.py:188-272 per level in torch ops, positives gathered as the reference
    does, for float64 autograd."""
    cls_scores, bbox_preds, dir_preds = outs
    labels_l, lw_l, bt_l, bw_l, dt_l, dw_l, num_pos, _ = targets
    avg = num_pos.to(dtype)
    out = dict(loss_cls=[], loss_bbox=[], loss_dir=[])
    for c, b, d, labels, lw, bt, bw, dt, dw in zip(cls_scores, bbox_preds, dir_preds, labels_l,
                                                   lw_l, bt_l, bw_l, dt_l, dw_l):
        labels = labels.reshape(-1)
        c = c.to(dtype).permute(0, 2, 3, 1).reshape(-1, head.num_classes)
        out["loss_cls"].append(focal_restatement(c, labels, lw.reshape(-1).to(dtype), 2.0, 0.25)
                               / avg)
        b = b.to(dtype).permute(0, 2, 3, 1).reshape(-1, head.box_code_size)
        d = d.to(dtype).permute(0, 2, 3, 1).reshape(-1, 2)
        pos = torch.nonzero((labels >= 0) & (labels < head.num_classes)).reshape(-1)
        pb, pt = b[pos], bt.reshape(-1, head.box_code_size)[pos].to(dtype)
        pw = bw.reshape(-1, head.box_code_size)[pos].to(dtype)
        if len(pos) > 0:
            cw = head.train_cfg.get("code_weight")
            if cw:
                pw = pw * pw.new_tensor(cw)
            pb, pt = head.add_sin_difference(pb, pt)
            diff = (pb - pt).abs()
            beta = 1.0 / 9.0
            l1 = torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)
            out["loss_bbox"].append(2.0 * (l1 * pw).sum() / avg)
            ce = F.cross_entropy(d[pos], dt.reshape(-1)[pos], reduction="none")
            out["loss_dir"].append(0.2 * (ce * dw.reshape(-1)[pos].to(dtype)).sum() / avg)
        else:
            out["loss_bbox"].append(pb.sum())
            out["loss_dir"].append(d[pos].sum())
    return out


@pytest.mark.parametrize("kind,counts", [("kitti", (0, 1, 7)), ("nus", (7, 0)), ("kitti", (0, 0))])
def test_loss_and_gradients_against_float64_autograd(dev, kind, counts):
    """The tolerance tests/test_gpu_center_head.py applies to its loss (rtol 2e-6 on the values
    against the float64 restatement on the head's own targets, 1e-5 of the scale on the
    gradients); a sample without ground truth, and a batch without any (num_pos == 0 and the
    max(., 1) factors)."""
    head = _head(dev, kind)
    sizes = [(8, 6)] if kind == "kitti" else [(8, 6), (4, 3)]
    levels = head.anchor_generator.grid_anchors(sizes, dev)
    gt = [ground_truth(levels[0], c, 3 + k, head.box_code_size, head.dir_offset)
          for k, c in enumerate(counts)]
    boxes, labels = [g[0].to(dev) for g in gt], [g[1].to(dev) for g in gt]
    torch.manual_seed(4)
    feats = [torch.randn((len(counts), 16, *s), device=dev) for s in sizes]
    outs = head(feats)
    leaves = [[t.detach().clone().requires_grad_() for t in lvl] for lvl in outs]
    losses = head.loss(*leaves, boxes, labels, None)
    assert sorted(losses) == ["loss_bbox", "loss_cls", "loss_dir"]
    total = sum(sum(v) for v in losses.values())
    total.backward()
    targets = head.anchor_target_3d([levels] * len(counts), boxes, [None] * len(counts),
                                    gt_labels_list=labels, num_classes=head.num_classes,
                                    sampling=False)
    ref = [[t.detach().double().requires_grad_() for t in lvl] for lvl in outs]
    want = loss_restatement(head, ref, targets)
    sum(sum(v) for v in want.values()).backward()
    for k in losses:
        for lvl, (g, w) in enumerate(zip(losses[k], want[k])):
            print(kind, counts, k, lvl, float(g.detach()), float(w.detach()))
            np.testing.assert_allclose(float(g.detach()), float(w.detach()), rtol=2e-6, err_msg=k)
    for kind_i in range(3):
        for lvl in range(len(sizes)):
            g, w = leaves[kind_i][lvl].grad, ref[kind_i][lvl].grad
            scale = float(w.abs().max()) + 1e-12
            assert float((g.double() - w).abs().max()) <= 1e-5 * scale, (kind_i, lvl)
    if sum(counts) == 0:
        assert float(sum(losses["loss_bbox"])) == 0.0 and float(targets[6]) == len(counts)
        assert all(float(t.grad.abs().max()) == 0.0 for t in leaves[1])


# ---------------------------------------------------------------- get_bboxes
def loop_bboxes(head, outs, cfg):
    """get_bboxes_single + box3d_multiclass_nms as the reference loops: per sample, per level,
    per class, over the single-list NMS (stable sorts)."""
    from msmdfusion_amd import anchor_head as A
    from msmdfusion_amd import iou3d
    cls_scores, bbox_preds, dir_preds = outs
    code = head.box_code_size
    sizes = [c.shape[-2:] for c in cls_scores]
    anchors_l = [a.reshape(-1, code) for a in
                 head.anchor_generator.grid_anchors(sizes, cls_scores[0].device)]
    results = []
    for i in range(cls_scores[0].shape[0]):
        mb, ms, md = [], [], []
        for c, b, d, anchors in zip(cls_scores, bbox_preds, dir_preds, anchors_l):
            d = d[i].permute(1, 2, 0).reshape(-1, 2)
            ds = torch.max(d, dim=-1)[1]
            s = c[i].permute(1, 2, 0).reshape(-1, head.num_classes).sigmoid()
            b = b[i].permute(1, 2, 0).reshape(-1, code)
            if cfg["nms_pre"] > 0 and s.shape[0] > cfg["nms_pre"]:
                _, top = s.max(dim=1)[0].topk(cfg["nms_pre"])
                anchors, b, s, ds = anchors[top], b[top], s[top], ds[top]
            mb.append(head.bbox_coder.decode(anchors, b))
            ms.append(s)
            md.append(ds)
        mb, ms, md = torch.cat(mb), torch.cat(ms), torch.cat(md)
        bev = A.xywhr2xyxyr(mb[:, [0, 1, 3, 4, 6]])
        bb, ss, ll, dd = [], [], [], []
        for k in range(head.num_classes):
            m = ms[:, k] > cfg["score_thr"]
            if not m.any():
                continue
            sc, bv = ms[m, k], bev[m]
            if cfg["use_rotate_nms"]:
                sel = iou3d.nms_gpu(bv, sc, cfg["nms_thr"])
            else:
                sel = iou3d.nms_normal_gpu(bv, sc, cfg["nms_thr"])
            bb.append(mb[m][sel])
            ss.append(sc[sel])
            ll.append(torch.full((len(sel),), k, dtype=torch.long, device=sc.device))
            dd.append(md[m][sel])
        if bb:
            bb, ss, ll, dd = torch.cat(bb), torch.cat(ss), torch.cat(ll), torch.cat(dd)
            if bb.shape[0] > cfg["max_num"]:
                inds = torch.sort(ss, descending=True, stable=True)[1][:cfg["max_num"]]
                bb, ss, ll, dd = bb[inds], ss[inds], ll[inds], dd[inds]
            rot = A.limit_period(bb[..., 6] - head.dir_offset, head.dir_limit_offset, np.pi)
            bb = bb.clone()
            bb[..., 6] = rot + head.dir_offset + np.pi * dd.to(bb.dtype)
        else:
            bb, ss, ll = ms.new_zeros((0, code)), ms.new_zeros((0,)), ms.new_zeros((0,)).long()
        results.append((bb, ss, ll))
    return results


@pytest.mark.parametrize("rotate", [True, False])
@pytest.mark.parametrize("nms_pre", [40, 400])
def test_get_bboxes_equals_the_per_sample_per_class_loop(dev, rotate, nms_pre):
    """Rotated and normal NMS, nms_pre below and above the level size (288 / 72 anchors), a
    class with nothing above score_thr, more than max_num survivors, equal scores."""
    cfg = dict(use_rotate_nms=rotate, nms_across_levels=False, nms_thr=0.2, score_thr=0.3,
               min_bbox_size=0, nms_pre=nms_pre, max_num=15)
    head = _head(dev, "nus", test_cfg=cfg).eval()
    torch.manual_seed(7)
    B, A_, C = 3, head.num_anchors, head.num_classes
    outs = ([], [], [])
    for (h, w) in [(8, 6), (4, 3)]:
        cls = torch.randn((B, A_, C, h, w), device=dev)
        cls[:, :, 0] = (torch.round(cls[:, :, 0] * 2) / 2 - 0.25).clamp(max=1.0)   # equal scores
        cls[:, :, 1] = torch.rand((B, A_, h, w), device=dev) + 1.5    # distinct, the top-k key
        cls[:, :, 2] = -6.0                                           # never above score_thr
        outs[0].append(cls.view(B, A_ * C, h, w))
        outs[1].append(torch.randn((B, A_ * 9, h, w), device=dev) * 0.3)
        outs[2].append(torch.randn((B, A_ * 2, h, w), device=dev))
    with torch.no_grad():
        got = head.get_bboxes(*outs, [None] * B)
        want = loop_bboxes(head, outs, cfg)
    kept = 0
    for g, w in zip(got, want):
        assert g[2].dtype == torch.long
        assert torch.equal(g[2], w[2])
        assert torch.equal(g[1], w[1])
        assert torch.equal(g[0], w[0])
        kept += g[1].numel()
        assert not (g[2] == 2).any()
    assert kept == 15 * B                      # more than max_num survived everywhere: the cut
    one = head.get_bboxes_single([c[1] for c in outs[0]], [b[1] for b in outs[1]],
                                 [d[1] for d in outs[2]], None, None)
    assert torch.equal(one[0], got[1][0]) and torch.equal(one[2], got[1][2])
    with pytest.raises(NotImplementedError, match="nms_pre"):
        head.get_bboxes(*outs, [None] * B, cfg=dict(cfg, nms_pre=-1))
    with pytest.raises(NotImplementedError, match="nms_pre"):
        head.get_bboxes(*outs, [None] * B, cfg=dict(cfg, nms_pre=9000))


# ---------------------------------------------------------------- no host wait
def test_targets_and_loss_do_not_wait_for_the_device(dev):
    """anchor_target_3d and loss return while the stream still holds work queued before them
    (the means of tests/test_gpu_pointnet_ops.py); get_bboxes reads the kept counts once."""
    head = _head(dev, "kitti", assign_per_class=True)
    levels = head.anchor_generator.grid_anchors([(8, 6)], dev)
    gt = [ground_truth(levels[0], c, 20 + k) for k, c in enumerate((5, 0))]
    boxes, labels = [g[0].to(dev) for g in gt], [g[1].to(dev) for g in gt]
    feats = [torch.randn((2, 16, 8, 6), device=dev)]

    def work():
        outs = head(feats)
        losses = head.loss(*outs, boxes, labels, None)
        sum(sum(v) for v in losses.values()).backward()
        return outs

    big = torch.randn((8192, 8192), device=dev)
    work()                                              # warm: allocations, caches, module load
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    for _ in range(8):
        big = big @ big * 1e-4                          # tens of milliseconds of queued work
    outs = work()
    assert not stream.query(), "anchor_target_3d / loss synchronised with the device"
    torch.cuda.synchronize()
    # get_bboxes: every synchronisation warns under the debug mode; exactly one may, the read of
    # the kept counts
    import warnings
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            head.get_bboxes(*[[t.detach() for t in lvl] for lvl in outs], [None, None])
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchroniz" in str(w.message).lower()
             and "prototype" not in str(w.message)]
    assert len(syncs) <= 1, [str(w.message) for w in syncs]


# ---------------------------------------------------------------- detectors
def _cloud(dev, rng_, n=3000, seed=4):
    rs = np.random.RandomState(seed)
    pts = []
    for _ in range(2):
        p = rs.uniform(0, 1, (n, 4)).astype(np.float32)
        p[:, 0] = rng_[0] + p[:, 0] * (rng_[3] - rng_[0]) * 0.999
        p[:, 1] = rng_[1] + p[:, 1] * (rng_[4] - rng_[1]) * 0.999
        p[:, 2] = rs.uniform(-2.5, 0.5, n)
        pts.append(torch.from_numpy(p).to(dev))
    return pts


def _train_and_infer(det, points, dev, size):
    gt = [torch.tensor([[4.0, 1.0, -1.6, 1.6, 3.9, 1.56, 0.3],
                        [3.0, -2.0, -0.6, 0.6, 0.8, 1.73, 1.0]], device=dev),
          torch.zeros((0, 7), device=dev)]
    labels = [torch.tensor([2, 0], device=dev), torch.zeros((0,), dtype=torch.long, device=dev)]
    det.train()
    losses = det(points, return_loss=True, gt_bboxes_3d=gt, gt_labels_3d=labels)
    assert sorted(losses) == ["loss_bbox", "loss_cls", "loss_dir"]
    total = sum(sum(v) for v in losses.values())
    assert torch.isfinite(total)
    total.backward()
    grads = [p.grad for p in det.parameters() if p.requires_grad]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    assert float(det.bbox_head.conv_reg.weight.grad.abs().sum()) > 0
    det.eval()
    with torch.no_grad():
        out = det.simple_test(points)
    assert len(out) == 2
    for r in out:
        n = r["scores_3d"].shape[0]
        assert r["boxes_3d"].shape == (n, 7) and r["labels_3d"].shape == (n,) and n <= 50
        if n:
            assert 0 <= int(r["labels_3d"].min()) and int(r["labels_3d"].max()) < 3
            assert float(r["scores_3d"].min()) > 0.1


def test_voxelnet_from_the_pointpillars_config_trains_and_infers(dev):
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.registry import build_detector
    model = copy.deepcopy(C.POINTPILLARS_SECFPN_KITTI["model"])
    rng_ = [0, -6.4, -3, 12.8, 6.4, 1]
    model["voxel_layer"].update(point_cloud_range=rng_, max_voxels=(6400, 6400))
    model["voxel_encoder"].update(point_cloud_range=rng_)
    model["middle_encoder"].update(output_shape=[80, 80])
    for r in model["bbox_head"]["anchor_generator"]["ranges"]:
        r[0:2], r[3:5] = [0, -6.4], [12.8, 6.4]
    torch.manual_seed(3)
    det = build_detector(model).to(dev)
    assert type(det).__name__ == "VoxelNet" and type(det.bbox_head).__name__ == "Anchor3DHead"
    assert {k.split(".")[0] for k in det.state_dict()} == {"voxel_encoder", "backbone", "neck",
                                                          "bbox_head"}
    _train_and_infer(det, _cloud(dev, rng_), dev, 40)
    assert float(det.voxel_encoder.pfn_layers[0].linear.weight.grad.abs().sum()) > 0


def test_voxelnet_from_the_second_config_trains_and_infers(dev):
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.registry import build_detector
    model = copy.deepcopy(C.SECOND_SECFPN_KITTI["model"])
    rng_ = [0, -3.2, -3, 6.4, 3.2, 1]
    model["voxel_layer"].update(point_cloud_range=rng_, max_voxels=(8000, 8000))
    model["middle_encoder"].update(sparse_shape=[41, 128, 128])
    for r in model["bbox_head"]["anchor_generator"]["ranges"]:
        r[0:2], r[3:5] = [0, -3.2], [6.4, 3.2]
    torch.manual_seed(3)
    det = build_detector(model).to(dev)
    assert type(det.middle_encoder).__name__ == "SparseEncoder"
    _train_and_infer(det, _cloud(dev, rng_, n=4000), dev, 16)


# ---------------------------------------------------------------- against the reference's outputs
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchor_head_vectors.npz")
GOLD_TEST_CFG = dict(use_rotate_nms=True, nms_across_levels=False, nms_thr=0.2, score_thr=0.3,
                     min_bbox_size=0, nms_pre=30, max_num=12)
GOLD_CASES = {"k": ("kitti", False), "kc": ("kitti", True), "n": ("nus", False)}
TARGET_NAMES = ("labels", "label_weights", "bbox_targets", "bbox_weights", "dir_targets",
                "dir_weights")


@pytest.fixture(scope="module")
def gold():
    """The reference's own Anchor3DHead / AnchorTrainMixin / MaxIoUAssigner outputs
    (tests/golden/make_anchor_head_golden.py); read-only."""
    return np.load(GOLD)


def _gold_head(dev, tag):
    kind, per_class = GOLD_CASES[tag]
    head = _head(dev, kind, per_class, test_cfg=GOLD_TEST_CFG)
    sizes = [(8, 6)] if kind == "kitti" else [(8, 6), (4, 3)]
    return head, sizes, head.anchor_generator.grid_anchors(sizes, dev)


def _gold_truth(gold, tag, dev):
    return ([torch.from_numpy(gold["%s_gt_boxes_%d" % (tag, b)]).to(dev) for b in range(2)],
            [torch.from_numpy(gold["%s_gt_labels_%d" % (tag, b)]).to(dev) for b in range(2)])


@pytest.mark.parametrize("tag", sorted(GOLD_CASES))
def test_assigner_equals_the_reference(gold, dev, tag):
    """assigned_gt exact and max_overlaps bitwise against the reference's MaxIoUAssigner, per
    sample and per assigner, all segments of the case in ONE call."""
    from msmdfusion_amd import anchor_head as A
    from msmdfusion_amd import kernels as K
    head, sizes, levels = _gold_head(dev, tag)
    boxes, labels = _gold_truth(gold, tag, dev)
    assigners = head.bbox_assigner if isinstance(head.bbox_assigner, list) else [head.bbox_assigner]
    segs, offs, gts, goff, thr = [], [0], [], [0], []
    for b in range(2):
        for i, asg in enumerate(assigners):
            key = "%s_assign_gt_inds_s%d_a%d" % (tag, b, i)
            if key not in gold.files:
                continue
            if isinstance(head.bbox_assigner, list):
                cur = levels[0][..., i, :, :].reshape(-1, 7)
                m = labels[b] == i if head.assign_per_class else torch.ones_like(labels[b]).bool()
            else:
                cur = torch.cat([a.reshape(-1, head.box_code_size) for a in levels])
                m = torch.ones_like(labels[b]).bool()
            segs.append((b, i, cur))
            offs.append(offs[-1] + cur.shape[0])
            gts.append(boxes[b][m])
            goff.append(goff[-1] + int(m.sum()))
            thr.append((asg.pos_iou_thr, asg.neg_iou_thr, asg.min_pos_iou))
    assert len(segs) >= 2
    assigned, overlaps, num_pos = K.anchor_assign(
        A.nearest_bev(torch.cat([s[2] for s in segs])), offs, A.nearest_bev(torch.cat(gts)),
        torch.tensor(goff, dtype=torch.int32).to(dev), [t[0] for t in thr], [t[1] for t in thr],
        [t[2] for t in thr])
    for s, (b, i, _) in enumerate(segs):
        want = gold["%s_assign_gt_inds_s%d_a%d" % (tag, b, i)]
        np.testing.assert_array_equal(assigned[offs[s]:offs[s + 1]].cpu().numpy(), want)
        np.testing.assert_array_equal(
            overlaps[offs[s]:offs[s + 1]].cpu().numpy().view(np.int32),
            gold["%s_assign_max_overlaps_s%d_a%d" % (tag, b, i)].view(np.int32))
        assert int(num_pos[s]) == int((want > 0).sum())


@pytest.mark.parametrize("tag", sorted(GOLD_CASES))
def test_anchor_target_3d_equals_the_reference(gold, dev, tag):
    """labels, all weights and dir_targets exact against the reference's anchor_target_3d;
    bbox_targets against the reference's float64 run on the same inputs, within 4 x the error
    its float32 run shows (the yardstick of tests/test_gpu_pillar.py), floored at one ulp."""
    head, sizes, levels = _gold_head(dev, tag)
    boxes, labels = _gold_truth(gold, tag, dev)
    got = head.anchor_target_3d([levels, levels], boxes, [None, None], gt_labels_list=labels,
                                num_classes=3, sampling=False)
    positives = 0
    for lvl in range(len(sizes)):
        for k, name in enumerate(TARGET_NAMES):
            want = gold["%s_tgt_%s_l%d" % (tag, name, lvl)]
            g = got[k][lvl].cpu().numpy()
            assert g.shape == want.shape and g.dtype == want.dtype, (name, lvl)
            if name != "bbox_targets":
                np.testing.assert_array_equal(g, want, err_msg="%s l%d" % (name, lvl))
                continue
            e64 = gold["%s_tgt_bbox_targets64_l%d" % (tag, lvl)]
            scale = np.maximum(np.abs(e64), 1.0)
            own = float((np.abs(want.astype(np.float64) - e64) / scale).max())
            err = float((np.abs(g.astype(np.float64) - e64) / scale).max())
            print(tag, lvl, "bbox_targets err", err, "reference float32 err", own)
            assert err <= 4 * max(own, ULP), (err, own)
            pos = gold["%s_tgt_bbox_weights_l%d" % (tag, lvl)][..., 0] > 0
            positives += int(pos.sum())
            np.testing.assert_array_equal(g[~pos], want[~pos])
    assert positives > 0
    assert int(got[6]) == int(gold["%s_num_total_pos" % tag])
    assert int(got[7]) == int(gold["%s_num_total_neg" % tag])


def _gold_preds(gold, tag, levels, dev, dtype=torch.float32):
    return [[torch.from_numpy(gold["%s_pred_%s_l%d" % (tag, name, lvl)]).to(dev, dtype)
             .requires_grad_() for lvl in range(levels)] for name in ("cls", "bbox", "dir")]


@pytest.mark.parametrize("tag", ["k", "n"])
def test_loss_equals_the_reference(gold, dev, tag):
    """The tolerance tests/test_gpu_center_head.py applies to its loss: values rtol 2e-6
    against the reference's; gradients of all three conv outputs within 1e-5 of the scale of
    float64 autograd on the GOLDEN targets, and rtol 2e-4 / atol 2e-6 x scale of the
    reference's own float32 gradients.  Case k holds the sample without ground truth; case n a
    level without positives (the num_pos == 0 branch)."""
    head, sizes, levels = _gold_head(dev, tag)
    boxes, labels = _gold_truth(gold, tag, dev)
    preds = _gold_preds(gold, tag, len(sizes), dev)
    losses = head.loss(*preds, boxes, labels, None)
    sum(sum(v) for v in losses.values()).backward()
    for k in ("loss_cls", "loss_bbox", "loss_dir"):
        got = [float(v.detach()) for v in losses[k]]
        print(tag, k, got, gold["%s_%s" % (tag, k)].tolist())
    for k in ("loss_cls", "loss_bbox", "loss_dir"):
        np.testing.assert_allclose([float(v.detach()) for v in losses[k]],
                                   gold["%s_%s" % (tag, k)], rtol=2e-6, err_msg=k)
    targets = [[torch.from_numpy(gold["%s_tgt_%s_l%d" % (tag, name, lvl)]).to(dev)
                for lvl in range(len(sizes))] for name in TARGET_NAMES]
    targets += [torch.tensor(float(gold["%s_num_total_pos" % tag]), device=dev), None]
    ref = _gold_preds(gold, tag, len(sizes), dev, torch.float64)
    sum(sum(v) for v in loss_restatement(head, ref, targets).values()).backward()
    for i, name in enumerate(("cls", "bbox", "dir")):
        for lvl in range(len(sizes)):
            g, w = preds[i][lvl].grad, ref[i][lvl].grad
            scale = float(w.abs().max()) + 1e-12
            assert float((g.double() - w).abs().max()) <= 1e-5 * scale, (name, lvl)
            np.testing.assert_allclose(g.cpu().numpy(), gold["%s_grad_%s_l%d" % (tag, name, lvl)],
                                       rtol=2e-4, atol=2e-6 * scale, err_msg="%s %d" % (name, lvl))


@pytest.mark.parametrize("tag", ["k", "n"])
def test_get_bboxes_equals_the_reference(gold, dev, tag):
    """The same detections in the same order as the reference's get_bboxes (labels exact);
    coordinates and scores within 1e-5, the bound tests/test_gpu_center_head.py uses for device
    sigmoid / exp against the host's."""
    head, sizes, levels = _gold_head(dev, tag)
    preds = _gold_preds(gold, tag, len(sizes), dev)
    with torch.no_grad():
        got = head.eval().get_bboxes(*[[t.detach() for t in p] for p in preds], [None, None])
    for i, (b, s, l) in enumerate(got):
        np.testing.assert_array_equal(l.cpu().numpy(), gold["%s_det_s%d_labels" % (tag, i)])
        np.testing.assert_allclose(s.cpu().numpy(), gold["%s_det_s%d_scores" % (tag, i)],
                                   rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(b.cpu().numpy(), gold["%s_det_s%d_bboxes" % (tag, i)],
                                   rtol=1e-5, atol=1e-5)
        assert l.numel() == 12
