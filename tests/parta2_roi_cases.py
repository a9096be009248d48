"""Case builders and float64 restatements for Part-A2's second-stage targets
(tests/test_parta2_second_stage_cpu.py, tests/test_gpu_parta2_roi_ops.py,
tests/test_gpu_parta2_second_stage.py).

Every builder ASSERTS what makes the discrete results well defined, with the oracle's 3-D IoU
(oracle/head_loss.boxes_iou3d, the float32 arithmetic of the reference's CUDA kernel):
  - no same-class IoU within MARGIN of a threshold in use (assigner, piece bounds, cls thresholds);
  - per proposal the two largest same-class IoUs differ by more than MARGIN, unless the case is
    about a tie (`twins`);
  - keys are pairwise distinct unless the case is about equal keys;
  - the canonical relative yaw of every same-class pair is at least 1e-3 from pi/2 and 3pi/2;
  - NMS candidates have distinct scores and no pair IoU within MARGIN of nms_thr
    (assert_nms_margins).
"""
import numpy as np

F32 = np.float32
MARGIN = 1e-4
YAW_MARGIN = 1e-3
THR = dict(pos=0.55, neg=0.55, min_pos=0.55)
PIECES = (0.55, 0.1)
CLS_THR = (0.75, 0.25)


def iou3d(a, b):
    from oracle import head_loss as OH
    a, b = np.asarray(a, F32).reshape(-1, 7), np.asarray(b, F32).reshape(-1, 7)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return np.zeros((a.shape[0], b.shape[0]), F32)
    return OH.boxes_iou3d(a, b, "iou")


def pair_iou(props, gt):
    """[P, G]: the assigner's iou_calculator(gt_bboxes, bboxes), transposed (the float32 polygon
    area is not symmetric in its arguments)."""
    return np.ascontiguousarray(iou3d(gt, props).T)


def make_gt(rng, count, classes, spread=12.0):
    """[count, 7] float32 boxes on a lattice `spread` apart (they never touch) and labels."""
    slots = np.arange(count)
    side = int(np.ceil(np.sqrt(max(count, 1))))
    centre = np.stack([slots % side, slots // side, np.zeros(count)], 1) * spread \
        + rng.uniform(-1.0, 1.0, (count, 3))
    size = rng.uniform(1.5, 4.0, (count, 3))
    yaw = rng.uniform(-3.0, 3.0, (count, 1))
    labels = rng.randint(0, classes, count).astype(np.int64)
    return np.concatenate([centre, size, yaw], 1).astype(F32), labels


def make_proposals(rng, count, gt, gt_labels, classes):
    """[count, 7] proposals and labels: jittered copies of ground truths of the same class
    (from near copies to bare overlaps, some turned by about pi: the other side of the
    orientation flip), copies under another class, and boxes that overlap nothing."""
    props = np.zeros((count, 7), np.float64)
    labels = rng.randint(0, classes, count).astype(np.int64)
    for i in range(count):
        kind = rng.randint(0, 10)
        if gt.shape[0] == 0 or kind == 9:
            props[i] = np.concatenate([rng.uniform(-60, -20, 2), rng.uniform(-1, 1, 1),
                                       rng.uniform(1.5, 4.0, 3), rng.uniform(-3, 3, 1)])
            continue
        g = rng.randint(0, gt.shape[0])
        scale = (0.02, 0.05, 0.1, 0.2, 0.35)[rng.randint(0, 5)]
        box = gt[g].astype(np.float64)
        box[:3] += rng.uniform(-1, 1, 3) * scale * box[3:6]
        box[3:6] *= 1 + rng.uniform(-1, 1, 3) * scale
        box[6] += rng.uniform(-1, 1) * scale + (np.pi if rng.randint(0, 3) == 0 else 0.0)
        props[i] = box
        if kind < 8 and gt_labels[g] >= 0:
            labels[i] = gt_labels[g]
    return props.astype(F32), labels


def class_mask(prop_labels, gt_labels, classes, single):
    """[P, G] bool: the pairs for which an IoU is formed."""
    if single:
        return np.ones((len(prop_labels), len(gt_labels)), bool)
    same = prop_labels[:, None] == gt_labels[None, :]
    return same & (gt_labels[None, :] >= 0) & (gt_labels[None, :] < classes)


def canonical_yaw(props, gt):
    """(gt yaw - roi yaw mod 2pi) mod 2pi in float64 [P, G]."""
    two_pi = 2 * np.pi
    return np.mod(gt[None, :, 6].astype(np.float64) - np.mod(props[:, None, 6].astype(np.float64),
                                                             two_pi), two_pi)


def assert_margins(props, prop_labels, gt, gt_labels, classes, single=False, twins=False,
                   thresholds=None):
    """See the module docstring.  -> the masked IoU matrix [P, G] (float32)."""
    thresholds = list(thresholds if thresholds is not None else
                      list(THR.values()) + list(PIECES) + list(CLS_THR))
    iou = pair_iou(props, gt)
    mask = class_mask(prop_labels, gt_labels, classes, single)
    used = np.where(mask, iou, 0).astype(np.float64)
    for t in thresholds:
        near = np.abs(used - t) < MARGIN
        assert not (near & mask).any(), ("an IoU within the margin of %g" % t)
    if used.shape[1] >= 2 and not twins:
        top = np.sort(used, axis=1)[:, -2:]
        tied = (top[:, 1] > 0) & (top[:, 1] - top[:, 0] <= MARGIN)
        assert not tied.any(), "two same-class IoUs of one proposal within the margin"
    if used.size:
        rel = canonical_yaw(props, gt)
        for edge in (np.pi / 2, 3 * np.pi / 2):
            close = (np.abs(rel - edge) < YAW_MARGIN) & mask & (used > 0)
            assert not close.any(), "a canonical yaw on the edge of the orientation flip"
    return np.where(mask, iou, 0).astype(F32)


def make_case(seed, prop_counts, gt_counts, classes=3, single=False):
    """A batch: per sample proposals / labels / ground truths / labels (float32 / int64), with
    the margins asserted; a sample's draw is repeated with the next seed until they hold."""
    assert len(prop_counts) == len(gt_counts)
    case = dict(props=[], prop_labels=[], gt=[], gt_labels=[], classes=classes, single=single)
    for b, (p, g) in enumerate(zip(prop_counts, gt_counts)):
        for attempt in range(50):
            rng = np.random.RandomState(seed * 1000 + b * 50 + attempt)
            gt, gt_labels = make_gt(rng, g, classes)
            props, prop_labels = make_proposals(rng, p, gt, gt_labels, classes)
            try:
                assert_margins(props, prop_labels, gt, gt_labels, classes, single)
            except AssertionError:
                continue
            break
        else:
            raise AssertionError("no draw of sample %d keeps the margins" % b)
        case["props"].append(props), case["prop_labels"].append(prop_labels)
        case["gt"].append(gt), case["gt_labels"].append(gt_labels)
    return case


def make_keys(seed, count, equal=False):
    """float32 keys in [0, 1): pairwise distinct, or (equal=True) drawn from four values."""
    rng = np.random.RandomState(seed)
    if equal:
        return (rng.randint(0, 4, count) / 4.0).astype(F32)
    keys = rng.permutation(max(count, 1) * 4)[:count].astype(np.float64) / (max(count, 1) * 4)
    keys = keys.astype(F32)
    assert len(np.unique(keys)) == count
    return keys


def assert_nms_margins(boxes, probs, score_thr, nms_thr, rotate):
    """What makes multi-class NMS well defined: per class, the scores of the candidates at or
    above its score_thr are pairwise distinct and none lies within 1e-6 of the threshold, and no
    pair of their BEV boxes has an IoU within MARGIN of nms_thr.  boxes [n, 7], probs [n, C]."""
    import iou3d_ref as IR
    boxes, probs = np.asarray(boxes, F32), np.asarray(probs, F32)
    classes = probs.shape[1]
    score_thr = list(score_thr) if isinstance(score_thr, (list, tuple)) else [score_thr] * classes
    half = boxes[:, 3:5] / 2
    xyxyr = np.concatenate([boxes[:, :2] - half, boxes[:, :2] + half, boxes[:, 6:7]], 1)
    for k in range(classes):
        assert (np.abs(probs[:, k] - score_thr[k]) > 1e-6).all(), "a score on score_thr"
        rows = np.nonzero(probs[:, k] >= score_thr[k])[0]
        assert len(np.unique(probs[rows, k])) == len(rows), "equal NMS scores"
        if len(rows) < 2:
            continue
        iou = IR.iou_bev(xyxyr[rows], xyxyr[rows], np.float64) if rotate else \
            IR.iou_normal(xyxyr[rows, :4], xyxyr[rows, :4]).astype(np.float64)
        assert (np.abs(iou - nms_thr) > MARGIN).all(), "a pair IoU within the margin of nms_thr"


# ------------------------------------------------------------------ sampler laws
def counts_of(gt_inds, overlaps, thrs):
    neg = gt_inds == 0
    pieces = []
    for k, hi in enumerate(thrs):
        lo = 0.0 if k == len(thrs) - 1 else thrs[k + 1]
        pieces.append(int((neg & (overlaps >= F32(lo)) & (overlaps < F32(hi))).sum()))
    return int((gt_inds > 0).sum()), pieces, int(neg.sum()) - sum(pieces)


SAMPLER_LAWS = [
    # num, pos_fraction, fractions, thrs, ub, (#pos, #piece0, #piece1[, #piece2], #outside)
    (16, 0.55, [0.8, 0.2], [0.55, 0.1], -1, (20, 30, 30, 0)),    # positives above the quota
    (16, 0.55, [0.8, 0.2], [0.55, 0.1], -1, (3, 30, 30, 0)),     # below
    (16, 0.55, [0.8, 0.2], [0.55, 0.1], -1, (3, 2, 30, 0)),      # piece 0 under-full: extend_num
    (16, 0.55, [0.8, 0.2], [0.55, 0.1], -1, (3, 30, 1, 0)),      # the last piece under-full
    (16, 0.55, [0.8, 0.2], [0.55, 0.1], -1, (3, 4, 3, 2)),       # all negatives fewer than expected
    (16, 0.55, [0.8, 0.2], [0.55, 0.1], 2, (2, 30, 30, 0)),      # neg_pos_ub binds
    (16, 0.55, [0.8, 0.2], [0.55, 0.1], 2, (0, 30, 30, 0)),      # ... with max(1, 0) positives
    (1, 0.55, [0.8, 0.2], [0.55, 0.1], -1, (5, 9, 9, 0)),        # num 1: no positive is expected
    (128, 0.55, [0.8, 0.2], [0.55, 0.1], -1, (90, 200, 200, 5)),
    (16, 0.55, [1.0], [0.55], -1, (3, 40, 0)),                   # one piece
    (16, 0.55, [1.0], [0.4], -1, (3, 5, 30)),                    # ... most negatives outside it
    (32, 0.3, [0.5, 0.3, 0.2], [0.55, 0.3, 0.1], -1, (4, 3, 40, 40, 0)),   # three pieces
    (32, 0.3, [0.5, 0.3, 0.2], [0.55, 0.3, 0.1], -1, (4, 40, 2, 40, 0)),
    (32, 0.3, [0.5, 0.3, 0.2], [0.55, 0.3, 0.1], -1, (4, 40, 40, 1, 0)),
]


def law_inputs(law, seed):
    """gt_inds / max_overlaps realising the category counts of a law, shuffled."""
    num, pos_fraction, fractions, thrs, ub, counts = law
    rng = np.random.RandomState(seed)
    inds, ov = [], []
    inds += [1] * counts[0]
    ov += list(rng.uniform(0.6, 0.9, counts[0]))
    for k, hi in enumerate(thrs):
        lo = 0.0 if k == len(thrs) - 1 else thrs[k + 1]
        inds += [0] * counts[1 + k]
        ov += list(rng.uniform(lo + 0.01, hi - 0.01, counts[1 + k]))
    inds += [0] * counts[-1]
    ov += list(rng.uniform(thrs[0] + 0.01, 0.99, counts[-1]))
    inds += [-1] * 7                                      # ignored rows take part in nothing
    ov += list(rng.uniform(0.0, 1.0, 7))
    order = rng.permutation(len(inds))
    return np.asarray(inds, np.int64)[order], np.asarray(ov, np.float32)[order]



# ------------------------------------------------------------------ restatements (numpy)
def assign_ref(iou, mask, prop_labels, gt_labels, classes, single, thr=THR):
    """Class-aware MaxIoUAssigner on a masked float32 IoU matrix, in the merged convention.
    -> gt_inds [P] (int64), max_overlaps [P] (float32), labels [P]."""
    p, g = iou.shape
    gt_inds = np.zeros(p, np.int64)
    overlaps = np.zeros(p, F32)
    labels = np.full(p, -1, np.int64)
    groups = [None] if single else range(classes)
    for c in groups:
        rows = np.arange(p) if single else np.nonzero(prop_labels == c)[0]
        cols = np.arange(g) if single else np.nonzero(gt_labels == c)[0]
        if rows.size == 0:
            continue
        if cols.size == 0:
            gt_inds[rows], overlaps[rows], labels[rows] = 0, 0, -1
            continue
        sub = iou[np.ix_(rows, cols)]
        best, arg = sub.max(1), sub.argmax(1)              # argmax: the lowest index on ties
        res = np.full(rows.size, -1, np.int64)
        res[(best >= 0) & (best < F32(thr["neg"]))] = 0
        res[best >= F32(thr["pos"])] = arg[best >= F32(thr["pos"])] + 1
        gmax = sub.max(0)
        for j in range(cols.size):
            if gmax[j] >= F32(thr["min_pos"]):
                res[sub[:, j] == gmax[j]] = j + 1
        gt_inds[rows] = np.where(res > 0, cols[np.clip(res - 1, 0, None)] + 1, res)
        overlaps[rows] = best
        labels[rows] = np.where(res > 0, gt_labels[cols[np.clip(res - 1, 0, None)]], -1)
    return gt_inds, overlaps, labels


def quotas_ref(n_pos_all, piece_counts, outside, num, pos_fraction, fractions, neg_pos_ub=-1):
    """The sampler's counts from the category counts: -> (n_pos, per-piece taken, outside taken).
    piece_counts: negatives per piece; outside: negatives no piece holds."""
    expected_pos = int(num * pos_fraction)
    n_pos = min(n_pos_all, expected_pos)
    expected_neg = num - n_pos
    if neg_pos_ub >= 0:
        expected_neg = min(expected_neg, int(neg_pos_ub * max(1, n_pos)))
    if sum(piece_counts) + outside <= expected_neg:
        return n_pos, list(piece_counts), outside
    taken, extend = [], 0
    for k, have in enumerate(piece_counts):
        want = expected_neg - sum(taken) if k == len(piece_counts) - 1 \
            else int(expected_neg * fractions[k]) + extend
        if have < want:
            taken.append(have)
            extend += want - have
        else:
            taken.append(want)
            extend = 0
    return n_pos, taken, 0


def bbox_targets_ref(rois, gts):
    """parta2_bbox_head.py:428-453 in float64: positive RoIs [n, 7] and their ground truths
    [n, 7] -> targets [n, 7]."""
    rois, ct = np.asarray(rois, np.float64), np.asarray(gts, np.float64).copy()
    two_pi = 2 * np.pi
    roi_ry = np.mod(rois[:, 6], two_pi)
    ct[:, 0:3] -= rois[:, 0:3]
    ct[:, 6] -= roi_ry
    angle = -(roi_ry + np.pi / 2)
    c, s = np.cos(angle), np.sin(angle)
    x, y = ct[:, 0].copy(), ct[:, 1].copy()
    ct[:, 0], ct[:, 1] = x * c + y * s, -x * s + y * c
    ry = np.mod(ct[:, 6], two_pi)
    opposite = (ry > np.pi * 0.5) & (ry < np.pi * 1.5)
    ry[opposite] = np.mod(ry[opposite] + np.pi, two_pi)
    ry[ry > np.pi] -= two_pi
    ry = np.clip(ry, -np.pi / 2, np.pi / 2)
    wa, la, ha = rois[:, 3], rois[:, 4], rois[:, 5]
    diagonal = np.sqrt(la**2 + wa**2)
    return np.stack([ct[:, 0] / diagonal, ct[:, 1] / diagonal,
                     (ct[:, 2] + ct[:, 5] / 2 - ha / 2) / ha, np.log(ct[:, 3] / wa),
                     np.log(ct[:, 4] / la), np.log(ct[:, 5] / ha), ry], 1)


# ------------------------------------------------------------------ PartA2BboxHead restated
def pooled_features(seed, rois, size, seg_channels=16, part_channels=4, fill=0.35):
    """Pooled RoI features [R, size, size, size, C] (float32 numpy): a cell is active with
    probability `fill` (every RoI keeps at least one); active cells carry positive part
    features -- so "sum != 0" does not hang on a summation order -- and signed seg features."""
    rng = np.random.RandomState(seed)
    active = rng.uniform(size=(rois, size, size, size)) < fill
    active[:, 0, 0, 0] = True
    part = rng.uniform(0.05, 1.0, (rois, size, size, size, part_channels)) * active[..., None]
    seg = rng.normal(size=(rois, size, size, size, seg_channels)) * active[..., None]
    assert (part >= 0).all() and ((part.sum(-1) != 0) == active).all()
    return seg.astype(F32), part.astype(F32)


class DenseBboxHead:
    """PartA2BboxHead.forward and the reference's loss (parta2_bbox_head.py:233-354) restated
    on dense tensors in any dtype, on the CPU: a SubM conv is a dense conv3d evaluated at the
    active sites, BatchNorm runs over the active rows only (batch statistics in train mode),
    the 2x2x2 max-pool takes the active inputs of a window (they follow a ReLU, so from 0).
    The twin owns a deep copy of the head's parameters: gradients are compared by name."""

    def __init__(self, head, dtype):
        import copy
        import torch
        self.torch, self.dtype = torch, dtype
        self.head = copy.deepcopy(head).cpu().to(dtype)
        self.head.train(head.training)

    def _module(self, block, x, mask):
        """One make_sparse_convmodule: SubM conv, BatchNorm1d over the active rows, ReLU."""
        torch = self.torch
        conv, norm = block[0], block[1]
        y = torch.nn.functional.conv3d(x, conv.weight.permute(0, 4, 1, 2, 3), padding=1) * mask
        count = mask.sum()
        shape = (1, -1, 1, 1, 1)
        if norm.training:
            mean = y.sum((0, 2, 3, 4)) / count
            var = (((y - mean.view(shape)) * mask) ** 2).sum((0, 2, 3, 4)) / count
        else:
            mean, var = norm.running_mean, norm.running_var
        y = (y - mean.view(shape)) / torch.sqrt(var.view(shape) + norm.eps)
        y = y * norm.weight.view(shape) + norm.bias.view(shape)
        return torch.relu(y) * mask

    def _stack(self, blocks, x, mask):
        for block in blocks:
            x = self._module(block, x, mask)
        return x

    def forward(self, seg_feats, part_feats):
        torch, h = self.torch, self.head
        part = torch.as_tensor(part_feats).to(self.dtype)
        seg = torch.as_tensor(seg_feats).to(self.dtype)
        mask = (part.sum(-1) != 0).to(self.dtype)[:, None]                  # [R, 1, X, Y, Z]
        x_part = self._stack(h.part_conv, part.permute(0, 4, 1, 2, 3) * mask, mask)
        x_seg = self._stack(h.seg_conv, seg.permute(0, 4, 1, 2, 3) * mask, mask)
        x = torch.cat((x_seg, x_part), dim=1)
        x = self._stack(h.conv_down.merge_conv, x, mask)
        x = torch.nn.functional.max_pool3d(x, 2, 2)
        mask = torch.nn.functional.max_pool3d(mask, 2, 2)
        x = self._stack(h.conv_down.down_conv, x, mask)
        shared = h.shared_fc(x.reshape(x.shape[0], -1, 1))
        cls_score = h.conv_cls(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        bbox_pred = h.conv_reg(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        return cls_score, bbox_pred

    def corners(self, boxes):
        torch = self.torch
        unit = torch.tensor([[-0.5, -0.5, 0], [-0.5, -0.5, 1], [-0.5, 0.5, 1], [-0.5, 0.5, 0],
                             [0.5, -0.5, 0], [0.5, -0.5, 1], [0.5, 0.5, 1], [0.5, 0.5, 0]],
                            dtype=boxes.dtype)
        c = boxes[:, None, 3:6] * unit[None]
        cs, sn = torch.cos(boxes[:, 6])[:, None], torch.sin(boxes[:, 6])[:, None]
        x, y = c[..., 0] * cs + c[..., 1] * sn, -c[..., 0] * sn + c[..., 1] * cs
        return torch.stack([x, y, c[..., 2]], -1) + boxes[:, None, :3]

    def loss(self, cls_score, bbox_pred, rois, labels, bbox_targets, pos_gt_bboxes, reg_mask,
             label_weights, bbox_weights):
        """:283-354 as written (boolean gathers); loss_corner reduced by its mean, which is
        what the detector's loss parser does with the reference's vector."""
        torch, h = self.torch, self.head
        cast = lambda t: torch.as_tensor(t).to(self.dtype)                      # noqa: E731
        rois, labels, bbox_targets, pos_gt_bboxes = map(cast, (rois, labels, bbox_targets,
                                                               pos_gt_bboxes))
        label_weights, bbox_weights = cast(label_weights), cast(bbox_weights)
        losses = dict(loss_cls=h.loss_cls(cls_score.view(-1), labels, label_weights))
        pos_inds = torch.as_tensor(reg_mask) > 0
        if pos_inds.any() == 0:
            zero = cls_score.new_tensor(0)
            return dict(losses, loss_bbox=zero, loss_corner=zero)
        pos_bbox_pred = bbox_pred.view(cls_score.shape[0], -1)[pos_inds]
        weights = bbox_weights[pos_inds].view(-1, 1).repeat(1, pos_bbox_pred.shape[-1])
        losses["loss_bbox"] = h.loss_bbox(pos_bbox_pred.unsqueeze(0), bbox_targets.unsqueeze(0),
                                          weights.unsqueeze(0))
        pos_rois = rois[..., 1:].view(-1, 7)[pos_inds]
        anchors = pos_rois.clone().detach()
        anchors[..., 0:3] = 0
        pred = h.bbox_coder.decode(anchors, pos_bbox_pred.view(-1, 7)).view(-1, 7)
        angle = pos_rois[..., 6] + np.pi / 2
        cs, sn = torch.cos(angle), torch.sin(angle)
        centre = torch.stack([pred[:, 0] * cs + pred[:, 1] * sn, -pred[:, 0] * sn + pred[:, 1] * cs,
                              pred[:, 2]], -1) + pos_rois[:, 0:3]
        pred = torch.cat([centre, pred[:, 3:]], -1)
        flip = pos_gt_bboxes.clone()
        flip[:, 6] += np.pi
        a = self.corners(pred)
        dist = torch.min(torch.norm(a - self.corners(pos_gt_bboxes), dim=2),
                         torch.norm(a - self.corners(flip), dim=2))
        quadratic = torch.clamp(dist, max=1)
        losses["loss_corner"] = (0.5 * quadratic**2 + (dist - quadratic)).mean(dim=1).mean()
        return losses
