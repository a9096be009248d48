"""H3DNet's second stage restated in plain torch, for float32 and float64:

    surface_line_center_ref   DepthInstance3DBoxes.get_surface_line_center
                              (core/bbox/structures/depth_box3d.py:277-330), op for op, with its
                              rotation quirk (row r is turned by the yaw of box r % n)
    cue_targets_single_ref    H3DBboxHead.get_targets_single
                              (models/roi_heads/bbox_heads/h3d_bbox_head.py:761-932)
    batch_cue_targets_ref     get_targets (:655-759): the empty-sample padding and the stack

torch.min / torch.argmax are written out (first_min): the lowest index among equal minima, and
the first NaN wins.  A Trace records every distance that is compared with a threshold and every
nearest / second-nearest pair; assert_margins is the condition under which the discrete outputs
are well defined, and every generated case must pass it."""
import torch

THRESHOLDS = ("near_threshold", "far_threshold", "label_surface_threshold",
              "label_line_threshold", "mask_surface_threshold", "mask_line_threshold")
TARGET_NAMES = ("cues_objectness_label", "cues_sem_label", "proposal_objectness_label",
                "cues_mask", "cues_match_mask", "proposal_objectness_mask",
                "cues_matching_label", "obj_surface_line_center")
DISCRETE = TARGET_NAMES[:7]
THRESHOLD_MARGIN, GAP_MARGIN = 1e-3, 1e-4
MASKED_ASSIGNMENTS = 7       # per sample, as in the reference: each is a nonzero, a host read


class Trace:
    def __init__(self):
        self.compared = []      # (what, distances, threshold)
        self.gaps = []          # (what, nearest, second nearest) squared distances


def first_min(d):
    """d [n, m] -> (values [n], indices [n]) of torch.min(d, dim=1) with its rule spelled out:
    the lowest index among the minima; a NaN is smaller than everything, the first one wins."""
    m = d.shape[1]
    nan = torch.isnan(d)
    low = torch.where(nan, torch.full_like(d, float("inf")), d).min(dim=1, keepdim=True)[0]
    hit = torch.where(nan.any(dim=1, keepdim=True), nan, d == low)
    idx = torch.where(hit, torch.arange(m, device=d.device).expand_as(d),
                      torch.full(d.shape, m, device=d.device)).min(dim=1)[0]
    return torch.gather(d, 1, idx[:, None])[:, 0], idx


def first_argmax(scores):
    """torch.argmax(scores, dim=1): the lowest index among the maxima, a NaN is a maximum."""
    return first_min(-scores)[1]


def sq_dist(a, b):
    """chamfer_distance's l2 matrix (chamfer_distance.py:50-55): [n, 3], [m, 3] -> [n, m]."""
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def _second(d, idx, ref_points):
    """The smallest entry of each row of d that belongs to a point which is no exact copy of
    the chosen one (inf where there is none)."""
    chosen = ref_points[idx]                                              # [n, 3]
    copy = (ref_points[None, :, :] == chosen[:, None, :]).all(-1)         # [n, m]
    return torch.where(copy, torch.full_like(d, float("inf")), d).min(dim=1)[0]


def surface_line_center_ref(center, dims, yaw):
    """gravity centres [n, 3], sizes [n, 3], yaws [n] -> ([n * 6, 3], [n * 12, 3])."""
    n = center.shape[0]
    center = center.view(-1, 1, 3)
    rot_sin, rot_cos = torch.sin(-yaw), torch.cos(-yaw)
    rot_mat_t = yaw.new_zeros((n, 3, 3))
    rot_mat_t[..., 0, 0] = rot_cos
    rot_mat_t[..., 0, 1] = -rot_sin
    rot_mat_t[..., 1, 0] = rot_sin
    rot_mat_t[..., 1, 1] = rot_cos
    rot_mat_t[..., 2, 2] = 1
    out = []
    for offset in ([[0, 0, 1], [0, 0, -1], [0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0]],
                   [[1, 0, 1], [-1, 0, 1], [0, 1, 1], [0, -1, 1], [1, 0, -1], [-1, 0, -1],
                    [0, 1, -1], [0, -1, -1], [1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0]]):
        k = len(offset)
        offset = torch.tensor(offset, dtype=dims.dtype, device=dims.device).view(1, k, 3) / 2
        local = (offset * dims.reshape(n, 1, 3).repeat(1, k, 1)).reshape(-1, 3)
        rot = rot_mat_t.repeat(k, 1, 1)
        local = torch.matmul(local.unsqueeze(-2), rot.transpose(2, 1)).squeeze(-2)
        out.append(center.repeat(1, k, 1).reshape(-1, 3) + local)
    return out[0], out[1]


def cue_targets_single_ref(aggregated, gt_boxes, gt_labels, surface_pred, line_pred, surface_obj,
                           line_obj, surface_sem, line_sem, cfg, dtype, trace=None):
    """One sample.  gt_boxes [G, 7] = (gravity centre, sizes, yaw), G >= 1; the rest as
    get_targets_single takes them.  Floats are raised to `dtype` first.  -> TARGET_NAMES."""
    aggregated, gt_boxes, surface_pred, line_pred, surface_obj, line_obj = [
        t.to(dtype) for t in (aggregated, gt_boxes, surface_pred, line_pred, surface_obj,
                              line_obj)]
    p, dev = aggregated.shape[0], aggregated.device
    gt_center = gt_boxes[:, :3]
    d = sq_dist(aggregated, gt_center)
    dist1, assignment = first_min(d)
    euclid1 = torch.sqrt(dist1 + 1e-6)
    gt_sem = gt_labels[assignment]

    obj_surface, obj_line = surface_line_center_ref(gt_center, gt_boxes[:, 3:6], gt_boxes[:, 6])
    obj_surface = obj_surface.reshape(-1, 6, 3).transpose(0, 1)[:, assignment].reshape(-1, 3)
    obj_line = obj_line.reshape(-1, 12, 3).transpose(0, 1)[:, assignment].reshape(-1, 3)

    surface_cls = first_argmax(surface_sem).float()
    line_cls = first_argmax(line_sem).float()
    ds = sq_dist(obj_surface, surface_pred)
    dl = sq_dist(obj_line, line_pred)
    dist_surface, surface_ind = first_min(ds)
    dist_line, line_ind = first_min(dl)
    surface_sel, line_sel = surface_pred[surface_ind], line_pred[line_ind]
    surface_sel_sem, line_sel_sem = surface_cls[surface_ind], line_cls[line_ind]
    surface_sel_sem_gt, line_sel_sem_gt = gt_sem.repeat(6).float(), gt_sem.repeat(12).float()

    euclid_surface = torch.sqrt(dist_surface + 1e-6)
    euclid_line = torch.sqrt(dist_line + 1e-6)
    euclid_obj_surface = torch.sqrt(((surface_obj - surface_sel) ** 2).sum(dim=-1) + 1e-6)
    euclid_obj_line = torch.sqrt(torch.sum((line_obj - line_sel) ** 2, dim=-1) + 1e-6)

    if trace is not None:
        trace.compared += [("near", euclid1, cfg["near_threshold"]),
                           ("far", euclid1, cfg["far_threshold"]),
                           ("label_surface", euclid_obj_surface, cfg["label_surface_threshold"]),
                           ("mask_surface", euclid_surface, cfg["mask_surface_threshold"]),
                           ("label_line", euclid_obj_line, cfg["label_line_threshold"]),
                           ("mask_line", euclid_line, cfg["mask_line_threshold"])]
        trace.gaps += [("gt", dist1, _second(d, assignment, gt_center)),
                       ("surface", dist_surface, _second(ds, surface_ind, surface_pred)),
                       ("line", dist_line, _second(dl, line_ind, line_pred))]

    proposal_label = torch.zeros(p, dtype=torch.long, device=dev)
    proposal_mask = torch.zeros(p, dtype=dtype, device=dev)
    proposal_label[euclid1 < cfg["near_threshold"]] = 1
    proposal_mask[euclid1 < cfg["near_threshold"]] = 1
    proposal_mask[euclid1 > cfg["far_threshold"]] = 1

    label_surface = torch.zeros(p * 6, dtype=torch.long, device=dev)
    label_line = torch.zeros(p * 12, dtype=torch.long, device=dev)
    label_surface_sem = torch.zeros(p * 6, dtype=torch.long, device=dev)
    label_line_sem = torch.zeros(p * 12, dtype=torch.long, device=dev)
    on_surface = (euclid_obj_surface < cfg["label_surface_threshold"]) * \
        (euclid_surface < cfg["mask_surface_threshold"])
    on_line = (euclid_obj_line < cfg["label_line_threshold"]) * \
        (euclid_line < cfg["mask_line_threshold"])
    label_surface[on_surface] = 1
    label_surface_sem[on_surface * (surface_sel_sem == surface_sel_sem_gt)] = 1
    label_line[on_line] = 1
    label_line_sem[on_line * (line_sel_sem == line_sel_sem_gt)] = 1

    cues_objectness_label = torch.cat((label_surface, label_line), 0)
    cues_sem_label = torch.cat((label_surface_sem, label_line_sem), 0)
    cues_mask = torch.cat((proposal_mask.repeat(6), proposal_mask.repeat(12)), 0)
    label_surface *= proposal_label.repeat(6)
    label_line *= proposal_label.repeat(12)
    cues_matching_label = torch.cat((label_surface, label_line), 0)
    cues_match_mask = (torch.sum(cues_objectness_label.view(18, p), dim=0) >= 1).to(dtype)
    obj_surface_line_center = torch.cat((obj_surface, obj_line), 0)
    return (cues_objectness_label, cues_sem_label, proposal_label, cues_mask, cues_match_mask,
            proposal_mask, cues_matching_label, obj_surface_line_center)


def pad_empty(gt_boxes, gt_labels):
    """get_targets :685-698 on copies: an empty sample becomes one zero box with label 0."""
    boxes, labels = [], []
    for b, l in zip(gt_boxes, gt_labels):
        if len(l) == 0:
            b, l = b.new_zeros((1, b.shape[-1])), l.new_zeros(1)
        boxes.append(b)
        labels.append(l)
    return boxes, labels


def batch_cue_targets_ref(sample, cfg, dtype, trace=None):
    """sample: the dictionary of tests/h3d_cases.py (batched tensors, lists of ground truths in
    gravity-centre form).  -> TARGET_NAMES, stacked over the batch."""
    boxes, labels = pad_empty(sample["gt_boxes"], sample["gt_labels"])
    p = sample["aggregated"].shape[1]
    rows = []
    for b in range(len(boxes)):
        rows.append(cue_targets_single_ref(
            sample["aggregated"][b], boxes[b], labels[b], sample["surface_pred"][b],
            sample["line_pred"][b], sample["cue_obj"][b, :6 * p], sample["cue_obj"][b, 6 * p:],
            sample["surface_sem"][b], sample["line_sem"][b], cfg, dtype, trace))
    return tuple(torch.stack(col) for col in zip(*rows))


def assert_margins(t32, t64):
    """The discrete outcomes are well defined: no compared distance within 1e-3 of its threshold
    in float64 (and on the same side in float32), and the nearest and the second-nearest squared
    distance at least 1e-4 apart, relative -- exact copies of the chosen point excepted."""
    assert len(t32.compared) == len(t64.compared) and len(t32.gaps) == len(t64.gaps)
    for (what, d32, thr), (_, d64, _) in zip(t32.compared, t64.compared):
        assert not torch.isnan(d64).any(), what
        away = (d64 - thr).abs()
        assert float(away.min()) >= THRESHOLD_MARGIN, (what, float(away.min()))
        assert torch.equal(d32 < thr, d64 < thr) and torch.equal(d32 > thr, d64 > thr), what
    for (what, _, _), (_, near, second) in zip(t32.gaps, t64.gaps):
        finite = torch.isfinite(second)
        rel = (second[finite] - near[finite]) / second[finite].clamp_min(1e-30)
        if rel.numel():
            assert float(rel.min()) >= GAP_MARGIN, (what, float(rel.min()))
