"""Inputs for the H3DNet cue-target tests and golden vectors.

A case is built so that its discrete outcomes are well defined (tests/h3d_ref.py,
assert_margins) by construction rather than by luck:

  * ground-truth centres sit on a lattice 8 apart with a jitter below 1, sizes are 2 .. 3:
    a proposal's nearest centre is never in doubt;
  * a proposal is a centre plus an offset whose length is drawn from bands that stay 0.05 clear
    of near_threshold and far_threshold;
  * a predicted primitive centre is either a ground-truth cue centre plus an offset from bands
    clear of the mask threshold, or a distractor far from every box;
  * a proposal's own cue centre is the primitive its row selects plus an offset from bands clear
    of the label threshold.

What construction cannot exclude (two cue centres of one box that the rotation quirk turns onto
each other, say) is caught by the margin assertion: make_case asserts it on the float32 and
float64 restatements of its one draw and fails where it does not hold, so every caller's seed is
a fixed one whose draw passes.  Everything is float32 data; the float64 restatement reads the
same numbers."""
import numpy as np
import torch

import h3d_ref as R

CFG = dict(near_threshold=0.3, far_threshold=0.6, label_surface_threshold=0.3,
           label_line_threshold=0.3, mask_surface_threshold=0.3, mask_line_threshold=0.3)
YAWS = (0.3, -1.1, 2.0, 0.75, -2.6, 1.4)
CLEAR = 0.05


def _directions(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _banded(rng, n, bands):
    """n lengths, each uniform in one of `bands` (chosen uniformly)."""
    pick = rng.integers(0, len(bands), size=n)
    lo = np.array([b[0] for b in bands])[pick]
    hi = np.array([b[1] for b in bands])[pick]
    return lo + (hi - lo) * rng.random(n)


def make_boxes(rng, count, with_yaw, cell=0):
    """[count, 7] float32 boxes in gravity-centre form, centres on a lattice 8 apart."""
    slots = rng.permutation(216)[:count] if count <= 216 else np.arange(count)
    grid = np.stack([slots % 6, (slots // 6) % 6, slots // 36], axis=1).astype(np.float64)
    centre = grid * 8.0 + rng.uniform(-0.9, 0.9, size=(count, 3)) + cell
    size = rng.uniform(2.0, 3.0, size=(count, 3))
    yaw = np.array([YAWS[i % len(YAWS)] for i in range(count)]) if with_yaw else np.zeros(count)
    return torch.from_numpy(np.concatenate([centre, size, yaw[:, None]], axis=1)).float()


def _sample(rng, boxes, labels, p, ns, nl, classes, cfg):
    """One sample around `boxes` ([G, 7], G >= 1, the padded zero box of an empty sample
    included).  -> aggregated [P, 3], surface_pred, line_pred, surface_sem, line_sem, cue_obj."""
    g = boxes.shape[0]
    centre = boxes[:, :3].double().numpy()
    near, far = cfg["near_threshold"], cfg["far_threshold"]
    bands = [(0.0, near - CLEAR), (near + CLEAR, far - CLEAR), (far + CLEAR, far + 0.6)]
    owner = rng.integers(0, g, size=p)
    aggregated = centre[owner] + _directions(rng, p) * _banded(rng, p, bands)[:, None]
    aggregated = torch.from_numpy(aggregated).float()

    b64 = boxes.double()
    cues = R.surface_line_center_ref(b64[:, :3], b64[:, 3:6], b64[:, 6])
    preds, sems = [], []
    for targets, n, thr in ((cues[0].numpy(), ns, cfg["mask_surface_threshold"]),
                            (cues[1].numpy(), nl, cfg["mask_line_threshold"])):
        k = targets.shape[0] // g
        which = rng.permutation(targets.shape[0])[:max(1, (2 * n) // 3)]
        which = which[:n]
        close = targets[which] + _directions(rng, len(which)) * _banded(
            rng, len(which), [(0.0, thr - CLEAR), (thr + CLEAR, thr + 0.25)])[:, None]
        away = rng.uniform(-400.0, -200.0, size=(n - len(which), 3))
        order = rng.permutation(n)
        preds.append(torch.from_numpy(np.concatenate([close, away])[order]).float())
        score = rng.normal(size=(n, classes))
        hit = rng.random(len(which)) < 0.6          # these primitives vote for their box's class
        score[np.arange(len(which))[hit], labels.numpy()[which // k][hit]] += 8.0
        sems.append(torch.from_numpy(score[order]).float())

    # the proposal's own cue centres: around the primitive each row selects
    dtype = torch.float64
    assign = R.first_min(R.sq_dist(aggregated.double(), b64[:, :3]))[1]
    own = []
    for cue, pred, k, thr in ((cues[0], preds[0], 6, cfg["label_surface_threshold"]),
                              (cues[1], preds[1], 12, cfg["label_line_threshold"])):
        rows = cue.reshape(-1, k, 3).transpose(0, 1)[:, assign].reshape(-1, 3)
        sel = pred.to(dtype)[R.first_min(R.sq_dist(rows, pred.to(dtype)))[1]].numpy()
        m = sel.shape[0]
        own.append(sel + _directions(rng, m) * _banded(
            rng, m, [(0.0, thr - CLEAR), (thr + CLEAR, thr + 0.4)])[:, None])
    cue_obj = torch.from_numpy(np.concatenate(own)).float()
    return aggregated, preds[0], preds[1], sems[0], sems[1], cue_obj


def draw_case(seed, counts, p, ns, nl, classes=18, with_yaw=True, cfg=CFG):
    rng = np.random.default_rng(seed)
    gt_boxes = [make_boxes(rng, c, with_yaw) if c else torch.zeros((0, 7)) for c in counts]
    gt_labels = [torch.from_numpy(rng.integers(0, classes, size=c)).long() for c in counts]
    padded = R.pad_empty(gt_boxes, gt_labels)
    cols = [_sample(rng, b, l, p, ns, nl, classes, cfg) for b, l in zip(*padded)]
    names = ("aggregated", "surface_pred", "line_pred", "surface_sem", "line_sem", "cue_obj")
    case = {n: torch.stack(c).contiguous() for n, c in zip(names, zip(*cols))}
    case.update(gt_boxes=gt_boxes, gt_labels=gt_labels, with_yaw=with_yaw, classes=classes)
    return case


def reference(case, cfg=CFG, margins=True):
    """-> (float32 results, float64 results) of the restated loop, the margins asserted."""
    t32, t64 = R.Trace(), R.Trace()
    r32 = R.batch_cue_targets_ref(case, cfg, torch.float32, t32)
    r64 = R.batch_cue_targets_ref(case, cfg, torch.float64, t64)
    if margins:
        R.assert_margins(t32, t64)
        for name, a, b in zip(R.DISCRETE, r32, r64):
            assert torch.equal(a.double(), b.double()), name
    return r32, r64


def make_case(seed, counts, p, ns, nl, classes=18, with_yaw=True, cfg=CFG):
    """draw_case, with the margins asserted on the draw: a seed whose draw violates them is a
    failure, not something to step over.  The callers' seeds are fixed."""
    case = draw_case(seed, counts, p, ns, nl, classes, with_yaw, cfg)
    reference(case, cfg)
    return case
