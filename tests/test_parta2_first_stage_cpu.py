"""Part-A2's first stage without a GPU (COVERAGE n9): PointwiseSemanticHead and PartA2RPNHead
against tests/golden/parta2_first_stage_vectors.npz, which the reference's own classes produced
on the CPU (tests/golden/make_parta2_first_stage_golden.py).

The only tolerance is the project's usual one: 4 x the reference's own float32 error against its
float64 run, measured from the golden's two recordings, with a floor of one float32 ulp at the
magnitude of the values (np.finfo(float32).eps * max(1, max |value|)) -- below that a float32
result cannot be told from the float64 one.

points_in_boxes needs a GPU in this package (test_ssd3d_head_cpu.py pins that), so the
composition path of get_targets runs here with LiDARBoxes.points_in_boxes served by the numpy
predicate of tests/roiaware_ref.py, the stand-in the golden script gave the reference.
"""
import copy
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parta2_cases as PC  # noqa: E402
import roiaware_ref as RR  # noqa: E402

from msmdfusion_amd import configs as C  # noqa: E402
from msmdfusion_amd import registry  # noqa: E402
from msmdfusion_amd.head_loss import LiDARBoxes  # noqa: E402
from msmdfusion_amd.parta2_rpn_head import PartA2RPNHead  # noqa: E402
from msmdfusion_amd.semantic_head import PointwiseSemanticHead, voxel_centers  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = float(np.finfo(np.float32).eps)
SEM_CASES = {"b2": 2, "b1": 1, "empty": 2, "nopos": 2}
RPN_CFGS = ("train", "test", "quirk", "none")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "parta2_first_stage_vectors.npz")))


def bound(ref32, ref64, unit=False):
    """4 x the reference's float32 error against float64, floored at one float32 ulp at the
    values' magnitude (unit: at 1.0, the part targets' floor)."""
    ref32, ref64 = np.asarray(ref32, np.float64), np.asarray(ref64, np.float64)
    err = float(np.abs(ref32 - ref64).max()) if ref32.size else 0.0
    scale = max(1.0, float(np.abs(ref64).max())) if ref64.size and not unit else 1.0
    return 4.0 * err + EPS * scale


def close(got, ref32, ref64, what, unit=False):
    got = np.asarray(got, np.float64)
    assert got.shape == np.asarray(ref64).shape, what
    if got.size:
        worst = float(np.abs(got - np.asarray(ref64, np.float64)).max())
        limit = bound(ref32, ref64, unit)
        assert worst <= limit, "%s: %.3e > %.3e" % (what, worst, limit)


def semantic_head(gold, dtype=torch.float32, **kw):
    head = PointwiseSemanticHead(in_channels=16, num_classes=3, **kw)
    head.load_state_dict({k: torch.from_numpy(gold["sem_weight_" + k])
                          for k in gold["sem_state_keys"]})
    return head.to(dtype)


def semantic_inputs(gold, tag, device="cpu"):
    p = "sem_%s_" % tag
    n = gold[p + "centres"].shape[0]
    coors = np.zeros((n, 4), np.int32)
    coors[:, 0] = gold[p + "ids"]
    voxels_dict = dict(coors=torch.from_numpy(coors).to(device),
                       voxel_centers=torch.from_numpy(gold[p + "centres"]).to(device))
    boxes = [LiDARBoxes(torch.from_numpy(gold[p + "boxes_%d" % b]).reshape(-1, 7))
             for b in range(SEM_CASES[tag])]
    labels = [torch.from_numpy(gold[p + "labels_%d" % b]) for b in range(SEM_CASES[tag])]
    return voxels_dict, boxes, labels


def single64(gold, tag):
    p = "sem_%s_" % tag
    return (np.concatenate([gold[p + "single64_seg_%d" % b] for b in range(SEM_CASES[tag])]),
            np.concatenate([gold[p + "single64_part_%d" % b] for b in range(SEM_CASES[tag])]))


@pytest.fixture
def numpy_points_in_boxes(monkeypatch):
    def points_in_boxes(self, points):
        first = RR.points_in_boxes_first(points.detach().float().numpy()[None],
                                         self.tensor[:, :7].numpy()[None])[0]
        return torch.from_numpy(first.astype(np.int32))
    monkeypatch.setattr(LiDARBoxes, "points_in_boxes", points_in_boxes)


# ----------------------------------------------------------------------------- semantic head
@pytest.mark.parametrize("tag", sorted(SEM_CASES))
def test_composed_targets_match_the_reference(gold, tag, numpy_points_in_boxes):
    head = semantic_head(gold, fused=False)
    voxels_dict, boxes, labels = semantic_inputs(gold, tag)
    kept = [b.tensor.clone() for b in boxes], [l.clone() for l in labels]
    targets = head.get_targets(voxels_dict, boxes, labels)
    p = "sem_%s_" % tag
    seg64, part64 = single64(gold, tag)
    assert np.array_equal(gold[p + "seg_targets"], seg64)        # the golden's own two runs agree
    assert targets["seg_targets"].dtype == torch.long
    assert np.array_equal(targets["seg_targets"].numpy(), gold[p + "seg_targets"])
    assert targets["part_targets"].dtype == torch.float32
    close(targets["part_targets"].numpy(), gold[p + "part_targets"], part64, tag + " part",
          unit=True)
    for b, l, kb, kl in zip(boxes, labels, *kept):                # the lists are left untouched
        assert torch.equal(b.tensor, kb) and torch.equal(l, kl)
    # the case holds what it is for
    seg = gold[p + "seg_targets"]
    if tag == "nopos":
        assert ((seg == 3)).all()
    else:
        assert (seg == -1).any() and (seg == 3).any() and ((seg >= 0) & (seg < 3)).any()


@pytest.mark.parametrize("tag", sorted(SEM_CASES))
def test_get_targets_single_in_float64(gold, tag, numpy_points_in_boxes):
    head = semantic_head(gold, fused=False)
    _, boxes, labels = semantic_inputs(gold, tag)
    p = "sem_%s_" % tag
    for b in range(SEM_CASES[tag]):
        rows = torch.from_numpy(gold[p + "centres"][gold[p + "ids"] == b]).double()
        seg, part = head.get_targets_single(rows, boxes[b], labels[b])
        assert np.array_equal(seg.numpy(), gold[p + "single64_seg_%d" % b])
        assert part.dtype == torch.float64
        ref = gold[p + "single64_part_%d" % b]
        assert np.abs(part.numpy() - ref).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(ref).max(
            initial=0.0))


@pytest.mark.parametrize("tag", sorted(SEM_CASES))
def test_forward_loss_and_gradients_match_the_reference(gold, tag):
    p = "sem_%s_" % tag
    head = semantic_head(gold)
    res = head(torch.from_numpy(gold[p + "x"]))
    for k in ("seg_preds", "part_preds", "part_feats"):
        close(res[k].detach().numpy(), gold[p + "fwd_" + k], gold[p + "fwd64_" + k], tag + " " + k)
    # the zeroing below seg_score_thr and the detach
    below = gold[p + "fwd_part_feats"][:, 3] <= 0.3
    assert below.any() and (res["part_feats"].detach().numpy()[below, :3] == 0).all()
    assert not res["part_feats"].requires_grad
    targets = dict(seg_targets=torch.from_numpy(gold[p + "seg_targets"]),
                   part_targets=torch.from_numpy(gold[p + "part_targets"]))
    losses = head.loss(res, targets)
    assert sorted(losses) == ["loss_part", "loss_seg"]
    (losses["loss_seg"] + losses["loss_part"]).backward()
    for k in ("loss_seg", "loss_part"):
        close(losses[k].detach().numpy(), gold[p + k], gold[p + k + "64"], tag + " " + k)
    for k, prm in head.named_parameters():
        assert torch.isfinite(prm.grad).all()
        close(prm.grad.numpy(), gold[p + "grad_" + k], gold[p + "grad64_" + k], tag + " grad " + k)


def test_a_batch_without_a_positive_row(gold):
    p = "sem_nopos_"
    head = semantic_head(gold)
    res = head(torch.from_numpy(gold[p + "x"]))
    targets = dict(seg_targets=torch.from_numpy(gold[p + "seg_targets"]),
                   part_targets=torch.from_numpy(gold[p + "part_targets"]))
    losses = head.loss(res, targets)
    assert float(losses["loss_part"].detach()) == 0.0 and float(gold[p + "loss_part"]) == 0.0
    (losses["loss_seg"] + losses["loss_part"]).backward()
    for prm in head.parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all()
    assert float(head.seg_reg_layer.weight.grad.abs().max()) == 0.0
    # a NaN part target in a row that is not positive stays out of the sum
    targets["part_targets"] = torch.full_like(targets["part_targets"], float("nan"))
    assert float(head.loss(head(torch.from_numpy(gold[p + "x"])), targets)["loss_part"].detach()) == 0.0


def test_voxel_centers_is_the_literal_formula():
    rs = np.random.RandomState(0)
    zyx = torch.from_numpy(rs.randint(0, 40, (50, 3)).astype(np.int32))
    voxel_size, pc_range = [0.05, 0.05, 0.1], [0, -40, -3, 70.4, 40, 1]
    want = (zyx[:, [2, 1, 0]] + 0.5) * torch.tensor(voxel_size) + torch.tensor(pc_range[0:3])
    got = voxel_centers(zyx, voxel_size, pc_range)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    batched = torch.cat([torch.full((50, 1), 3, dtype=torch.int32), zyx], 1)
    assert torch.equal(voxel_centers(batched, voxel_size, pc_range), want)


def _signature(cls, drop=()):
    params = [q for q in list(inspect.signature(cls.__init__).parameters.values())[1:]
              if q.name not in drop]
    return json.loads(json.dumps([[q.name, "<required>" if q.default is inspect.Parameter.empty
                                   else q.default] for q in params]))


def test_constructors_state_dicts_and_registries(gold):
    assert _signature(PointwiseSemanticHead, drop=("fused",)) == json.loads(str(gold["sem_signature"]))
    rpn_sig = _signature(PartA2RPNHead)
    assert rpn_sig == json.loads(str(gold["rpn_signature"]))
    head = PointwiseSemanticHead(in_channels=16)
    assert (head.extra_width, head.num_classes, head.seg_score_thr) == (0.2, 3, 0.3)
    assert head.fused is True
    assert list(head.state_dict()) == list(gold["sem_state_keys"])
    for k, v in head.state_dict().items():
        assert tuple(v.shape) == gold["sem_weight_" + k].shape, k
    for name in ("seg_cls_layer", "seg_reg_layer", "loss_seg", "loss_part"):
        assert hasattr(head, name)
    assert head.loss_seg.reduction == "sum" and head.loss_part.use_sigmoid

    registry.build_head(dict(type="PointwiseSemanticHead", in_channels=4))     # fills HEADS
    assert registry.HEADS.get("PointwiseSemanticHead") is PointwiseSemanticHead
    assert registry.HEADS.get("PartA2RPNHead") is PartA2RPNHead


def test_configs_match_the_reference_and_build_unmodified():
    fx = json.load(open(os.path.join(GOLDEN, "reference_parta2_configs.json")))
    norm = lambda o: json.loads(json.dumps(o))                                  # noqa: E731
    for cfg, key, classes, anchors in ((C.PARTA2_SECFPN_KITTI_3CLASS, "kitti-3d-3class", 3, 6),
                                       (C.PARTA2_SECFPN_KITTI_CAR, "kitti-3d-car", 1, 2)):
        assert norm(cfg) == fx[key]
        before = copy.deepcopy(cfg)
        model = cfg["model"]
        rpn = registry.build_head(dict(model["rpn_head"], train_cfg=model["train_cfg"]["rpn"],
                                       test_cfg=model["test_cfg"]["rpn"]))
        sem = registry.build_head(model["roi_head"]["semantic_head"])
        assert cfg == before
        assert isinstance(rpn, PartA2RPNHead) and isinstance(sem, PointwiseSemanticHead)
        assert rpn.num_classes == sem.num_classes == classes and rpn.num_anchors == anchors
        assert tuple(rpn.conv_cls.weight.shape) == (anchors * classes, 512, 1, 1)
        assert tuple(sem.seg_cls_layer.weight.shape) == (1, 16)
        # the config's nms_pre fits the NMS kernel's segment bound
        assert rpn._check_nms_bound(model["train_cfg"]["rpn_proposal"], [(200, 176)]) == 9000


# ------------------------------------------------------------------------------------- RPN
def rpn_head(gold, dtype=torch.float32):
    head = PartA2RPNHead(**PC.rpn_head_cfg())
    head.load_state_dict({k: torch.from_numpy(gold["rpn_weight_" + k])
                          for k in gold["rpn_state_keys"]})
    return head.to(dtype)


def test_rpn_state_dict_and_forward(gold):
    head = rpn_head(gold)
    assert list(head.state_dict()) == list(gold["rpn_state_keys"])
    for k, v in head.state_dict().items():
        assert tuple(v.shape) == gold["rpn_weight_" + k].shape, k
    cls, reg, dr = head([torch.from_numpy(gold["rpn_feats"])])
    head64 = rpn_head(gold, torch.float64)
    cls64, reg64, dr64 = head64([torch.from_numpy(gold["rpn_feats"]).double()])
    for got, name, ref64 in ((cls, "cls", cls64), (reg, "bbox", reg64), (dr, "dir", dr64)):
        close(got[0].detach().numpy(), gold["rpn_pred_" + name], ref64[0].detach().numpy(), name)


@pytest.mark.parametrize("tag", RPN_CFGS)
def test_rpn_composition_matches_the_reference(gold, tag):
    """The per-sample loop (tests/parta2_cases.rpn_loop: the head's own generator, coder and
    direction fix around the numpy NMS) against the reference's get_bboxes."""
    head = rpn_head(gold)
    cfg = PC.RPN_CFGS[tag]
    preds = [[torch.from_numpy(gold["rpn_pred_" + k]).clone()] for k in ("cls", "bbox", "dir")]
    if tag == "none":
        preds[0][0][1] -= 30.0
    results = PC.rpn_loop(head, *preds, cfg)
    for i, r in enumerate(results):
        p, p64 = "rpn_%s_s%d_" % (tag, i), "rpn_%s_s%d64_" % (tag, i)
        assert np.array_equal(r["labels_3d"].numpy(), gold[p + "labels_3d"])
        assert r["labels_3d"].dtype == torch.from_numpy(gold[p + "labels_3d"]).dtype
        for k in ("boxes_3d", "scores_3d", "cls_preds"):
            close(r[k].numpy(), gold[p + k], gold[p64 + k], "%s %d %s" % (tag, i, k))
    if tag == "none":
        assert results[1]["labels_3d"].dtype == torch.float32
        assert tuple(results[1]["cls_preds"].shape) == (0, 3)
    if tag == "quirk":
        assert float(results[0]["cls_preds"].min()) < 0          # raw logits
    else:
        assert float(results[0]["cls_preds"].min()) > 0          # post-sigmoid rows


def test_rpn_refuses_an_nms_pre_beyond_the_kernel_bound(gold):
    head = rpn_head(gold)
    with pytest.raises(NotImplementedError):
        head._check_nms_bound(dict(nms_pre=20000), [(8, 6)])
    with pytest.raises(NotImplementedError):
        head._check_nms_bound(dict(nms_pre=-1), [(8, 6)])


# ----------------------------------------------------------------------------------- C ABI
def test_c_abi_refusals():
    import ctypes
    from msmdfusion_amd._lib import lib
    assert lib.msmd_semantic_gt_chunk() == 64
    fn = lib.msmd_semantic_targets_f32
    p = ctypes.c_void_p(256)                 # (never dereferenced: every call is refused)
    INVALID, RANGE = -1, -5
    ok = [p, p, p, p, p, 1, p, 10, 2, 4, 3, p, p, None]

    def call(**kw):
        names = ("centers", "ids", "gt", "big", "labels", "is64", "counts", "n", "batch", "g",
                 "classes", "seg", "part", "stream")
        args = dict(zip(names, ok))
        args.update(kw)
        return fn(*[args[k] for k in names])

    for name in ("centers", "ids", "gt", "big", "labels", "counts", "seg", "part"):
        assert call(**{name: None}) == INVALID, name
    assert call(n=-1) == INVALID and call(batch=-1) == INVALID and call(g=-1) == INVALID
    assert call(classes=0) == INVALID and call(is64=2) == INVALID
    assert call(batch=1 << 20, g=1 << 12) == RANGE
    assert call(n=0, centers=None, ids=None, seg=None, part=None) == 0       # nothing to do
    assert call(n=0, classes=0) == INVALID                                    # still validated
