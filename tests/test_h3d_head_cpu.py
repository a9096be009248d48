"""H3DNet's second stage without a GPU: the restatement of tests/h3d_ref.py and the plain-torch
DepthBoxes.get_surface_line_center against tests/golden/h3d_bbox_head_vectors.npz (the
reference's own outputs, make_h3d_bbox_head_golden.py), MSELoss on literals, the ground-truth
padding, the host-side refusals of the new C-ABI entry points, H3DBboxHead's state-dict keys and
shapes against the reference's own, the HEADS / DETECTORS entries, configs.H3DNET_SCANNET against
its fixture with the config left untouched by a build, and the refusal of rpn targets that are
neither 13 nor 14."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import h3d_cases as HC  # noqa: E402
import h3d_ref as R  # noqa: E402

CASES = {"yaw": 2, "no_yaw": 2, "single_yaw": 1, "single": 1}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "h3d_bbox_head_vectors.npz")))


def _t(a):
    return torch.from_numpy(np.asarray(a))


def gold_case(gold, name):
    """-> the case dictionary of tests/h3d_cases.py, from the stored inputs."""
    case = {k: _t(gold["%s/%s" % (name, k)]) for k in (
        "aggregated", "surface_pred", "line_pred", "surface_sem", "line_sem", "cue_obj")}
    case["gt_boxes"] = [_t(gold["%s/%d/gravity_boxes" % (name, b)]).reshape(-1, 7)
                        for b in range(CASES[name])]
    case["gt_labels"] = [_t(gold["%s/%d/labels" % (name, b)]).long().reshape(-1)
                         for b in range(CASES[name])]
    return case


def test_the_golden_holds_the_cases_the_issue_names(gold):
    assert [float(v) for v in gold["cfg"]] == [HC.CFG[k] for k in R.THRESHOLDS]
    counts = [gold["%s/%d/labels" % (n, b)].shape[0] for n in CASES for b in range(CASES[n])]
    assert sorted(counts) == [0, 1, 2, 3, 4, 5]
    yaws = np.concatenate([gold["yaw/%d/boxes" % b][:, 6] for b in range(2)])
    assert len(set(np.round(yaws, 3)) - {0.0}) >= 3
    assert not gold["no_yaw/0/boxes"][:, 6].any()
    assert gold["yaw/aggregated"].shape == (2, 16, 3) and gold["yaw/surface_sem"].shape[2] == 18


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_reference(gold, name):
    case = gold_case(gold, name)
    r32, r64 = HC.reference(case)                       # the margins hold on the stored inputs
    for k, key in enumerate(R.TARGET_NAMES):
        g32, g64 = _t(gold["%s/f32/%s" % (name, key)]), _t(gold["%s/f64/%s" % (name, key)])
        if key in R.DISCRETE:
            assert r32[k].dtype == g32.dtype, key
            assert torch.equal(r32[k], g32) and torch.equal(r64[k].double(), g64.double()), key
        else:
            assert float((r64[k] - g64).abs().max()) < 1e-12
            assert float((r32[k] - g32).abs().max()) < 1e-5
    assert float(r32[0].sum()) > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_torch_surface_line_center_equals_the_reference(gold, name):
    from msmdfusion_amd.head_loss import DepthBoxes, surface_line_center_torch
    seen = 0
    for b in range(CASES[name]):
        boxes = _t(gold["%s/%d/boxes" % (name, b)]).reshape(-1, 7)
        if not len(boxes):
            continue
        seen += 1
        got = DepthBoxes(boxes, with_yaw=bool(gold[name + "/with_yaw"])).get_surface_line_center()
        g = _t(gold["%s/%d/gravity_boxes" % (name, b)]).double()
        got64 = surface_line_center_torch(g[:, :3], g[:, 3:6], g[:, 6])
        ref64 = R.surface_line_center_ref(g[:, :3], g[:, 3:6], g[:, 6])
        for k, key in enumerate(("surface_center", "line_center")):
            g32 = _t(gold["%s/%d/f32/%s" % (name, b, key)])
            g64 = _t(gold["%s/%d/f64/%s" % (name, b, key)])
            assert got[k].shape == g32.shape and got[k].dtype == torch.float32
            assert float((got64[k] - g64).abs().max()) < 1e-12
            assert float((ref64[k] - g64).abs().max()) < 1e-12
            assert float((got[k].double() - g64).abs().max()) <= \
                4 * float((g32.double() - g64).abs().max()) + 1e-7
    assert seen


def test_the_rotation_index_is_the_row_not_the_box(gold):
    """Row r of the reference is turned by box r % n: with three yaws the own-box reading is
    visibly another function."""
    g = _t(gold["yaw/0/gravity_boxes"]).double()
    n = g.shape[0]
    ref = _t(gold["yaw/0/f64/surface_center"]).view(n, 6, 3)
    own_c, own_s = torch.cos(-g[:, 6]), torch.sin(-g[:, 6])
    plus_x_own = g[:, :3] + torch.stack((own_c, own_s, torch.zeros(n).double()), 1) * \
        g[:, 3:4] / 2
    assert float((ref[:, 4] - plus_x_own).abs().max()) > 1e-2
    rows = (torch.arange(n) * 6 + 4) % n
    c, s = torch.cos(-g[rows, 6]), torch.sin(-g[rows, 6])
    plus_x = g[:, :3] + torch.stack((c, s, torch.zeros(n).double()), 1) * g[:, 3:4] / 2
    assert float((ref[:, 4] - plus_x).abs().max()) < 1e-12


def test_mse_loss_is_mmdets_arithmetic():
    from msmdfusion_amd.losses import MSELoss, build_loss
    pred = torch.tensor([[1.0, 2.0], [0.0, -1.0]])
    target = torch.tensor([[0.0, 2.0], [2.0, 1.0]])
    weight = torch.tensor([[1.0, 1.0], [0.5, 0.0]])
    none = build_loss(dict(type="MSELoss", reduction="none", loss_weight=2.0))
    assert isinstance(none, MSELoss)
    assert torch.equal(none(pred, target), torch.tensor([[2.0, 0.0], [8.0, 8.0]]))
    assert torch.equal(none(pred, target, weight=weight), torch.tensor([[2.0, 0.0], [4.0, 0.0]]))
    # reduction 'none' ignores avg_factor (mmdet weight_reduce_loss)
    assert torch.equal(none(pred, target, weight=weight, avg_factor=3.0),
                       torch.tensor([[2.0, 0.0], [4.0, 0.0]]))
    mean = MSELoss()
    assert float(mean(pred, target)) == 9.0 / 4
    assert float(mean(pred, target, weight=weight)) == 3.0 / 4
    assert float(mean(pred, target, weight=weight, avg_factor=2.0)) == 1.5
    assert float(mean(pred, target, reduction_override="sum")) == 9.0
    assert float(MSELoss(reduction="sum", loss_weight=0.5)(pred, target, weight=weight)) == 1.5
    with pytest.raises(ValueError):
        MSELoss(reduction="sum")(pred, target, avg_factor=2.0)


def test_padding_leaves_the_callers_lists_untouched(gold):
    from msmdfusion_amd import h3d_head as H
    from msmdfusion_amd.head_loss import DepthBoxes
    tensors = [_t(gold["no_yaw/%d/boxes" % b]).reshape(-1, 7) for b in range(2)]
    boxes = [DepthBoxes(t, with_yaw=False) for t in tensors]
    labels = [_t(gold["no_yaw/%d/labels" % b]).long().reshape(-1) for b in range(2)]
    kept_boxes, kept_labels = list(boxes), [l.clone() for l in labels]
    padded, lab, counts = H.pad_ground_truths(boxes, labels, torch.device("cpu"))
    assert all(a is b for a, b in zip(boxes, kept_boxes)) and len(boxes[1]) == 0
    assert all(torch.equal(a, b) for a, b in zip(labels, kept_labels))
    assert torch.equal(boxes[0].tensor, tensors[0])
    assert padded.shape == (2, 4, 7) and counts.tolist() == [4, 1] and counts.dtype == torch.int32
    assert torch.equal(padded[0], _t(gold["no_yaw/0/gravity_boxes"]))
    assert not padded[1].any() and not lab[1].any() and torch.equal(lab[0], labels[0])
    # plain tensors serve as well, and a batch of empty samples still has one column
    padded, lab, counts = H.pad_ground_truths([torch.zeros(0, 7)], [torch.zeros(0).long()],
                                              torch.device("cpu"))
    assert padded.shape == (1, 1, 7) and counts.tolist() == [1]
    with pytest.raises(ValueError):
        H.pad_ground_truths([torch.zeros(2, 7)], [torch.zeros(3).long()], torch.device("cpu"))
    assert H.TARGET_NAMES == R.TARGET_NAMES and H.K.H3D_CUE_THRESHOLDS == R.THRESHOLDS


def test_first_min_spells_out_torch_min():
    d = torch.tensor([[3.0, 1.0, 1.0], [float("nan"), 0.0, float("nan")], [2.0, 2.0, 2.0]])
    val, idx = R.first_min(d)
    assert idx.tolist() == [1, 0, 0] and val[0] == 1 and torch.isnan(val[1])
    assert R.first_argmax(torch.tensor([[1.0, 5.0, 5.0], [0.0, float("nan"), 9.0]])).tolist() == \
        [1, 1]


# ---------------------------------------------------------------------------- C-ABI refusals
def test_new_entry_points_refuse_bad_arguments_on_the_host():
    """Nothing is enqueued: these calls return before the first launch (no GPU needed)."""
    from msmdfusion_amd._lib import lib
    p = ctypes.c_void_p(256)                            # a non-null, aligned, never-read address
    INVALID, RANGE = -1, -5
    assert lib.msmd_h3d_cue_gt_chunk() == 64 and lib.msmd_h3d_cue_pred_chunk() == 256
    assert lib.msmd_h3d_cue_proposals() == 14

    fwd, bwd = lib.msmd_box_cue_centers_f32, lib.msmd_box_cue_centers_bwd_f32
    assert fwd(None, 4, p, p, None) == INVALID and fwd(p, 4, None, p, None) == INVALID
    assert fwd(p, 4, p, None, None) == INVALID and fwd(p, -1, p, p, None) == INVALID
    assert fwd(p, 1 << 26, p, p, None) == RANGE and fwd(None, 0, None, None, None) == 0
    for k in range(4):
        a = [p, p, p, p]
        a[k] = None
        assert bwd(a[0], 4, a[1], a[2], a[3], None) == INVALID, k
    assert bwd(p, -1, p, p, p, None) == INVALID and bwd(p, 1 << 26, p, p, p, None) == RANGE
    assert bwd(None, 0, None, None, None, None) == 0

    fn = lib.msmd_h3d_cue_targets_f32

    def call(**kw):
        a = dict(ins=[p] * 10, b=2, p=16, g=4, ns=40, nl=30, c=18, thr=[0.3, 0.6, 0.3, 0.3, 0.3, 0.3],
                 outs=[p] * 8)
        a.update(kw)
        return fn(*a["ins"], a["b"], a["p"], a["g"], a["ns"], a["nl"], a["c"], *a["thr"],
                  *a["outs"], None)

    for k in range(10):
        assert call(ins=[None if j == k else p for j in range(10)]) == INVALID, k
    for k in range(8):
        assert call(outs=[None if j == k else p for j in range(8)]) == INVALID, k
    for name in ("b", "p", "g", "ns", "nl", "c"):
        assert call(**{name: -1}) == INVALID, name
    for name in ("g", "ns", "nl", "c"):
        assert call(**{name: 0}) == INVALID, name
    for k in range(6):
        thr = [0.3] * 6
        thr[k] = float("nan")
        assert call(thr=thr) == INVALID, k
    assert call(c=4097) == RANGE and call(b=1 << 12, p=1 << 14) == RANGE
    assert call(b=1 << 12, ns=1 << 18) == RANGE and call(b=1 << 12, nl=1 << 18) == RANGE
    assert call(b=1 << 12, g=1 << 17) == RANGE
    assert call(b=0) == 0 and call(p=0) == 0               # nothing to do


def test_python_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    from msmdfusion_amd import kernels as K
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.box_cue_centers_forward(z(2, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.h3d_cue_targets(z(1, 4, 3), z(1, 2, 7), z(1, dtype=torch.int32),
                          z(1, 2, dtype=torch.long), z(1, 5, 3), z(1, 5, 3), z(1, 5, 3),
                          z(1, 5, 3), z(1, 24, 3), z(1, 48, 3), HC.CFG)
    assert K.H3D_CUE_TARGET_NAMES == R.TARGET_NAMES


# ------------------------------------------------------- the head, the RoI head, the detector
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_h3d_bbox_head_golden as MH  # noqa: E402  (the head cases' config)


@pytest.mark.parametrize("name", sorted(MH.HEAD_CASES))
def test_state_dict_keys_equal_the_references(gold, name):
    """The key list is what the reference's own H3DBboxHead.__init__ gave (the generator built
    it), shapes included: its checkpoints load."""
    import copy
    from msmdfusion_amd import registry
    from msmdfusion_amd.h3d_head import H3DBboxHead
    _, with_yaw, bins, _ = MH.HEAD_CASES[name]
    cfg = dict(MH.head_cfg(with_yaw, bins), type="H3DBboxHead")
    before = copy.deepcopy(cfg)
    head = registry.build_head(cfg)
    assert cfg == before                                  # mlp_channels lists included
    assert isinstance(head, H3DBboxHead)
    state = head.state_dict()
    assert list(state) == [str(k) for k in gold[name + "/state_keys"]]
    for k, v in state.items():
        assert tuple(v.shape) == gold["%s/state/%s" % (name, k)].shape, k
    head.load_state_dict({k: _t(gold["%s/state/%s" % (name, k)]) for k in state})
    assert head.with_angle == with_yaw and head.num_dir_bins == bins


def test_registries_and_the_model_config_fixture():
    import copy
    import json
    from msmdfusion_amd import configs as C, detector, registry
    from msmdfusion_amd.h3d_head import H3DBboxHead, H3DRoIHead
    from msmdfusion_amd.primitive_head import PrimitiveHead
    from msmdfusion_amd.vote_head import VoteHead
    registry.build_head                                            # the import below registers
    from msmdfusion_amd import h3d_head  # noqa: F401
    assert registry.HEADS.get("H3DBboxHead") is H3DBboxHead
    assert registry.HEADS.get("H3DRoIHead") is H3DRoIHead
    assert registry.DETECTORS.get("H3DNet") is detector.H3DNet
    fx = json.load(open(os.path.join(HERE, "golden", "reference_h3dnet_model_config.json")))
    norm = lambda o: json.loads(json.dumps(o))   # noqa: E731  (tuples -> lists)
    assert norm(C.H3DNET_SCANNET) == fx
    model = C.H3DNET_SCANNET["model"]
    assert model["backbone"] is C.H3DNET_SCANNET_BACKBONE
    assert model["roi_head"]["primitive_list"][2] is C.H3DNET_PRIMITIVE_LINE
    before = copy.deepcopy(C.H3DNET_SCANNET)
    net = registry.build_detector(model)
    assert C.H3DNET_SCANNET == before
    assert model["roi_head"]["bbox_head"]["suface_matching_cfg"]["mlp_channels"] == [134, 128, 64, 32]
    assert "train_cfg" not in model["roi_head"]["bbox_head"]      # the caller's dict stays
    assert isinstance(net.rpn_head, VoteHead) and isinstance(net.roi_head, H3DRoIHead)
    assert isinstance(net.roi_head.bbox_head, H3DBboxHead)
    assert all(isinstance(h, PrimitiveHead) for h in net.roi_head.primitive_heads)
    assert [h.primitive_mode for h in net.roi_head.primitive_heads] == ["z", "xy", "line"]
    # the two stages get their own halves of train_cfg / test_cfg (two_stage.py)
    assert net.rpn_head.train_cfg == model["train_cfg"]["rpn"]
    assert net.roi_head.bbox_head.train_cfg == model["train_cfg"]["rcnn"]
    assert net.roi_head.bbox_head.test_cfg == model["test_cfg"]["rcnn"]
    assert net.roi_head.bbox_head.bbox_pred[3].weight.shape[0] == 2 + 3 + 24 * 2 + 18 * 4 + 18
    with pytest.raises(AssertionError):
        registry.build_head(dict(model["roi_head"], primitive_list=model["roi_head"][
            "primitive_list"][:2]))


def test_loss_takes_thirteen_or_fourteen_rpn_targets_and_nothing_else():
    """The tuple is taken apart before anything runs, so the refusal needs no GPU; that 13 and
    14 give the same losses is tested on the GPU."""
    from msmdfusion_amd import registry
    head = registry.build_head(dict(MH.head_cfg(False, 1), type="H3DBboxHead"))
    for n in (0, 12, 15):
        with pytest.raises(ValueError, match="13 or 14"):
            head.loss({}, None, [], [], rpn_targets=(torch.zeros(1),) * n)
