"""H3DBboxHead on the GPU against the reference's own outputs in
tests/golden/h3d_bbox_head_vectors.npz.

h3d_head.get_targets (H3DBboxHead.get_targets for the batch, one kernel call): discrete outputs
exact, obj_surface_line_center within 4 x the reference's float32 error against its float64 run,
under sync-debug mode.  The whole head, built from the generator's config with the reference's
weights: forward's outputs, every loss term and the gradients of all parameters, of the proposals
and of the primitive centres under the same criterion, with this project's PointSAModule as the
matchers; loss and the get_targets method under sync-debug mode; 13 against 14 rpn targets;
get_bboxes on the reference's suffix-mixed decode, batched against one call per sample; the
reference test's shapes."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import h3d_cases as HC  # noqa: E402
import h3d_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = {"yaw": 2, "no_yaw": 2, "single_yaw": 1, "single": 1}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "h3d_bbox_head_vectors.npz")))


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _inputs(gold, name, dev):
    from msmdfusion_amd.head_loss import DepthBoxes
    p = gold[name + "/aggregated"].shape[1]
    cue = _t(gold[name + "/cue_obj"]).to(dev)
    preds = dict(aggregated_points=_t(gold[name + "/aggregated"]).to(dev),
                 surface_center_pred=_t(gold[name + "/surface_pred"]).to(dev),
                 pred_line_center=_t(gold[name + "/line_pred"]).to(dev),
                 surface_center_object=cue[:, :6 * p], line_center_object=cue[:, 6 * p:],
                 surface_sem_pred=_t(gold[name + "/surface_sem"]).to(dev),
                 sem_cls_scores_line=_t(gold[name + "/line_sem"]).to(dev))
    with_yaw = bool(gold[name + "/with_yaw"])
    boxes = [DepthBoxes(_t(gold["%s/%d/boxes" % (name, b)]).reshape(-1, 7).to(dev),
                        with_yaw=with_yaw) for b in range(CASES[name])]
    labels = [_t(gold["%s/%d/labels" % (name, b)]).long().reshape(-1).to(dev)
              for b in range(CASES[name])]
    return preds, boxes, labels


@pytest.mark.parametrize("name", sorted(CASES))
def test_get_targets_against_the_reference(dev, gold, name):
    from msmdfusion_amd import h3d_head as H
    preds, boxes, labels = _inputs(gold, name, dev)
    lengths = [len(b) for b in boxes]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = H.get_targets(preds, boxes, labels, HC.CFG)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert [len(b) for b in boxes] == lengths                  # the caller's lists stay
    assert len(got) == len(R.TARGET_NAMES)
    for k, key in enumerate(R.TARGET_NAMES):
        g32, g64 = _t(gold["%s/f32/%s" % (name, key)]), _t(gold["%s/f64/%s" % (name, key)])
        out = got[k].cpu()
        assert out.dtype == g32.dtype and out.shape == g32.shape, key
        if key in R.DISCRETE:
            assert torch.equal(out, g32), key
        else:
            bound = 4 * float((g32.double() - g64).abs().max())
            err = float((out.double() - g64).abs().max())
            print("%s %s: err %.3e bound %.3e" % (name, key, err, bound))
            assert err <= bound, (key, err, bound)
    assert float(got[0].sum()) > 0 and float(got[6].sum()) > 0


# ------------------------------------------------------------------ H3DBboxHead, the whole head
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_h3d_bbox_head_golden as MH  # noqa: E402  (the head cases' config and key lists)

HEAD_CASES = sorted(MH.HEAD_CASES)


ULP = float(np.finfo(np.float32).eps)


def _close(out, g32, g64, what):
    """The 4 x criterion in the form the other head tests use (test_gpu_vote_head.py): the error
    against the reference's float64 run is at most four times the error of the reference's own
    float32 run, which counts as one ulp of the tensor's largest entry at the least -- on a
    tensor of one or two numbers it is anything from nothing upwards by chance."""
    bound = 4 * max(float((g32.double() - g64).abs().max()), ULP * float(g64.abs().max()))
    err = float((out.detach().cpu().double() - g64).abs().max())
    print("%s: err %.3e bound %.3e" % (what, err, bound))
    assert out.shape == g64.shape, what
    assert err <= bound, (what, err, bound)


def _head_case(gold, name, dev):
    """-> (this project's head with the reference's weights, forward inputs, rpn targets in the
    reference's 13-tuple order, the rpn head's unsuffixed predictions, boxes, labels)."""
    from msmdfusion_amd import registry
    from msmdfusion_amd.head_loss import DepthBoxes
    counts, with_yaw, bins, _ = MH.HEAD_CASES[name]
    cfg = MH.head_cfg(with_yaw, bins)
    head = registry.build_head(dict(cfg, type="H3DBboxHead"))
    keys = [str(k) for k in gold[name + "/state_keys"]]
    assert list(head.state_dict()) == keys
    head.load_state_dict({k: _t(gold["%s/state/%s" % (name, k)]) for k in keys})
    head = head.to(dev).train()
    ins = {k: _t(gold["%s/in/%s" % (name, k)]).to(dev) for k in MH.FORWARD_INPUTS}
    rpn = tuple(_t(gold["%s/rpn/%s" % (name, k)]).to(dev) for k in MH.RPN_TARGETS)
    rpn_preds = {k: _t(gold["%s/rpn_pred/%s" % (name, k)]).to(dev) for k in MH.RPN_KEYS}
    boxes = [DepthBoxes(_t(gold["%s/%d/boxes" % (name, b)]).to(dev), with_yaw=with_yaw)
             for b in range(len(counts))]
    labels = [_t(gold["%s/%d/labels" % (name, b)]).long().to(dev) for b in range(len(counts))]
    return head, ins, rpn, rpn_preds, boxes, labels


@pytest.mark.parametrize("name", HEAD_CASES)
def test_forward_loss_and_gradients_against_the_reference(dev, gold, name):
    """forward's outputs, every loss term and the gradient of the summed loss for every parameter,
    the proposals and the primitive centres, against the reference's own H3DBboxHead.  The
    matchers are this project's PointSAModule, so the ball-query rule of the generator's
    stand-in is pinned against the real op as well.  A convolution bias under a training-mode
    BatchNorm has a gradient that is zero analytically, where the 4 x criterion compares
    round-off with round-off; it is asserted to vanish against its convolution's weight
    gradient instead (a wrong bias gradient has that magnitude)."""
    head, ins, rpn, rpn_preds, boxes, labels = _head_case(gold, name, dev)
    feats = {k: v.clone().requires_grad_(k in MH.GRAD_INPUTS) for k, v in ins.items()}
    out = head(feats, "vote")
    assert list(out) == [str(k) for k in gold[name + "/out_keys"]]
    for k, v in out.items():
        _close(v, _t(gold["%s/f32/out/%s" % (name, k)]), _t(gold["%s/f64/out/%s" % (name, k)]),
               "out " + k)
    preds = dict(feats, **out)
    preds.update(rpn_preds)
    points = preds["aggregated_points"]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = head.loss(preds, points, boxes, labels, rpn_targets=rpn)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert list(losses) == [str(k) for k in gold[name + "/loss_keys"]]
    for k, v in losses.items():
        _close(v, _t(gold["%s/f32/loss/%s" % (name, k)]), _t(gold["%s/f64/loss/%s" % (name, k)]),
               "loss " + k)
    # VoteHead.get_targets' 14-tuple: assigned_center_targets, the eighth, is dropped
    with torch.no_grad():
        again = head.loss(preds, points, boxes, labels,
                          rpn_targets=rpn[:7] + (torch.zeros_like(rpn[6]),) + rpn[7:])
    assert all(torch.equal(losses[k], again[k]) for k in losses)
    with pytest.raises(ValueError):
        head.loss(preds, points, boxes, labels, rpn_targets=rpn[:12])

    sum(losses.values()).backward()
    grads = {"param/" + k: p.grad for k, p in head.named_parameters()}
    grads.update({"input/" + k: feats[k].grad for k in MH.GRAD_INPUTS})
    for k, g in grads.items():
        assert g is not None, k
        g64 = _t(gold["%s/f64/grad/%s" % (name, k)])
        if k.endswith(".conv.bias"):
            weight = _t(gold["%s/f64/grad/%s" % (name, k[:-4] + "weight")])
            assert float(g.abs().max()) <= 1e-4 * float(weight.abs().max()), k
            continue
        _close(g, _t(gold["%s/f32/grad/%s" % (name, k)]), g64, "grad " + k)


@pytest.mark.parametrize("name", HEAD_CASES)
def test_head_get_targets_method_against_the_reference(dev, gold, name):
    head, ins, rpn, rpn_preds, boxes, labels = _head_case(gold, name, dev)
    with torch.no_grad():
        preds = dict(ins, **head(dict(ins), "vote"))
    lengths = [len(b) for b in boxes]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = head.get_targets(preds["aggregated_points"], boxes, labels, None, None, preds)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert [len(b) for b in boxes] == lengths
    for k, key in enumerate(R.TARGET_NAMES):
        g32 = _t(gold["%s/f32/target/%s" % (name, key)])
        if key in R.DISCRETE:
            assert torch.equal(got[k].cpu(), g32), key
        else:
            _close(got[k], g32, _t(gold["%s/f64/target/%s" % (name, key)]), key)


@pytest.mark.parametrize("name", HEAD_CASES)
@pytest.mark.parametrize("per_class", (True, False))
def test_get_bboxes_mixes_suffixes_and_equals_a_per_sample_loop(dev, gold, name, per_class):
    """get_bboxes(suffix='_optimized') takes the class scores, the direction class and the size
    class from the rpn head: its boxes are the reference's suffix-mixed decode, and the batched
    NMS gives what one call per sample gives on that decode."""
    from msmdfusion_amd.vote_head import multiclass_nms_batch
    head, ins, rpn, rpn_preds, boxes, labels = _head_case(gold, name, dev)
    head.test_cfg = dict(head.test_cfg, per_class_proposal=per_class, score_thr=0.3)
    with torch.no_grad():
        preds = dict(ins, **head(dict(ins), "vote"))
        preds.update(rpn_preds)
        # points: a cloud around every decoded box, so that some boxes hold more than 5 points
        decode32, decode64 = _t(gold[name + "/f32/decode"]), _t(gold[name + "/f64/decode"])
        rng = np.random.default_rng(3)
        centre = decode32[:, ::2, :3].repeat_interleave(12, dim=1)
        points = (centre + torch.from_numpy(rng.normal(size=centre.shape)).float() * 0.3).to(dev)
        results = head.get_bboxes(points, preds, None, suffix="_optimized")
        obj = torch.softmax(preds["obj_scores_optimized"], -1)[..., -1]
        sem = torch.softmax(preds["sem_scores"], -1)
        assert len(results) == decode32.shape[0]
        kept = 0
        for b, (box, score, label) in enumerate(results):
            want = multiclass_nms_batch(obj[b:b + 1], sem[b:b + 1], decode32[b:b + 1].to(dev),
                                        points[b:b + 1], head.bbox_coder.with_rot,
                                        head.test_cfg)[0]
            assert torch.equal(label, want[2]) and torch.equal(score, want[1])
            assert box.tensor.shape == want[0].tensor.shape
            # both decodes lie within 4 x and 1 x the reference's float32 error of its float64
            # one (asserted below); the bottom centre adds half a size to z
            if len(label):
                assert float((box.tensor - want[0].tensor).abs().max()) <= \
                    8 * float((decode32.double() - decode64).abs().max())
            kept += len(label)
            # the unsuffixed decode is another set of boxes
        assert kept > 0
        mixed = head.bbox_coder.decode(dict(
            center=preds["center_optimized"], dir_class=preds["dir_class"],
            dir_res=preds["dir_res_optimized"], size_class=preds["size_class"],
            size_res=preds["size_res_optimized"]))
        _close(mixed, decode32, decode64, "decode")
        own = head.bbox_coder.decode(preds, suffix="_optimized")
        assert float((own - mixed).abs().max()) > 1e-2


def test_the_reference_tests_shapes(dev):
    """tests/test_models/test_heads/test_heads.py:591-700: 128 points, 64 proposals, hand-made
    13 rpn targets -> every loss finite and every key there."""
    from msmdfusion_amd import configs as C, registry
    from msmdfusion_amd.head_loss import DepthBoxes
    torch.manual_seed(0)
    cfg = dict(C.H3DNET_SCANNET["model"]["roi_head"]["bbox_head"],
               train_cfg=C.H3DNET_SCANNET["model"]["train_cfg"]["rcnn"],
               test_cfg=C.H3DNET_SCANNET["model"]["test_cfg"]["rcnn"])
    head = registry.build_head(cfg).to(dev).train()
    b, p, n = 1, 64, 128
    r = lambda *s: torch.rand(*s, device=dev)                                 # noqa: E731
    feats = dict(aggregated_points=r(b, p, 3), aggregated_features=r(b, 128, p),
                 proposal_list=r(b, p, 7), pred_z_center=r(b, n, 3), pred_xy_center=r(b, n, 3),
                 sem_cls_scores_z=r(b, n, 18), sem_cls_scores_xy=r(b, n, 18),
                 aggregated_features_z=r(b, 128, n), aggregated_features_xy=r(b, 128, n),
                 pred_line_center=r(b, n, 3), aggregated_features_line=r(b, 128, n),
                 sem_cls_scores_line=r(b, n, 18))
    out = head(feats, "vote")
    assert out["center_optimized"].shape == (b, p, 3) and out["size_res_optimized"].shape == \
        (b, p, 18, 3) and out["matching_score"].shape == (b, 18 * p, 2)
    feats.update(out)
    boxes = [DepthBoxes(torch.tensor([[0.3, 0.4, 0.1, 0.5, 0.6, 0.4], [0.7, 0.2, 0.2, 0.3, 0.3, 0.5]],
                                     device=dev), box_dim=6, with_yaw=False)]
    labels = [torch.tensor([2, 7], device=dev)]
    ints = lambda high, *s: torch.randint(0, high, s, device=dev)             # noqa: E731
    rpn = (r(b, 20, 9), ints(2, b, 20), ints(18, b, p), r(b, p, 3), ints(1, b, p), r(b, p),
           r(b, 2, 3), ints(18, b, p), torch.ones(b, 2, device=dev).long(), ints(2, b, p),
           r(b, p) / p, r(b, p) / p, r(b, 2) / 2)
    losses = head.loss(feats, [r(n, 4)], boxes, labels, rpn_targets=rpn)
    assert len(losses) == 12 and all(bool(torch.isfinite(v)) for v in losses.values())
    assert float(losses["primitive_objectness_loss"].detach()) >= 0
