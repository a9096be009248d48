"""PrimitiveHead on the GPU: whole-batch targets against the per-sample loop of
tests/primitive_ref.py (with and without masks, an empty-GT sample), no host read; the three
sample modes; the reference test's shapes (tests/test_models/test_heads/test_heads.py
test_primitive_head); loss gradients against float64 autograd of a restated loss; one training
step of backbone -> three heads."""
import copy
import os
import sys

import pytest
import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import primitive_cases as PC  # noqa: E402
import primitive_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = ("z", "xy", "line")
NUM_DIMS = {"z": 2, "xy": 1, "line": 0}


def _head_cfg(mode, num_point=64, channels=32, train_cfg=PC.SMALL_CFG):
    from msmdfusion_amd import configs as C
    cfg = copy.deepcopy({"z": C.H3DNET_PRIMITIVE_Z, "xy": C.H3DNET_PRIMITIVE_XY,
                         "line": C.H3DNET_PRIMITIVE_LINE}[mode])
    cfg["vote_module_cfg"].update(in_channels=channels, conv_channels=(channels, channels))
    cfg["vote_aggregation_cfg"].update(num_point=num_point, mlp_channels=[channels, 32, 32, 32])
    cfg["feat_channels"] = (32, 32)
    cfg["train_cfg"] = dict(train_cfg)
    return cfg


def _build(mode, dev, **kw):
    from msmdfusion_amd import registry
    torch.manual_seed(1)
    return registry.build_head(_head_cfg(mode, **kw)).to(dev)


def _scene(dev, with_yaw=True, n=512, seeds=64):
    from msmdfusion_amd.head_loss import DepthBoxes
    samples = [PC.make_sample(31, n, [150, 120, 90], with_yaw=with_yaw),
               PC.make_sample(32, n, [200, 60], with_yaw=with_yaw)]
    g = torch.Generator().manual_seed(4)
    seed_indices = torch.stack([torch.randperm(n, generator=g)[:seeds] for _ in samples])
    points = torch.stack([s["points"] for s in samples])
    seed_points = torch.gather(points[..., :3], 1, seed_indices[..., None].expand(-1, -1, 3))
    boxes = [DepthBoxes(s["boxes"].to(dev), with_yaw=with_yaw) for s in samples]
    labels = [torch.arange(len(s["boxes"]), device=dev) for s in samples]
    return samples, points.to(dev), boxes, labels, seed_points.to(dev), \
        seed_indices.to(dev).int()


def _loop_targets(samples, corners, sems, insts, mode, cfg, seed_points, seed_indices, dtype):
    """primitive_head.py:293-325 over the restated per-sample loop, on the CPU."""
    outs = [R.primitive_targets_ref(s["points"], sem, inst, c, s["with_yaw"], mode, 18, cfg, dtype)
            for s, sem, inst, c in zip(samples, sems, insts, corners)]
    mask = torch.stack([o[0] for o in outs])
    offset = torch.stack([o[1] for o in outs])
    sem = torch.stack([o[2] for o in outs])
    inds = seed_indices.long()
    centre = torch.gather(offset, 1, inds[..., None].expand(-1, -1, 3)) + seed_points.to(dtype)
    seed_sem = torch.gather(sem, 1, inds[..., None].expand(-1, -1, sem.shape[-1]))
    dims = NUM_DIMS[mode]
    rows = inds.numel()
    return (mask, offset, centre.reshape(rows, 1, 3),
            seed_sem[:, :, 3:3 + dims].reshape(rows, 1, dims),
            seed_sem[:, :, -1].long(), torch.gather(mask, 1, inds))


@pytest.mark.parametrize("with_yaw", [True, False])
def test_get_targets_equals_the_per_sample_loop_without_a_host_read(dev, with_yaw):
    from msmdfusion_amd.primitive_head import prepare_primitive_inputs
    samples, points, boxes, labels, seed_points, seed_indices = _scene(dev, with_yaw)
    sems = [s["sem"].to(dev) for s in samples]
    insts = [s["inst"].to(dev) for s in samples]
    heads = {m: _build(m, dev) for m in MODES}
    preds = {m: {"aggregated_points_" + m: seed_points.new_zeros(seed_points.shape),
                 "seed_points": seed_points, "seed_indices": seed_indices} for m in MODES}
    heads["z"].get_targets(points, boxes, labels, sems, insts, preds["z"])      # warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        prepared = prepare_primitive_inputs(points, boxes, labels, sems, insts, 18)
        shared = {m: heads[m].get_targets(points, boxes, labels, sems, insts, preds[m],
                                          prepared=prepared) for m in MODES}
        own = {m: heads[m].get_targets(points, boxes, labels, sems, insts, preds[m])
               for m in MODES}
    finally:
        torch.cuda.set_sync_debug_mode("default")
    corners = [b.corners.cpu() for b in boxes]
    for mode in MODES:
        args = (samples, corners, [s["sem"] for s in samples], [s["inst"] for s in samples],
                mode, PC.SMALL_CFG, seed_points.cpu(), seed_indices.cpu())
        want32 = _loop_targets(*args, torch.float32)
        want64 = _loop_targets(*args, torch.float64)
        assert float(want32[0].sum()) > 0
        for k, (got, other, a, b) in enumerate(zip(shared[mode], own[mode], want32, want64)):
            assert torch.equal(got, other), (mode, k)
            got = got.cpu()
            assert got.shape == a.shape and got.dtype == a.dtype, (mode, k)
            if k in (0, 4, 5):
                assert torch.equal(got, a), (mode, k)
            else:
                bound = 4 * float((a.double() - b).abs().max()) if a.numel() else 0.0
                err = float((got.double() - b).abs().max()) if a.numel() else 0.0
                assert err <= bound, (mode, k, err, bound)


def test_masks_derived_from_the_boxes_and_an_empty_sample(dev):
    """Masks None: semantic / instance labels come from points_in_boxes (:358-369); a sample
    without ground truth gets the zero box and no targets."""
    from msmdfusion_amd.head_loss import DepthBoxes
    from msmdfusion_amd.primitive_head import prepare_primitive_inputs
    samples, points, boxes, labels, seed_points, seed_indices = _scene(dev)
    boxes[1] = DepthBoxes(torch.zeros((0, 7), device=dev))
    labels = [torch.tensor([3, 7, 11], device=dev), torch.zeros((0,), dtype=torch.long, device=dev)]
    torch.cuda.set_sync_debug_mode("error")
    try:
        prepared = prepare_primitive_inputs(points, boxes, labels, None, None, 18)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(boxes[1]) == 0 and labels[1].numel() == 0          # the caller's lists are intact
    sem = prepared["sem"].view(2, -1).cpu()
    inst = prepared["inst"].view(2, -1).cpu()
    assert bool((sem[1] == 18).all()) and bool((inst[1] == 1).all())
    inside = sem[0] != 18
    assert 0 < int(inside.sum()) < sem.shape[1]
    assert set(sem[0][inside].tolist()) <= {3, 7, 11} and set(inst[0][inside].tolist()) <= {0, 1, 2}
    corners = [boxes[0].corners.cpu(), torch.zeros((1, 8, 3))]
    for mode in MODES:
        head = _build(mode, dev)
        preds = {"aggregated_points_" + mode: seed_points, "seed_points": seed_points,
                 "seed_indices": seed_indices}
        got = head.get_targets(points, boxes, labels, None, None, preds, prepared=prepared)
        want = _loop_targets(samples, corners, list(sem), list(inst), mode, PC.SMALL_CFG,
                             seed_points.cpu(), seed_indices.cpu(), torch.float32)
        assert torch.equal(got[0].cpu(), want[0]) and float(got[0][1].sum()) == 0
        assert float(got[0][0].sum()) > 0
        assert torch.equal(got[4].cpu(), want[4])
        torch.testing.assert_close(got[1].cpu(), want[1], rtol=0, atol=2e-5)


@pytest.mark.parametrize("sample_mod", ["vote", "seed", "random"])
def test_forward_keys_and_sample_modes(dev, sample_mod):
    for mode in MODES:
        head = _build(mode, dev, num_point=64)       # one proposal per seed, as :181-182 needs
        feats = dict(fp_xyz_net0=[torch.rand((2, 64, 3), device=dev)],
                     hd_feature=torch.rand((2, 32, 64), device=dev))
        ret = head(feats, sample_mod)
        keys = {"pred_flag_", "vote_", "vote_features_", "aggregated_points_",
                "aggregated_features_", "aggregated_indices_", "center_", "sem_cls_scores_"}
        want = {k + mode for k in keys} | {"pred_%s_ind" % mode, "pred_%s_center" % mode}
        if mode != "line":
            want.add("size_residuals_" + mode)
        assert set(ret) == want
        assert ret["center_" + mode].shape == (2, 64, 3)
        assert ret["pred_flag_" + mode].shape == (2, 2, 64)
        assert ret["sem_cls_scores_" + mode].shape == (2, 64, 18)
        assert ret["aggregated_indices_" + mode].shape == (2, 64)
        assert ret["aggregated_indices_" + mode].dtype == torch.int32
        centre, ind = ret["pred_%s_center" % mode], ret["pred_%s_ind" % mode]
        prob = F.softmax(ret["pred_flag_" + mode], dim=1)[:, 1]
        assert ind.shape == (2, 64) and torch.equal(ind, (prob > 0.5).float())
        moved = ret["center_" + mode] + 100.0 * (1 - ind)[..., None]
        assert torch.equal(centre, moved)


def test_the_reference_tests_shapes_give_finite_non_negative_losses(dev):
    from msmdfusion_amd import configs as C, registry
    from msmdfusion_amd.head_loss import DepthBoxes
    torch.manual_seed(0)
    for mode, cfg in (("z", C.H3DNET_PRIMITIVE_Z), ("xy", C.H3DNET_PRIMITIVE_XY),
                      ("line", C.H3DNET_PRIMITIVE_LINE)):
        cfg = copy.deepcopy(cfg)
        cfg["vote_aggregation_cfg"]["num_point"] = 64
        head = registry.build_head(cfg).to(dev)
        fp_xyz = [torch.rand([2, 64, 3], device=dev)]
        feats = dict(fp_xyz_net0=fp_xyz, hd_feature=torch.rand([2, 256, 64], device=dev),
                     fp_indices_net0=[torch.randint(0, 64, [2, 64], device=dev)])
        ret = head(feats, "vote")
        assert ret["center_" + mode].shape == (2, 64, 3)
        assert ret["sem_cls_scores_" + mode].shape == (2, 64, 18)
        assert ret["aggregated_points_" + mode].shape == (2, 64, 3)
        if mode == "z":
            assert ret["size_residuals_z"].shape == (2, 64, 2)
        points = torch.rand([2, 1024, 3], device=dev)
        ret["seed_points"], ret["seed_indices"] = fp_xyz[0], feats["fp_indices_net0"][0]
        boxes = [DepthBoxes(torch.rand([4, 7], device=dev)) for _ in range(2)]
        labels = list(torch.randint(0, 18, [2, 4], device=dev))
        sem = list(torch.randint(0, 19, [2, 1024], device=dev))
        inst = list(torch.randint(0, 4, [2, 1024], device=dev))
        losses = head.loss(ret, points, boxes, labels, sem, inst)
        assert set(losses) == {k + mode for k in ("flag_loss_", "vote_loss_", "center_loss_",
                                                  "size_loss_", "sem_loss_")}
        for name, value in losses.items():
            assert bool(torch.isfinite(value)) and float(value.detach()) >= 0, name
    with pytest.raises(AssertionError):
        bad = copy.deepcopy(C.H3DNET_PRIMITIVE_Z)
        bad["vote_module_cfg"]["in_channels"] = "xyz"
        registry.build_head(bad)


def _loss64(head, preds, targets):
    """primitive_head.py:188-257 and compute_primitive_loss restated in float64 torch: the
    Chamfer terms are one-to-one here (one prediction, one target per proposal)."""
    mode = head.primitive_mode
    point_mask, point_offset, centre, semantic, cls_label, seed_mask = \
        [t.double() if t.is_floating_point() else t for t in targets]
    # mmdet's CrossEntropyLoss: the class-weighted terms, then a plain mean over the seeds
    flag = F.cross_entropy(preds["pred_flag_" + mode], seed_mask.long(), reduction="none",
                           weight=preds["pred_flag_" + mode].new_tensor(
                               head.objectness_loss.class_weight)).mean() * \
        head.objectness_loss.loss_weight
    inds = preds["seed_indices"].long()
    vote_mask = torch.gather(point_mask, 1, inds)
    gt_votes = torch.gather(point_offset, 1, inds[..., None].expand(-1, -1, 3)) + preds["seed_points"]
    weight = vote_mask / (vote_mask.sum() + 1e-6)
    vote = ((preds["vote_" + mode] - gt_votes).abs().sum(-1) * weight).sum() * \
        head.vote_module.vote_loss.loss_dst_weight
    weight = seed_mask / (seed_mask.sum() + 1e-6)
    flat = weight.reshape(-1)
    centre_loss = ((preds["center_" + mode].reshape(-1, 3) - centre[:, 0]).abs().sum(-1)
                   * flat).sum() * head.center_loss.loss_dst_weight
    out = {"flag_loss_" + mode: flag, "vote_loss_" + mode: vote,
           "center_loss_" + mode: centre_loss}
    if mode != "line":
        dims = head.num_dims
        out["size_loss_" + mode] = ((preds["size_residuals_" + mode].reshape(-1, dims)
                                     - semantic[:, 0]).abs().sum(-1) * flat).sum() * \
            head.semantic_reg_loss.loss_dst_weight
    ce = F.cross_entropy(preds["sem_cls_scores_" + mode].transpose(2, 1), cls_label,
                         reduction="none")
    out["sem_loss_" + mode] = (ce * weight).sum() * head.semantic_cls_loss.loss_weight
    return out


@pytest.mark.parametrize("mode", MODES)
def test_losses_and_gradients_match_float64_autograd(dev, mode):
    samples, points, boxes, labels, seed_points, seed_indices = _scene(dev)
    sems = [s["sem"].to(dev) for s in samples]
    insts = [s["inst"].to(dev) for s in samples]
    head = _build(mode, dev)
    g = torch.Generator().manual_seed(8)
    names = ["pred_flag_", "vote_", "center_", "sem_cls_scores_"] + \
        (["size_residuals_"] if mode != "line" else [])
    shapes = {"pred_flag_": (2, 2, 64), "vote_": (2, 64, 3), "center_": (2, 64, 3),
              "sem_cls_scores_": (2, 64, 18), "size_residuals_": (2, 64, NUM_DIMS[mode])}
    leaves = {k + mode: torch.randn(shapes[k], generator=g).to(dev).requires_grad_()
              for k in names}
    preds = dict(leaves, seed_points=seed_points, seed_indices=seed_indices)
    preds["aggregated_points_" + mode] = seed_points
    preds["vote_" + mode] = leaves["vote_" + mode] + seed_points     # near the seeds
    targets = head.get_targets(points, boxes, labels, sems, insts, preds)
    assert float(targets[5].sum()) > 0
    losses = head.loss_from_targets(preds, targets)
    sum(losses.values()).backward()
    leaves64 = {k: v.detach().double().requires_grad_() for k, v in leaves.items()}
    preds64 = dict(leaves64, seed_points=seed_points.double(), seed_indices=seed_indices)
    preds64["vote_" + mode] = leaves64["vote_" + mode] + seed_points.double()
    want = _loss64(head, preds64, targets)
    sum(want.values()).backward()
    if mode == "line":
        assert float(losses["size_loss_line"]) == 0
    for name, value in want.items():
        torch.testing.assert_close(losses[name].double(), value, rtol=1e-5, atol=1e-6)
    for name, leaf in leaves.items():
        torch.testing.assert_close(leaf.grad.double(), leaves64[name].grad, rtol=1e-5, atol=1e-7)


def test_one_training_step_backbone_three_heads(dev):
    from msmdfusion_amd import registry
    from msmdfusion_amd.head_loss import DepthBoxes
    from msmdfusion_amd.primitive_head import prepare_primitive_inputs
    torch.manual_seed(3)
    sassg = dict(type="PointNet2SASSG", in_channels=4, num_points=(256, 128, 64, 32),
                 radius=(0.4, 0.8, 1.6, 2.4), num_samples=(16, 16, 8, 8),
                 sa_channels=((16, 16, 32), (32, 32, 32), (32, 32, 32), (32, 32, 32)),
                 fp_channels=((32, 32), (32, 32)), norm_cfg=dict(type="BN2d"))
    backbone = registry.build_backbone(dict(type="MultiBackbone", num_streams=2,
                                            suffixes=["net0", "net1"], backbones=sassg)).to(dev)
    heads = [_build(m, dev, num_point=128) for m in MODES]
    samples, points, boxes, labels, _, _ = _scene(dev)
    sems = [s["sem"].to(dev) for s in samples]
    insts = [s["inst"].to(dev) for s in samples]
    feats = backbone(points)
    assert feats["hd_feature"].shape == (2, 32, 128)
    torch.cuda.synchronize()
    # forward and targets of the three heads under the debug mode: nothing is read back.  The
    # loss terms are summed outside it: CrossEntropyLoss uploads its class weights with a
    # blocking host-to-device copy, which the mode reports like a read.
    torch.cuda.set_sync_debug_mode("error")
    try:
        prepared = prepare_primitive_inputs(points, boxes, labels, sems, insts, 18)
        rets, targets = [], []
        for head in heads:
            ret = head(feats, "vote")
            ret["seed_points"] = feats["fp_xyz_net0"][-1]
            ret["seed_indices"] = feats["fp_indices_net0"][-1]
            rets.append(ret)
            targets.append(head.get_targets(points, boxes, labels, sems, insts, ret,
                                            prepared=prepared))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    total = 0
    for head, ret, target in zip(heads, rets, targets):
        assert float(target[5].sum()) > 0
        total = total + sum(head.loss_from_targets(ret, target).values())
    total.backward()
    assert bool(torch.isfinite(total))
    for module in [backbone] + heads:
        for name, p in module.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name


# ------------------------------------------------------------------ the reference's own vectors
def _gold():
    import numpy as np
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                "primitive_head_vectors.npz"))


def _gold_modules():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_primitive_head_golden as M
    return M


def _bound(ref32, ref64, floor_of=None):
    """4 x the reference's own float32-against-float64 difference; where a value is one more
    float32 operation away from it (centre = offset + seed), plus that operation's rounding:
    one float32 ulp of the largest magnitude."""
    import numpy as np
    bound = 4 * float(np.abs(ref32.astype(np.float64) - ref64).max()) if ref64.size else 0.0
    if floor_of is not None and floor_of.size:
        bound += float(np.spacing(np.float32(np.abs(floor_of).max())))
    return bound


def test_targets_match_the_reference_vectors(dev):
    """Every case of tests/golden/primitive_head_vectors.npz (both yaw forms, a label gap, a
    count and a variance failure, a background-only sample, an empty-GT sample with masks None,
    the config's 100 / 101 straddle) through PrimitiveHead.get_targets on the GPU."""
    import numpy as np
    from msmdfusion_amd import registry
    from msmdfusion_amd.head_loss import DepthBoxes
    gold, M = _gold(), _gold_modules()
    keys = ("dist_thresh", "var_thresh", "lower_thresh", "num_point", "num_point_line",
            "line_thresh")
    for name in M.cases():
        cfg = dict(zip(keys, gold[name + "/cfg"].tolist()))
        cfg["num_point"], cfg["num_point_line"] = int(cfg["num_point"]), int(cfg["num_point_line"])
        with_yaw, masks = bool(gold[name + "/with_yaw"]), bool(gold[name + "/masks"])
        points = torch.from_numpy(gold[name + "/points"]).to(dev)
        batch = points.shape[0]
        boxes = [DepthBoxes(torch.from_numpy(gold["%s/%d/boxes" % (name, b)]).reshape(-1, 7).to(dev),
                            with_yaw=with_yaw) for b in range(batch)]
        labels = [torch.from_numpy(gold["%s/%d/labels" % (name, b)]).to(dev) for b in range(batch)]
        sems = [torch.from_numpy(gold["%s/%d/sem" % (name, b)]).to(dev) for b in range(batch)] \
            if masks else None
        insts = [torch.from_numpy(gold["%s/%d/inst" % (name, b)]).to(dev) for b in range(batch)] \
            if masks else None
        seed_indices = torch.from_numpy(gold[name + "/seed_indices"]).to(dev)
        seed_points = torch.gather(points[..., :3], 1, seed_indices[..., None].expand(-1, -1, 3))
        for mode in MODES:
            head = registry.build_head(dict(type="PrimitiveHead", **M.head_cfg(mode, cfg))).to(dev)
            preds = {"aggregated_points_" + mode: seed_points, "seed_points": seed_points,
                     "seed_indices": seed_indices}
            got = [t.cpu().numpy() for t in
                   head.get_targets(points, boxes, labels, sems, insts, preds)]
            want = [gold["%s/targets/%s/%d" % (name, mode, k)] for k in range(6)]
            per = {tag: {k: np.stack([gold["%s/%d/%s/%s/%s" % (name, b, mode, tag, k)]
                                      for b in range(batch)]) for k in ("mask", "sem", "offset")}
                   for tag in ("f32", "f64")}
            what = (name, mode)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[0], per["f32"]["mask"]), what
            assert np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5]), what
            assert got[1].shape == want[1].shape and got[2].shape == want[2].shape, what
            assert got[3].shape == want[3].shape, what
            off = _bound(per["f32"]["offset"], per["f64"]["offset"])
            assert float(np.abs(got[1] - per["f64"]["offset"]).max()) <= off, what
            # the gathered targets are stored in float32 only: |got - f32| <= |got - f64| +
            # |f32 - f64| <= (1 + 1 / 4) x the bound
            centre = _bound(per["f32"]["offset"], per["f64"]["offset"], floor_of=want[2])
            assert float(np.abs(got[2].astype(np.float64) - want[2]).max()) <= 1.25 * centre, what
            size = _bound(per["f32"]["sem"], per["f64"]["sem"])
            if want[3].size:
                assert float(np.abs(got[3].astype(np.float64) - want[3]).max()) <= 1.25 * size, what


@pytest.mark.parametrize("mode", MODES)
def test_decode_and_losses_match_the_reference_vectors(dev, mode):
    """Decode and the primitive centre exactly (one float32 operation each); the losses and their
    input gradients of the "yaw" case, targets computed on the GPU, within 4 x the reference's
    float32-against-float64 difference plus 4 float32 ulps of the largest value (the kernels'
    Chamfer and the device's softmax round their last operations on their own)."""
    import numpy as np
    from msmdfusion_amd import registry
    from msmdfusion_amd.head_loss import DepthBoxes
    gold, M = _gold(), _gold_modules()
    head = registry.build_head(dict(type="PrimitiveHead",
                                    **M.head_cfg(mode, M.PC.SMALL_CFG))).to(dev)
    predictions = torch.from_numpy(gold["decode/%s/predictions" % mode]).to(dev)
    centre = torch.from_numpy(gold["decode/%s/center_%s" % (mode, mode)]).to(dev)
    points = torch.from_numpy(gold["yaw/points"]).to(dev)
    seed_indices = torch.from_numpy(gold["yaw/seed_indices"]).to(dev)
    seed_points = torch.gather(points[..., :3], 1, seed_indices[..., None].expand(-1, -1, 3))
    decoded = head.primitive_decode_scores(predictions, seed_points)
    for k, v in decoded.items():
        assert np.array_equal(v.cpu().numpy(), gold["decode/%s/%s" % (mode, k)]), k
    pred_centre, pred_ind = head.get_primitive_center(
        torch.from_numpy(gold["decode/%s/flag" % mode]).to(dev), centre)
    assert np.array_equal(pred_ind.cpu().numpy(), gold["decode/%s/pred_ind" % mode])
    assert np.array_equal(pred_centre.cpu().numpy(), gold["decode/%s/pred_center" % mode])

    boxes = [DepthBoxes(torch.from_numpy(gold["yaw/%d/boxes" % b]).to(dev)) for b in range(2)]
    labels = [torch.from_numpy(gold["yaw/%d/labels" % b]).to(dev) for b in range(2)]
    sems = [torch.from_numpy(gold["yaw/%d/sem" % b]).to(dev) for b in range(2)]
    insts = [torch.from_numpy(gold["yaw/%d/inst" % b]).to(dev) for b in range(2)]
    prefix = "loss/%s/f32/" % mode
    leaves = {k[len(prefix + "in/"):]: torch.from_numpy(gold[k]).to(dev).requires_grad_()
              for k in gold.files if k.startswith(prefix + "in/")}
    preds = dict(leaves, seed_points=seed_points, seed_indices=seed_indices)
    preds["aggregated_points_" + mode] = seed_points
    losses = head.loss(preds, points, boxes, labels, sems, insts)
    sum(losses.values()).backward()

    def close(got, g32, g64, what):
        bound = _bound(np.asarray(g32), np.asarray(g64)) + \
            4 * float(np.spacing(np.float32(np.abs(g64).max())))
        err = float(np.abs(np.asarray(got, np.float64) - g64).max())
        print(what, "err %.3e bound %.3e" % (err, bound))
        assert err <= bound, (what, err, bound)
    for name, value in losses.items():
        close(value.detach().cpu().numpy(), gold["loss/%s/f32/%s" % (mode, name)],
              gold["loss/%s/f64/%s" % (mode, name)], name)
    for name, leaf in leaves.items():
        close(leaf.grad.cpu().numpy(), gold["loss/%s/f32/grad/%s" % (mode, name)],
              gold["loss/%s/f64/grad/%s" % (mode, name)], "grad " + name)
