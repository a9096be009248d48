"""ImVoteNet (stage 2) on the GPU, built from configs.IMVOTENET_STAGE2_SUNRGBD with the point
counts cut down: a training step, an inference step, the no-host-read stretch from fusion through
sampling, fused against composed fusion, and the state dict under the reference's key names."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import imvote_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = 256
LOSSES = ["center_loss", "dir_class_loss", "dir_res_loss", "objectness_loss", "semantic_loss",
          "size_class_loss", "size_res_loss", "vote_loss"]


@pytest.fixture(autouse=True)
def _leave_the_global_rng_alone(dev):
    with torch.random.fork_rng(devices=[dev]):
        yield


def _reduced():
    """2048 input points, 256 seeds (fp_xyz[-1] is the second SA level), num_sampled_seed 256,
    64 proposals."""
    from msmdfusion_amd import configs as C
    model = copy.deepcopy(C.IMVOTENET_STAGE2_SUNRGBD["model"])
    model["pts_backbone"]["num_points"] = (512, SEEDS, 128, 64)
    model["num_sampled_seed"] = SEEDS
    for tower in ("joint", "pts", "img"):
        model["pts_bbox_heads"][tower]["vote_aggregation_cfg"]["num_point"] = 64
    return model


class _Detector2D(torch.nn.Module):
    """The injected image branch: hands out fixed detections; its parameter must stay frozen
    and without a gradient."""

    def __init__(self, boxes):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(1))
        self.boxes = boxes

    def forward(self, img, img_metas):
        return [b * self.weight for b in self.boxes]


def _scene(dev, n=2048):
    """Two clouds inside the camera's frustum, back-projected from pixels so that every point
    -- the seeds are a subset -- lands well inside a pixel and inside the image (the
    composition's gather, like the reference's, asserts on the device otherwise); ground truths
    around some of the points; images, calibration, metas and 2-D detections (12 and none)."""
    from msmdfusion_amd.head_loss import DepthBoxes
    rng = np.random.default_rng(5)
    case = R.make_case(3, n, (12, 0), 10)
    points, boxes, labels = [], [], []
    for b in range(2):
        g = 3 + b
        xyz = case["seeds"][b]
        centre = xyz[rng.integers(0, n, g)].astype(np.float64)
        size = rng.uniform(0.6, 1.4, (g, 3))
        points.append(torch.from_numpy(np.concatenate(
            [xyz, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)).to(dev))
        row = np.concatenate([centre, size, rng.uniform(-3, 3, (g, 1))], 1)
        boxes.append(DepthBoxes(torch.from_numpy(row.astype(np.float32)).to(dev), box_dim=7,
                                with_yaw=True))
        labels.append(torch.from_numpy(rng.integers(0, 10, g)).to(dev))
    imgs, bboxes_2d, _, metas, calibs = R.to_torch(case, dev)
    return dict(points=points, gt_bboxes_3d=boxes, gt_labels_3d=labels, img=imgs,
                img_metas=metas, calib=calibs, bboxes_2d=bboxes_2d)


def _model(dev, **injected):
    from msmdfusion_amd.registry import build_detector
    torch.manual_seed(0)
    return build_detector(_reduced(), **injected).to(dev)


def test_training_step(dev):
    scene = _scene(dev)
    det2d = _Detector2D(scene.pop("bboxes_2d")).to(dev)
    model = _model(dev, img_detector=det2d).train()
    gen = torch.Generator(device=dev).manual_seed(1)
    drop = torch.Generator().manual_seed(2)
    towers = model.tower_losses(scene["points"], scene["img"], scene["img_metas"], scene["calib"],
                                None, scene["gt_bboxes_3d"], scene["gt_labels_3d"],
                                generator=gen, drop_generator=drop)
    losses = model.combine_losses(towers)
    assert sorted(losses) == LOSSES and len(towers) == 3
    for k in LOSSES:
        assert bool(torch.isfinite(losses[k])), k
        want = sum(w * t[k] for w, t in zip([0.4, 0.3, 0.3], towers))
        assert abs(float(losses[k]) - float(want)) <= 1e-6 * max(1.0, abs(float(want))), k
    sum(losses.values()).backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    for prefix in ("img_mlp.", "pts_bbox_head_joint.", "pts_bbox_head_pts.", "pts_bbox_head_img.",
                   "pts_backbone."):
        got = [k for k, g in grads.items() if k.startswith(prefix) and g is not None
               and bool((g != 0).any())]
        assert got, prefix
    assert all(bool(torch.isfinite(g).all()) for g in grads.values() if g is not None)
    # the injected image side: frozen, no gradient, no keys of ours
    assert det2d.weight.requires_grad is False and det2d.weight.grad is None
    assert not any("img_detector" in k for k in model.state_dict())
    # forward_train is the same thing under the same generators
    again = model.forward_train(generator=torch.Generator(device=dev).manual_seed(1),
                                drop_generator=torch.Generator().manual_seed(2), **scene)
    for k in LOSSES:
        assert torch.equal(again[k], losses[k]), k


def test_inference_step(dev):
    from msmdfusion_amd.head_loss import DepthBoxes
    scene = _scene(dev)
    model = _model(dev).eval()
    with torch.no_grad():
        results = model.simple_test(scene["points"], scene["img_metas"], scene["img"],
                                    calibs=scene["calib"], bboxes_2d=scene["bboxes_2d"])
    assert len(results) == 2
    for res in results:
        boxes, scores, labels = res["boxes_3d"], res["scores_3d"], res["labels_3d"]
        assert isinstance(boxes, DepthBoxes) and boxes.with_yaw
        n = len(boxes)
        assert scores.shape == (n,) and labels.shape == (n,)
        assert n == 0 or (0 <= int(labels.min()) and int(labels.max()) < 10)
        assert bool(torch.isfinite(boxes.tensor).all()) and bool((scores >= 0).all())


def test_fusion_through_sampling_reads_nothing_back(dev):
    scene = _scene(dev)
    model = _model(dev).eval()
    with torch.no_grad():
        seeds, feats, inds = model.extract_pts_feat(torch.stack(scene["points"]))
        assert tuple(seeds.shape) == (2, SEEDS, 3)
        gen = torch.Generator(device=dev).manual_seed(3)
        model.fuse_and_sample(scene["img"], scene["bboxes_2d"], seeds, feats, inds,
                              scene["img_metas"], scene["calib"], generator=gen)      # warm
        torch.cuda.synchronize()
        gen.manual_seed(3)
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = model.fuse_and_sample(scene["img"], scene["bboxes_2d"], seeds, feats, inds,
                                        scene["img_metas"], scene["calib"], generator=gen)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    s3d, f3d, fimg, sidx = out
    assert tuple(s3d.shape) == (2, SEEDS, 3) and tuple(f3d.shape) == (2, 256, SEEDS)
    assert tuple(fimg.shape) == (2, 256, SEEDS) and tuple(sidx.shape) == (2, SEEDS)
    # the gathered rows belong together: the sampled seed is the point its index names
    cloud = torch.stack(scene["points"])
    for b in range(2):
        assert torch.equal(cloud[b][sidx[b].long(), :3], s3d[b])


def test_fused_and_composed_fusion_give_the_same_losses(dev):
    scene = _scene(dev)
    model = _model(dev).train()

    def run(composed):
        layer = model.fusion_layer
        if composed:
            layer.forward = layer.forward_composed
        try:
            torch.manual_seed(4)
            return model.forward_train(generator=torch.Generator(device=dev).manual_seed(1),
                                       drop_generator=torch.Generator().manual_seed(2), **scene)
        finally:
            layer.__dict__.pop("forward", None)

    fused, composed = run(False), run(True)
    for k in LOSSES:
        # the cue rows differ by float32 roundings (1e-6); a loss is a sum of ~500 terms
        assert abs(float(fused[k]) - float(composed[k])) <= 1e-3 * max(1.0, abs(float(fused[k]))), k


def test_state_dict_round_trips_under_the_reference_names(dev):
    model = _model(dev)
    sd = model.state_dict()
    prefixes = {k.split(".")[0] for k in sd}
    assert prefixes == {"pts_backbone", "pts_bbox_head_joint", "pts_bbox_head_pts",
                        "pts_bbox_head_img", "img_mlp"}
    for k in ("img_mlp.mlp.layer0.conv.weight", "img_mlp.mlp.layer0.conv.bias",
              "img_mlp.mlp.layer1.bn.running_mean", "pts_backbone.SA_modules.0.mlps.0.layer0.conv.weight",
              "pts_bbox_head_joint.vote_module.vote_conv.0.conv.weight",
              "pts_bbox_head_img.conv_pred.conv_cls.weight"):
        assert k in sd, k
    other = _model(dev)
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    missing, unexpected = other.load_state_dict(copy.deepcopy(sd), strict=True)
    assert not missing and not unexpected
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k]), k
