"""The H3DNet detector built from configs.H3DNET_SCANNET, shrunk to a few hundred points and 16
proposals: one training step, one inference step, the state-dict keys."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
POINTS, PROPOSALS = 512, 16


def _reduced():
    """512 input points, set abstraction down to (128, 64, 32, 16) points: 64 seeds.  The rpn
    head takes 16 proposals; a primitive head takes one centre per seed, as in the reference's
    config (its flags are per seed); the matchers of the bbox head follow the proposals (6 and
    12 cue centres each)."""
    from msmdfusion_amd import configs as C
    model = copy.deepcopy(C.H3DNET_SCANNET["model"])
    model["backbone"]["backbones"]["num_points"] = (128, 64, 32, 16)
    model["rpn_head"]["vote_aggregation_cfg"]["num_point"] = PROPOSALS
    for primitive in model["roi_head"]["primitive_list"]:
        primitive["vote_aggregation_cfg"]["num_point"] = 64
    head = model["roi_head"]["bbox_head"]
    head["num_proposal"] = PROPOSALS
    head["suface_matching_cfg"]["num_point"] = PROPOSALS * 6
    head["line_matching_cfg"]["num_point"] = PROPOSALS * 12
    return model


def _scene(dev, batch=2, n=POINTS):
    from msmdfusion_amd.head_loss import DepthBoxes
    rng = np.random.default_rng(5)
    points, boxes, labels, semantic, instance = [], [], [], [], []
    for b in range(batch):
        g = 2 + b
        centre = rng.uniform(-2, 2, (g, 3)) * [1, 1, 0] + [0, 0, 0.1]
        size = rng.uniform(0.6, 1.6, (g, 3))
        owner = rng.integers(0, g + 1, n)                       # g = background
        inside = owner < g
        at = np.minimum(owner, g - 1)
        xyz = rng.uniform(-3, 3, (n, 3)) * [1, 1, 0.3] + [0, 0, 1]
        xyz[inside] = (centre[at] + [0, 0, 0.5] * size[at] +
                       rng.uniform(-0.5, 0.5, (n, 3)) * size[at])[inside]
        points.append(torch.from_numpy(np.concatenate(
            [xyz, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)).to(dev))
        boxes.append(DepthBoxes(torch.from_numpy(np.concatenate([centre, size], 1).astype(
            np.float32)).to(dev), box_dim=6, with_yaw=False))
        label = rng.integers(0, 18, g)
        labels.append(torch.from_numpy(label).to(dev))
        semantic.append(torch.from_numpy(np.where(inside, label[at], 18)).to(dev))
        instance.append(torch.from_numpy(owner).to(dev))
    return points, boxes, labels, dict(pts_semantic_mask=semantic, pts_instance_mask=instance)


@pytest.fixture(scope="module")
def model(dev):
    from msmdfusion_amd.registry import build_detector
    torch.manual_seed(0)
    return build_detector(_reduced()).to(dev)


def test_training_step(dev, model):
    points, boxes, labels, extra = _scene(dev)
    model.train()
    optimiser = torch.optim.SGD(model.parameters(), lr=1e-3)
    kept = [len(b) for b in boxes]
    losses = model.forward_train(points, None, boxes, labels, **extra)
    assert [len(b) for b in boxes] == kept
    want = {"vote_loss", "objectness_loss", "semantic_loss", "center_loss", "dir_class_loss",
            "dir_res_loss", "size_class_loss", "size_res_loss"}
    want |= {k + "_optimized" for k in want if k != "vote_loss"}
    want |= {"%s_%s" % (k, m) for m in ("z", "xy", "line")
             for k in ("flag_loss", "vote_loss", "center_loss", "size_loss", "sem_loss")}
    want |= {"primitive_objectness_loss", "primitive_sem_loss", "primitive_matching_loss",
             "primitive_sem_matching_loss", "primitive_centroid_reg_loss"}
    assert set(losses) == want
    assert all(bool(torch.isfinite(v).all()) for v in losses.values())
    total = sum(losses.values())
    total.backward()
    for prefix in ("backbone.", "rpn_head.", "roi_head.primitive_z.", "roi_head.primitive_xy.",
                   "roi_head.primitive_line.", "roi_head.bbox_head."):
        named = [(k, p) for k, p in model.named_parameters() if k.startswith(prefix)]
        assert named, prefix
        missing = [k for k, p in named if p.grad is None]
        assert not missing, missing
        assert all(bool(torch.isfinite(p.grad).all()) for _, p in named), prefix
    before = [p.detach().clone() for p in model.parameters()]
    optimiser.step()
    assert any(not torch.equal(a, p) for a, p in zip(before, model.parameters()))


def test_inference_step(dev, model):
    from msmdfusion_amd.head_loss import DepthBoxes
    points, _, _, _ = _scene(dev)
    model.eval()
    with torch.no_grad():
        results = model.simple_test(points)
    assert len(results) == 2
    for res in results:
        boxes, scores, labels = res["boxes_3d"], res["scores_3d"], res["labels_3d"]
        n = len(boxes)
        assert isinstance(boxes, DepthBoxes) and not boxes.with_yaw
        assert scores.shape == (n,) and labels.shape == (n,) and n % 18 == 0
        assert n == 0 or (0 <= int(labels.min()) and int(labels.max()) < 18)
        assert bool(torch.isfinite(boxes.tensor).all()) and bool((scores >= 0).all())


def test_state_dict_keys_carry_the_reference_attribute_names(model):
    keys = list(model.state_dict())
    for prefix in ("backbone.backbone_list.0.", "backbone.aggregation_layers.layer0.", "rpn_head.vote_module.",
                   "rpn_head.conv_pred.", "roi_head.primitive_z.flag_conv.",
                   "roi_head.primitive_xy.vote_aggregation.", "roi_head.primitive_line.conv_pred.",
                   "roi_head.bbox_head.surface_center_matcher.mlps.0.layer0.conv.weight",
                   "roi_head.bbox_head.line_center_matcher.", "roi_head.bbox_head.matching_conv.conv.",
                   "roi_head.bbox_head.matching_pred.weight",
                   "roi_head.bbox_head.semantic_matching_conv.bn.",
                   "roi_head.bbox_head.semantic_matching_pred.bias",
                   "roi_head.bbox_head.surface_feats_aggregation.1.conv.",
                   "roi_head.bbox_head.line_feats_aggregation.0.bn.",
                   "roi_head.bbox_head.bbox_pred.0.conv.weight", "roi_head.bbox_head.bbox_pred.3.bias"):
        assert any(k.startswith(prefix) for k in keys), prefix
    tops = {k.split(".")[0] for k in keys}
    assert tops == {"backbone", "rpn_head", "roi_head"}
    assert {k.split(".")[1] for k in keys if k.startswith("roi_head.")} == \
        {"primitive_z", "primitive_xy", "primitive_line", "bbox_head"}
