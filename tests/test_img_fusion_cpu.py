"""TransFusionHeadLC (fuse_img=True) on the CPU: the composition path against the outputs of the
reference's own forward_single (tests/golden/img_fusion_vectors.npz, made by
tests/golden/make_img_fusion_golden.py), the numpy restatements of tests/img_fusion_ref.py
against the same file, configs, registry routing, refusals, C-ABI argument validation and the
BatchNorm closed forms."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import img_fusion_ref as R  # noqa: E402
from img_fusion_ref import CFG, gold_inputs, gold_metas, lc_head, loss_of  # noqa: E402

from msmdfusion_amd import fusion_head as FH  # noqa: E402
from msmdfusion_amd.fusion_head import TransFusionHeadLC  # noqa: E402
from msmdfusion_amd.head import PositionEmbeddingLearned, TransFusionHead  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "img_fusion_vectors.npz"))


@pytest.fixture(scope="module")
def proto():
    return lc_head(fused=False)


def _check(ours, gold, tag, key):
    ok, err, margin = R.within_reference_error(ours, gold[tag + "f32/" + key],
                                               gold[tag + "f64/" + key])
    assert ok, "%s%s: error %.3g > margin %.3g" % (tag, key, err, margin)


@pytest.mark.parametrize("batch", [2, 1])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_composition_matches_the_reference(gold, proto, batch, mode):
    head = copy.deepcopy(proto).train(mode == "train")
    x, img = gold_inputs(batch)
    keep = img.clone()
    with torch.no_grad():
        (res,) = head.forward_single(x, img, gold_metas(gold, batch))
    tag = "B%d_%s_" % (batch, mode)
    assert torch.equal(img, keep)                                   # the image input is left alone
    np.testing.assert_array_equal(head.on_the_image_mask.numpy(), gold[tag + "f64/on_the_image_mask"])
    np.testing.assert_array_equal(head.query_labels.numpy(), gold[tag + "f64/query_labels"])
    assert sorted(res) == sorted(["center", "height", "dim", "rot", "vel", "heatmap",
                                  "query_heatmap_score", "dense_heatmap"])
    for k, v in res.items():
        _check(v.numpy(), gold, tag, k)
    if mode == "train":
        for k, v in head.state_dict().items():
            if "running_" in k:
                _check(v.numpy(), gold, tag, "buf/" + k)
            elif "num_batches_tracked" in k:
                assert int(v) == int(gold[tag + "f64/buf/" + k]), k


def test_the_golden_scene_has_the_promised_groups(gold):
    count = gold["B2_train_f64/count"]
    assert count[0, 2] == 0 and count[1, 0] == 1 and count[1, 1] == 2 and count[1, 2] >= 8
    assert count[0, 0] >= 2 and count[0, 1] >= 2
    mask = gold["B2_train_f64/on_the_image_mask"]
    assert mask.any() and not mask.all()


def test_composition_gradients_match_the_reference(gold, proto):
    head = copy.deepcopy(proto).train()
    x, img = gold_inputs(2)
    x.requires_grad_(True), img.requires_grad_(True)
    (res,) = head.forward_single(x, img, gold_metas(gold, 2))
    loss_of(res).backward()
    _check(x.grad.numpy(), gold, "B2_train_", "grad_x")
    _check(img.grad.numpy(), gold, "B2_train_", "grad_img")
    assert float(img.grad.abs().max()) > 0


def test_numpy_geometry_matches_the_reference(gold):
    """The restated geometry reproduces the reference's on_the_image_mask and member counts
    from the boxes its own forward saw (float32 and float64)."""
    pos3d, boxes = gold["B2_train_f64/pos3d"], gold["B2_train_f64/boxes"]
    params = FH.geometry_params(gold_metas(gold, 2), CFG["num_views"], skip_flow=False)
    for dtype in (np.float64, np.float32):
        g = R.geometry(pos3d.astype(dtype), boxes.astype(dtype), params.astype(dtype),
                       CFG["out_size_factor_img"], dtype)
        np.testing.assert_array_equal(g["mask"], gold["B2_train_f64/on_the_image_mask"])
        np.testing.assert_array_equal(g["count"], gold["B2_train_f64/count"])
        assert (g["winner"][0][g["on"][0, 0] & g["on"][0, 1]] == 1).all()      # the later view wins


def test_numpy_attention_matches_the_masked_attention():
    """dense_attention == torch's attention under the reference's log-mask (:996-1003)."""
    rng = np.random.RandomState(3)
    h, w, heads, c, rows = 5, 7, 2, 16, 6
    q, k, v = rng.standard_normal((rows, c)), rng.standard_normal((1, h * w, c)), \
        rng.standard_normal((1, h * w, c))
    centre = np.stack([rng.randint(0, w, rows), rng.randint(0, h, rows)], 1)
    radius = rng.randint(0, 4, rows)
    sigma = ((radius * 2 + 1) / 6.0).astype(np.float32)
    view = np.zeros(rows, np.int64)
    ours = R.dense_attention(q, k, v, view, centre, sigma, rows, 1, h, w, heads)
    pos = FH.TransFusionHead.create_2D_grid(h, w)
    dist = (torch.from_numpy(centre).int()[:, None, :] - (pos - 0.5)).norm(dim=-1) ** 2
    mask = (-dist / (2 * torch.from_numpy(sigma)[:, None] ** 2)).exp()
    mask[mask < torch.finfo(torch.float32).eps] = 0
    tq, tk, tv = (torch.from_numpy(a).double() for a in (q, k[0], v[0]))
    d = c // heads
    want = torch.cat([torch.softmax(tq[:, s:s + d] @ tk[:, s:s + d].T / d ** 0.5
                                    + mask.log().double(), -1) @ tv[:, s:s + d]
                      for s in range(0, c, d)], 1)
    np.testing.assert_allclose(ours, want.numpy(), rtol=1e-5, atol=1e-6)


def test_window_membership_equals_the_thresholded_mask():
    """exp(-d2 / 2 sigma^2) >= eps as the kernels compute it == the reference's thresholded
    mask (sqrt, square, divide, exp in torch float32), for every radius 0..64 and every d2 of a
    128 x 128 map."""
    d2 = np.unique((np.arange(128)[:, None] ** 2 + np.arange(128)[None] ** 2).reshape(-1))
    xy = [(a, b) for a in range(128) for b in range(128)]
    by_d2 = {}
    for a, b in xy:
        by_d2.setdefault(a * a + b * b, (a, b))
    cells = torch.tensor([by_d2[int(v)] for v in d2], dtype=torch.float32)     # [N, 2]
    centre = torch.zeros((1, 1, 2), dtype=torch.int32)
    dist = (centre - cells[None]).norm(dim=-1) ** 2                            # [1, N]
    for radius in range(65):
        sigma = (torch.tensor([radius], dtype=torch.int32) * 2 + 1) / 6.0
        mask = (-dist / (2 * sigma[:, None] ** 2)).exp()
        want = ~(mask < torch.finfo(torch.float32).eps)
        got = R.window(d2.astype(np.float32), sigma.numpy()[0])
        assert np.array_equal(got, want[0].numpy()), radius


def test_dropout_mix_is_a_fair_coin():
    keep = R.keep_mask(12345678901234567, 0.25, 3, 2, 4096)
    assert keep.shape == (3, 2, 4096)
    n = keep.size
    assert abs(keep.mean() - 0.75) <= 4 * np.sqrt(0.25 * 0.75 / n)
    assert not np.array_equal(keep[0, 0], keep[0, 1]) and not np.array_equal(keep[0], keep[1])
    assert R.keep_mask(5, 0.0, 2, 2, 64).all()
    # the documented constants, one value by hand
    x = R._fmix(np.uint64(1))
    assert int(x) == 0x514E28B7                                       # murmur3 fmix32(1)


def test_state_dict_of_the_voxel_lc_config():
    from msmdfusion_amd import configs as C
    head = C.build_head(C.TRANSFUSION_VOXEL_LC)
    assert type(head) is TransFusionHeadLC and head.num_views == 6
    sd = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    assert sd["shared_conv_img.weight"] == (128, 256, 3, 3)
    assert sd["heatmap_head_img.0.conv.weight"] == (128, 128, 3, 3)
    assert sd["heatmap_head_img.1.weight"] == (10, 128, 3, 3)
    assert sd["fc.0.weight"] == (128, 128, 1)
    assert sd["prediction_heads.1.center.0.conv.weight"] == (64, 256, 1)
    assert sd["prediction_heads.0.center.0.conv.weight"] == (64, 128, 1)
    assert len(head.decoder) == 1 + 1 + 6
    assert "decoder.1.self_attn.in_proj_weight" in sd
    for i in range(2, 8):
        assert "decoder.%d.multihead_attn.in_proj_weight" % i in sd
        assert "decoder.%d.self_attn.in_proj_weight" % i not in sd
        assert "decoder.%d.self_posembed.position_embedding_head.1.running_mean" % i in sd
    assert all(m.momentum == 0.1 for m in head.modules()
               if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)))
    pillar = C.build_head(C.TRANSFUSION_PILLAR_LC)
    assert type(pillar) is TransFusionHeadLC
    assert tuple(pillar.state_dict()["shared_conv.weight"].shape) == (128, 384, 3, 3)


def test_batchnorms_run_on_torchs_own_kernels_under_the_same_keys():
    """Every BatchNorm of the LC head is the native-kernel form (MIOpen's training statistics
    lose digits on the position grids): same keys, same values as nn.BatchNorm on the CPU."""
    head = lc_head(fused=False)
    norms = [m for m in head.modules() if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d))]
    assert len(norms) > 20 and all(isinstance(m, FH._NativeBatchNorm) for m in norms)
    assert all(m.momentum == 0.1 for m in norms)
    plain = nn.BatchNorm1d(6).train()
    ours = FH.use_native_batchnorm(nn.Sequential(copy.deepcopy(plain)))[0]
    assert sorted(ours.state_dict()) == sorted(plain.state_dict())
    x = torch.randn(3, 6, 11)
    assert torch.equal(ours(x), plain(x)) and torch.equal(ours.running_var, plain.running_var)


def test_lc_configs_equal_the_reference_dicts():
    from msmdfusion_amd import configs as C
    fx = json.load(open(os.path.join(GOLDEN, "reference_transfusion_lc_configs.json")))
    norm = lambda o: json.loads(json.dumps(o))   # tuples -> lists
    assert norm(C.TRANSFUSION_VOXEL_LC) == fx["transfusion_nusc_voxel_LC"]
    assert norm(C.TRANSFUSION_PILLAR_LC) == fx["transfusion_nusc_pillar_LC"]


def test_registry_routes_fuse_img_to_the_lc_class():
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.registry import HEADS, build_head
    m = C.TRANSFUSION_PILLAR_LC["model"]
    cfg = dict(m["pts_bbox_head"], train_cfg=m["train_cfg"]["pts"], test_cfg=m["test_cfg"]["pts"])
    assert cfg["type"] == "TransFusionHead" and cfg["fuse_img"]
    assert type(build_head(cfg)) is TransFusionHeadLC
    assert HEADS.get("TransFusionHeadLC") is TransFusionHeadLC
    plain = dict(cfg, fuse_img=False)
    for k in ("num_views", "in_channels_img", "out_size_factor_img"):
        plain.pop(k)
    assert type(build_head(plain)) is TransFusionHead
    from msmdfusion_amd.detector import _build_head
    assert type(_build_head(m["pts_bbox_head"], m["train_cfg"], m["test_cfg"], False)) \
        is TransFusionHeadLC


def test_refusals():
    args = {k: v for k, v in CFG.items()}
    with pytest.raises(NotImplementedError, match="TransFusionHeadLC"):
        TransFusionHead(fuse_img=True, **{k: v for k, v in args.items()
                                          if k not in ("num_views", "in_channels_img",
                                                       "out_size_factor_img")})
    with pytest.raises(ValueError, match="num_views"):
        TransFusionHeadLC(**dict(args, num_views=0))
    with pytest.raises(ValueError, match="fuse_img"):
        TransFusionHeadLC(**dict(args, fuse_img=False))
    with pytest.raises(NotImplementedError, match="initialize_by_heatmap"):
        TransFusionHeadLC(**dict(args, initialize_by_heatmap=False))
    head = lc_head(fused=False)
    x, img = gold_inputs(2)
    with pytest.raises(ValueError, match="img_inputs"):
        head.forward_single(x, None, None)
    with pytest.raises(ValueError, match="num_views"):
        head.forward_single(x, img[:5], [{}, {}])
    from msmdfusion_amd import head_loss as HL
    two = TransFusionHeadLC(**dict(args, num_decoder_layers=2, auxiliary=True))
    with pytest.raises(NotImplementedError, match="ill-defined"):
        HL.loss(two, [], [], None)


def test_kernel_wrappers_validate_their_arguments():
    from msmdfusion_amd import kernels as K
    assert K.gauss_attn_supported(128, 8) and K.gauss_attn_supported(32, 4)
    assert K.gauss_attn_supported(64, 2) and K.gauss_attn_supported(256, 8)
    assert not K.gauss_attn_supported(64, 1) and not K.gauss_attn_supported(512, 16)
    assert not K.gauss_attn_supported(48, 5) and not K.gauss_attn_supported(24, 8)
    assert K.IMG_GEOMETRY_MAX_QUERIES >= 1024 and K.IMG_GEOMETRY_MAX_VIEWS >= 8
    assert K.GAUSS_ATTN_KEY_TILE == 256 and K.GAUSS_ATTN_ROW_CHUNK == 64
    pos, boxes, params = torch.zeros((1, 3, 4)), torch.zeros((1, 4, 7)), torch.zeros((1, 2, 20))
    with pytest.raises(RuntimeError, match="CUDA"):
        K.img_query_geometry(pos, boxes, params, 4)
    q, kv = torch.zeros((4, 32)), torch.zeros((2, 6, 32))
    ints = torch.zeros((4,), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA"):
        K.gauss_attn_forward(q, kv, kv, ints, torch.zeros((4, 2), dtype=torch.int32),
                             torch.ones(4), 2, 2, 3, 4)
    from msmdfusion_amd._lib import lib
    # the C ABI refuses what the kernels are not built for before touching a pointer
    assert lib.msmd_img_query_geometry_f32(*([None] * 3), 1, 2000, 2, 4.0, *([None] * 13)) == -3
    assert lib.msmd_img_query_geometry_f32(*([None] * 3), 1, 10, 9, 4.0, *([None] * 13)) == -3
    assert lib.msmd_img_query_geometry_f32(*([None] * 3), 1, 10, 0, 4.0, *([None] * 13)) == -1
    assert lib.msmd_img_query_geometry_f32(*([None] * 3), 1, 10, 2, 0.0, *([None] * 13)) == -1
    fwd = lambda c, heads, p=0.0, h=2, w=2: lib.msmd_gauss_attn_fwd_f32(
        *([None] * 6), 1, 4, 2, h, w, c, heads, p, 0, None, None, None)
    assert fwd(64, 1) == -3 and fwd(512, 16) == -3 and fwd(48, 5) == -3
    assert fwd(32, 4, p=1.0) == -1 and fwd(32, 4, p=-0.1) == -1 and fwd(32, 4, h=0) == -1
    assert fwd(32, 4) == -1                                         # null pointers
    assert lib.msmd_gauss_attn_bwd_f32(*([None] * 9), 1, 4, 2, 2, 2, 64, 1, 0.0, 0,
                                       *([None] * 5)) == -3


def _literal_groups(pe, pos, member, valid):
    """The reference's sequence: one module call per valid group, in order."""
    out = torch.zeros(pos.shape[0], pos.shape[1], pe.position_embedding_head[0].weight.shape[0],
                      dtype=pos.dtype)
    for g in range(pos.shape[0]):
        if valid[g]:
            idx = torch.where(member[g])[0]
            out[g, idx] = pe(pos[g, idx][None])[0].t()
    return out


@pytest.mark.parametrize("train", [True, False])
def test_bn_closed_forms_equal_the_literal_sequence(train):
    torch.manual_seed(0)
    G, N, C = 7, 9, 6
    pe = PositionEmbeddingLearned(2, C).double()
    bn = pe.position_embedding_head[1]
    bn.momentum = 0.1
    with torch.no_grad():
        bn.running_mean.normal_(), bn.running_var.uniform_(0.5, 2)
        bn.weight.uniform_(0.5, 1.5), bn.bias.normal_()
    pe.train(train)
    pos = torch.randn(G, N, 2, dtype=torch.float64) * 3
    on = torch.rand(G, N) < 0.6
    on[1], on[4] = False, False
    on[4, 2] = True                                    # an empty group and a group of one
    on[5, :2], on[5, 2:] = True, False                 # a group of exactly two
    valid = on.sum(1) > 1
    member = on & valid[:, None]
    pos[~member] = float("nan")                        # must be selected away
    a, b = copy.deepcopy(pe), copy.deepcopy(pe)
    want = _literal_groups(a, torch.nan_to_num(pos), member, valid)
    got = FH.posembed_groups(b, pos.clone().requires_grad_(False), member, valid)
    torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10)
    for name in ("running_mean", "running_var"):
        torch.testing.assert_close(getattr(b.position_embedding_head[1], name),
                                   getattr(a.position_embedding_head[1], name),
                                   rtol=1e-10, atol=1e-12)
    assert int(b.position_embedding_head[1].num_batches_tracked) == \
        int(a.position_embedding_head[1].num_batches_tracked) == (int(valid.sum()) if train else 0)
    # gradients stay finite although the unused positions are NaN
    c = copy.deepcopy(pe)
    FH.posembed_groups(c, pos, member, valid).sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in c.parameters())

    # the same positions `k` times
    a, b = copy.deepcopy(pe), copy.deepcopy(pe)
    grid = torch.randn(1, 11, 2, dtype=torch.float64)
    for _ in range(int(valid.sum())):
        want = a(grid)
    got = FH.posembed_repeated(b, grid, valid.sum())
    torch.testing.assert_close(got.transpose(1, 2), want, rtol=1e-10, atol=1e-10)
    for name in ("running_mean", "running_var", "num_batches_tracked"):
        torch.testing.assert_close(getattr(b.position_embedding_head[1], name),
                                   getattr(a.position_embedding_head[1], name),
                                   rtol=1e-10, atol=1e-12)
    # zero calls leave the statistics alone
    b2 = copy.deepcopy(pe)
    FH.posembed_repeated(b2, grid, torch.zeros((), dtype=torch.long))
    assert torch.equal(b2.position_embedding_head[1].running_mean, bn.running_mean)
    assert int(b2.position_embedding_head[1].num_batches_tracked) == 0


def test_base_head_still_refuses_fuse_img():
    from msmdfusion_amd import configs as C
    args = {k: v for k, v in C._PTS_BBOX_HEAD.items() if k != "type"}
    with pytest.raises(NotImplementedError):
        TransFusionHead(fuse_img=True, test_cfg=dict(C._TEST_CFG_PTS), **args)
