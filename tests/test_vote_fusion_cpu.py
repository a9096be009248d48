"""ImVoteNet's pieces without a GPU: VoteFusion's composition and the tests' restatement against
the reference's own outputs (tests/golden/vote_fusion_vectors.npz, written by
make_vote_fusion_golden.py), the 'DEPTH' 3-D flow, the 2-D transforms, the composed parameter
block, the batched sample_valid_seeds, MLP / ImVoteNet key names, the config fixture and the
C-ABI refusals."""
import ctypes
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import imvote_ref as R  # noqa: E402

from msmdfusion_amd import fusion_layers as FL  # noqa: E402
from msmdfusion_amd.fusion_layers import VoteFusion  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _case(g, name, dtype=torch.float32):
    meta = json.loads(str(g[name + "/meta"]))
    b = g[name + "/seeds"].shape[0]
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)      # noqa: E731
    return (meta, t(g[name + "/imgs"].astype(np.float32)),
            [t(g[name + "/boxes/%d" % i]) for i in range(b)], t(g[name + "/seeds"]),
            dict(Rt=t(g[name + "/Rt"]), K=t(g[name + "/K"])))


CASES = ("c10", "c3")


@pytest.mark.parametrize("name", CASES)
def test_composed_equals_the_reference(golden, name):
    meta, imgs, boxes, seeds, calibs = _case(golden, name)
    layer = VoteFusion(meta["num_classes"], meta["max_imvote_per_pixel"])
    before = imgs.clone()
    feat, mask = layer.forward_composed(imgs, boxes, seeds, meta["metas"], calibs)
    assert torch.equal(imgs, before), "the input image was modified"
    assert mask.dtype == torch.bool and torch.equal(mask, torch.from_numpy(golden[name + "/mask"]))
    assert torch.equal(feat, torch.from_numpy(golden[name + "/feat32"]))
    # CPU tensors take the composition through forward() as well
    f2, m2 = layer(imgs, boxes, seeds, meta["metas"], calibs)
    assert torch.equal(f2, feat) and torch.equal(m2, mask)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("dtype", (torch.float32, torch.float64))
def test_restatement_equals_the_reference(golden, name, dtype):
    meta, imgs, boxes, seeds, calibs = _case(golden, name, dtype)
    k = meta["max_imvote_per_pixel"]
    feat, mask, det = R.vote_fusion_ref(imgs, boxes, seeds, meta["metas"], calibs,
                                        meta["num_classes"], k, dtype=dtype)
    want = golden[name + ("/feat32" if dtype == torch.float32 else "/feat64")]
    assert torch.equal(mask, torch.from_numpy(golden[name + "/mask"]))
    assert torch.equal(feat, torch.from_numpy(want))
    for i, d in enumerate(det):
        assert np.array_equal(d["uv"].numpy(), golden[name + "/uv_origin/%d" % i])
        if boxes[i].shape[0]:
            # chosen slots: exact wherever the slot is visible (in a box, or conf == 1)
            vis = np.floor(golden[name + "/chosen_score/%d" % i]) != 0
            assert np.array_equal(d["chosen"].numpy()[vis], golden[name + "/chosen/%d" % i][vis])
            inb = np.take_along_axis(np.concatenate(
                [golden[name + "/in_box/%d" % i],
                 np.zeros((seeds.shape[1], max(k - boxes[i].shape[0], 0)), bool)], 1),
                golden[name + "/chosen/%d" % i].astype(np.int64), 1)
            assert np.array_equal(d["in_box"].numpy()[vis], inb[vis])


def test_golden_covers_the_cases(golden):
    """What the issue asks the vectors to hold."""
    g = golden
    meta = json.loads(str(g["c10/meta"]))
    nbs = [g["c10/boxes/%d" % i].shape[0] for i in range(3)]
    assert nbs == [7, 0, 2] and meta["max_imvote_per_pixel"] == 3
    flows = sorted(json.dumps(m.get("transformation_3d_flow", [])) for m in meta["metas"])
    assert flows == sorted(json.dumps(f) for f in ([], ["HF", "R", "S", "T"], ["R", "S", "T", "HF"]))
    assert any(m.get("flip") and "scale_factor" in m for m in meta["metas"])
    assert any(not m.get("flip") and "scale_factor" in m for m in meta["metas"])
    assert (g["c10/boxes/0"][:, 4] == 1.0).sum() == 1
    assert json.loads(str(g["c3/meta"]))["num_classes"] == 3
    # an out-of-box pair with conf == 1: valid with zero cues
    m = torch.from_numpy(g["c10/mask"])[0]
    f = torch.from_numpy(g["c10/feat32"])[0]
    zero_valid = m & (f[:15].abs().sum(0) == 0)
    assert int(zero_valid.sum()) > 0
    # the box-free sample: slot 0 valid, the others not, zero cues
    s = g["c10/seeds"].shape[1]
    assert g["c10/mask"][1, :s].all() and not g["c10/mask"][1, s:].any()
    assert not g["c10/feat32"][1, :15].any()


# ---- the 3-D flow ------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ("a", "b", "vf"))
def test_depth_flow_matches_the_reference(golden, tag):
    meta = json.loads(str(golden["flow/%s/meta" % tag]))
    pts = torch.from_numpy(golden["flow/pts"])
    for rev in (False, True):
        name = "flow/%s/%s" % (tag, "reverse" if rev else "forward")
        got32 = FL.apply_3d_transformation(pts, "DEPTH", meta, reverse=rev)
        assert torch.equal(got32, torch.from_numpy(golden[name + "32"]))
        got64 = FL.apply_3d_transformation(pts.double(), "DEPTH", meta, reverse=rev)
        assert torch.equal(got64, torch.from_numpy(golden[name + "64"]))


def test_flow_matrix_matches_the_stepwise_flow_for_every_order():
    rng = np.random.RandomState(3)
    pts = torch.from_numpy(rng.uniform(-3, 3, (17, 3)))
    a = 0.4
    full = dict(pcd_rotation=[[np.cos(a), np.sin(a), 0], [-np.sin(a), np.cos(a), 0], [0, 0, 1.0]],
                pcd_scale_factor=1.07, pcd_trans=[0.3, -0.2, 0.1], pcd_horizontal_flip=True,
                pcd_vertical_flip=True)
    metas = [dict(full, transformation_3d_flow=list(p))
             for p in itertools.permutations(["T", "S", "R", "HF", "VF"])]
    metas += [dict(), dict(transformation_3d_flow=["R", "S", "T", "HF", "VF"]),    # the defaults
              dict(transformation_3d_flow=["HF", "VF"], pcd_horizontal_flip=True),
              dict(transformation_3d_flow=["T", "S"], pcd_trans=[1.0, 2.0, 3.0])]
    for coords in ("DEPTH", "LIDAR"):
        for meta in metas:
            for rev in (False, True):
                m = FL.flow_matrix(meta, reverse=rev, coords_type=coords)
                want = FL.apply_3d_transformation(pts, coords, meta, reverse=rev).numpy()
                got = pts.numpy() @ m[:3, :3].T + m[:3, 3]
                assert np.abs(got - want).max() <= 1e-12, (coords, meta, rev)
    # 'LIDAR' is the default and 'CAMERA' is still not built
    assert np.array_equal(FL.flow_matrix(metas[5]), FL.flow_matrix(metas[5], coords_type="LIDAR"))
    with pytest.raises(NotImplementedError):
        FL.apply_3d_transformation(pts, "CAMERA", metas[0])
    with pytest.raises(NotImplementedError):
        FL.flow_matrix(metas[0], coords_type="CAMERA")


# ---- the 2-D transforms ------------------------------------------------------------------------
def test_2d_transforms_match_the_reference_and_round_trip(golden):
    meta = json.loads(str(golden["t2d/meta"]))
    bx, uv = torch.from_numpy(golden["t2d/boxes"]), torch.from_numpy(golden["t2d/uv"])
    for o2n in (False, True):
        assert torch.equal(FL.bbox_2d_transform(meta, bx, o2n),
                           torch.from_numpy(golden["t2d/boxes_%d" % o2n]))
        assert torch.equal(FL.coord_2d_transform(meta, uv, o2n),
                           torch.from_numpy(golden["t2d/uv_%d" % o2n]))
    b64, u64 = bx.double(), uv.double()
    back = FL.bbox_2d_transform(meta, FL.bbox_2d_transform(meta, b64, False), True)
    assert (back - b64).abs().max() < 1e-12
    back = FL.coord_2d_transform(meta, FL.coord_2d_transform(meta, u64, True), False)
    assert (back - u64).abs().max() < 1e-12
    assert torch.equal(bx, torch.from_numpy(golden["t2d/boxes"]))       # inputs untouched


# ---- the parameter block -----------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_parameter_block_reproduces_the_camera_coordinates(golden, name):
    meta, _, _, seeds, calibs = _case(golden, name, torch.float64)
    # (float64 before the single rounding: the composition itself)
    b = seeds.shape[0]
    p = _params64(meta["metas"], calibs)
    for i in range(b):
        m_cam = p[i, :12].reshape(3, 4)
        cam = seeds[i].numpy() @ m_cam[:, :3].T + m_cam[:, 3]
        want = golden[name + "/xyz_cam64/%d" % i]
        assert np.abs(cam - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        assert np.array_equal(p[i, 12:21].reshape(3, 3), golden[name + "/K"][i])
        assert p[i, 40] == golden[name + "/K"][i, 0, 0]
    p32 = FL.vote_fusion_params(meta["metas"], calibs)
    assert p32.dtype == torch.float32 and tuple(p32.shape) == (b, 41)
    assert np.array_equal(p32.numpy(), p.astype(np.float32))
    # numpy / list calibration is taken as well
    p_np = FL.vote_fusion_params(meta["metas"], dict(Rt=golden[name + "/Rt"], K=golden[name + "/K"]))
    assert torch.equal(p_np, p32)


def _params64(metas, calibs):
    """vote_fusion_params before its rounding, recomputed step by step in numpy float64."""
    out = []
    d2c = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]])
    c2d = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0.0]])
    for i, m in enumerate(metas):
        rt, k = calibs["Rt"][i].numpy(), calibs["K"][i].numpy()
        rev = FL.flow_matrix(m, reverse=True, coords_type="DEPTH")
        fwd = FL.flow_matrix(m, reverse=False, coords_type="DEPTH")
        m_cam = (d2c @ rt.T) @ rev[:3]
        m_vote = np.concatenate([fwd[:3, :3] @ (rt @ c2d), fwd[:3, 3:]], 1)
        tail = list(m.get("scale_factor", [1.0, 1.0])[:2]) + list(m.get("img_crop_offset", [0, 0])) \
            + [1.0 if m.get("flip", False) else 0.0] + [float(v) for v in m["img_shape"][:2]]
        out.append(np.concatenate([m_cam.reshape(-1), k.reshape(-1), m_vote.reshape(-1), tail,
                                   [k[0, 0]]]))
    return np.stack(out)


def test_vote_matrix_includes_the_flows_translation():
    """The reference applies the whole forward flow -- translation included -- to the lifted
    offset; m_vote reproduces that."""
    meta = dict(img_shape=[36, 50, 3], transformation_3d_flow=["T"], pcd_trans=[0.5, -0.25, 2.0])
    p = FL.vote_fusion_params([meta], dict(Rt=np.eye(3)[None], K=np.eye(3)[None]))[0].numpy()
    assert np.array_equal(p[21:33].reshape(3, 4)[:, 3], np.float32([0.5, -0.25, 2.0]))
    assert np.array_equal(p[:12].reshape(3, 4)[:, 3], np.float32([-0.5, 2.0, 0.25]))


# ---- constructor, registries, keys, config --------------------------------------------------
def test_constructor_and_registries():
    from msmdfusion_amd import detector, registry as Rg
    layer = Rg.build_fusion_layer(dict(type="VoteFusion", num_classes=7, max_imvote_per_pixel=2))
    assert isinstance(layer, VoteFusion) and "VoteFusion" in Rg.FUSION_LAYERS
    assert layer.num_classes == 7 and layer.max_imvote_per_pixel == 2
    assert VoteFusion().num_classes == 10 and VoteFusion().max_imvote_per_pixel == 3
    assert not list(layer.parameters())
    assert "ImVoteNet" in Rg.DETECTORS and detector.ImVoteNet is not None
    # output shapes: [B, 5 + classes + 3, K S] and [B, K S]
    c = R.make_case(1, 5, (2, 0), 7)
    f, m = layer(*R.to_torch(c))
    assert tuple(f.shape) == (2, 5 + 7 + 3, 2 * 5) and tuple(m.shape) == (2, 2 * 5)


def test_short_box_lists_and_large_k_take_zero_slots():
    """Nb < K: the missing boxes count as score 0; K above the fused cap is the composition."""
    c = R.make_case(2, 9, (2, 1), 4)
    args = R.to_torch(c)
    for k in (3, 9):
        layer = VoteFusion(4, k)
        f, m = layer(*args)
        fr, mr, _ = R.vote_fusion_ref(*args, 4, k, dtype=torch.float32)
        assert torch.equal(f, fr) and torch.equal(m, mr)
        s = 9
        assert not m[0].reshape(k, s)[2:].any() and not f[0, :9].reshape(9, k, s)[:, 2:].any()


def test_mlp_and_imvotenet_keys(golden):
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.detector import MLP, build_detector
    keys = json.loads(str(golden["mlp/keys"]))
    mlp = MLP(in_channel=18, conv_channels=(8, 6))
    assert list(mlp.state_dict()) == keys
    mlp.load_state_dict({k: torch.from_numpy(golden["mlp/state/" + k]) for k in keys})
    mlp.eval()
    y = mlp(torch.from_numpy(golden["mlp/x"]))
    assert (y - torch.from_numpy(golden["mlp/y"])).abs().max() <= 1e-5
    cfg = json.loads(json.dumps(C.IMVOTENET_STAGE2_SUNRGBD["model"]))
    det = build_detector(cfg)
    sd = set(det.state_dict())
    big = MLP(**cfg["img_mlp"])
    assert {"img_mlp." + k for k in big.state_dict()} <= sd
    assert "img_mlp.mlp.layer0.conv.weight" in sd and "img_mlp.mlp.layer1.bn.running_var" in sd
    prefixes = {k.split(".")[0] for k in sd}
    assert prefixes == {"pts_backbone", "pts_bbox_head_joint", "pts_bbox_head_pts",
                        "pts_bbox_head_img", "img_mlp"}
    vote = build_detector(json.loads(json.dumps(C.VOTENET_SUNRGBD["model"])))
    assert {k.replace("backbone.", "pts_backbone.", 1) for k in vote.state_dict()
            if k.startswith("backbone.")} <= sd
    # the pts / img towers are VoteNet's head; the joint tower takes 512 channels
    head = {k[len("bbox_head."):] for k in vote.state_dict() if k.startswith("bbox_head.")}
    for tower in ("pts_bbox_head_pts", "pts_bbox_head_img", "pts_bbox_head_joint"):
        assert {tower + "." + k for k in head} <= sd
    assert tuple(det.state_dict()["pts_bbox_head_joint.vote_module.vote_conv.0.conv.weight"].shape) \
        == (512, 512, 1)
    assert tuple(det.state_dict()["pts_bbox_head_pts.vote_module.vote_conv.0.conv.weight"].shape) \
        == (256, 256, 1)
    assert det.loss_weights == [0.4, 0.3, 0.3] and det.num_sampled_seed == 1024
    assert det.max_imvote_per_pixel == 3 and isinstance(det.fusion_layer, VoteFusion)
    with pytest.raises(NotImplementedError):
        det.forward_train(points=None)


def test_config_matches_the_reference_file():
    from msmdfusion_amd import configs as C
    fx = json.load(open(os.path.join(HERE, "golden", "reference_imvotenet_config.json")))
    norm = lambda o: json.loads(json.dumps(o))      # noqa: E731
    assert norm(C.IMVOTENET_STAGE2_SUNRGBD["model"]) == fx["model"]
    assert fx["injected"] == ["img_backbone", "img_neck", "img_rpn_head", "img_roi_head"]
    assert not set(fx["injected"]) & set(C.IMVOTENET_STAGE2_SUNRGBD["model"])


# ---- the C ABI -----------------------------------------------------------------------------
def test_c_abi_refusals():
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd._lib import lib
    assert K.VOTE_FUSION_MAX_K == lib.msmd_vote_fusion_max_k() == 8
    p = ctypes.c_void_p(256)
    off = (ctypes.c_int * 3)(0, 2, 5)

    def call(k=3, classes=10, offsets=off, total=5):
        return lib.msmd_vote_fusion_f32(p, 2, 16, p, total, p, offsets, p, 48, 64, p, classes, k,
                                        p, p, None)
    for bad in (dict(k=0), dict(k=-1), dict(k=9), dict(classes=0),
                dict(offsets=(ctypes.c_int * 3)(1, 2, 5)),        # does not start at 0
                dict(offsets=(ctypes.c_int * 3)(0, 3, 2), total=2),   # decreases
                dict(total=6),                                    # does not end at the total
                dict(offsets=None)):
        assert call(**bad) == -1, bad
    assert lib.msmd_vote_fusion_f32(None, 0, 16, None, 0, None, None, None, 0, 0, None, 10, 3,
                                    None, None, None) == 0        # an empty batch: nothing to do
    # CPU tensors described as device tensors are refused by the wrapper
    c = R.make_case(0, 4, (1, 0), 3)
    imgs, boxes, seeds, metas, calibs = R.to_torch(c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.vote_fusion(seeds, torch.cat(boxes), torch.tensor([0, 1, 1], dtype=torch.int32),
                      [0, 1, 1], imgs, FL.vote_fusion_params(metas, calibs), 3, 3)


# ---- sample_valid_seeds --------------------------------------------------------------------
S = 16
COUNTS = (0, 1, S - 1, S, S + 1, 3 * S)


def _masks(seed):
    rng = np.random.RandomState(seed)
    m = np.zeros((len(COUNTS), 3 * S), bool)
    for row, cnt in enumerate(COUNTS):
        m[row, rng.permutation(3 * S)[:cnt]] = True
    return torch.from_numpy(m)


def test_sample_valid_seeds_properties(golden):
    from msmdfusion_amd.detector import sample_valid_seeds
    seen = set()
    for seed in range(20):
        mask = _masks(seed) if seed else torch.from_numpy(golden["svs/mask"])
        gen = torch.Generator().manual_seed(seed)
        out = sample_valid_seeds(mask, S, generator=gen)
        ref = R.sample_valid_seeds_loop(mask, S, generator=torch.Generator().manual_seed(seed))
        assert out.dtype == torch.int64 and tuple(out.shape) == (len(COUNTS), S)
        for row, cnt in enumerate(COUNTS):
            valid = torch.nonzero(mask[row]).squeeze(-1).tolist()
            got = out[row].tolist()
            if cnt >= S:
                assert len(set(got)) == S and set(got) <= set(valid)
                if cnt == S:
                    assert set(got) == set(ref[row].tolist())
            else:
                assert got[:cnt] == valid                       # ascending
                diff = set(range(S)) - {v % S for v in valid}
                rest = got[cnt:]
                assert len(set(rest)) == len(rest) and set(rest) <= diff
                if len(diff) == S - cnt:
                    assert set(got) == set(ref[row].tolist())
        seen.add(tuple(out[5].tolist()))
    assert len(seen) > 1, "the draw does not depend on the generator"
    # the golden's own draw (the reference's code) has the same structure
    inds = golden["svs/inds"]
    assert sorted(inds[0].tolist()) == list(range(S))           # nothing valid: a permutation
    # N below num_sampled_seed: everything valid, then the rest of the difference set
    few = sample_valid_seeds(torch.ones((1, 5), dtype=torch.bool), 8,
                             generator=torch.Generator().manual_seed(0))[0].tolist()
    assert few[:5] == [0, 1, 2, 3, 4] and sorted(few[5:]) == [5, 6, 7]


def test_sample_valid_seeds_is_uniform():
    """The law, not the stream: over many draws every valid index is taken equally often."""
    from msmdfusion_amd.detector import sample_valid_seeds
    mask = torch.zeros((1, 24), dtype=torch.bool)
    mask[0, ::2] = True                                         # 12 valid, sample 4
    gen = torch.Generator().manual_seed(1)
    hits = torch.zeros(24)
    n = 3000
    for _ in range(n):
        hits[sample_valid_seeds(mask, 4, generator=gen)[0]] += 1
    assert hits[1::2].sum() == 0
    # binomial(n, 1/3): mean 1000, sigma 25.8; six sigma
    assert (hits[::2] - n / 3).abs().max() < 6 * (n * (1 / 3) * (2 / 3)) ** 0.5
