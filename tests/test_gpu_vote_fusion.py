"""VoteFusion's fused kernel (csrc/vote_fusion.hip) on the GPU: against the reference's own
outputs, against the composition (the reference's op sequence) across the kernel's edges, hand
cases for every rule of the selection, and the process properties (no host read, no
[seed, box] tensor, bitwise repeatable).

The float criterion is the project's standing one: per geometric group (xz rows 0-1, ray_angle
rows 2-4) the fused path's largest absolute error against a float64 run may be at most MARGIN
times the largest error of the reference's float32 op sequence on the same inputs against the
same float64 run; where that error is zero, equality.  Discrete outputs (mask, in-box structure,
semantic and texture rows) are exact: the inputs are generated for the uv rounding to be well
defined (tests/imvote_ref.py, tests/golden/make_vote_fusion_golden.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import imvote_ref as R  # noqa: E402

from msmdfusion_amd.fusion_layers import VoteFusion  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 4.0
GROUPS = (("xz", slice(0, 2)), ("ray_angle", slice(2, 5)))


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _check_groups(got, ref32, ref64, what):
    """The 4x rule per geometric group; prints each figure before it asserts."""
    for name, rows in GROUPS:
        err = float((got[:, rows].double() - ref64[:, rows]).abs().max())
        own = float((ref32[:, rows].double() - ref64[:, rows]).abs().max())
        print("%s %s: fused %.3e, float32 op sequence %.3e" % (what, name, err, own))
        if own == 0.0:
            assert err == 0.0, (what, name)
        else:
            assert err <= MARGIN * own, (what, name, err, own)


def _check_discrete(feat, mask, ref_feat, ref_mask, num_classes, what):
    assert mask.dtype == torch.bool and torch.equal(mask, ref_mask), what
    # in-box structure: where the cue block is non-zero
    assert torch.equal(feat[:, 2:5] != 0, ref_feat[:, 2:5] != 0), what
    sem = slice(5, 5 + num_classes)
    assert torch.equal(feat[:, sem], ref_feat[:, sem].to(feat.dtype)), what
    assert torch.equal(feat[:, 5 + num_classes:], ref_feat[:, 5 + num_classes:].to(feat.dtype)), what


@pytest.mark.parametrize("name", ("c10", "c3"))
def test_against_the_reference(golden, dev, name):
    g = golden
    meta = json.loads(str(g[name + "/meta"]))
    b = g[name + "/seeds"].shape[0]
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dev)     # noqa: E731
    layer = VoteFusion(meta["num_classes"], meta["max_imvote_per_pixel"])
    imgs = t(g[name + "/imgs"])
    before = imgs.clone()
    for calibs in (dict(Rt=t(g[name + "/Rt"]), K=t(g[name + "/K"])),             # on the device
                   dict(Rt=g[name + "/Rt"], K=g[name + "/K"])):                  # on the host
        feat, mask = layer(imgs, [t(g[name + "/boxes/%d" % i]) for i in range(b)],
                           t(g[name + "/seeds"]), meta["metas"], calibs)
        ref32 = torch.from_numpy(g[name + "/feat32"]).to(dev)
        ref64 = torch.from_numpy(g[name + "/feat64"]).to(dev)
        _check_discrete(feat, mask, ref32, torch.from_numpy(g[name + "/mask"]).to(dev),
                        meta["num_classes"], name)
        _check_groups(feat, ref32, ref64, name)
    assert torch.equal(imgs, before)


# ---- against the composition, across the kernel's edges ----------------------------------------
def _run_both(dev, case, k):
    args = R.to_torch(case, dev)
    layer = VoteFusion(case["num_classes"], k)
    feat, mask = layer(*args)
    comp_f, comp_m = layer.forward_composed(*args)
    a64 = R.to_torch(case, dev, torch.float64)
    ref64, mask64, _ = R.vote_fusion_ref(*a64, case["num_classes"], k, dtype=torch.float64)
    assert torch.equal(comp_m, mask64)              # the inputs are well defined
    return feat, mask, comp_f, comp_m, ref64


@pytest.mark.parametrize("s", (1, 63, 64, 65, 257))
def test_seed_counts(dev, s):
    case = R.make_case(10 + s, s, (5, 0, 0), 10)        # empty middle and empty last sample
    feat, mask, comp_f, comp_m, ref64 = _run_both(dev, case, 3)
    _check_discrete(feat, mask, comp_f, comp_m, 10, "S=%d" % s)
    _check_groups(feat, comp_f, ref64, "S=%d" % s)


@pytest.mark.parametrize("nb", (0, 1, 2, 3, 63, 64, 65, 131))
@pytest.mark.parametrize("k", (1, 3, 8, 9))
def test_box_counts_and_k(dev, nb, k):
    from msmdfusion_amd import kernels as K
    classes = 1 if nb in (1, 64) else 10
    case = R.make_case(100 + nb, 70, (nb, 0, max(nb - 1, 0)), classes)
    feat, mask, comp_f, comp_m, ref64 = _run_both(dev, case, k)
    what = "Nb=%d K=%d" % (nb, k)
    if k > K.VOTE_FUSION_MAX_K:                       # the composition serves it
        assert torch.equal(feat, comp_f) and torch.equal(mask, comp_m)
        return
    _check_discrete(feat, mask, comp_f, comp_m, classes, what)
    _check_groups(feat, comp_f, ref64, what)


# ---- hand cases ----------------------------------------------------------------------------
def _hand(dev, boxes, pixels, k=3, num_classes=4, depth=2.0, img_hw=(20, 30), nan_rows=()):
    """One sample, identity flow and calibration tilt, scale 1: seeds that project onto the
    given integer pixels (uv_origin = pixel)."""
    f, cx, cy = 40.0, 15.0, 10.0
    kmat = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    u, v = np.array(pixels, dtype=np.float64).T + 1.0
    cam = np.stack([(u - cx) / f, (v - cy) / f, np.ones(len(u))]) * depth
    seeds = np.stack([cam[0], cam[2], -cam[1]], 1).astype(np.float32)      # DEPTH = (x, z, -y)
    for r in nan_rows:
        seeds[r] = np.nan
    h, w = img_hw
    rng = np.random.RandomState(0)
    img = rng.randint(1, 256, (1, 3, h, w)).astype(np.float32)
    meta = dict(img_shape=[h, w, 3])
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dev)     # noqa: E731
    args = (t(img), [t(np.asarray(boxes, dtype=np.float32).reshape(-1, 6))], t(seeds[None]),
            [meta], dict(Rt=np.eye(3)[None], K=kmat[None]))
    layer = VoteFusion(num_classes, k)
    feat, mask = layer(*args)
    s = len(pixels)
    c = 5 + num_classes + 3
    return feat[0].reshape(c, k, s), mask[0].reshape(k, s), img[0], args, layer


def test_equal_confidence_goes_to_the_lower_index(dev):
    boxes = [[2.5, 2.5, 20.5, 15.5, 0.5, 2], [1.5, 1.5, 25.5, 18.5, 0.5, 1],
             [0.5, 0.5, 28.5, 19.5, 0.5, 3]]
    feat, mask, _, args, layer = _hand(dev, boxes, [(10, 8)], k=2)
    assert mask[:, 0].tolist() == [True, True]
    assert feat[5 + 2, 0, 0] == 0.5 and feat[5 + 1, 1, 0] == 0.5      # box 0, then box 1
    assert feat[5 + 3].abs().sum() == 0
    comp_f, comp_m = layer.forward_composed(*args)                    # the composition's rule too
    assert torch.equal(comp_m[0].reshape(2, 1), mask)
    assert torch.equal(comp_f[0, 5:9].reshape(4, 2, 1), feat[5:9])


def test_mask_is_the_floor_of_the_score(dev):
    # pixel (10, 8): outside box 0 (conf 1.0), inside box 1 (conf 0.0), outside box 2 (conf 0.9)
    boxes = [[20.5, 2.5, 28.5, 15.5, 1.0, 0], [1.5, 1.5, 15.5, 18.5, 0.0, 1],
             [20.5, 2.5, 28.5, 15.5, 0.9, 2]]
    feat, mask, _, _, _ = _hand(dev, boxes, [(10, 8)], k=3)
    # scores 1.0 (out, conf 1) and 1.0 (in, conf 0) tie: the lower index first; then 0.9
    assert mask[:, 0].tolist() == [True, True, False]
    assert feat[:9, 0, 0].abs().sum() == 0                    # conf == 1 out of box: zero cues
    assert feat[2:5, 1, 0].abs().sum() > 0                    # conf == 0 in box: geometric cues
    assert feat[5:9, 1, 0].abs().sum() == 0                   # ... and a zero semantic cue
    assert feat[:9, 2, 0].abs().sum() == 0


def test_a_seed_on_a_box_edge_is_outside(dev):
    boxes = [[10.0, 2.0, 20.0, 15.0, 0.7, 1]]
    pixels = [(10, 8), (20, 8), (15, 2), (15, 15), (11, 3), (19, 14)]
    feat, mask, _, _, _ = _hand(dev, boxes, pixels, k=1)
    assert mask[0].tolist() == [False, False, False, False, True, True]
    assert (feat[5 + 1, 0] != 0).tolist() == [False, False, False, False, True, True]


def test_a_seed_outside_the_image_has_no_texture(dev):
    boxes = [[-50.5, -50.5, 80.5, 60.5, 0.6, 2]]
    pixels = [(12, 9), (-3, 9), (30, 9), (12, -1), (12, 20), (29, 19), (0, 0)]
    feat, mask, img, _, _ = _hand(dev, boxes, pixels, k=2)
    inside = [True, False, False, False, False, True, True]
    for j, (px, ok) in enumerate(zip(pixels, inside)):
        want = img[:, px[1], px[0]] / np.float32(255.) if ok else np.zeros(3, np.float32)
        for k in range(2):                                    # every slot, valid or not
            assert np.array_equal(feat[9:, k, j].cpu().numpy(), want), (px, k)
    # the other rows are unaffected: every seed is in the box
    assert mask[0].all() and not mask[1].any()
    assert bool((feat[5 + 2, 0] == np.float32(0.6)).all()) and bool((feat[2:5, 0] != 0).any(0).all())


def test_a_class_out_of_range_has_no_semantic_cue(dev):
    boxes = [[1.5, 1.5, 25.5, 18.5, 0.8, 4], [1.5, 1.5, 25.5, 18.5, 0.7, -1],
             [1.5, 1.5, 25.5, 18.5, 0.6, 3]]
    feat, mask, _, _, _ = _hand(dev, boxes, [(10, 8)], k=3, num_classes=4)
    assert mask[:, 0].tolist() == [True, True, True]
    assert feat[5:9, 0, 0].abs().sum() == 0 and feat[5:9, 1, 0].abs().sum() == 0
    assert feat[5 + 3, 2, 0] == np.float32(0.6)
    assert bool((feat[2:5, :, 0] != 0).any(0).all())          # the geometric cues are there


def test_nan_seeds_write_their_columns_and_leave_the_neighbours(dev):
    from msmdfusion_amd import fusion_layers as FL
    from msmdfusion_amd import kernels as K
    boxes = [[1.5, 1.5, 25.5, 18.5, 0.8, 1], [3.5, 2.5, 20.5, 15.5, 0.4, 2]]
    pixels = [(4 + (j % 20), 3 + (j % 11)) for j in range(70)]
    nan_rows = (0, 17, 63, 64, 69)
    clean, clean_mask, _, _, _ = _hand(dev, boxes, pixels, k=2)
    feat, mask, _, args, _ = _hand(dev, boxes, pixels, k=2, nan_rows=nan_rows)
    keep = [j for j in range(70) if j not in nan_rows]
    assert torch.equal(feat[:, :, keep], clean[:, :, keep])
    assert torch.equal(mask[:, keep], clean_mask[:, keep])
    # every NaN-seed column is written: the same call into a NaN-filled buffer gives the same
    imgs, bxs, seeds, metas, calibs = args
    again_f = torch.full((1, 12, 140), float("nan"), device=dev)
    again_m = torch.full((1, 140), 255, dtype=torch.uint8, device=dev)
    params = FL.vote_fusion_params(metas, calibs).to(dev)
    off = torch.tensor([0, 2], dtype=torch.int32, device=dev)
    from msmdfusion_amd._lib import check, lib
    check(lib.msmd_vote_fusion_f32(seeds.data_ptr(), 1, 70, bxs[0].data_ptr(), 2, off.data_ptr(),
                                   (K.C.c_int * 2)(0, 2), imgs.data_ptr(), 20, 30,
                                   params.data_ptr(), 4, 2, again_f.data_ptr(),
                                   again_m.data_ptr(), None), "msmd_vote_fusion_f32")
    torch.cuda.synchronize()
    again_f, again_m = again_f[0].reshape(12, 2, 70), again_m[0].reshape(2, 70)
    rows = list(nan_rows)
    assert bool((again_m[:, rows] <= 1).all())
    assert torch.equal(again_m.bool(), mask)
    assert torch.equal(torch.isnan(again_f[:, :, rows]), torch.isnan(feat[:, :, rows]))
    assert torch.equal(torch.nan_to_num(again_f), torch.nan_to_num(feat))
    # what a NaN seed gets: no box holds it, a zero semantic and texture cue, an invalid mask
    assert not mask[:, rows].any()
    assert feat[5:, :, rows].abs().sum() == 0


# ---- process properties ----------------------------------------------------------------------
def _config_shape(dev, b=8, s=1024, nb=100):
    case = R.make_case(7, s, (nb,) * b, 10, img_hw=(36, 50))
    return R.to_torch(case, dev)


def test_no_host_read(dev):
    args = _config_shape(dev, b=2, s=257, nb=70)
    layer = VoteFusion(10, 3)
    want_f, want_m = layer(*args)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        feat, mask = layer(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(feat, want_f) and torch.equal(mask, want_m)


def test_peak_memory_and_repeatability_at_the_configs_shape(dev):
    args = _config_shape(dev)
    layer = VoteFusion(10, 3)
    first_f, first_m = layer(*args)                    # (warm: code objects, pinned buffers)
    out_bytes = first_f.numel() * 4 + first_m.numel()
    assert tuple(first_f.shape) == (8, 18, 3 * 1024) and tuple(first_m.shape) == (8, 3 * 1024)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    feat, mask = layer(*args)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak %d bytes, outputs %d bytes" % (peak, out_bytes))
    assert peak < 2 * out_bytes                        # no [S, Nb] tensor: that alone is 6 MB a sample
    assert torch.equal(feat, first_f) and torch.equal(mask, first_m)
    assert int(mask.sum()) > 0 and bool(torch.isfinite(feat).all())
