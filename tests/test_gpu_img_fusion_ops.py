"""The two native kernels of TransFusionHead's image stage (csrc/img_fusion.hip) on the GPU:
the query geometry against its numpy restatement, the Gaussian-window attention (forward,
backward, dropout) against the reference's dense log-mask attention in float64, and their
process properties (no host read, no [P, H W] tensor, bitwise repeatable).

The float criterion is the project's standing one: the kernel's largest absolute error against
float64 may be at most 4 times the largest error of the float32 restatement / composition
against the same float64 result, floored at float32 eps of the result's scale
(img_fusion_ref.within_reference_error).  Discrete outputs are exact on inputs that meet the
generator's conditions (img_fusion_ref.geometry_is_safe)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import img_fusion_ref as R  # noqa: E402

from msmdfusion_amd import kernels as K  # noqa: E402

pytestmark = pytest.mark.gpu

PAD_H, PAD_W, OSF = 48, 80, 4.0
TILE, CHUNK = 256, 64           # K.GAUSS_ATTN_KEY_TILE, K.GAUSS_ATTN_ROW_CHUNK


def _within(ours, ref32, ref64, what):
    ok, err, margin = R.within_reference_error(ours, ref32, ref64)
    print("%s: kernel %.3e, margin %.3e" % (what, err, margin))
    assert ok, (what, err, margin)


# ------------------------------------------------------------------ geometry
def _params(V, flip, crop, scale):
    """Pinhole views along +z that look at overlapping strips: 0.4 W apart."""
    prm = np.zeros((V, 20))
    f = 0.5 * PAD_W / scale
    for v in range(V):
        c = (0.5 * PAD_W + (v - 0.5 * (V - 1)) * 0.4 * PAD_W) / scale
        prm[v, :12] = np.array([[f, 0, c, 0], [0, f, 0.5 * PAD_H / scale, 0], [0, 0, 1.0, 0]]).reshape(-1)
        prm[v, 12:] = [scale, scale, crop[0], crop[1], float(flip), PAD_W - 3.0, PAD_H, PAD_W]
    return prm


def _scene(B, V, P, seed, flip=False, crop=(0.0, 0.0), scale=1.0):
    """Random queries and boxes in front of (and 10 % behind) the cameras, re-drawn until the
    discrete results are well defined in float32."""
    for attempt in range(200):
        rng = np.random.RandomState(seed + 1000 * attempt)
        z = rng.uniform(2, 30, (B, P)) * np.where(rng.rand(B, P) < 0.1, -1, 1)
        x, y = rng.uniform(-1.6, 1.6, (B, P)) * abs(z), rng.uniform(-0.8, 0.8, (B, P)) * abs(z)
        pos3d = np.stack([x, y, z], 1)
        dims = rng.uniform(0.3, 4.0, (B, P, 3))
        boxes = np.concatenate([x[..., None], y[..., None], (z - dims[..., 2] / 2)[..., None], dims,
                                rng.uniform(-3.2, 3.2, (B, P, 1))], -1)
        params = np.stack([_params(V, flip, crop, scale)] * B).astype(np.float32)
        pos3d, boxes = pos3d.astype(np.float32), boxes.astype(np.float32)
        g64 = R.geometry(pos3d.astype(np.float64), boxes.astype(np.float64),
                         params.astype(np.float64), OSF, np.float64)
        g32 = R.geometry(pos3d, boxes, params, OSF, np.float32)
        if R.geometry_is_safe(g64, g32, OSF, PAD_H, PAD_W, PAD_H // 4, PAD_W // 4):
            return pos3d, boxes, params, g64, g32
    raise AssertionError("no well-defined scene found")


def _run_geometry(dev, pos3d, boxes, params):
    return K.img_query_geometry(torch.from_numpy(pos3d).to(dev), torch.from_numpy(boxes).to(dev),
                                torch.from_numpy(params).to(dev), OSF)


def _check_geometry(geo, g64, g32, what):
    on = g64["on"]
    assert np.array_equal(geo.on.cpu().numpy(), on), what
    assert np.array_equal(geo.count.cpu().numpy(), g64["count"]), what
    assert np.array_equal(geo.valid.cpu().numpy(), g64["valid"]), what
    assert np.array_equal(geo.winner.cpu().numpy(), g64["winner"]), what
    assert np.array_equal(geo.mask.cpu().numpy(), g64["mask"]), what
    assert np.array_equal(geo.centre.cpu().numpy()[on], g64["centre"][on]), what
    assert np.array_equal(geo.radius.cpu().numpy()[on], g64["radius"][on]), what
    assert np.array_equal(geo.sigma.cpu().numpy()[on], g32["sigma"][on]), what
    has = g64["mask"]
    assert np.array_equal(geo.win_centre.cpu().numpy(), g64["win_centre"]), what
    assert np.array_equal(geo.win_sigma.cpu().numpy()[has], g32["win_sigma"][has]), what
    assert not geo.win_sigma.cpu().numpy()[~has].any(), what
    if on.any():
        _within(geo.pos.cpu().numpy()[on], g32["pos"][on], g64["pos"][on], what + " pos")
    if has.any():
        _within(geo.win_pos.cpu().numpy()[has], g32["win_pos"][has], g64["win_pos"][has],
                what + " win_pos")


@pytest.mark.parametrize("B,V,P", [(1, 1, 1), (1, 2, 2), (2, 1, 63), (2, 2, 64), (3, 6, 65),
                                   (2, 6, 200), (3, 2, 257), (1, 6, 1024)])
def test_geometry_shapes(dev, B, V, P):
    pos3d, boxes, params, g64, g32 = _scene(B, V, P, seed=B * 100 + V * 10 + P)
    _check_geometry(_run_geometry(dev, pos3d, boxes, params), g64, g32, "B%d V%d P%d" % (B, V, P))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("crop", [(0.0, 0.0), (3.0, 2.0)])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_geometry_flip_crop_scale(dev, flip, crop, scale):
    pos3d, boxes, params, g64, g32 = _scene(2, 3, 130, seed=7, flip=flip, crop=crop, scale=scale)
    assert g64["on"].any() and (g64["on"].sum(1) >= 2).any()
    _check_geometry(_run_geometry(dev, pos3d, boxes, params), g64, g32,
                    "flip %s crop %s scale %s" % (flip, crop, scale))


def _place(params, v, u, w_, z):
    """The point whose final pixel in view v is (u, w_) at depth z (no flip)."""
    m, (sx, sy, cx, cy) = params[v, :12].reshape(3, 4), params[v, 12:16]
    return ((u + cx) / sx - m[0, 2]) * z / m[0, 0], ((w_ + cy) / sy - m[1, 2]) * z / m[1, 1], z


def test_geometry_groups_of_zero_one_two_and_a_query_in_three_views(dev):
    """View v shows view 0's pixels shifted by 32 v.  Sample 0: nobody on any image.  Sample 1:
    view 0 holds one query (a group of one: skipped), view 2 two.  Sample 2: two queries in all
    three views -- the highest valid view wins -- and one that only view 0 sees."""
    V, P = 3, 5
    prm = _params(V, False, (0.0, 0.0), 1.0)
    pos = np.zeros((3, 3, P))
    pos[:, 0], pos[:, 2] = 1e4, 5.0                         # far off every image
    pos[1, :, 0] = _place(prm, 0, 60.3, 10.3, 5.0)          # view 0 only (view 1: 92.3)
    pos[1, :, 1] = _place(prm, 2, 5.3, 20.3, 7.0)           # view 2 only (view 1: -26.7)
    pos[1, :, 2] = _place(prm, 2, 10.7, 21.3, 7.0)
    pos[2, :, 0] = _place(prm, 0, 5.3, 20.3, 6.0)           # views 0, 1 (37.3), 2 (69.3)
    pos[2, :, 1] = _place(prm, 0, 10.7, 21.3, 6.0)
    pos[2, :, 2] = _place(prm, 0, 60.3, 5.3, 9.0)           # view 0 only
    boxes = np.zeros((3, P, 7))
    boxes[..., :2], boxes[..., 2] = np.moveaxis(pos[:, :2], 1, -1), pos[:, 2] - 0.5
    boxes[..., 3:6], boxes[..., 6] = 1.0, 0.3
    pos, boxes = pos.astype(np.float32), boxes.astype(np.float32)
    params = np.stack([prm] * 3).astype(np.float32)
    g64 = R.geometry(pos.astype(np.float64), boxes.astype(np.float64), params.astype(np.float64),
                     OSF, np.float64)
    g32 = R.geometry(pos, boxes, params, OSF, np.float32)
    assert R.geometry_is_safe(g64, g32, OSF, PAD_H, PAD_W, 12, 20)
    assert g64["count"].tolist() == [[0, 0, 0], [1, 0, 2], [3, 2, 2]]
    assert g64["winner"][1].tolist() == [-1, 2, 2, -1, -1]  # the single member of view 0: skipped
    assert g64["winner"][2].tolist() == [2, 2, 0, -1, -1]
    _check_geometry(_run_geometry(dev, pos, boxes, params), g64, g32, "groups")


def test_geometry_behind_camera_corners_and_nan_rows(dev):
    pos3d, boxes, params, g64, g32 = _scene(2, 2, 70, seed=3)
    boxes[0, :4, 3:6], boxes[0, 4:8, 3:6] = 8000.0, 80.0      # corners behind the camera plane
    boxes[0, :8, 2] = pos3d[0, 2, :8] - boxes[0, :8, 5] / 2
    boxes[1, 5:9], pos3d[1, :, 7:9] = np.nan, np.nan
    g64 = R.geometry(pos3d.astype(np.float64), boxes.astype(np.float64),
                     params.astype(np.float64), OSF, np.float64)
    g32 = R.geometry(pos3d, boxes, params, OSF, np.float32)
    geo = _run_geometry(dev, pos3d, boxes, params)
    rad = geo.radius.cpu().numpy()
    assert (rad[1, :, 5:9] == R.INT_MAX).all() and not geo.on.cpu().numpy()[1, :, 7:9].any()
    assert (geo.winner.cpu().numpy()[1, 7:9] == -1).all()
    assert (rad >= 0).all()                                    # saturated, never wrapped
    over = g64["radius_arg"] > 2.0 ** 32                       # clearly past int32
    assert over[0, :, :4].any() and (rad[over] == R.INT_MAX).all()
    huge = (g32["radius"] > 2 ** 20) & (g32["radius"] < 2 ** 30)
    assert huge[0, :, 4:8].any()
    assert (abs(rad[huge] - g32["radius"][huge]) <= 1e-4 * g32["radius"][huge]).all()
    assert np.array_equal(geo.on.cpu().numpy(), g32["on"])
    assert np.array_equal(geo.winner.cpu().numpy(), g32["winner"])
    assert bool(torch.isfinite(geo.win_pos).all()) and bool(torch.isfinite(geo.win_sigma).all())


def test_geometry_reads_nothing_back(dev):
    pos3d, boxes, params, g64, g32 = _scene(2, 6, 200, seed=11)
    args = [torch.from_numpy(a).to(dev) for a in (pos3d, boxes, params)]
    want = K.img_query_geometry(*args, OSF)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        geo = K.img_query_geometry(*args, OSF)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(geo.winner, want.winner) and torch.equal(geo.pos, want.pos)


# ------------------------------------------------------------------ attention
def _attn_case(seed, B, V, P, h, w, c, heads, radius, centre=None, dead=0.3):
    rng = np.random.RandomState(seed)
    rows = B * P
    q = rng.standard_normal((rows, c)).astype(np.float32)
    k = rng.standard_normal((B * V, h * w, c)).astype(np.float32)
    v = rng.standard_normal((B * V, h * w, c)).astype(np.float32)
    view = rng.randint(0, V, rows).astype(np.int32)
    view[rng.rand(rows) < dead] = -1
    if centre is None:
        centre = np.stack([rng.randint(0, w, rows), rng.randint(0, h, rows)], 1)
    centre = np.broadcast_to(np.asarray(centre), (rows, 2)).astype(np.int32).copy()
    rad = np.broadcast_to(np.asarray(radius), (rows,)) if radius is not None \
        else rng.randint(0, 7, rows)
    sigma = ((rad.astype(np.int32) * 2 + 1) / 6.0).astype(np.float32)
    return dict(q=q, k=k, v=v, view=view, centre=centre, sigma=sigma,
                shape=(P, V, h, w, heads))


def _dense(case, dtype, keep=None, p=0.0, grad=None):
    P, V, h, w, heads = case["shape"]
    q, k, v = (torch.from_numpy(case[n]).to(dtype).requires_grad_(grad is not None)
               for n in ("q", "k", "v"))
    out = R.dense_attention_torch(q, k, v, case["view"], case["centre"], case["sigma"], P, V, h, w,
                                  heads, keep, p)
    if grad is None:
        return out.detach().numpy()
    out.backward(torch.from_numpy(grad).to(dtype))
    return out.detach().numpy(), q.grad.numpy(), k.grad.numpy(), v.grad.numpy()


def _check_attention(dev, case, what, p=0.0, seed=0):
    P, V, h, w, heads = case["shape"]
    rows, c = case["q"].shape
    keep = R.keep_mask(seed, p, rows, heads, h * w) if p > 0 else None
    grad = np.random.RandomState(99).standard_normal((rows, c)).astype(np.float32)
    ref64 = _dense(case, torch.float64, keep, p, grad)
    ref32 = _dense(case, torch.float32, keep, p, grad)
    t = {n: torch.from_numpy(case[n]).to(dev) for n in ("q", "k", "v", "view", "centre", "sigma")}
    for n in ("q", "k", "v"):
        t[n].requires_grad_(True)
    out = K.gauss_attn(t["q"], t["k"], t["v"], t["view"], t["centre"], t["sigma"], V, h, w, heads,
                       p, seed)
    out.backward(torch.from_numpy(grad).to(dev))
    got = (out.detach(), t["q"].grad, t["k"].grad, t["v"].grad)
    assert all(bool(torch.isfinite(g).all()) for g in got), what
    dead = torch.from_numpy(case["view"] < 0).to(dev)
    assert not bool(got[0][dead].any()) and not bool(got[1][dead].any()), what
    for name, g, r32, r64 in zip(("out", "dq", "dk", "dv"), got, ref32, ref64):
        _within(g.cpu().numpy(), r32, r64, "%s %s" % (what, name))


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (7, 12), (14, 25)])
@pytest.mark.parametrize("c,heads", [(32, 4), (128, 8), (64, 2)])
def test_attention_maps_and_widths(dev, h, w, c, heads):
    case = _attn_case(h * 100 + c, 2, 2, 9, h, w, c, heads, None)
    _check_attention(dev, case, "%dx%d %d/%d" % (h, w, c, heads))


@pytest.mark.parametrize("radius", [0, 1, 5, 40])
def test_attention_radii(dev, radius):
    """radius 0: only the centre key survives; 40: the window covers the whole 7 x 12 map."""
    case = _attn_case(radius, 2, 3, 11, 7, 12, 32, 4, radius)
    member = R.window(R.key_d2(case["centre"], 7, 12), case["sigma"][:, None])
    assert (member.sum(1) == {0: 1, 40: 84}.get(radius, member.sum(1))).all()
    _check_attention(dev, case, "radius %d" % radius)


@pytest.mark.parametrize("border,centre", [("left", (0, 3)), ("right", (11, 3)), ("top", (5, 0)),
                                           ("bottom", (5, 6)), ("corner", (11, 6))])
def test_attention_windows_clipped_by_the_borders(dev, border, centre):
    case = _attn_case(5, 1, 2, 6, 7, 12, 32, 4, 3, centre=centre, dead=0.0)
    _check_attention(dev, case, "clipped " + border)


@pytest.mark.parametrize("P", [1, CHUNK - 1, CHUNK, CHUNK + 1, 200],
                         ids=lambda p: "rows%d_chunk%d" % (p, CHUNK))
def test_attention_rows_around_the_chunk_and_one_shared_key(dev, P):
    """All rows of a sample share one centre: the key-stationary pass sums up to 200 rows into
    one key, across row chunks."""
    case = _attn_case(P, 1, 1, P, 3, 5, 32, 4, 1, centre=(2, 1), dead=0.1 if P > 1 else 0.0)
    _check_attention(dev, case, "P %d" % P)


@pytest.mark.parametrize("h,w", [(15, 17), (16, 16), (3, 86)],
                         ids=lambda v: "n%d" % v)
def test_attention_keys_around_the_tile(dev, h, w):
    """h w = 255, 256, 258 keys: below, at and above one key tile (256) of the dK / dV pass."""
    assert h * w in (TILE - 1, TILE, TILE + 2)
    case = _attn_case(h, 2, 2, 7, h, w, 32, 4, 40)
    _check_attention(dev, case, "%d keys" % (h * w))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_dropout_matches_the_restated_mask(dev, p):
    case = _attn_case(17, 2, 2, 13, 7, 12, 32, 4, None)
    _check_attention(dev, case, "dropout %.1f" % p, p=p, seed=0x1234567899)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_keeps_the_binomial_fraction(dev, p):
    """Uniform weights over a 56 x 100 full-map window and v = 1: out (1 - p) is the kept
    fraction of n = 5600 keys, binomial with standard deviation sqrt(p (1 - p) / n)."""
    h, w, c, heads = 56, 100, 32, 4
    n = h * w
    q = torch.zeros((1, c), device=dev)
    k = torch.zeros((1, n, c), device=dev)
    v = torch.ones((1, n, c), device=dev)
    view = torch.zeros((1,), dtype=torch.int32, device=dev)
    centre = torch.tensor([[50, 28]], dtype=torch.int32, device=dev)
    sigma = torch.full((1,), 1e4, device=dev)               # exp(-d2 / 2 sigma^2) = 1 - O(1e-5)
    out, _ = K.gauss_attn_forward(q, k, v, view, centre, sigma, 1, h, w, heads, p, seed=77)
    kept = out.cpu().numpy().reshape(heads, c // heads)[:, 0] * (1 - float(np.float32(p)))
    std = math.sqrt(p * (1 - p) / n)
    print("kept fractions", kept, "expected", 1 - p, "+-", std)
    assert (abs(kept - (1 - p)) <= 4 * std + 1e-4).all()
    want = R.keep_mask(77, p, 1, heads, n).mean(-1)[0]
    assert np.allclose(kept, want, atol=1e-4)


def _config_case(dev):
    case = _attn_case(1, 2, 6, 200, 56, 100, 128, 8, None, dead=0.2)
    t = {n: torch.from_numpy(case[n]).to(dev) for n in ("q", "k", "v", "view", "centre", "sigma")}
    return t, (6, 56, 100, 8)


def test_attention_memory_repeatability_and_no_host_read_at_the_configs_shape(dev):
    t, shape = _config_case(dev)
    args = (t["q"], t["k"], t["v"], t["view"], t["centre"], t["sigma"]) + shape
    grad = torch.randn_like(t["q"])
    out0, lse0 = K.gauss_attn_forward(*args, 0.1, 5)
    back0 = K.gauss_attn_backward(t["q"], t["k"], t["v"], out0, grad, lse0, t["view"], t["centre"],
                                  t["sigma"], *shape, 0.1, 5)
    torch.cuda.synchronize()
    out_bytes = out0.numel() * 4 + lse0.numel() * 4
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out1, lse1 = K.gauss_attn_forward(*args, 0.1, 5)
        peak = torch.cuda.max_memory_allocated() - base
        back1 = K.gauss_attn_backward(t["q"], t["k"], t["v"], out1, grad, lse1, t["view"],
                                      t["centre"], t["sigma"], *shape, 0.1, 5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    print("forward peak %d bytes, outputs + lse %d bytes; a [P, H W] tensor would be %d"
          % (peak, out_bytes, 400 * 5600 * 4))
    assert peak < 2 * out_bytes                  # (allocator rounding; the dense mask is 9 MB)
    assert torch.equal(out0, out1) and torch.equal(lse0, lse1)
    for a, b in zip(back0, back1):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(out1).all()) and float(out1.abs().max()) > 0
    assert float(back1[1].abs().max()) > 0 and float(back1[2].abs().max()) > 0


def test_wrappers_refuse_what_is_not_built(dev):
    t, shape = _config_case(dev)
    with pytest.raises(ValueError, match="8, 16 or 32"):
        K.gauss_attn_forward(t["q"], t["k"], t["v"], t["view"], t["centre"], t["sigma"], 6, 56,
                             100, 2)
    with pytest.raises(ValueError, match="dropout"):
        K.gauss_attn_forward(t["q"], t["k"], t["v"], t["view"], t["centre"], t["sigma"], 6, 56,
                             100, 8, dropout=1.0)
    with pytest.raises(RuntimeError, match="float32|dtype"):
        K.gauss_attn_forward(t["q"].double(), t["k"], t["v"], t["view"], t["centre"], t["sigma"],
                             6, 56, 100, 8)
    big = torch.zeros((1, 3, 1025), device=dev)
    with pytest.raises(ValueError, match="queries"):
        K.img_query_geometry(big, torch.zeros((1, 1025, 7), device=dev),
                             torch.zeros((1, 2, 20), device=dev), 4)
    with pytest.raises(ValueError, match="views"):
        K.img_query_geometry(big[..., :4].contiguous(), torch.zeros((1, 4, 7), device=dev),
                             torch.zeros((1, 9, 20), device=dev), 4)
