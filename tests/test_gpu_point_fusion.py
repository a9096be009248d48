"""PointFusion's fused sampler (csrc/point_sample.hip) on the GPU, through PointFusion,
DynamicVFE and DynamicMVXFasterRCNN.

The float64 comparisons use the yardstick of test_gpu_pillar.py, measured on the same GPU and
the same inputs: the error of the float32 torch composition (the reference's op sequence around
F.grid_sample) against the same composition in float64.  The fused result may err by at most
MARGIN times that, with a floor of FLOOR.  Bilinear sampling with zero padding is continuous in
the coordinate, so no entries are excluded.  The criterion is applied to cases with at least 64
in-view points, where a single lucky rounding cannot set the yardstick; smaller cases use maps
at most 64 pixels wide -- one float32 ulp of a coordinate is below 4e-6 px there -- and are held
to TOL of the largest expected entry against the float64 restatement."""
import copy

import numpy as np
import pytest
import torch

import point_fusion_fixture as PF

pytestmark = pytest.mark.gpu

TOL = 1e-4       # the project's feature tolerance, of the expected tensor's largest entry
MARGIN = 4.0
FLOOR = 1e-6
MIN_IN_VIEW = 64


def _special_points(l2i, pad_h, pad_w, h, w):
    """Pixel centres of an (h, w) level under both align_corners settings, every border within
    one level pixel inside and outside, far outside (1e30 after projection)."""
    sx, sy = pad_w / w, pad_h / h
    us = [(k + 0.5) * sx for k in range(min(w, 4))] + \
        [k * pad_w / max(w - 1, 1) for k in range(min(w, 4))]
    vs = [(k + 0.5) * sy for k in range(min(h, 4))] + \
        [k * pad_h / max(h - 1, 1) for k in range(min(h, 4))]
    edge_u = [-sx, -0.5 * sx, 0.0, 0.5 * sx, sx, pad_w - sx, pad_w - 0.5 * sx, pad_w,
              pad_w + 0.5 * sx, pad_w + sx]
    edge_v = [-sy, -0.5 * sy, 0.0, 0.5 * sy, sy, pad_h - sy, pad_h - 0.5 * sy, pad_h,
              pad_h + 0.5 * sy, pad_h + sy]
    uv = [(u, v) for u in us for v in vs] + [(u, v) for u in edge_u for v in edge_v]
    u, v = np.array(uv).T
    pts = PF.pixels_to_points(l2i, u, v, np.full(len(u), 7.0))
    far = np.array([[1.0, 1e28, 0.0], [1.0, 0.0, -1e28], [1.0, -1e28, 1e28]])
    return np.concatenate([pts, far]).astype(np.float32)


def _aug(meta, flip):
    meta.update(img_crop_offset=[3.5, -2.25], scale_factor=[0.9, 0.8, 0.9, 0.8], flip=flip,
                transformation_3d_flow=["R", "S", "T", "HF"],
                pcd_rotation=[[0.96, 0.28, 0], [-0.28, 0.96, 0], [0, 0, 1.0]],
                pcd_scale_factor=1.04, pcd_trans=[0.3, -0.2, 0.1], pcd_horizontal_flip=True)


def _make(dev, sizes, levels, pad, align, aug=False, seed=0, special=True, channels_last=False):
    """sizes: points per sample; levels: (C, H, W) per level -> (module, maps, pts, metas)."""
    rng = np.random.RandomState(seed)
    mod = PF.sampler([c for c, _, _ in levels], align_corners=align).to(dev)
    b = len(sizes)
    maps = [torch.from_numpy(rng.randn(b, c, h, w).astype(np.float32)).to(dev)
            for c, h, w in levels]
    if channels_last:
        maps = [m.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for m in maps]
    pts, metas = [], []
    for i, n in enumerate(sizes):
        l2i = PF.camera(pad[0], pad[1], seed + i)
        meta = dict(lidar2img=l2i.tolist(), input_shape=list(pad),
                    img_shape=[pad[0] - 4, pad[1] - 6, 3])
        p = PF.cloud(n, pad[0], pad[1], l2i, seed=seed + 10 * i)
        if special and n >= 200:
            sp = _special_points(l2i, pad[0], pad[1], levels[0][1], levels[0][2])[:n // 2]
            p[-len(sp):, :3] = sp
        if aug:
            # the detector sees the augmented cloud; the metas take it back
            from msmdfusion_amd.fusion_layers import apply_3d_transformation
            _aug(meta, flip=i % 2 == 0)
            p[:, :3] = apply_3d_transformation(torch.from_numpy(p[:, :3].copy()).double(), "LIDAR",
                                               meta).float().numpy()
        pts.append(torch.from_numpy(p).to(dev))
        metas.append(meta)
    return mod, maps, pts, metas


def _judge(tag, got, y32, y64, in_view, widest):
    base, err = PF.scaled_err(y32, y64), PF.scaled_err(got, y64)
    print("%s: in view %d  fp32 composition %.3e  fused %.3e  ratio %.2f"
          % (tag, in_view, base, err, err / max(base, 1e-30)))
    if in_view >= MIN_IN_VIEW:
        assert err <= max(MARGIN * base, FLOOR)
    else:
        assert widest <= 64, "a small case must use maps at most 64 pixels wide"
        assert err <= TOL


def _forward_check(tag, mod, maps, pts, metas):
    before = [t.clone() for t in maps + pts]
    assert mod.fused_ok(maps, pts)
    with torch.no_grad():
        got = mod.obtain_mlvl_feats(maps, pts, metas)
    y64 = PF.restate(mod, maps, pts, metas, torch.float64)
    y32 = PF.restate(mod, maps, pts, metas, torch.float32)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(y64.shape)
    assert all(torch.equal(a, b) for a, b in zip(maps + pts, before)), "an input was written"
    in_view = int((y64.abs().sum(1) > 0).sum())
    _judge(tag, got, y32, y64, in_view, max(m.shape[3] for m in maps))
    return got


SMALL_PAD, BIG_PAD = (48, 160), (384, 1248)
FORWARD = {
    "N0": ((0,), [(4, 6, 20)], SMALL_PAD, True, False),
    "N1": ((1,), [(4, 6, 20)], SMALL_PAD, True, False),
    "N17": ((17,), [(4, 6, 20)], SMALL_PAD, False, False),
    "N63-C3-C4-noalign": ((63,), [(3, 6, 20), (4, 2, 3)], SMALL_PAD, False, False),
    "N64-C16": ((64,), [(16, 6, 20)], SMALL_PAD, True, True),
    "N65-C1": ((65,), [(1, 6, 20)], SMALL_PAD, False, False),
    "N257-C128-C129-1x1": ((257,), [(128, 6, 20), (129, 2, 3), (4, 1, 1)], SMALL_PAD, True, True),
    "N257-1x1-noalign": ((257,), [(4, 1, 1), (16, 2, 3)], SMALL_PAD, False, True),
    "N300-C256-raw": ((300,), [(256, 6, 20)], SMALL_PAD, True, False),
    "B2-L3": ((130, 150), [(16, 12, 39), (8, 6, 20), (4, 2, 3)], SMALL_PAD, False, True),
    "N4099-B3-L5-96x312": ((2000, 0, 2099), [(8, 96, 312), (16, 48, 156), (4, 24, 78),
                                             (12, 12, 39), (4, 6, 20)], BIG_PAD, False, True),
    "N4099-B3-L5-align": ((2000, 0, 2099), [(8, 96, 312), (16, 48, 156), (4, 24, 78),
                                            (12, 12, 39), (4, 6, 20)], BIG_PAD, True, True),
}


@pytest.mark.parametrize("tag", list(FORWARD))
def test_forward_against_float64(dev, tag):
    sizes, levels, pad, align, aug = FORWARD[tag]
    mod, maps, pts, metas = _make(dev, sizes, levels, pad, align, aug, seed=len(tag))
    got = _forward_check(tag, mod, maps, pts, metas)
    assert tuple(got.shape) == (sum(sizes), sum(c for c, _, _ in levels))
    # channels-last maps are used as they lie and give the same bytes
    cl = [m.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for m in maps]
    with torch.no_grad():
        assert torch.equal(mod.obtain_mlvl_feats(cl, pts, metas), got)
    # the clouds already concatenated (as DynamicVFE hands them over): the same bytes
    if sum(sizes):
        with torch.no_grad():
            again = mod.obtain_mlvl_feats(maps, pts, metas, pts_cat=torch.cat(pts, 0))
        assert torch.equal(again, got)


def test_reference_literal_on_the_fused_path(dev):
    from msmdfusion_amd.fusion_layers import PointFusion
    fuse = PointFusion(1, 1, 1, 1, lateral_conv=False, img_levels=[0]).to(dev)
    img_feat, variants, expected = PF.reference_literal_inputs()
    for pts, meta in variants:
        assert fuse.fused_ok([img_feat.to(dev)], [pts.to(dev)])
        out = fuse.obtain_mlvl_feats([img_feat.to(dev)], [pts.to(dev)], [meta])
        assert torch.allclose(expected, out.cpu().view(-1), 1e-4)


def _golden_run(name, dev, fused):
    mod, (feats, pts, pts_feats, metas), info = PF.golden_case(name, dev)
    feats = [f.requires_grad_() for f in feats]
    pts_feats = pts_feats.requires_grad_()
    if fused:
        assert mod.fused_ok(feats, pts)
        out = mod(feats, pts, pts_feats, metas)
    else:
        img_pts = mod.obtain_mlvl_feats_composed(feats, pts, metas)
        out = mod.img_transform(img_pts) + mod.pts_transform(pts_feats)
        out = torch.relu(out) if mod.activate_out else out
        out = mod.fuse_conv(out) if mod.fuse_out else out
    (out * PF.arr(name, "grad_out", dev)).sum().backward()
    grads = {k: p.grad for k, p in mod.named_parameters()}
    return mod, out, grads, [f.grad for f in feats], pts_feats.grad


@pytest.mark.parametrize("name", PF.golden()[1])
def test_golden_cases_on_the_fused_path(dev, name):
    mod, out, grads, gmaps, gpf = _golden_run(name, dev, fused=True)
    assert PF.scaled_err(out, PF.arr(name, "out64")) <= TOL
    for k, err in PF.param_grad_errs(name, grads).items():
        assert err <= TOL, k
    for i, g in enumerate(gmaps):
        assert PF.scaled_err(g, PF.arr(name, "grad_map/%d" % i)) <= TOL, i
    assert PF.scaled_err(gpf, PF.arr(name, "grad_pts_feats")) <= TOL
    z = PF.golden()[0]
    for k in [k for k in z.files if k.startswith(name + "/after/") and "num_batches" not in k]:
        key = k[len(name + "/after/"):]
        assert PF.scaled_err(mod.state_dict()[key], torch.from_numpy(z[k])) <= TOL, key


@pytest.mark.parametrize("name", PF.golden()[1])
def test_fused_equals_composition_on_the_golden_cases(dev, name):
    a, out_a, grads_a, gm_a, _ = _golden_run(name, dev, fused=True)
    b, out_b, grads_b, gm_b, _ = _golden_run(name, dev, fused=False)
    assert PF.scaled_err(out_a, out_b) <= TOL
    errs_a, errs_b = PF.param_grad_errs(name, grads_a), PF.param_grad_errs(name, grads_b)
    for k in grads_a:
        assert errs_a[k] <= TOL and errs_b[k] <= TOL, k
    for x, y in zip(gm_a, gm_b):
        assert PF.scaled_err(x, y) <= TOL
    for k, v in b.state_dict().items():
        if "running" in k:
            assert PF.scaled_err(a.state_dict()[k], v) <= TOL, k


def test_nan_and_inf_rows_read_zeros_and_disturb_nothing(dev):
    mod, maps, pts, metas = _make(dev, (300, 257), [(16, 12, 39), (3, 6, 20)], SMALL_PAD, False,
                                  aug=True, seed=5)
    with torch.no_grad():
        clean = mod.obtain_mlvl_feats(maps, pts, metas)
    bad = [p.clone() for p in pts]
    rows = {0: [0, 17, 64, 299], 1: [1, 128, 256]}
    vals = [float("nan"), float("inf"), -float("inf")]
    for b, rr in rows.items():
        for j, r in enumerate(rr):
            bad[b][r, j % 3] = vals[j % 3]
    with torch.no_grad():
        got = mod.obtain_mlvl_feats(maps, bad, metas)
    hit = torch.zeros(557, dtype=torch.bool, device=dev)
    hit[rows[0]] = True
    hit[[300 + r for r in rows[1]]] = True
    assert float(got[hit].abs().max()) == 0.0
    assert torch.equal(got[~hit], clean[~hit])
    assert torch.isfinite(got).all()


def test_a_nan_map_cell_reaches_only_the_points_that_touch_it(dev):
    from msmdfusion_amd import kernels as K
    captured = {}
    real = K.point_sample_forward

    def spy(points, batch, maps, align):
        captured.update(points=points, batch=batch, shapes=[tuple(m.shape) for m in maps],
                        align=align)
        return real(points, batch, maps, align)

    mod, maps, pts, metas = _make(dev, (400,), [(8, 6, 20), (4, 3, 10)], SMALL_PAD, True, seed=6)
    with torch.no_grad():
        clean = mod.obtain_mlvl_feats(maps, pts, metas)
        maps[1][0, :, 1, 4] = float("nan")
        K.point_sample_forward = spy
        try:
            got = mod.obtain_mlvl_feats(maps, pts, metas)
        finally:
            K.point_sample_forward = real
    index = K.point_sample_index(captured["points"], captured["batch"], captured["shapes"],
                                 captured["align"])
    target = 6 * 20 + 1 * 10 + 4
    touch = (index.cell.view(400, 2, 4) == target).any(-1).any(-1)
    assert 0 < int(touch.sum()) < 400
    assert torch.equal(torch.isnan(got).any(1), touch)
    assert torch.equal(got[~touch], clean[~touch])
    assert not torch.isnan(got[:, :8]).any()


# ---------------------------------------------------------------- backward
def _backward_check(tag, mod, maps, pts, metas, seed=0):
    maps = [m.requires_grad_() for m in maps]
    out = mod.obtain_mlvl_feats(maps, pts, metas)
    g = torch.from_numpy(np.random.RandomState(seed).randn(*out.shape).astype(np.float32)).to(
        out.device)
    got = torch.autograd.grad((out * g).sum(), maps)
    refs = {}
    for dtype in (torch.float32, torch.float64):
        ms = [m.detach().to(dtype).requires_grad_() for m in maps]
        y = mod.obtain_mlvl_feats_composed(ms, [p.to(dtype) for p in pts], metas)
        refs[dtype] = (y, torch.autograd.grad((y * g.to(dtype)).sum(), ms))
    in_view = int((refs[torch.float64][0].abs().sum(1) > 0).sum())
    widest = max(m.shape[3] for m in maps)
    for i, (a, b32, b64) in enumerate(zip(got, refs[torch.float32][1], refs[torch.float64][1])):
        assert a.dtype == torch.float32 and tuple(a.shape) == tuple(b64.shape)
        _judge("%s grad level %d" % (tag, i), a, b32, b64, in_view, widest)
    return got


@pytest.mark.parametrize("tag", ["N63-C3-C4-noalign", "N257-C128-C129-1x1", "N257-1x1-noalign",
                                 "B2-L3", "N4099-B3-L5-96x312", "N4099-B3-L5-align"])
def test_map_gradients_against_float64_autograd(dev, tag):
    sizes, levels, pad, align, aug = FORWARD[tag]
    mod, maps, pts, metas = _make(dev, sizes, levels, pad, align, aug, seed=len(tag))
    grads = _backward_check(tag, mod, maps, pts, metas)
    for g, m in zip(grads, maps):
        # channels-last buffers viewed as NCHW
        assert g.permute(0, 2, 3, 1).is_contiguous() and tuple(g.shape) == tuple(m.shape)


def _pile(dev, counts, h, w, c, align=False, corner=False, pad=SMALL_PAD):
    """counts[i] points on (the centre of, or the corner shared by four cells at) cell i of a
    fixed list of cells of one (h, w) level."""
    l2i = PF.camera(pad[0], pad[1], 3)
    cells = [(0, 0), (h - 1, w - 1), (h // 2, w // 2), (0, w - 1)]
    sx, sy = pad[1] / w, pad[0] / h
    u, v = [], []
    for (y, x), n in zip(cells, counts):
        shift = 1.0 if corner else 0.5
        u += [(x + shift) * sx] * n
        v += [(y + shift) * sy] * n
    rng = np.random.RandomState(1)
    p = PF.pixels_to_points(l2i, np.array(u), np.array(v), rng.uniform(3, 30, len(u)))
    mod = PF.sampler([c], align_corners=align).to(dev)
    maps = [torch.from_numpy(rng.randn(1, c, h, w).astype(np.float32)).to(dev)]
    meta = dict(lidar2img=l2i.tolist(), input_shape=list(pad), img_shape=[pad[0], pad[1], 3])
    return mod, maps, [torch.from_numpy(p.astype(np.float32)).to(dev)], [meta], cells


def test_8192_points_on_one_cell_take_the_chunked_path(dev):
    mod, maps, pts, metas, _ = _pile(dev, [8192], 2, 3, 8)
    _backward_check("8192 on one cell", mod, maps, pts, metas)
    mod, maps, pts, metas, _ = _pile(dev, [8192], 1, 1, 5, align=True)      # a 1x1 level, scalar
    _backward_check("8192 on a 1x1 level", mod, maps, pts, metas)


def test_list_lengths_around_the_chunk(dev):
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd.fusion_layers import sample_params
    k = K.POINT_SAMPLE_BWD_CHUNK
    mod, maps, pts, metas, cells = _pile(dev, [k - 1, k, k + 1, 3], 6, 20, 12)
    _backward_check("chunk -1 / 0 / +1", mod, maps, pts, metas)
    params = torch.from_numpy(np.stack([sample_params(metas[0])]).astype(np.float32)).to(dev)
    starts = [0, pts[0].shape[0]]
    batch = K.PointSampleBatch(starts, torch.tensor(starts, dtype=torch.int32, device=dev), params)
    index = K.point_sample_index(pts[0], batch, [(1, 6, 20, 12)], False)
    lens = (index.start[1:] - index.start[:-1]).cpu()
    got = sorted(int(lens[y * 20 + x]) for y, x in cells)
    assert got == [3, k - 1, k, k + 1], got
    pieces = (index.piece_start[1:] - index.piece_start[:-1]).cpu()
    assert int(pieces[(6 // 2) * 20 + 20 // 2]) == 2
    assert torch.equal(pieces, torch.where(lens > k, (lens + k - 1) // k, torch.zeros_like(lens)))
    # every list ascends, and the lists partition the in-bounds contributions
    order, cell = index.order.cpu(), index.cell.cpu()
    total = int(index.start[-1])
    assert total == int((cell >= 0).sum())
    for c in [y * 20 + x for y, x in cells]:
        lst = order[int(index.start[c]):int(index.start[c + 1])]
        assert bool((lst[1:] > lst[:-1]).all()) and bool((cell[lst.long()] == c).all())


def test_a_point_on_four_cells_that_straddle_two_chunks(dev):
    from msmdfusion_amd import kernels as K
    k = K.POINT_SAMPLE_BWD_CHUNK
    mod, maps, pts, metas, _ = _pile(dev, [0, 0, k + 1, 0], 6, 20, 16, corner=True)
    grads = _backward_check("corner of four cells", mod, maps, pts, metas)
    # four cells carry k + 1 contributions each: two chunks per cell
    touched = int((grads[0].abs().sum(1) > 0).sum())
    assert touched == 4, touched


def test_untouched_cells_are_exact_zeros_in_a_nan_buffer(dev):
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd.fusion_layers import sample_params
    mod, maps, pts, metas, _ = _pile(dev, [70, 5, 0, 1], 6, 20, 8)
    shapes = [(1, 6, 20, 8), (1, 1, 1, 4)]
    params = torch.from_numpy(np.stack([sample_params(metas[0])]).astype(np.float32)).to(dev)
    starts = [0, pts[0].shape[0]]
    batch = K.PointSampleBatch(starts, torch.tensor(starts, dtype=torch.int32, device=dev), params)
    index = K.point_sample_index(pts[0], batch, shapes, False)
    g = torch.randn(76, 12, device=dev)
    bufs = [torch.full(s, float("nan"), device=dev) for s in shapes]
    grads = K.point_sample_backward(g, index, shapes, grads=bufs)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(grads, bufs))
    lens = index.start[1:] - index.start[:-1]
    empty = (lens[:120] == 0).view(1, 6, 20)
    assert int(empty.sum()) >= 100
    assert torch.isfinite(grads[0]).all() and torch.isfinite(grads[1]).all()
    assert float(grads[0][empty].abs().max()) == 0.0
    assert float(grads[0][~empty].abs().sum()) > 0 and float(grads[1].abs().sum()) > 0


def _flagship(dev, n_per=18000, channels=128):
    levels = [(channels, 96, 312), (channels, 48, 156), (channels, 24, 78), (channels, 12, 39),
              (channels, 6, 20)]
    return _make(dev, (n_per, n_per), levels, BIG_PAD, False, aug=True, seed=9,
                 channels_last=True)


def test_two_runs_give_the_same_bytes(dev):
    """B = 2, N = 2 x 18000, five levels of 128 channels, maps from 96x312 to 6x20."""
    mod, maps, pts, metas = _flagship(dev)
    runs = []
    for _ in range(2):
        ms = [m.detach().requires_grad_() for m in maps]
        out = mod.obtain_mlvl_feats(ms, pts, metas)
        assert tuple(out.shape) == (36000, 640)
        g = torch.autograd.grad((out * torch.cos(out)).sum(), ms)
        runs.append((out.detach(), g))
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b) and torch.isfinite(a).all()


def test_fall_backs_take_the_composition_path(dev):
    sizes, levels, pad = (257,), [(8, 6, 20), (4, 2, 3)], SMALL_PAD
    for kw in (dict(aligned=False), dict(padding_mode="border")):
        _, maps, pts, metas = _make(dev, sizes, levels, pad, True, seed=11)
        mod = PF.sampler([8, 4], **kw).to(dev)
        assert not mod.fused_ok(maps, pts)
        with torch.no_grad():
            got = mod.obtain_mlvl_feats(maps, pts, metas)
        if "padding_mode" in kw:       # (nearest is discontinuous: compared in float32 only)
            assert PF.scaled_err(got, PF.restate(mod, maps, pts, metas, torch.float64)) <= TOL
        assert torch.equal(got, PF.restate(mod, maps, pts, metas, torch.float32))
    mod, maps, pts, metas = _make(dev, sizes, levels, pad, True, seed=11)
    pts = [p[:, :3].clone().requires_grad_() for p in pts]
    assert not mod.fused_ok(maps, pts)
    out = mod.obtain_mlvl_feats(maps, pts, metas)
    assert PF.scaled_err(out, PF.restate(mod, maps, [p.detach() for p in pts], metas,
                                         torch.float64)) <= TOL
    out.sum().backward()
    assert pts[0].grad is not None and float(pts[0].grad.abs().sum()) > 0
    assert not mod.fused_ok([m.double() for m in maps], [p.detach() for p in pts])
    assert not mod.fused_ok([m.cpu() for m in maps], [p.detach().cpu() for p in pts])


def test_forward_makes_no_host_read_and_allocates_only_its_output(dev):
    levels = [(128, 96, 312), (128, 48, 156), (128, 24, 78), (128, 12, 39), (128, 6, 20)]
    mod, maps, pts, metas = _make(dev, (2000, 0, 2099), levels, BIG_PAD, False, aug=True, seed=2,
                                  channels_last=True)
    cat = torch.cat(pts, 0)
    with torch.no_grad():
        mod.obtain_mlvl_feats(maps, pts, metas, pts_cat=cat)       # (first-call set-up)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = mod.obtain_mlvl_feats(maps, pts, metas, pts_cat=cat)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    assert tuple(out.shape) == (4099, 640)
    assert peak <= out.numel() * 4 + (1 << 20), peak


# ---------------------------------------------------------------- DynamicVFE and the detector
VS, RG = (0.2, 0.2, 0.4), (0.0, -3.2, -3.0, 6.4, 3.2, 1.0)


def _scene(dev, seed=4, n=(1500, 1100), c=8, pad=(96, 320)):
    """Clouds in the range in front of the camera, image features of three levels, metas."""
    rng = np.random.RandomState(seed)
    pts, metas = [], []
    for i, k in enumerate(n):
        p = rng.uniform(0, 1, (k, 4)).astype(np.float32)
        p[:, 0] = RG[0] + 0.3 + p[:, 0] * (RG[3] - RG[0] - 0.3) * 0.999
        p[:, 1] = RG[1] + p[:, 1] * (RG[4] - RG[1]) * 0.999
        p[:, 2] = rng.uniform(-2.5, 0.5, k)
        pts.append(torch.from_numpy(p).to(dev))
        metas.append(dict(lidar2img=PF.camera(pad[0], pad[1], seed + i).tolist(),
                          input_shape=list(pad), img_shape=[pad[0], pad[1], 3],
                          flip=bool(i % 2), scale_factor=[0.95, 0.9, 0.95, 0.9]))
    feats = [torch.from_numpy(rng.randn(len(n), c, pad[0] // s, pad[1] // s).astype(np.float32))
             .to(dev) for s in (4, 8, 16, 32, 64)]
    return pts, feats, metas


@pytest.mark.parametrize("training", [True, False])
def test_dynamic_vfe_with_the_layer_equals_its_parts(dev, training):
    from msmdfusion_amd.dynamic_scatter import scatter_index, scatter_reduce
    from msmdfusion_amd.registry import build_voxel_encoder
    from msmdfusion_amd.voxelize import Voxelization
    torch.manual_seed(1)
    enc = build_voxel_encoder(dict(
        type="DynamicVFE", in_channels=4, feat_channels=[16, 16], with_cluster_center=True,
        with_voxel_center=True, voxel_size=VS, point_cloud_range=RG,
        fusion_layer=dict(type="PointFusion", img_channels=8, pts_channels=16, mid_channels=12,
                          out_channels=20, img_levels=[0, 1, 2], align_corners=False))).to(dev)
    enc.train(training)
    pts, feats, metas = _scene(dev)
    vox = Voxelization(voxel_size=VS, point_cloud_range=RG, max_num_points=-1, max_voxels=(-1, -1))
    coors = torch.cat([torch.nn.functional.pad(vox(p), (1, 0), value=b)
                       for b, p in enumerate(pts)], 0)
    cat = torch.cat(pts, 0)
    parts = copy.deepcopy(enc)
    out, out_coors = enc(cat, coors, points=pts, img_feats=feats, img_metas=metas)
    assert out.shape[1] == 20 and out.shape[0] == out_coors.shape[0]
    layer = parts.fusion_layer
    parts.fusion_layer, parts.return_point_feats = None, True
    index = scatter_index(coors.contiguous())
    point_feats = parts(cat, coors, index=index)
    fused = layer(feats, pts, point_feats, metas)
    exp = scatter_reduce(fused, index, parts.vfe_scatter.reduce_type)
    assert torch.equal(out_coors, index.voxel_coors)
    assert PF.scaled_err(out, exp) <= TOL
    g = torch.randn_like(out)
    (out * g).sum().backward()
    (exp * g).sum().backward()
    parts.fusion_layer = layer
    mine, theirs = dict(enc.named_parameters()), dict(parts.named_parameters())
    assert set(mine) == set(theirs)
    for k, p in mine.items():
        assert p.grad is not None and float(p.grad.abs().sum()) > 0, k
        assert PF.scaled_err(p.grad, theirs[k].grad) <= TOL, k


def test_dynamic_mvx_faster_rcnn_trains_and_infers(dev):
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.registry import build_detector
    model = copy.deepcopy(C.MVXNET_DV_SECOND_KITTI)
    rng_ = list(RG)
    model["pts_voxel_layer"].update(point_cloud_range=rng_)
    model["pts_voxel_encoder"].update(point_cloud_range=rng_)
    model["pts_voxel_encoder"]["fusion_layer"].update(img_channels=16)
    model["pts_middle_encoder"].update(sparse_shape=[41, 128, 128])
    for r in model["pts_bbox_head"]["anchor_generator"]["ranges"]:
        r[0:2], r[3:5] = [0, -3.2], [6.4, 3.2]
    torch.manual_seed(3)
    det = build_detector(model).to(dev)
    assert type(det).__name__ == "DynamicMVXFasterRCNN"
    pts, feats, metas = _scene(dev, n=(4000, 3500), c=16)
    gt = [torch.tensor([[4.0, 1.0, -1.6, 1.6, 3.9, 1.56, 0.3],
                        [3.0, -2.0, -0.6, 0.6, 0.8, 1.73, 1.0]], device=dev),
          torch.zeros((0, 7), device=dev)]
    labels = [torch.tensor([2, 0], device=dev), torch.zeros((0,), dtype=torch.long, device=dev)]
    det.train()
    losses = det(pts, return_loss=True, gt_bboxes_3d=gt, gt_labels_3d=labels, img_feats=feats,
                 img_metas=metas)
    assert sorted(losses) == ["loss_bbox", "loss_cls", "loss_dir"]
    total = sum(sum(v) for v in losses.values())
    assert torch.isfinite(total)
    total.backward()
    layer = det.pts_voxel_encoder.fusion_layer
    for k, p in layer.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        assert float(p.grad.abs().sum()) > 0, k
    det.eval()
    with torch.no_grad():
        out = det.simple_test(pts, img_metas=metas, img_feats=feats)
    assert len(out) == 2
    for r in out:
        n = r["scores_3d"].shape[0]
        assert r["boxes_3d"].shape == (n, 7) and r["labels_3d"].shape == (n,) and n <= 50
    # the image features may also come from an injected image branch
    class Branch(torch.nn.Module):
        def forward(self, img):
            return feats
    det.img_backbone = Branch()
    img = torch.zeros(2, 3, 96, 320, device=dev)
    plain = [{k: v for k, v in m.items() if k != "input_shape"} for m in metas]
    with torch.no_grad():
        _, by_keyword = det.extract_feat(pts, img_metas=metas, img_feats=feats)
        got_feats, by_branch = det.extract_feat(pts, img=img, img_metas=plain)
        again = det.simple_test(pts, img_metas=plain, img=img)
    assert got_feats is feats and plain[0]["input_shape"] == img.shape[-2:]
    assert len(again) == 2
    for a, b in zip(by_keyword, by_branch):
        assert PF.scaled_err(a, b) <= TOL
