"""Dynamic voxelization and DynamicScatter on the GPU (csrc/dynamic_voxel.hip): coordinates
bit-exact against a float32 numpy restatement of voxelization_cuda.cu:25-61, the scatter
against a numpy restatement of scatter_points_cuda.cu, DynamicScatter against the reference's
per-sample loop, DynamicSimpleVFE against HardSimpleVFE, DynamicVFE against a torch
restatement of voxel_encoder.py:92-286, and the detector's dynamic path."""
import numpy as np
import pytest
import torch

from msmdfusion_amd import synthetic as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

VS, RG = S.VOXEL_SIZE, S.POINT_CLOUD_RANGE


def _np(x):
    return x.detach().cpu().numpy()


def np_dynamic_voxelize(pts, vs, rg, init):
    """voxelization_cuda.cu:25-61 in float32, write pattern included."""
    out = init.copy()
    vs = np.asarray(vs, np.float32)
    lo = np.asarray(rg[:3], np.float32)
    hi = np.asarray(rg[3:], np.float32)
    grid = np.round((hi - lo) / vs).astype(np.int64)
    q = [np.floor((pts[:, j].astype(np.float32) - lo[j]) / vs[j]).astype(np.int64) for j in range(3)]
    bad = [(q[j] < 0) | (q[j] >= grid[j]) for j in range(3)]
    bx, by, bz = bad[0], ~bad[0] & bad[1], ~bad[0] & ~bad[1] & bad[2]
    ok = ~bad[0] & ~bad[1] & ~bad[2]
    out[bx, 0] = -1
    out[by, 0:2] = -1
    out[bz, 0:3] = -1
    out[ok, 0], out[ok, 1], out[ok, 2] = q[2][ok], q[1][ok], q[0][ok]
    return out


def np_scatter(feats, coors, reduce):
    """scatter_points_cuda.cu:246-306: rows in lexicographic order, sums in float64."""
    valid = (coors >= 0).all(1)
    cmap = np.full(coors.shape[0], -1, np.int32)
    if not valid.any():
        return (np.zeros((0, feats.shape[1])), np.zeros((0, coors.shape[1]), np.int32), cmap,
                np.zeros(0, np.int32), np.zeros((0, feats.shape[1]), np.int64))
    uniq, inv = np.unique(coors[valid], axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cmap[valid] = inv
    m, c = uniq.shape[0], feats.shape[1]
    counts = np.bincount(inv, minlength=m).astype(np.int32)
    pid = np.nonzero(valid)[0]
    f = feats[valid].astype(np.float64)
    out = np.zeros((m, c))
    arg = np.zeros((m, c), np.int64)
    if reduce == "max":
        out[:] = -np.inf
        np.maximum.at(out, inv, f)
        first = np.full((m, c), feats.shape[0], np.int64)
        eq = f == out[inv]
        for ch in range(c):
            np.minimum.at(first[:, ch], inv[eq[:, ch]], pid[eq[:, ch]])
        arg = first
    else:
        np.add.at(out, inv, f)
        if reduce == "mean":
            out /= counts[:, None]
    return out, uniq.astype(np.int32), cmap, counts, arg


def _edge_points():
    lo, hi = np.array(RG[:3], np.float32), np.array(RG[3:], np.float32)
    mid = (lo + hi) / 2
    rows = [lo, hi, np.array([lo[0], hi[1], mid[2]], np.float32)]
    for ax in range(3):
        for v in (lo[ax] - 0.01, hi[ax], hi[ax] + 1.0):
            p = mid.copy()
            p[ax] = v
            rows.append(p)
    for v in ([lo[0] - 1, lo[1] - 1, mid[2]], [mid[0], lo[1] - 1, lo[2] - 1],
              [lo[0] - 1, mid[1], hi[2] + 1]):
        rows.append(np.array(v, np.float32))
    e = np.stack(rows).astype(np.float32)
    return np.concatenate([e, np.ones((e.shape[0], 2), np.float32)], 1)


def test_dynamic_voxelize_bit_exact(dev):
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd.integration import voxel_layer
    pts = np.concatenate([S.lidar_sweep(3, n_az=600), _edge_points()])
    d = torch.from_numpy(pts).to(dev)
    for fill in (0, 7):
        init = np.full((pts.shape[0], 3), fill, np.int32)
        exp = np_dynamic_voxelize(pts, VS, RG, init)
        got = torch.from_numpy(init).to(dev)
        voxel_layer.dynamic_voxelize(d, got, VS, RG, 3)
        assert np.array_equal(_np(got), exp), fill
        got2 = K.dynamic_voxelize(d, VS, RG, torch.from_numpy(init).to(dev))
        assert np.array_equal(_np(got2), exp)
    # the edge rows pin which slots receive -1 (x: slot 0, y: 0-1, z: 0-2)
    ep = _edge_points()
    e = np_dynamic_voxelize(ep, VS, RG, np.full((ep.shape[0], 3), 7, np.int32))
    assert (e == -1).any(1).sum() >= 8 and (e == 7).any()
    # the set of valid voxels equals hard voxelization with caps no tighter than the data
    c = np_dynamic_voxelize(pts, VS, RG, np.zeros((pts.shape[0], 3), np.int32))
    uniq, cnt = np.unique(c[(c >= 0).all(1)], axis=0, return_counts=True)
    for use_ref in ((False, True) if O.have_ref() else (False,)):
        _, hc, _ = O.hard_voxelize(pts, VS, RG, int(cnt.max()), uniq.shape[0], use_ref=use_ref)
        assert np.array_equal(np.unique(hc, axis=0), uniq)


def test_voxelization_module_dynamic(dev):
    from msmdfusion_amd.integration import voxel_layer
    from msmdfusion_amd.voxelize import Voxelization, voxelization
    pts = torch.from_numpy(np.concatenate([S.lidar_sweep(4, n_az=300), _edge_points()])).to(dev)
    exp = torch.zeros((pts.shape[0], 3), dtype=torch.int32, device=dev)
    voxel_layer.dynamic_voxelize(pts, exp, VS, RG, 3)
    for mp, mv in ((-1, 20000), (10, -1)):
        got = Voxelization(VS, RG, mp, mv)(pts)
        assert got.dtype == torch.int32 and torch.equal(got, exp)
        assert torch.equal(voxelization(pts, VS, RG, mp, mv), exp)


def _random_coors(rng, n, ndim, extent=6, bad_frac=0.1):
    c = rng.randint(0, extent, size=(n, ndim)).astype(np.int32)
    bad = rng.rand(n) < bad_frac
    col = rng.randint(0, ndim, size=n)
    c[bad, col[bad]] = rng.choice([-1, -3, -100], size=bad.sum())
    return c


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("ndim", [3, 4])
@pytest.mark.parametrize("c", [3, 5, 64, 128])
def test_forward_parity(dev, reduce, ndim, c):
    from msmdfusion_amd.integration import voxel_layer
    rng = np.random.RandomState(ndim * 1000 + c)
    n = 6000
    coors = _random_coors(rng, n, ndim, extent=5 if ndim == 4 else 9)
    feats = rng.randn(n, c).astype(np.float32)
    feats[rng.rand(n, c) < 0.2] = 0.5           # ties for max
    out, oc, cmap, cnt = voxel_layer.dynamic_point_to_voxel_forward(
        torch.from_numpy(feats).to(dev), torch.from_numpy(coors).to(dev), reduce)
    e_out, e_oc, e_map, e_cnt, _ = np_scatter(feats, coors, reduce)
    assert np.array_equal(_np(oc), e_oc) and np.array_equal(_np(cmap), e_map)
    assert np.array_equal(_np(cnt), e_cnt if reduce == "mean" else np.zeros_like(e_cnt))
    if reduce == "max":
        assert np.array_equal(_np(out), e_out.astype(np.float32))
    else:
        assert np.allclose(_np(out), e_out, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("case", ["one_voxel", "all_invalid", "empty", "negative"])
def test_forward_edges(dev, case):
    from msmdfusion_amd.integration import voxel_layer
    rng = np.random.RandomState(1)
    n = 0 if case == "empty" else 3000
    if case == "one_voxel":
        coors = np.tile(np.array([[1, 2, 3]], np.int32), (n, 1))
    elif case == "all_invalid":
        coors = np.full((n, 3), -1, np.int32)
    else:
        coors = _random_coors(rng, n, 3, bad_frac=0.5)
        if n:
            coors[::7, 1] = -5
    feats = rng.randn(n, 5).astype(np.float32)
    for reduce in ("sum", "mean", "max"):
        out, oc, cmap, cnt = voxel_layer.dynamic_point_to_voxel_forward(
            torch.from_numpy(feats).to(dev), torch.from_numpy(coors).to(dev), reduce)
        e_out, e_oc, e_map, e_cnt, _ = np_scatter(feats, coors, reduce)
        assert np.array_equal(_np(oc), e_oc) and np.array_equal(_np(cmap), e_map)
        assert out.shape == (e_oc.shape[0], 5)
        assert np.allclose(_np(out), e_out, rtol=1e-5, atol=1e-5)
        if reduce == "mean":
            assert np.array_equal(_np(cnt), e_cnt)


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_backward(dev, reduce):
    from msmdfusion_amd.dynamic_scatter import dynamic_scatter
    from msmdfusion_amd.integration import voxel_layer
    rng = np.random.RandomState(5)
    n, c = 5000, 7
    coors = _random_coors(rng, n, 4, extent=4)
    feats = rng.randn(n, c).astype(np.float32)
    feats[rng.rand(n, c) < 0.5] = 1.25          # deliberate ties of the maximum
    e_out, _, e_map, e_cnt, e_arg = np_scatter(feats, coors, reduce)
    g = rng.randn(e_out.shape[0], c).astype(np.float32)
    exp = np.zeros((n, c), np.float32)
    valid = e_map >= 0
    if reduce == "sum":
        exp[valid] = g[e_map[valid]]
    elif reduce == "mean":
        exp[valid] = g[e_map[valid]] / e_cnt[e_map[valid]][:, None].astype(np.float32)
    else:
        for v in range(e_out.shape[0]):
            exp[e_arg[v], np.arange(c)] = g[v]
    df = torch.from_numpy(feats).to(dev)
    dc = torch.from_numpy(coors).to(dev)
    dg = torch.from_numpy(g).to(dev)
    # the shim: reference argument list, grad_feats filled in place
    out, oc, cmap, cnt = voxel_layer.dynamic_point_to_voxel_forward(df, dc, reduce)
    gf = torch.full_like(df, 3.0)
    voxel_layer.dynamic_point_to_voxel_backward(gf, dg, df, out, cmap, cnt, reduce)
    assert np.array_equal(_np(gf), exp)
    assert not _np(gf)[~valid].any()
    # autograd: the argmax of the forward itself
    x = df.clone().requires_grad_(True)
    y, _ = dynamic_scatter(x, dc, reduce)
    y.backward(dg)
    assert np.array_equal(_np(x.grad), exp)


def test_mean_bitwise_reproducible(dev):
    from msmdfusion_amd.dynamic_scatter import dynamic_scatter
    rng = np.random.RandomState(7)
    n = 4 * 290000
    b = np.repeat(np.arange(4, dtype=np.int32), n // 4)
    zyx = rng.randint(0, 12, size=(n, 3)).astype(np.int32)      # ~800 points per voxel
    coors = torch.from_numpy(np.concatenate([b[:, None], zyx], 1)).to(dev)
    feats = torch.from_numpy(rng.randn(n, 16).astype(np.float32) * 100).to(dev)
    a, ca = dynamic_scatter(feats, coors, "mean")
    b2, cb = dynamic_scatter(feats, coors, "mean")
    torch.cuda.synchronize()
    assert torch.equal(ca, cb)
    assert np.array_equal(_np(a).view(np.int32), _np(b2).view(np.int32))


def test_dynamic_scatter_matches_reference_loop(dev):
    from msmdfusion_amd.dynamic_scatter import DynamicScatter, dynamic_scatter
    rng = np.random.RandomState(9)
    sizes = [3000, 0, 2500, 4000]
    coors = np.concatenate([np.concatenate([np.full((s, 1), b, np.int32),
                                            _random_coors(rng, s, 3, extent=10)], 1)
                            for b, s in enumerate(sizes)])
    feats = torch.from_numpy(rng.randn(coors.shape[0], 6).astype(np.float32)).to(dev)
    dc = torch.from_numpy(coors).to(dev)
    for avg in (True, False):
        mod = DynamicScatter(VS, RG, avg)
        got, got_c = mod(feats, dc)
        # scatter_points.py:99-114, restated: per sample, batch column padded back
        voxels, vcoors = [], []
        for i in range(int(dc[-1, 0]) + 1):
            inds = torch.where(dc[:, 0] == i)
            if inds[0].numel() == 0:
                continue
            v, vc = dynamic_scatter(feats[inds].contiguous(), dc[inds][:, 1:].contiguous(),
                                    mod.reduce_type)
            vcoors.append(torch.nn.functional.pad(vc, (1, 0), mode="constant", value=i))
            voxels.append(v)
        assert torch.equal(got_c, torch.cat(vcoors))
        assert torch.equal(got, torch.cat(voxels))      # same points, same order per voxel


def test_dynamic_simple_vfe_matches_hard(dev):
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd.voxel_encoder import DynamicSimpleVFE, HardSimpleVFE
    pts = torch.from_numpy(S.lidar_sweep(11, n_az=500)).to(dev)
    coors = K.dynamic_voxelize(pts, VS, RG)
    c = _np(coors)
    _, cnt = np.unique(c[(c >= 0).all(1)], axis=0, return_counts=True)
    # uncapped: caps no tighter than the data
    voxels, hc, num, _ = K.hard_voxelize(pts, VS, RG, int(cnt.max()), cnt.shape[0])
    assert int(num.sum()) == int(cnt.sum())
    hard = HardSimpleVFE(5)(voxels, num, hc)
    dyn, dc = DynamicSimpleVFE(VS, RG)(pts, coors)
    ho = np.lexsort(_np(hc).T[::-1])
    assert np.array_equal(_np(hc)[ho], _np(dc))
    assert np.allclose(_np(hard)[ho], _np(dyn), rtol=1e-6, atol=1e-6)


def _torch_dynamic_vfe(m, features, coors):
    """voxel_encoder.py:220-286 on torch.unique (in-range inputs); max picks the smallest
    point index among ties, the reference's traceback."""
    uniq, inv = torch.unique(coors, dim=0, return_inverse=True)
    n, mv = features.shape[0], uniq.shape[0]
    cnt = torch.bincount(inv, minlength=mv).float()

    def scatter(x, mode):
        c = x.shape[1]
        ie = inv[:, None].expand(-1, c)
        if mode == "mean":
            return x.new_zeros((mv, c)).index_add(0, inv, x) / cnt[:, None]
        mx = x.new_full((mv, c), -float("inf")).scatter_reduce(0, ie, x.detach(), "amax")
        ids = torch.arange(n, device=x.device)[:, None].expand(-1, c)
        ids = torch.where(x.detach() == mx[inv], ids, torch.full_like(ids, n))
        first = torch.full((mv, c), n, device=x.device, dtype=torch.long).scatter_reduce(
            0, ie, ids, "amin")
        return torch.gather(x, 0, first)

    ls = [features]
    if m._with_cluster_center:
        ls.append(features[:, :3] - scatter(features, "mean")[inv][:, :3])
    if m._with_voxel_center:
        f = features.new_zeros((n, 3))
        f[:, 0] = features[:, 0] - (coors[:, 3].type_as(features) * m.vx + m.x_offset)
        f[:, 1] = features[:, 1] - (coors[:, 2].type_as(features) * m.vy + m.y_offset)
        f[:, 2] = features[:, 2] - (coors[:, 1].type_as(features) * m.vz + m.z_offset)
        ls.append(f)
    x = torch.cat(ls, -1)
    mode = "mean" if m.vfe_scatter.average_points else "max"
    for i, vfe in enumerate(m.vfe_layers):
        pf = vfe(x)
        vf = scatter(pf, mode)
        if i != len(m.vfe_layers) - 1:
            x = torch.cat([pf, vf[inv]], 1)
    return vf, uniq


@pytest.mark.parametrize("mode", ["max", "avg"])
@pytest.mark.parametrize("train", [True, False])
def test_dynamic_vfe_matches_torch_restatement(dev, mode, train):
    import copy
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd.voxel_encoder import DynamicVFE
    vs = [0.6, 0.6, 2.0]
    clouds = [S.lidar_sweep(s, n_az=200) for s in (1, 2)]
    pts, coors = [], []
    for b, p in enumerate(clouds):
        d = torch.from_numpy(p).to(dev)
        c = K.dynamic_voxelize(d, vs, RG)
        keep = (c >= 0).all(1)
        pts.append(d[keep])
        coors.append(torch.nn.functional.pad(c[keep], (1, 0), value=b))
    pts, coors = torch.cat(pts), torch.cat(coors)
    torch.manual_seed(0)
    m = DynamicVFE(in_channels=5, feat_channels=[32, 32], with_cluster_center=True,
                   with_voxel_center=True, voxel_size=vs, point_cloud_range=RG,
                   mode=mode).to(dev)
    for p in m.parameters():
        p.data.uniform_(-0.5, 0.5)
    m.train(train)
    r = copy.deepcopy(m)
    x1 = pts.clone().requires_grad_(True)
    x2 = pts.clone().requires_grad_(True)
    got, gc = m(x1, coors)
    exp, ec = _torch_dynamic_vfe(r, x2, coors)
    assert torch.equal(gc, ec.int())
    assert torch.allclose(got, exp, rtol=1e-5, atol=1e-5)
    g = torch.randn_like(got)
    got.backward(g)
    exp.backward(g)
    assert torch.allclose(x1.grad, x2.grad, rtol=1e-4, atol=1e-4)
    for (name, a), b in zip(m.named_parameters(), r.parameters()):
        assert torch.allclose(a.grad, b.grad, rtol=1e-4, atol=1e-4), name


def test_shim_rejects_bad_arguments(dev):
    from msmdfusion_amd.integration import voxel_layer
    pts = torch.from_numpy(S.lidar_sweep(0, n_az=64)).to(dev)
    n = pts.shape[0]
    ok = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    feats = torch.randn(n, 4, device=dev)
    torch.cuda.synchronize()
    bad_voxelize = [(pts.cpu(), ok), (pts, ok.cpu()), (pts, ok.long()), (pts.double(), ok),
                    (pts, ok[:-1]), (pts, torch.zeros((n, 4), dtype=torch.int32, device=dev)),
                    (pts, torch.zeros((3, n), dtype=torch.int32, device=dev).t())]
    for p, c in bad_voxelize:
        with pytest.raises(RuntimeError):
            voxel_layer.dynamic_voxelize(p, c, VS, RG, 3)
    bad_fwd = [(feats.cpu(), ok.cpu(), "max"), (feats.double(), ok, "max"),
               (feats, ok.long(), "mean"), (feats[:-1], ok, "sum"), (feats, ok, "min"),
               (feats, ok, "avg")]
    for f, c, r in bad_fwd:
        with pytest.raises(RuntimeError):
            voxel_layer.dynamic_point_to_voxel_forward(f, c, r)
    out, oc, cmap, cnt = voxel_layer.dynamic_point_to_voxel_forward(feats, ok, "mean")
    with pytest.raises(RuntimeError):
        voxel_layer.dynamic_point_to_voxel_backward(torch.zeros_like(feats), out, feats, out,
                                                    cmap, cnt, "median")
    with pytest.raises(RuntimeError):
        voxel_layer.dynamic_point_to_voxel_backward(torch.zeros_like(feats).cpu(), out, feats,
                                                    out, cmap, cnt, "mean")


def test_host_validation_enqueues_nothing(dev):
    """A refused call returns before any launch: a capture of it holds no kernel."""
    from msmdfusion_amd import _lib
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rc = [_lib.lib.msmd_dynamic_voxelize(None, -1, 5, None, None, 3, None, None),
              _lib.lib.msmd_scatter_index(None, 10, 9, None, None, None, None, None, None, None,
                                          0, None),
              _lib.lib.msmd_scatter_reduce_f32(None, 10, 4, None, None, 2, 5, None, None, None),
              _lib.lib.msmd_scatter_reduce_bwd_f32(None, 2, 10, 4, None, None, None, 1, None,
                                                   None),
              _lib.lib.msmd_scatter_gather_f32(None, 2, 0, None, 10, None, None)]
    assert all(r == -1 for r in rc)
    assert s.query()


def _dyn_detector(dev):
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.detector import build_detector
    cfg = dict(C.TRANSFUSION_L["model"])
    cfg["pts_voxel_layer"] = dict(cfg["pts_voxel_layer"], max_num_points=-1, max_voxels=(-1, -1))
    cfg["pts_voxel_encoder"] = dict(type="DynamicSimpleVFE", voxel_size=VS, point_cloud_range=RG)
    cfg.pop("pts_backbone"), cfg.pop("pts_neck")
    return build_detector(cfg).to(dev).eval()


def test_detector_dynamic_voxel_layer(dev):
    det = _dyn_detector(dev)
    clouds = [S.lidar_sweep(s, n_az=300) for s in (21, 22)]
    points = [torch.from_numpy(p).to(dev) for p in clouds]
    feats, coors = [], []
    for b, p in enumerate(clouds):
        c = np_dynamic_voxelize(p, VS, RG, np.zeros((p.shape[0], 3), np.int32))
        feats.append(p)
        coors.append(np.concatenate([np.full((p.shape[0], 1), b, np.int32), c], 1))
    mean, vc, _, _, _ = np_scatter(np.concatenate(feats), np.concatenate(coors), "mean")
    with torch.no_grad():
        exp, _ = det.pts_middle_encoder(torch.from_numpy(mean.astype(np.float32)).to(dev),
                                        torch.from_numpy(vc).to(dev), 2)
        got = det.extract_sparse_feat(points)
        got2 = det.extract_sparse_feat(points, prepared=det.prepare(points))
    assert torch.allclose(got, exp, rtol=1e-4, atol=1e-4)
    assert torch.equal(got, got2)
