"""PointNet++ op family on the GPU: the reference's known answers, bitwise agreement with the
numpy restatement (tests/pointnet_ref.py), the deterministic backward, QueryAndGroup, the
extension shims.

Clouds are drawn on a grid of multiples of 1/4 in [-4, 4] with duplicated points: every
squared distance is exact in float32, ties are exact and frequent."""
import os

import numpy as np
import pytest
import torch

import pointnet_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "pointnet_ops_vectors.npz"))
MARGIN = 4.0          # of torch's own float32 error against float64 (tests/test_gpu_pillar.py)


def g(name, dev):
    return torch.from_numpy(GOLDEN[name]).to(dev)


def grid_cloud(rs, b, n, dup=True):
    pts = rs.randint(-16, 17, size=(b, n, 3)).astype(np.float32) / 4
    if dup and n >= 4:
        pts[:, n // 2] = pts[:, 0]
        pts[:, n - 1] = pts[:, 1]
    return pts


def P():
    from msmdfusion_amd import pointnet_ops
    return pointnet_ops


# ---------------------------------------------------------------- golden vectors
def test_golden_vectors_through_the_kernels(dev):
    p = P()
    out = p.gather_points(g("gather_points__features", dev), g("gather_points__idx", dev))
    assert torch.allclose(out, g("gather_points__expected_output", dev))
    out = p.grouping_operation(g("grouping_points__festures", dev), g("grouping_points__idx", dev))
    assert torch.allclose(out, g("grouping_points__expected_output", dev))
    out = p.three_interpolate(g("three_interpolate__features", dev),
                              g("three_interpolate__idx", dev),
                              g("three_interpolate__weight", dev))
    assert torch.allclose(out, g("three_interpolate__expected_output", dev), 1e-4)
    dist, idx = p.three_nn(g("three_nn__unknown", dev), g("three_nn__known", dev))
    assert torch.allclose(dist, g("three_nn__expected_dist", dev), 1e-4)
    assert idx.dtype == torch.int32 and torch.all(idx == g("three_nn__expected_idx", dev))
    xyz, new_xyz = g("knn__xyz", dev), g("knn__new_xyz", dev)
    exp = g("knn__expected_idx", dev)
    assert torch.all(p.knn(5, xyz, new_xyz) == exp)
    assert torch.all(p.knn(5, xyz.transpose(1, 2).contiguous(),
                           new_xyz.transpose(1, 2).contiguous(), True) == exp)
    assert torch.all(p.knn(5, xyz, xyz) == g("knn__expected_idx_self", dev))
    idx = p.furthest_point_sample_with_dist(g("fps_with_dist__xyz_square_dist", dev), 3)
    assert idx.dtype == torch.int32 and torch.all(idx == g("fps_with_dist__expected_idx", dev))


# ---------------------------------------------------------------- gather / group forward
@pytest.mark.parametrize("b,c,n,npoint,nsample", [
    (1, 1, 1, 1, 1), (2, 3, 63, 17, 5), (3, 16, 65, 256, 32), (2, 129, 257, 17, 1),
    (1, 129, 1000, 256, 5), (3, 3, 1000, 1, 32), (2, 16, 65, 0, 5)])
def test_gather_and_group_equal_torch_gather(dev, b, c, n, npoint, nsample):
    p = P()
    gen = torch.Generator().manual_seed(n * 7 + c)
    feat = torch.randn((b, c, n), generator=gen).to(dev)
    idx = torch.randint(0, n, (b, npoint, nsample), generator=gen, dtype=torch.int32).to(dev)
    out = p.grouping_operation(feat, idx)
    assert tuple(out.shape) == (b, c, npoint, nsample) and out.dtype == torch.float32
    want = torch.gather(feat, 2, idx.long().view(b, 1, -1).expand(b, c, -1))
    assert torch.equal(out, want.view(b, c, npoint, nsample))
    idx1 = idx[:, :, 0].contiguous()
    out = p.gather_points(feat, idx1)
    assert tuple(out.shape) == (b, c, npoint)
    assert torch.equal(out, torch.gather(feat, 2, idx1.long()[:, None].expand(b, c, -1)))


def test_gather_passes_nan_and_inf_through(dev):
    p = P()
    feat = torch.tensor([[[float("nan"), float("inf"), -float("inf"), 1.5, -0.0]]], device=dev)
    idx = torch.tensor([[4, 0, 1, 2, 3, 0]], dtype=torch.int32, device=dev)
    for out in (p.gather_points(feat, idx), p.grouping_operation(feat, idx[:, :, None])[..., 0]):
        assert torch.equal(out.view(torch.int32), feat[:, :, idx[0].long()].view(torch.int32))


# ---------------------------------------------------------------- three_nn / three_interpolate
@pytest.mark.parametrize("m", [1, 2, 3, 64, 65, 1000])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_three_nn_is_bitwise_the_restatement(dev, n, m):
    from msmdfusion_amd import kernels as K
    rs = np.random.RandomState(n + m)
    unknown, known = grid_cloud(rs, 2, n), grid_cloud(rs, 2, m)
    dist2, idx = K.three_nn(torch.from_numpy(unknown).to(dev), torch.from_numpy(known).to(dev))
    e_dist2, e_idx = R.three_nn(unknown, known)
    assert np.array_equal(idx.cpu().numpy(), e_idx)
    assert np.array_equal(dist2.cpu().numpy().view(np.int32), e_dist2.view(np.int32))
    dist, idx2 = P().three_nn(torch.from_numpy(unknown).to(dev), torch.from_numpy(known).to(dev))
    assert np.array_equal(dist.cpu().numpy().view(np.int32), np.sqrt(e_dist2).view(np.int32))
    if m < 3:
        assert (idx2[:, :, m:] == 0).all() and torch.isinf(dist[:, :, m:]).all()


def test_three_nn_of_identical_points_takes_the_first_three(dev):
    known = torch.full((1, 70, 3), 0.25, device=dev)
    dist, idx = P().three_nn(torch.zeros((1, 5, 3), device=dev), known)
    assert torch.equal(idx, torch.tensor([0, 1, 2], dtype=torch.int32, device=dev).expand(1, 5, 3))
    assert (dist == dist[0, 0, 0]).all()


@pytest.mark.parametrize("c", [1, 5, 129])
def test_three_interpolate_is_bitwise_the_restatement(dev, c):
    rs = np.random.RandomState(c)
    b, m, n = 2, 77, 300
    feat = rs.randn(b, c, m).astype(np.float32)
    idx = rs.randint(0, m, size=(b, n, 3)).astype(np.int32)
    w = rs.rand(b, n, 3).astype(np.float32)
    w[:, ::7] = GOLDEN["three_interpolate__weight"][0, 1]       # near-zero weights
    out = P().three_interpolate(*(torch.from_numpy(a).to(dev) for a in (feat, idx, w)))
    assert np.array_equal(out.cpu().numpy().view(np.int32),
                          R.three_interpolate(feat, idx, w).view(np.int32))


# ---------------------------------------------------------------- knn
@pytest.mark.parametrize("k,n,npoint", [
    (1, 1, 1), (5, 5, 15), (16, 16, 17), (33, 129, 17), (128, 128, 15), (128, 1000, 300),
    (16, 1000, 300), (5, 129, 1), (1, 1000, 17), (33, 33, 300)])
def test_knn_is_exactly_the_restatement(dev, k, n, npoint):
    rs = np.random.RandomState(k * 31 + n)
    xyz, centres = grid_cloud(rs, 2, n), grid_cloud(rs, 2, npoint)
    txyz, tc = torch.from_numpy(xyz).to(dev), torch.from_numpy(centres).to(dev)
    idx = P().knn(k, txyz, tc)
    assert tuple(idx.shape) == (2, k, npoint) and idx.dtype == torch.int64
    assert np.array_equal(idx.cpu().numpy(), R.knn(k, xyz, centres))
    idx_t = P().knn(k, txyz.transpose(1, 2).contiguous(), tc.transpose(1, 2).contiguous(), True)
    assert torch.equal(idx_t, idx)


def test_knn_of_a_cloud_with_itself_puts_self_first_unless_duplicated(dev):
    rs = np.random.RandomState(3)
    xyz = grid_cloud(rs, 1, 400, dup=False)
    idx = P().knn(4, torch.from_numpy(xyz).to(dev), torch.from_numpy(xyz).to(dev))
    e = R.knn(4, xyz, xyz)
    assert np.array_equal(idx.cpu().numpy(), e)
    first = idx[0, 0].cpu().numpy()
    assert (first <= np.arange(400)).all()             # itself, or an earlier duplicate
    assert np.array_equal(xyz[0][first], xyz[0])


def test_knn_refusals_and_no_distance_matrix(dev):
    p = P()
    xyz = torch.zeros((1, 200, 3), device=dev)
    with pytest.raises(ValueError, match="k <= 128"):
        p.knn(129, xyz, xyz)
    with pytest.raises(ValueError, match="neighbours asked"):
        p.knn(5, xyz[:, :4].contiguous(), xyz)
    n = 4096
    pts = torch.from_numpy(grid_cloud(np.random.RandomState(0), 1, n)).to(dev)
    p.knn(16, pts, pts)                                 # warm: module load, LDS opt-in
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    idx = p.knn(16, pts, pts)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print("knn N = npoint = 4096, k = 16: peak grew by %d bytes" % grown)
    assert grown < n * n * 4 and idx.shape == (1, 16, n)


# ---------------------------------------------------------------- fps with dist
@pytest.mark.parametrize("n,ms", [(5, (1, 3, 5)), (64, (1, 3, 64)), (513, (1, 3, 513)),
                                  (1500, (1, 3, 1500))])
def test_fps_with_dist_equals_the_coordinate_form(dev, n, ms):
    from msmdfusion_amd import kernels as K
    rs = np.random.RandomState(n)
    xyz = torch.from_numpy(grid_cloud(rs, 2, n)).to(dev)
    d = xyz[:, :, None, :] - xyz[:, None, :, :]
    d = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]   # exact
    for m in ms:
        a = P().furthest_point_sample_with_dist(d.contiguous(), m)
        assert tuple(a.shape) == (2, m) and a.dtype == torch.int32
        assert torch.equal(a, K.furthest_point_sample(xyz, m)), (n, m)
    if n <= 513:
        assert np.array_equal(a.cpu().numpy(), R.fps_with_dist(d.cpu().numpy(), ms[-1]))


def test_fps_with_dist_streams_past_the_register_form(dev):
    """n > 16 * 1024 running minima do not fit the registers: the streaming kernel."""
    n = 16 * 1024 + 3
    gen = torch.Generator(device=dev).manual_seed(0)
    d = torch.rand((1, n, n), generator=gen, device=dev)
    idx = P().furthest_point_sample_with_dist(d, 6).cpu().numpy()[0]
    temp, old = np.full(n, 1e10, np.float32), 0
    assert idx[0] == 0
    for j in range(1, 6):
        temp = np.minimum(d[0, old].cpu().numpy(), temp)
        assert temp[idx[j]] == temp.max()              # random floats: no ties to order
        old = idx[j]


# ---------------------------------------------------------------- backward
def _ball_shaped(rs, b, n, npoint, nsample):
    """Ball-query-shaped groups: a few hits, then the first hit repeated."""
    idx = np.zeros((b, npoint, nsample), np.int32)
    for bb in range(b):
        for p_ in range(npoint):
            hits = np.sort(rs.choice(n, size=rs.randint(1, min(nsample, n) + 1), replace=False))
            idx[bb, p_] = hits[0]
            idx[bb, p_, :hits.size] = hits
    return idx


def _bwd_cases():
    rs = np.random.RandomState(11)
    yield "random", 3, 16, 300, rs.randint(0, 300, size=(3, 64, 8)).astype(np.int32)
    yield "all-zero", 3, 16, 50, np.zeros((3, 256, 32), np.int32)
    yield "ball-query", 3, 129, 200, _ball_shaped(rs, 3, 200, 96, 16)
    idx = rs.randint(0, 257, size=(3, 33, 5)).astype(np.int32)
    idx[idx == 100] = 99
    yield "unreferenced", 3, 1, 257, idx
    yield "random-129", 3, 129, 65, rs.randint(0, 65, size=(3, 17, 32)).astype(np.int32)


def _check_against_float64(got, grad, idx, n, weight, div, what):
    """|ours - float64| <= MARGIN * |torch float32 index_add_ - float64| + 1 ulp of the largest
    entry, as max-abs errors over the tensor."""
    b, c = grad.shape[:2]
    flat = idx.reshape(b, -1).long()
    gsrc = grad.reshape(b, c, -1)
    if div > 1:
        gsrc = gsrc.repeat_interleave(div, dim=2)
    if weight is not None:
        gsrc32 = gsrc * weight.reshape(b, 1, -1)
        gsrc64 = gsrc.double() * weight.reshape(b, 1, -1).double()
    else:
        gsrc32, gsrc64 = gsrc, gsrc.double()
    ref64 = torch.zeros((b, c, n), dtype=torch.float64, device=grad.device)
    ref32 = torch.zeros((b, c, n), dtype=torch.float32, device=grad.device)
    for bb in range(b):
        ref64[bb].index_add_(1, flat[bb], gsrc64[bb])
        ref32[bb].index_add_(1, flat[bb], gsrc32[bb])
    err = float((got.double() - ref64).abs().max())
    err_torch = float((ref32.double() - ref64).abs().max())
    ulp = float(np.spacing(np.float32(ref64.abs().max().item())))
    print("%s: err %.3e, torch float32 err %.3e, ulp %.3e" % (what, err, err_torch, ulp))
    assert err <= MARGIN * err_torch + ulp


@pytest.mark.parametrize("case", list(_bwd_cases()), ids=lambda c: c[0])
def test_group_and_gather_backward_are_bitwise_the_fixed_order_sum(dev, case):
    name, b, c, n, idx = case
    p = P()
    gen = torch.Generator().manual_seed(5)
    feat = torch.randn((b, c, n), generator=gen).to(dev).requires_grad_()
    go = torch.randn((b, c) + idx.shape[1:], generator=gen).to(dev)
    tidx = torch.from_numpy(idx).to(dev)
    p.grouping_operation(feat, tidx).backward(go)
    want = R.scatter_bwd(go.cpu().numpy(), idx, n)
    assert np.array_equal(feat.grad.cpu().numpy().view(np.int32), want.view(np.int32))
    _check_against_float64(feat.grad, go, tidx, n, None, 1, "group " + name)
    if name == "unreferenced":
        assert (feat.grad[:, :, 100] == 0).all() and (idx != 100).all()
    # gather_points: the same index, flattened to (B, M)
    feat2 = feat.detach().clone().requires_grad_()
    flat = tidx.view(b, -1)
    p.gather_points(feat2, flat).backward(go.view(b, c, -1))
    assert torch.equal(feat2.grad, feat.grad)


@pytest.mark.parametrize("c,m,n", [(1, 40, 300), (16, 3, 513), (129, 200, 64)])
def test_three_interpolate_backward_is_bitwise_the_fixed_order_sum(dev, c, m, n):
    rs = np.random.RandomState(c + m)
    b = 3
    idx = rs.randint(0, m, size=(b, n, 3)).astype(np.int32)
    idx[:, : n // 2] = 0                                  # a hot source
    if m > 5:
        idx[idx == 5] = 4                                 # ... and one nobody references
    w = rs.rand(b, n, 3).astype(np.float32)
    feat = torch.from_numpy(rs.randn(b, c, m).astype(np.float32)).to(dev).requires_grad_()
    tw = torch.from_numpy(w).to(dev).requires_grad_()
    go = torch.from_numpy(rs.randn(b, c, n).astype(np.float32)).to(dev)
    tidx = torch.from_numpy(idx).to(dev)
    P().three_interpolate(feat, tidx, tw).backward(go)
    assert tw.grad is None                                # as the reference: no weight gradient
    want = R.scatter_bwd(go.cpu().numpy(), idx, m, w, div=3)
    assert np.array_equal(feat.grad.cpu().numpy().view(np.int32), want.view(np.int32))
    if m > 5:
        assert (feat.grad[:, :, 5] == 0).all()
    _check_against_float64(feat.grad, go, tidx, m, tw.detach(), 3, "three_interpolate C%d" % c)


def test_backward_with_every_destination_on_one_source(dev):
    """npoint * nsample = 8192 destinations, all index 0."""
    b, c, n = 3, 16, 10
    idx = torch.zeros((b, 256, 32), dtype=torch.int32, device=dev)
    gen = torch.Generator().manual_seed(9)
    feat = torch.randn((b, c, n), generator=gen).to(dev).requires_grad_()
    go = torch.randn((b, c, 256, 32), generator=gen).to(dev)
    P().grouping_operation(feat, idx).backward(go)
    want = R.scatter_bwd(go.cpu().numpy(), idx.cpu().numpy(), n)
    assert np.array_equal(feat.grad.cpu().numpy().view(np.int32), want.view(np.int32))
    assert (feat.grad[:, :, 1:] == 0).all()
    _check_against_float64(feat.grad, go, idx, n, None, 1, "all-on-one")


def test_the_inverse_is_built_lazily_and_once(dev, monkeypatch):
    from msmdfusion_amd import kernels as K
    calls = []
    real = K.point_inverse_index
    monkeypatch.setattr(K, "point_inverse_index", lambda *a: calls.append(1) or real(*a))
    feat = torch.randn((2, 4, 30), device=dev, requires_grad=True)
    idx = torch.randint(0, 30, (2, 8, 4), dtype=torch.int32, device=dev)
    with torch.no_grad():
        P().grouping_operation(feat, idx)
    out = P().grouping_operation(feat, idx)
    assert calls == []                                    # forward pays nothing
    out.sum().backward(retain_graph=True)
    out.sum().backward()
    assert calls == [1]


# ---------------------------------------------------------------- QueryAndGroup
def _group_ref(feat, idx):
    b, c, _ = feat.shape
    return torch.gather(feat, 2, idx.long().view(b, 1, -1).expand(b, c, -1)).view(
        b, c, idx.shape[1], idx.shape[2])


# (use_xyz=False without features is no configuration: the reference asserts)
@pytest.mark.parametrize("use_xyz,with_features", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("normalize_xyz", [True, False])
@pytest.mark.parametrize("min_radius", [0, 0.5])
def test_query_and_group_equals_the_torch_restatement(dev, use_xyz, normalize_xyz, min_radius,
                                                      with_features):
    p = P()
    rs = np.random.RandomState(2)
    xyz = torch.from_numpy(grid_cloud(rs, 2, 500)).to(dev)
    centres = xyz[:, :40].contiguous()
    feat = torch.randn((2, 7, 500), device=dev) if with_features else None
    mod = p.QueryAndGroup(1.25, 9, min_radius=min_radius, use_xyz=use_xyz,
                          normalize_xyz=normalize_xyz, return_grouped_xyz=True)
    out, gxyz = mod(xyz, centres, feat)
    idx = p.ball_query(min_radius, 1.25, 9, xyz, centres)
    e_xyz = _group_ref(xyz.transpose(1, 2).contiguous(), idx)
    e_xyz = e_xyz - centres.transpose(1, 2).unsqueeze(-1)
    if normalize_xyz:
        e_xyz = e_xyz / 1.25
    assert torch.equal(gxyz, e_xyz)
    if with_features:
        e_feat = _group_ref(feat, idx)
        want = torch.cat([e_xyz, e_feat], dim=1) if use_xyz else e_feat
    else:
        want = e_xyz
    assert torch.equal(out, want)
    assert tuple(out.shape) == (2, (3 if use_xyz else 0) + (7 if with_features else 0), 40, 9)


def test_group_all(dev):
    p = P()
    xyz, feat = torch.randn((2, 30, 3), device=dev), torch.randn((2, 4, 30), device=dev)
    out = p.GroupAll()(xyz, None, feat)
    assert tuple(out.shape) == (2, 7, 1, 30) and torch.equal(out[:, :3, 0], xyz.transpose(1, 2))
    assert torch.equal(p.GroupAll(use_xyz=False)(xyz, None, feat), feat.unsqueeze(2))
    assert tuple(p.GroupAll()(xyz, None).shape) == (2, 3, 1, 30)


def test_points_sampler_modes(dev):
    p = P()
    rs = np.random.RandomState(4)
    xyz = torch.from_numpy(grid_cloud(rs, 2, 300)).to(dev)
    feat = torch.randn((2, 5, 300), device=dev)
    d = p.Points_Sampler([16], ["D-FPS"], [-1])(xyz, feat)
    assert torch.equal(d, p.furthest_point_sample(xyz, 16))
    f = p.Points_Sampler([16], ["F-FPS"], [-1])(xyz, feat)
    ff = torch.cat([xyz, feat.transpose(1, 2)], dim=2)
    assert torch.equal(f, p.furthest_point_sample_with_dist(
        p.calc_square_dist(ff, ff, norm=False), 16))
    fs = p.Points_Sampler([16], ["FS"], [-1])(xyz, feat)
    assert torch.equal(fs, torch.cat([f, d], dim=1))
    mix = p.Points_Sampler([8, 8], ["F-FPS", "D-FPS"], [100, -1])(xyz, feat)
    assert tuple(mix.shape) == (2, 16) and int(mix[:, :8].max()) < 100
    assert int(mix[:, 8:].min()) >= 100
    assert torch.equal(mix[:, 8:], p.furthest_point_sample(xyz[:, 100:].contiguous(), 8) + 100)


# ---------------------------------------------------------------- reproducibility
def test_forward_and_backward_are_bitwise_reproducible(dev):
    """B 4, N 16384, npoint 4096, nsample 32, C 64: QueryAndGroup, then three_interpolate back
    onto the cloud; two runs, forward and backward, bit for bit."""
    p = P()
    rs = np.random.RandomState(8)
    xyz = torch.from_numpy(grid_cloud(rs, 4, 16384)).to(dev)
    centres = xyz[:, :4096].contiguous()
    gen = torch.Generator().manual_seed(1)
    feat0 = torch.randn((4, 64, 16384), generator=gen).to(dev)
    go = torch.randn((4, 67, 16384), generator=gen).to(dev)
    grouper = p.QueryAndGroup(0.6, 32)

    def run():
        feat = feat0.clone().requires_grad_()
        grouped = grouper(xyz, centres, feat)                       # (4, 67, 4096, 32)
        pooled = grouped.max(dim=-1)[0]
        dist, idx = p.three_nn(xyz, centres)
        recip = 1.0 / (dist + 1e-8)
        weight = recip / recip.sum(dim=2, keepdim=True)
        out = p.three_interpolate(pooled.contiguous(), idx, weight)
        out.backward(go)
        return grouped.detach(), out.detach(), feat.grad

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert float(a[2].abs().max()) > 0


# ---------------------------------------------------------------- shims
def test_extension_shims(dev):
    from msmdfusion_amd.integration import (furthest_point_sample_ext, gather_points_ext,
                                            group_points_ext, interpolate_ext, knn_ext)
    p = P()
    rs = np.random.RandomState(6)
    b, c, n, npoint, ns = 2, 5, 60, 9, 4
    feat = torch.randn((b, c, n), device=dev)
    idx = torch.randint(0, n, (b, npoint, ns), dtype=torch.int32, device=dev)
    out = torch.zeros((b, c, npoint, ns), device=dev)
    assert group_points_ext.forward(b, c, n, npoint, ns, feat, idx, out) == 1
    assert torch.equal(out, p.grouping_operation(feat, idx))
    go = torch.randn_like(out)
    grad = torch.zeros((b, c, n), device=dev)
    group_points_ext.backward(b, c, n, npoint, ns, go, idx, grad)
    want = torch.from_numpy(R.scatter_bwd(go.cpu().numpy(), idx.cpu().numpy(), n)).to(dev)
    assert torch.equal(grad, want)
    group_points_ext.backward(b, c, n, npoint, ns, go, idx, grad)     # adds to what it is given
    assert torch.equal(grad, want + want)
    idx1 = idx[:, :, 0].contiguous()
    out1 = torch.zeros((b, c, npoint), device=dev)
    gather_points_ext.gather_points_wrapper(b, c, n, npoint, feat, idx1, out1)
    assert torch.equal(out1, p.gather_points(feat, idx1))
    grad1 = torch.ones((b, c, n), device=dev)
    gather_points_ext.gather_points_grad_wrapper(b, c, n, npoint, out1, idx1, grad1)
    assert torch.equal(grad1, 1 + torch.from_numpy(
        R.scatter_bwd(out1.cpu().numpy(), idx1.cpu().numpy(), n)).to(dev))
    # interpolate
    unknown = torch.from_numpy(grid_cloud(rs, b, 33)).to(dev)
    known = torch.from_numpy(grid_cloud(rs, b, n)).to(dev)
    dist2 = torch.zeros((b, 33, 3), device=dev)
    i3 = torch.zeros((b, 33, 3), dtype=torch.int32, device=dev)
    interpolate_ext.three_nn_wrapper(b, 33, n, unknown, known, dist2, i3)
    e_d2, e_i = R.three_nn(unknown.cpu().numpy(), known.cpu().numpy())
    assert np.array_equal(i3.cpu().numpy(), e_i) and np.array_equal(dist2.cpu().numpy(), e_d2)
    w = torch.rand((b, 33, 3), device=dev)
    o3 = torch.zeros((b, c, 33), device=dev)
    interpolate_ext.three_interpolate_wrapper(b, c, n, 33, feat, i3, w, o3)
    assert torch.equal(o3, p.three_interpolate(feat, i3, w))
    g3 = torch.zeros((b, c, n), device=dev)
    interpolate_ext.three_interpolate_grad_wrapper(b, c, 33, n, o3, i3, w, g3)
    assert np.array_equal(g3.cpu().numpy(), R.scatter_bwd(o3.cpu().numpy(), i3.cpu().numpy(), n,
                                                          w.cpu().numpy(), div=3))
    # knn: one batch element, coordinate-major, 1-based int64
    ind = torch.zeros((5, 33), dtype=torch.int64, device=dev)
    knn_ext.knn_wrapper(known[0].t().contiguous(), n, unknown[0].t().contiguous(), 33, ind, 5)
    assert torch.equal(ind - 1, p.knn(5, known[:1], unknown[:1])[0]) and int(ind.min()) >= 1
    # fps
    d = p.calc_square_dist(known, known, norm=False).contiguous()
    temp = torch.full((b, n), 1e10, device=dev)
    fidx = torch.zeros((b, 7), dtype=torch.int32, device=dev)
    furthest_point_sample_ext.furthest_point_sampling_with_dist_wrapper(b, n, 7, d, temp, fidx)
    assert torch.equal(fidx, p.furthest_point_sample_with_dist(d, 7))
    furthest_point_sample_ext.furthest_point_sampling_wrapper(b, n, 7, known, temp, fidx)
    assert torch.equal(fidx, p.furthest_point_sample(known, 7))
    with pytest.raises(RuntimeError, match="contiguous"):
        gather_points_ext.gather_points_wrapper(b, c, n, npoint, feat.transpose(1, 2), idx1, out1)


# ---------------------------------------------------------------- no host synchronisation
def test_the_ops_do_not_wait_for_the_device(dev):
    """Forward + backward return while the stream still holds work queued before them."""
    p = P()
    rs = np.random.RandomState(1)
    xyz = torch.from_numpy(grid_cloud(rs, 2, 2048)).to(dev)
    centres = xyz[:, :256].contiguous()
    feat = torch.randn((2, 16, 2048), device=dev, requires_grad=True)
    grouper = p.QueryAndGroup(0.8, 16)

    def work():
        pooled = grouper(xyz, centres, feat).max(dim=-1)[0]
        dist, idx = p.three_nn(xyz, centres)
        out = p.three_interpolate(pooled.contiguous(), idx, torch.softmax(-dist, dim=2))
        sel = p.gather_points(out, p.furthest_point_sample(xyz, 64))
        sel.sum().backward()
        p.knn(8, xyz, centres)
        p.furthest_point_sample_with_dist(p.calc_square_dist(centres, centres, False), 32)

    big = torch.randn((8192, 8192), device=dev)
    work()                                              # warm: allocations, module load
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    for _ in range(8):
        big = big @ big * 1e-4                          # tens of milliseconds of queued work
    work()
    assert not stream.query(), "an op synchronised with the device"
    torch.cuda.synchronize()
