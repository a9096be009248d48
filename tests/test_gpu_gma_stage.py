"""kernels.gma_stage -- both gate linears inside the stage assembly -- against the chain it
replaces on the same device: K.rows_linear for the two gates, then K.gma_assemble with the
sorted row lists.  The fused call keeps that chain's arithmetic and summation order, so every
comparison is torch.equal."""
import pytest
import torch

C2 = 64


def _case(dev, c3, n3=300, n_o3=150, n_o2=500, n_mix=70, p2=1, pm=1, nn_mode="holes", seed=0):
    g = torch.Generator(device=dev).manual_seed(1000 * c3 + n3 + n_o2 + n_mix + seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    ri = lambda hi, n: torch.randint(0, hi, (n,), device=dev, generator=g)
    n2 = 900
    if nn_mode == "holes":      # no target in rows 128..255, one target with 40 rows
        assert n3 == 300
        lo = torch.cat([torch.arange(0, 128, device=dev), torch.arange(256, 300, device=dev)])
        nn3 = lo[ri(lo.shape[0], n_o2)]
        nn3[1:121:3] = 290      # 40 rows (none of them among the -1 entries below)
        nn3[::3] = -1
        assert int((nn3 == 290).sum()) >= 40 and not ((nn3 >= 128) & (nn3 < 256)).any()
    elif nn_mode == "none":
        nn3 = torch.full((n_o2,), -1, dtype=torch.int64, device=dev)
    else:
        nn3 = ri(n3, n_o2)
        nn3[::3] = -1
    return dict(
        c3=c3, n3=n3, p2=p2, pm=pm, nn3=nn3, feat3=r(n3, c3), feat2=r(n2, C2), dummy=r(1, c3),
        conv3=r(n_o3, c3), rows_o2=ri(n2, n_o2), rows_m3=ri(n3, n_mix), rows_m2=ri(n2, n_mix),
        w_c=r(C2, c3) * 0.3, b_c=r(C2) * 0.1, w_g=r(C2, c3) * 0.3, b_g=r(C2) * 0.1,
        w=r(n_o3 + n_o2 + p2 + n_mix + pm, c3 + C2))


def _leaves(c):
    return [c[k].detach().clone().requires_grad_() for k in ("conv3", "w_c", "b_c", "w_g", "b_g")]


def _chain(c):
    """the parent's chain: two gate tables, then the one-launch assembly"""
    from msmdfusion_amd import kernels as K
    conv3, w_c, b_c, w_g, b_g = lv = _leaves(c)
    cross = K.rows_linear(c["feat3"], w_c, b_c, relu=True, x_tail=c["dummy"])
    gate = K.rows_linear(c["feat3"].index_select(0, c["rows_m3"]), w_g, b_g, relu=True)
    out = K.gma_assemble(conv3, cross, gate, c["feat3"], c["feat2"], c["nn3"], c["rows_o2"],
                         c["rows_m3"], c["rows_m2"], c["p2"], c["pm"],
                         segments=K.gma_nn_segments(c["nn3"], c["n3"]))
    (out * c["w"]).sum().backward()
    return out.detach(), [t.grad for t in lv]


def _fused(c):
    from msmdfusion_amd import kernels as K
    conv3, w_c, b_c, w_g, b_g = lv = _leaves(c)
    out = K.gma_stage(conv3, w_c, b_c, w_g, b_g, c["feat3"], c["dummy"], c["feat2"], c["nn3"],
                      c["rows_o2"], c["rows_m3"], c["rows_m2"], c["p2"], c["pm"],
                      K.gma_nn_segments(c["nn3"], c["n3"]))
    (out * c["w"]).sum().backward()
    return out.detach(), [t.grad for t in lv]


def _same(c):
    want, gw = _chain(c)
    got, gg = _fused(c)
    assert got.shape == want.shape and torch.equal(got, want)
    for name, a, b in zip(("d_conv3", "dW_c", "db_c", "dW_g", "db_g"), gg, gw):
        assert a is not None and b is not None, name
        assert torch.equal(a, b), "%s: max |diff| %.3e" % (name, float((a - b).abs().max()))
    return gg


@pytest.mark.gpu
@pytest.mark.parametrize("c3", [16, 32, 64, 128])
def test_gma_stage_equals_the_chain(dev, c3):
    """n3 = 300: table blocks of 128, 128 and 44 rows + the dummy row; no target in the middle
    block (an unflagged block between two flagged ones), one target with 40 rows, every third
    row on the dummy embedding; pad rows behind both row groups."""
    _same(_case(dev, c3))


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [
    ("all_dummy", dict(nn_mode="none", n_o2=1500)),     # > kDummyBlocks * 16 rows, no flag set
    ("no_only2d", dict(nn_mode="rand", n_o2=0)),
    ("no_mixed", dict(n_mix=0)),
    ("no_only3d", dict(n_o3=0)),
    ("one_voxel", dict(nn_mode="rand", n3=1)),
    ("two_gate_blocks", dict(n_mix=129)),
])
def test_gma_stage_edges_equal_the_chain(dev, name, kw):
    _same(_case(dev, 32, **kw))


@pytest.mark.gpu
def test_gma_stage_is_deterministic(dev):
    c = _case(dev, 64, seed=3)
    a, b = _fused(c), _fused(c)
    assert torch.equal(a[0], b[0])
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.gpu
def test_gma_stage_gradients_match_fp64_autograd_of_the_op_chain(dev):
    """float64 autograd through the reference's op-by-op chain (Linear + ReLU tables,
    index_select, multiply, pad, cat); criterion of
    test_gma_stage_gradients_match_fp64_autograd: 5e-4 of each tensor's largest entry."""
    c = _case(dev, 32, seed=5)
    got, gg = _fused(c)
    d = lambda t: t.double()
    conv3, w_c, b_c, w_g, b_g = lv = [d(t).requires_grad_() for t in
                                     (c["conv3"], c["w_c"], c["b_c"], c["w_g"], c["b_g"])]
    f3, f2, c3 = d(c["feat3"]), d(c["feat2"]), c["c3"]
    cross = torch.relu(torch.cat([f3, d(c["dummy"])], 0) @ w_c.t() + b_c)
    nn = torch.where(c["nn3"] >= 0, c["nn3"], torch.full_like(c["nn3"], c["n3"]))
    o2 = cross.index_select(0, nn) * f2.index_select(0, c["rows_o2"])
    o2 = torch.cat([o2, o2.new_zeros((c["p2"], C2))], 0)
    m3 = f3.index_select(0, c["rows_m3"])
    mixed = torch.cat([m3, torch.relu(m3 @ w_g.t() + b_g) * f2.index_select(0, c["rows_m2"])], -1)
    mixed = torch.cat([mixed, mixed.new_zeros((c["pm"], c3 + C2))], 0)
    ref = torch.cat([torch.nn.functional.pad(conv3, (0, C2)),
                     torch.nn.functional.pad(o2, (c3, 0)), mixed], 0)
    (ref * d(c["w"])).sum().backward()
    err = float((got.double() - ref.detach()).abs().max())
    assert err <= 5e-4 * float(ref.detach().abs().max()), err
    for name, a, t in zip(("d_conv3", "dW_c", "db_c", "dW_g", "db_g"), gg, lv):
        scale = float(t.grad.abs().max())
        err = float((a.double() - t.grad).abs().max())
        print("%s: |err| %.3e of max %.3e" % (name, err, scale))
        assert err <= 5e-4 * max(scale, 1e-6), "%s: |err| %.3e of max %.3e" % (name, err, scale)


@pytest.mark.gpu
def test_model_with_fused_gates_equals_the_gate_tables(dev):
    """The LC path with the gates inside the stage assembly and with the rows_linear tables:
    the same BEV map and the same gradient of every parameter, bit for bit."""
    import proc_prefetch_helper as H
    model = H.build_model(dev)
    clouds, virt = H.make_batch(dev)
    mm = model.path.multimodal_middle_encoder
    assert mm.fused_assembly and mm.fused_gates
    res = {}
    try:
        for on in (True, False):
            mm.fused_gates = on
            model.zero_grad(set_to_none=True)
            out = model(clouds, virt, prepared=model.prepare(clouds, virt))
            out.square().mean().backward()
            res[on] = (out.detach().clone(), {n: p.grad.clone() for n, p in
                                              model.named_parameters() if p.grad is not None})
    finally:
        mm.fused_gates = True
    assert torch.equal(res[True][0], res[False][0])
    assert res[True][1].keys() == res[False][1].keys()
    assert any("cross_gate_control" in n for n in res[True][1])
    assert any("gate_control" in n and "cross" not in n for n in res[True][1])
    for n, g in res[True][1].items():
        assert torch.equal(g, res[False][1][n]), n
