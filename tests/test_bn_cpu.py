"""The float64 BatchNorm restatement (bn_ref.py) against nn.BatchNorm1d in double with
autograd, the n = 1 rule by hand, the C-ABI refusals of the msmd_bn_* entry points (all return
before any launch: no GPU needed), the statistics arithmetic old and new as numbers, and the
ReLU cases of test_gpu_bn.py: their inputs leave (almost) nothing inside the mask band."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import bn_ref as R


# ------------------------------------------------------------------ restatement == torch double
@pytest.mark.parametrize("n", [2, 129])
@pytest.mark.parametrize("mode", ["train", "eval", "frozen"])
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (False, True), (True, True)])
def test_restatement_equals_torch_double(n, mode, relu, res):
    c, eps, mom = 12, 1e-3, 0.1
    case = R.plain_case(n, c, seed=n + 7, residual=res)
    bn = nn.BatchNorm1d(c, eps=eps, momentum=mom).double()
    with torch.no_grad():
        bn.weight.copy_(case["gamma"]); bn.bias.copy_(case["beta"])
        bn.running_mean.copy_(case["running_mean"]); bn.running_var.copy_(case["running_var"])
    bn.train(mode != "eval")
    if mode == "frozen":
        bn.track_running_stats = False
        bn.running_mean = bn.running_var = None      # (what _BatchNorm.forward then passes on)
    x = case["x"].double().requires_grad_(True)
    r = case["residual"].double().requires_grad_(True) if res else None
    t = bn(x) if r is None else bn(x) + r
    y = torch.relu(t) if relu else t
    y.backward(case["dy"].double())

    training = mode != "eval"
    fwd = R.forward(case["x"], case["gamma"], case["beta"],
                    None if mode == "frozen" else case["running_mean"],
                    None if mode == "frozen" else case["running_var"], training, mom, eps, relu,
                    case["residual"])
    bwd = R.backward(case["x"], case["dy"], case["gamma"], fwd["save_mean"], fwd["save_invstd"],
                     training, (fwd["t"] > 0) if relu else None)
    close = dict(rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(fwd["y"], y.detach(), **close)
    torch.testing.assert_close(bwd["dx"], x.grad, **close)
    torch.testing.assert_close(bwd["dgamma"], bn.weight.grad, **close)
    torch.testing.assert_close(bwd["dbeta"], bn.bias.grad, **close)
    if res:
        torch.testing.assert_close(bwd["dresidual"], r.grad, **close)
    if mode == "frozen":
        assert fwd["running_mean"] is None and fwd["running_var"] is None
    else:
        torch.testing.assert_close(fwd["running_mean"], bn.running_mean, **close)
        torch.testing.assert_close(fwd["running_var"], bn.running_var, **close)
    if training:
        torch.testing.assert_close(fwd["save_mean"], case["x"].double().mean(0), **close)
        torch.testing.assert_close(
            fwd["save_invstd"], 1 / torch.sqrt(case["x"].double().var(0, unbiased=False) + eps),
            **close)


def test_one_row_by_hand():
    """n = 1: mean = the row, variance 0, y = beta; running_var takes the BIASED variance (0),
    the kernel's stated rule where torch refuses the call; dx = 0, dgamma = 0, dbeta = dy."""
    x = torch.tensor([[3.0, -2.0]])
    gamma, beta = torch.tensor([2.0, 0.5]), torch.tensor([0.25, -1.0])
    rm, rv = torch.tensor([1.0, 1.0]), torch.tensor([4.0, 8.0])
    f = R.forward(x, gamma, beta, rm, rv, True, 0.25, 1e-3)
    assert torch.equal(f["save_mean"], x[0].double())
    assert torch.equal(f["save_invstd"], torch.full((2,), 1e-3, dtype=torch.float64).rsqrt())
    assert torch.equal(f["y"], beta.double()[None])
    assert torch.equal(f["running_mean"], torch.tensor([1.5, 0.25], dtype=torch.float64))
    assert torch.equal(f["running_var"], torch.tensor([3.0, 6.0], dtype=torch.float64))
    b = R.backward(x, torch.tensor([[1.0, -3.0]]), gamma, f["save_mean"], f["save_invstd"], True)
    assert torch.equal(b["dx"], torch.zeros(1, 2, dtype=torch.float64))
    assert torch.equal(b["dgamma"], torch.zeros(2, dtype=torch.float64))
    assert torch.equal(b["dbeta"], torch.tensor([1.0, -3.0], dtype=torch.float64))


# ------------------------------------------------------------------ C-ABI refusals
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -3
P = ctypes.c_void_p(4096)            # a non-null, 256-aligned address nothing dereferences


def _fwd(lib, n=10, c=8, x=P, gamma=P, beta=P, rm=P, rv=P, training=1, y=P, sm=P, si=P, ws=P,
         ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.msmd_bn_workspace_bytes(max(n, 0), max(c, 0))
    return lib.msmd_bn_act_fwd_f32(x, None, n, c, gamma, beta, rm, rv, training, 0.1, 1e-3, 1, y,
                                   sm, si, ws, ws_bytes, None)


def _part(lib, n=300, c=8, gamma=P, sm=P, part=P, n_partials=3, rows=128):
    return lib.msmd_bn_act_fwd_from_partials_f32(P, None, n, c, gamma, P, P, P, 0.1, 1e-3, 1, P,
                                                 sm, P, part, n_partials, rows, None)


def _bwd(lib, n=10, c=8, y=P, gamma=P, sm=P, relu=1, dgamma=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.msmd_bn_workspace_bytes(max(n, 0), max(c, 0))
    return lib.msmd_bn_act_bwd_f32(P, y, P, n, c, gamma, sm, P, 1, 1e-3, relu, P, None, dgamma, P, ws,
                                   ws_bytes, None)


def _rbwd(lib, n=10, c=8, gamma=P, beta=P, sm=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.msmd_bn_workspace_bytes(max(n, 0), max(c, 0))
    return lib.msmd_bn_relu_bwd_f32(P, P, n, c, gamma, beta, sm, P, 1, 1e-3, P, P, P, ws, ws_bytes,
                                    None)


def test_entry_points_refuse_before_any_launch():
    from msmdfusion_amd._lib import lib
    # channel counts without a kernel: the forwards say UNSUPPORTED for a positive c they do
    # not serve (c % 4 != 0, c > 1024) and INVALID for c = 0; the backwards INVALID throughout
    for call, codes in ((_fwd, (INVALID, UNSUPPORTED, UNSUPPORTED)),
                        (_part, (INVALID, UNSUPPORTED, UNSUPPORTED)),
                        (_bwd, (INVALID,) * 3), (_rbwd, (INVALID,) * 3)):
        for c, code in zip((0, 6, 1028), codes):
            assert call(lib, c=c) == code, (call.__name__, c)
        assert call(lib, n=-1) == INVALID, call.__name__
        assert call(lib, gamma=None) == INVALID, call.__name__
        assert call(lib, sm=None) == INVALID, call.__name__
    assert _rbwd(lib, beta=None) == INVALID
    assert _bwd(lib, dgamma=None) == INVALID
    # eval needs the running buffers; training does not (track_running_stats = False)
    assert _fwd(lib, training=0, rm=None) == INVALID
    assert _fwd(lib, training=0, rv=None) == INVALID
    # the masked backward needs y for its mask only with relu
    assert _bwd(lib, relu=1, y=None) == INVALID
    # partials: none, or not one per block of rows_per_partial rows
    assert _part(lib, n_partials=0) == INVALID
    assert _part(lib, part=None) == INVALID
    assert _part(lib, n_partials=2) == INVALID and _part(lib, rows=0) == INVALID
    # workspace: one byte short of what the call uses, or not 256-aligned.  c = 64, n = 129:
    # (two row blocks of [4][64] + [4][64]) fp64 sums = 6144 bytes, a multiple of the 256-byte
    # rounding
    need = lib.msmd_bn_workspace_bytes(129, 64)
    assert need == (2 * 4 + 4) * 64 * 8
    for call in (_fwd, _bwd, _rbwd):
        assert call(lib, n=129, c=64, ws_bytes=need - 1) == WORKSPACE, call.__name__
        assert call(lib, n=129, c=64, ws=ctypes.c_void_p(4096 + 128)) == WORKSPACE, call.__name__
        assert call(lib, n=129, c=64, ws=None, ws_bytes=0) == WORKSPACE, call.__name__
    # nothing to do is not an error
    assert _fwd(lib, n=0) == OK and _part(lib, n=0, n_partials=0) == OK


def test_workspace_bytes():
    from msmdfusion_amd._lib import lib
    for n, c in ((0, 4), (1, 4), (128, 4), (129, 8), (3000, 80), (33405, 1024)):
        got = lib.msmd_bn_workspace_bytes(n, c)
        blocks = max((n + 127) // 128, 1)
        assert got % 256 == 0 and 0 <= got - (blocks * 4 + 4) * c * 8 < 256, (n, c)


# ------------------------------------------------------------------ the statistics arithmetic
def _channel(ratio, n=3000, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.randn(n) + ratio).astype(np.float32)


def test_raw_sums_cancel_and_pivoted_sums_do_not():
    """Relative error of the biased variance against float64, n = 3000, unit-variance channel,
    mean / std = 0, 10, 100, 1000.  Measured here (numpy, the kernels' arithmetic restated):

        ratio   raw sum / sum of squares   pivoted sums (float32)   torch float32 (CPU)
        0       2.4e-08                    4.3e-08                  6.5e-09
        10      1.1e-05                    1.9e-07                  6.8e-09
        100     1.2e-04                    5.0e-08                  1.1e-08
        1000    2.1e-02                    2.2e-08                  1.5e-08

    The raw form is what csrc/bn.hip and the conv epilogue carried before; it fails the GPU
    file's criterion (4 x torch) from ratio 10 upward.  A constant channel at 1000.1 gave it a
    'variance' far from 0 before the clamp; the pivoted form gives 0 exactly."""
    for ratio in (0., 10., 100., 1000.):
        x = _channel(ratio)
        v64 = float(np.var(x.astype(np.float64)))
        v32 = float(torch.var(torch.from_numpy(x), unbiased=False))
        raw = abs(R.raw_sum_variance(x)[1] - v64) / v64
        piv = abs(R.pivot_variance(x)[1] - v64) / v64
        t32 = abs(v32 - v64) / v64
        print("ratio %6g: raw %.2g  pivoted %.2g  torch32 %.2g" % (ratio, raw, piv, t32))
        if ratio >= 10:     # the GPU file's criterion on the variance: the raw form misses it
            assert raw > 4 * t32 + 4 * R.EPS32, (ratio, raw, t32)
        # float32 rounding of 128 terms of the order of the spread, whatever the offset
        assert piv <= 128 * R.EPS32, (ratio, piv)
        m64 = float(np.mean(x.astype(np.float64)))
        assert abs(R.pivot_variance(x)[0] - m64) <= R.EPS32 * max(abs(m64), 1.0)
    for v in R.CONST_CHANNELS:
        x = np.full(3000, v, np.float32)
        assert R.pivot_variance(x) == (float(np.float32(v)), 0.0)
    assert abs(R.raw_sum_variance(np.full(3000, 1000.1, np.float32))[1]) > 0.1


# ------------------------------------------------------------------ the GPU file's ReLU inputs
def _band_share(case, training, eps=1e-3, mom=0.1):
    """Share of a ReLU case inside the mask band, with torch's float32 result taken on the CPU
    in place of the GPU's (the band is ~1e-6 wide either way)."""
    f = R.forward(case["x"], case["gamma"], case["beta"], case["running_mean"],
                  case["running_var"], training, mom, eps, True, case["residual"])
    if training and case["x"].shape[0] == 1:
        y32 = None
    else:
        y32 = torch.nn.functional.batch_norm(case["x"], case["running_mean"].clone(),
                                             case["running_var"].clone(), case["gamma"],
                                             case["beta"], training, mom, eps)
        if case["residual"] is not None:
            y32 = y32 + case["residual"]
        y32 = torch.relu(y32)
    t = f["t"]
    inside = (t.abs() <= R.bound(y32, f["y"])) & (t != 0)
    return float(inside.double().mean())


def test_relu_cases_leave_the_band_nearly_empty():
    """The seeds of test_gpu_bn.py's ReLU cases: the float64 reference alone leaves fewer than
    0.1 % of each case inside the band (exact zeros of t64 -- gamma = beta = 0 -- are not in
    it: the mask must be false there)."""
    cases = [R.plain_case(33405, 128, seed=77, residual=True)]
    for n in (129, 3000):
        cases += [R.mask_case(n), R.mask_case(n, residual=True)]
    cases.append(R.plain_case(257, 20, seed=21, residual=True))
    for n in (1, 2, 127, 128, 129, 257):
        for c in (4, 12, 20, 64, 260, 516, 1020, 1024):
            cases.append(R.plain_case(n, c, seed=n * 10007 + c))
    for case in cases:
        for training in (True, False):
            assert _band_share(case, training) < 1e-3, (case["x"].shape, training)
    z = R.mask_case(129)
    t = R.forward(z["x"], z["gamma"], z["beta"], None, None, True, 0.1, 1e-3, True)["t"]
    assert (t[:, 3] == 0).all() and (t[:, 4] == 0.25).all()
