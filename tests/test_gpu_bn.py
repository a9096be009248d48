"""csrc/bn.hip (BatchNorm1d + residual + ReLU, forward and backward) against the float64
restatement of bn_ref.py, at the shapes and values where the kernels take another path.

The criterion, for every quantity q in {y, save_mean, save_invstd, running_mean, running_var,
dx, dresidual, dgamma, dbeta}, per channel:

    max|q_kernel - q64| <= 4 * max|q_torch32 - q64| + 4 * eps32 * max|q64|

q_torch32 = torch's own float32 batch norm + add + relu with autograd on the GPU on the same
input, q64 = bn_ref.  No absolute tolerances in this file.

ReLU cases: the forward mask first (y_kernel > 0 must equal t64 > 0 wherever |t64| exceeds the
y bound; an exact zero of t64 must give a false mask; the rest -- the band -- is at most 0.1 %
of the case), then the backward against bn_ref GIVEN the kernel's own mask, so that dgamma /
dbeta do not hang on coin-flip elements while the arithmetic stays fully checked.  torch's
float32 error is measured the same way: against bn_ref given torch's own mask."""
import functools

import pytest
import torch
from torch import nn

import bn_ref as R

pytestmark = pytest.mark.gpu

FWD = ("y", "save_mean", "save_invstd", "running_mean", "running_var")
BWD = ("dx", "dresidual", "dgamma", "dbeta")
BAND_CAP = 1e-3


# ------------------------------------------------------------------ the three computations
def _dev(case, dev):
    return {k: (None if v is None else v.to(dev)) for k, v in case.items()}


def _torch32(case, dev, training, relu, eps, momentum):
    """torch's float32 result on the GPU -> dict of the nine quantities (None where torch has
    none).  n = 1 in training: torch refuses -> None."""
    c = _dev(case, dev)
    if training and c["x"].shape[0] == 1:
        return None
    x = c["x"].clone().requires_grad_(True)
    w, b = c["gamma"].clone().requires_grad_(True), c["beta"].clone().requires_grad_(True)
    res = None if c["residual"] is None else c["residual"].clone().requires_grad_(True)
    rm, rv = c["running_mean"].clone(), c["running_var"].clone()
    out, sm, si = torch.native_batch_norm(x, w, b, rm, rv, training, momentum, eps)
    if not training:
        sm, si = rm, 1.0 / torch.sqrt(rv + eps)
    t = out if res is None else out + res
    y = torch.relu(t) if relu else t
    y.backward(c["dy"])
    return dict(y=y.detach(), save_mean=sm.detach(), save_invstd=si.detach(), running_mean=rm,
                running_var=rv, dx=x.grad, dresidual=None if res is None else res.grad,
                dgamma=w.grad, dbeta=b.grad)


def _kernel(case, dev, training, relu, eps, momentum, recompute=False):
    """The raw K.* calls -> the nine quantities (the backward told the forward's eps, as bn_act
    tells it: it then takes the batch statistics again instead of working from the float32
    save_mean / save_invstd, whose rounding alone put dx at n = 2 and dgamma of some channels
    outside the criterion)."""
    from msmdfusion_amd import kernels as K
    c = _dev(case, dev)
    rm, rv = c["running_mean"].clone(), c["running_var"].clone()
    y, mean, invstd = K.bn_act_forward(c["x"], c["residual"], c["gamma"], c["beta"], rm, rv,
                                       training, momentum, eps, relu)
    if recompute:
        assert relu and c["residual"] is None
        dx, dg, db = K.bn_relu_backward(c["x"], c["dy"], c["gamma"], c["beta"], mean, invstd,
                                        training, eps)
        dres = None
    else:
        dx, dres, dg, db = K.bn_act_backward(c["x"], y, c["dy"], c["gamma"], mean, invstd,
                                             training, relu, c["residual"] is not None, eps)
    return dict(y=y, save_mean=mean, save_invstd=invstd, running_mean=rm, running_var=rv, dx=dx,
                dresidual=dres, dgamma=dg, dbeta=db)


def _module(case, dev, training, relu, eps, momentum, x=None, dy=None, stats=None, frozen=False):
    """bn_act on an nn.BatchNorm1d with autograd -> the quantities a module shows."""
    from msmdfusion_amd.spconv.functional import bn_act
    c = _dev(case, dev)
    cc = c["gamma"].numel()
    bn = nn.BatchNorm1d(cc, eps=eps, momentum=momentum).to(dev)
    with torch.no_grad():
        bn.weight.copy_(c["gamma"]); bn.bias.copy_(c["beta"])
        bn.running_mean.copy_(c["running_mean"]); bn.running_var.copy_(c["running_var"])
    bn.train(training)
    if frozen:
        bn.track_running_stats = False
    xa = (c["x"].clone() if x is None else x).requires_grad_(True)
    ra = None if c["residual"] is None else c["residual"].clone().requires_grad_(True)
    y = bn_act(xa, bn, relu=relu, residual=ra, stats=stats)
    y.backward(c["dy"] if dy is None else dy)
    return dict(y=y.detach(), running_mean=bn.running_mean.clone(),
                running_var=bn.running_var.clone(), dx=xa.grad,
                dresidual=None if ra is None else ra.grad, dgamma=bn.weight.grad,
                dbeta=bn.bias.grad)


def _ref(case, training, relu, eps, momentum, mask=None, fwd=None, frozen=False):
    """bn_ref -> the nine quantities; backward with `mask` (None with relu: its own)."""
    if fwd is None:
        fwd = R.forward(case["x"], case["gamma"], case["beta"],
                        None if frozen else case["running_mean"],
                        None if frozen else case["running_var"], training, momentum, eps, relu,
                        case["residual"])
        if frozen:
            fwd["running_mean"], fwd["running_var"] = case["running_mean"], case["running_var"]
    if relu and mask is None:
        mask = fwd["t"] > 0
    bwd = R.backward(case["x"], case["dy"], case["gamma"], fwd["save_mean"], fwd["save_invstd"],
                     training, mask if relu else None)
    if case["residual"] is None:
        bwd["dresidual"] = None
    out = dict(fwd)
    out.update(bwd)
    return out


def _compare(tag, got, t32, case, training, relu, eps, momentum, names=FWD + BWD, frozen=False):
    """The criterion on every named quantity; with relu the mask rule first."""
    ref = _ref(case, training, relu, eps, momentum, frozen=frozen)
    ref_k, ref_t = ref, ref
    if relu:
        yb = R.bound(None if t32 is None else t32["y"], ref["y"])
        t64 = ref["t"]
        mk = got["y"].cpu() > 0
        decided = (t64.abs() > yb) | (t64 == 0)
        share = float((~decided).double().mean())
        print("%s: band share %.3g" % (tag, share))
        assert torch.equal(mk[decided], (t64 > 0)[decided]), tag + ": ReLU mask outside the band"
        assert share <= BAND_CAP, (tag, share)
        ref_k = _ref(case, training, relu, eps, momentum, mask=mk, fwd=ref, frozen=frozen)
        if t32 is not None:
            ref_t = _ref(case, training, relu, eps, momentum, mask=t32["y"].cpu() > 0, fwd=ref,
                         frozen=frozen)
    bad = []
    for q in names:
        if q not in got:            # (bn_act does not show what the forward saved)
            continue
        if got[q] is None:
            assert ref_k[q] is None, (tag, q)
            continue
        ex, err, e32 = _excess(got[q], None if t32 is None else t32[q], ref_k[q], ref_t[q])
        print("%s %s: kernel error %.3g, torch float32 error %.3g, over the bound by %.3g"
              % (tag, q, err, e32, ex))
        if not ex <= 0:
            bad.append((q, "error %.3g" % err, "torch %.3g" % e32, "over by %.3g" % ex))
    assert not bad, (tag, bad)


def _excess(qk, q32, q64k, q64t):
    """-> (max over channels of kernel error - bound, and at that channel: the kernel's error,
    torch's error).  torch's error is taken against its own reference q64t (its own ReLU mask);
    q32 = None: the floor alone.  <= 0 passes; NaN fails."""
    err = R._chan_max(R._d(qk) - R._d(q64k))
    e32 = torch.zeros_like(err) if q32 is None else R._chan_max(R._d(q32) - R._d(q64t))
    ex = err - (4 * e32 + 4 * R.EPS32 * R._chan_max(q64k))
    if torch.isnan(ex).any():
        return float("inf"), float("nan"), float("nan")
    i = int(ex.reshape(-1).argmax())
    return float(ex.reshape(-1)[i]), float(err.reshape(-1)[i]), float(e32.reshape(-1)[i])


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("c", [4, 12, 20, 64, 260, 516, 1020, 1024])
@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 257])
def test_shapes_train_and_eval(dev, n, c):
    """One row block and two, a partial one, one row; one channel group (c = 4: a 256-term LDS
    reduction by one thread), idle threads in the statistics blocks (256 % (c/4) != 0: 12, 20,
    260 ..), one thread per channel group (c/4 in 129..256).  Raw calls with both backward
    entry points, and bn_act.  n = 1 in training is compared with bn_ref alone (its floor):
    the momentum is one that float32 holds exactly, or the kernel's float argument and the
    reference's double would be different inputs with nothing but the floor to cover it."""
    eps, mom = 1e-3, 0.125
    case = R.plain_case(n, c, seed=n * 10007 + c)
    for training in (True, False):
        tag = "n%d c%d %s" % (n, c, "train" if training else "eval")
        t32 = _torch32(case, dev, training, False, eps, mom)
        _compare(tag + " raw", _kernel(case, dev, training, False, eps, mom), t32, case, training,
                 False, eps, mom)
        _compare(tag + " bn_act", _module(case, dev, training, False, eps, mom), t32, case,
                 training, False, eps, mom)
        t32r = _torch32(case, dev, training, True, eps, mom)
        _compare(tag + " recompute", _kernel(case, dev, training, True, eps, mom, recompute=True),
                 t32r, case, training, True, eps, mom)


def test_one_row_running_var_takes_the_biased_variance(dev):
    """n = 1, training: running_var moves towards 0 (the kernel's stated rule; torch refuses)."""
    case = R.plain_case(1, 8, seed=5)
    got = _kernel(case, dev, True, False, 1e-3, 0.25)
    rv = case["running_var"].to(dev)
    assert torch.equal(got["running_var"], (torch.tensor(1.0, device=dev) - 0.25) * rv)
    assert torch.equal(got["save_mean"], case["x"][0].to(dev))
    assert torch.equal(got["y"][0], case["beta"].to(dev))


@pytest.mark.parametrize("n", [113 * 128 - 5, 128 * 128, 129 * 128, 261 * 128 - 3])
def test_block_counts_in_the_finalize_loop(dev, n):
    """combine_partials' 8-deep unrolled loop (from 113 row blocks): one trip for some lanes
    and none for others, exactly one, one plus a tail step, two plus a tail -- forward
    statistics and the backward's dgamma / dbeta."""
    eps, mom = 1e-3, 0.1
    case = R.plain_case(n, 8, seed=n)
    for training in (True, False):
        t32 = _torch32(case, dev, training, False, eps, mom)
        _compare("n%d %s" % (n, training), _kernel(case, dev, training, False, eps, mom), t32,
                 case, training, False, eps, mom)


# ------------------------------------------------------------------ grid stride
@functools.lru_cache(maxsize=None)
def _big():
    return R.plain_case(33405, 128, seed=77, residual=True)


def test_grid_stride_second_trip(dev):
    """n * c / 4 > 1 048 576: the apply kernels' grid-stride loops take a second trip
    (relu + residual, forward and backward)."""
    eps, mom = 1e-3, 0.1
    case = _big()
    assert case["x"].numel() // 4 > 4096 * 256
    t32 = _torch32(case, dev, True, True, eps, mom)
    _compare("grid stride", _kernel(case, dev, True, True, eps, mom), t32, case, True, True, eps,
             mom)


def test_reproducible(dev):
    """The same call twice: every output bit-equal (fixed summation order, no float atomics)."""
    case = _big()
    a = _kernel(case, dev, True, True, 1e-3, 0.1)
    b = _kernel(case, dev, True, True, 1e-3, 0.1)
    for q in FWD + BWD:
        assert torch.equal(a[q], b[q]), q


# ------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("eps", [1e-3, 1e-5])
@pytest.mark.parametrize("n", [3000, 129])
def test_channels_far_from_zero(dev, n, eps):
    """Channels 0, +-10, +-100, +-1000 standard deviations from zero in one tensor, and four
    constant channels: raw float32 sums of x and x*x cancel here (relative variance error
    1e-5 / 1e-4 / 2e-2 at ratio 10 / 100 / 1000: test_bn_cpu records it); the pivoted sums
    must be as good as torch.  A constant channel has batch variance 0 exactly."""
    mom = 0.1
    case = R.conditioning_case(n)
    t32 = _torch32(case, dev, True, False, eps, mom)
    got = _kernel(case, dev, True, False, eps, mom)
    _compare("cond n%d eps%g" % (n, eps), got, t32, case, True, False, eps, mom)
    _compare("cond bn_act n%d eps%g" % (n, eps), _module(case, dev, True, False, eps, mom), t32,
             case, True, False, eps, mom)
    rv = case["running_var"].to(dev)[12:]
    mom32 = torch.tensor(mom, dtype=torch.float32).double()      # (what the C call receives)
    zero_var = ((1.0 - mom32) * rv.double().cpu() + mom32 * 0.0).float()
    assert torch.equal(got["running_var"][12:].cpu(), zero_var)
    assert torch.equal(got["save_mean"][12:], case["x"][0, 12:].to(dev))
    e32 = torch.tensor(eps, dtype=torch.float32).double()
    assert torch.equal(got["save_invstd"][12:].cpu(),
                       (1.0 / torch.sqrt(e32)).float().expand(4))


@pytest.mark.parametrize("eps", [1e-3, 1e-5])
def test_eval_with_running_var_near_zero(dev, eps):
    """Eval mode, running_var in {0, 1e-12, 1e-6, 1} on the offset channels."""
    case = R.conditioning_case(129)
    case["running_var"] = torch.tensor([0.0, 1e-12, 1e-6, 1.0]).repeat(4)
    case["running_mean"] = case["x"].mean(0)
    t32 = _torch32(case, dev, False, False, eps, 0.1)
    _compare("eval rv~0", _kernel(case, dev, False, False, eps, 0.1), t32, case, False, False,
             eps, 0.1)
    _compare("eval rv~0 bn_act", _module(case, dev, False, False, eps, 0.1), t32, case, False,
             False, eps, 0.1)


@pytest.mark.parametrize("cout,spread,lo,hi", [(64, 1.0, 3., 30.), (64, 0.1, 30., 300.),
                                               (192, 1.0, 3., 30.), (192, 0.1, 30., 300.)])
def test_channels_far_from_zero_through_the_conv_epilogue(dev, cout, spread, lo, hi):
    """The same through msmd_spconv_fwd_split_stats: a SubM conv whose outputs sit about 10 /
    about 100 standard deviations from zero (features 1 + 0.01 randn, weights = a constant on
    the centre offset + noise) leaves the partials, bn_act(out, bn, stats=part) is compared
    with bn_ref on the conv's own output.  128-row tiles (cout = 64) and 256-row tiles
    (192), a partial last tile, stream-K and whole tiles."""
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd import synthetic as S
    cin, shape, eps, mom = 64, [11, 64, 64], 1e-3, 0.1
    idx = S.random_voxel_indices(2100, 2, shape, seed=cout)
    n = idx.shape[0]
    tr = K.split_tile_rows(cout)
    assert tr == (128 if cout == 64 else 256) and n % tr != 0
    nbr = K.rulebook_subm(torch.from_numpy(idx).to(dev), 2, shape, 3)
    plan = K.rulebook_plan(nbr, tile_rows=(tr,))
    g = torch.Generator().manual_seed(cout + int(10 * spread))
    f = (1 + 0.01 * torch.randn(n, cin, generator=g)).to(dev)
    w = spread * torch.randn(27, cin, cout, generator=g)
    w[13] += 1.0
    ws = K.pack_weight_split((w / cin).to(dev), 3)
    case = R.plain_case(n, cout, seed=cout)
    for pre in (plan["prefix"][tr], None):
        out, part = K.conv_forward_split(f, ws, plan["tiled"], n, cout, 3,
                                         row_order=plan["order"], tile_prefix=pre, bn_stats=True)
        assert part.shape == ((n + tr - 1) // tr, 3, cout)
        case["x"] = out.cpu()
        o64 = out.double()
        ratio = float((o64.mean(0).abs() / o64.std(0)).median())
        print("cout %d spread %g: median |mean| / std = %.1f" % (cout, spread, ratio))
        assert lo <= ratio <= hi, ratio
        t32 = _torch32(case, dev, True, False, eps, mom)
        got = _module(case, dev, True, False, eps, mom, x=out.clone(), stats=part)
        _compare("epilogue cout%d spread%g %s" % (cout, spread, "sk" if pre is not None else "tiles"),
                 got, t32, case, True, False, eps, mom)


# ------------------------------------------------------------------ ReLU mask paths
@pytest.mark.parametrize("n", [129, 3000])
def test_relu_mask_paths(dev, n):
    """gamma in {-1.5 .. 1.5} with exact zeros and negatives, beta = 0 on a gamma = 0 channel:
    the recompute backward (mask from x) and the masked backward with a residual (mask from y),
    training and eval."""
    eps, mom = 1e-3, 0.1
    for training in (True, False):
        case = R.mask_case(n)
        t32 = _torch32(case, dev, training, True, eps, mom)
        _compare("mask recompute n%d %s" % (n, training),
                 _kernel(case, dev, training, True, eps, mom, recompute=True), t32, case,
                 training, True, eps, mom)
        _compare("mask bn_act n%d %s" % (n, training), _module(case, dev, training, True, eps, mom),
                 t32, case, training, True, eps, mom)
        case = R.mask_case(n, residual=True)
        t32 = _torch32(case, dev, training, True, eps, mom)
        _compare("mask residual n%d %s" % (n, training), _kernel(case, dev, training, True, eps, mom),
                 t32, case, training, True, eps, mom)
        _compare("mask residual bn_act n%d %s" % (n, training),
                 _module(case, dev, training, True, eps, mom), t32, case, training, True, eps, mom)


# ------------------------------------------------------------------ channel isolation
@pytest.mark.parametrize("recompute", [False, True])
def test_a_nan_or_inf_stays_in_its_channel(dev, recompute):
    """A NaN in one channel and a +inf in another (both inside float4 groups shared with clean
    channels): every other channel's y, dx, dgamma, dbeta is bit-equal to the run without."""
    case = R.plain_case(300, 20, seed=9)
    clean = _kernel(case, dev, True, True, 1e-3, 0.1, recompute=recompute)
    dirty = dict(case)
    dirty["x"] = case["x"].clone()
    dirty["x"][7, 2] = float("nan")
    dirty["x"][150, 9] = float("inf")
    got = _kernel(dirty, dev, True, True, 1e-3, 0.1, recompute=recompute)
    keep = [i for i in range(20) if i not in (2, 9)]
    for q in ("y", "dx", "dgamma", "dbeta", "save_mean", "save_invstd"):
        assert torch.equal(got[q][..., keep], clean[q][..., keep]), q
    assert not torch.isfinite(got["save_mean"][[2, 9]]).any()


# ------------------------------------------------------------------ layout and refusals
def test_strided_inputs(dev):
    """x as a transposed view, dy non-contiguous: same results as the criterion demands."""
    eps, mom = 1e-3, 0.1
    case = R.plain_case(257, 20, seed=21, residual=True)
    xt = case["x"].t().contiguous().to(dev).t()
    dy = torch.stack([case["dy"], case["dy"]], 2).to(dev)[:, :, 0]
    assert not xt.is_contiguous() and not dy.is_contiguous()
    for training, frozen in ((True, False), (False, False), (True, True)):
        t32 = _torch32(case, dev, training, True, eps, mom)
        if frozen:      # no buffer moves
            t32["running_mean"], t32["running_var"] = case["running_mean"], case["running_var"]
        _compare("strided %s %s" % (training, frozen),
                 _module(case, dev, training, True, eps, mom, x=xt.detach(), dy=dy, frozen=frozen),
                 t32, case, training, True, eps, mom, frozen=frozen)


@pytest.mark.parametrize("c", [6, 1028])
def test_bn_act_falls_back_to_torch(dev, c):
    """c % 4 != 0 and c > 1024 have no kernel: bn_act returns torch's own result."""
    from msmdfusion_amd.spconv.functional import bn_act
    case = _dev(R.plain_case(130, c, seed=c, residual=True), dev)
    outs = []
    for fused in (True, False):
        bn = nn.BatchNorm1d(c, eps=1e-3, momentum=0.1).to(dev).train()
        with torch.no_grad():
            bn.weight.copy_(case["gamma"]); bn.bias.copy_(case["beta"])
        x = case["x"].clone().requires_grad_(True)
        y = bn_act(x, bn, relu=True, residual=case["residual"]) if fused else \
            torch.relu(bn(x) + case["residual"])
        y.backward(case["dy"])
        outs.append((y.detach(), x.grad, bn.weight.grad, bn.bias.grad, bn.running_mean,
                     bn.running_var, bn.num_batches_tracked))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_empty_input_comes_back(dev):
    from msmdfusion_amd.spconv.functional import bn_act
    bn = nn.BatchNorm1d(16).to(dev).train()
    x = torch.empty(0, 16, device=dev)
    assert bn_act(x, bn, relu=True) is x
    assert int(bn.num_batches_tracked) == 0
