"""The sparse-conv kernels (csrc/spconv_split.hip, spconv_wgrad_block.hip, spconv.hip) against
float64 at every scheduling edge.

Structure (tests *_exact): integer data with S = sum |a| |b| < 2^24, under which every bf16
product and every float32 partial sum in any order is exact -- every path must return the
float64 result bit for bit, whatever the tiling, the scheduling mode, the plane count.
Arithmetic (tests *_arithmetic, *_scaling, *_non_finite): unit-normal data judged by
e = max |out - ref64| / S against the float32 fused-multiply-add chain of the same sum.
A case id names the kernel, the instantiation, the widths, the row count, the kernel volume
and the mask recipe it pins (tests/conv_cases.py)."""

import functools

import numpy as np
import pytest
import torch

import conv_cases as C
import conv_ref as R
from msmdfusion_amd import kernels as K

pytestmark = pytest.mark.gpu

MODES = ("whole", "tiles", "streamk")      # split_tiles=False, the default, tile_prefix


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(dev):
    """A launch that left the device in error makes every later test fail for the wrong reason
    (and keeps launching on it): end the session at the test that caused it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit("device error after this test: %s" % err, returncode=3)


def t(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)


def f32(ref, dev):
    return torch.from_numpy(np.asarray(ref, np.float64).astype(np.float32)).to(dev)


def _flags_zero(dev):
    assert int(K._tile_counter(dev).abs().sum().item()) == 0, "tile counter / exchange flags"


def _same(out, want, what):
    """Bit-for-bit equality with a message that says where the kernel is wrong."""
    if torch.equal(out, want):
        return
    bad = (out != want).nonzero()
    r, c = bad[0].tolist()
    rows = torch.unique(bad[:, 0])
    raise AssertionError("%s: %d elements in %d rows differ (rows %d..%d); first at [%d, %d]: got "
                         "%r, want %r" % (what, bad.shape[0], rows.numel(), int(rows.min()),
                                          int(rows.max()), r, c, out[r, c].item(),
                                          want[r, c].item()))


def _split(dev, case, tab_d, order_d, prefix, fd, ws, planes, mode, bn=False):
    kw = dict(weight_flip=case.flip, row_order=order_d, bn_stats=bn)
    if mode == "whole":
        kw["split_tiles"] = False
    elif mode == "streamk":
        kw["tile_prefix"] = prefix
    return K.conv_forward_split(fd, ws, tab_d, case.n_out, case.c_out, planes, **kw)


def _tables(dev, case, row_order):
    """The case's table on the device (+ order, + the stream-K prefix, checked against its
    definition; the tile-order table checked against K.permute_cols)."""
    tab = C.fwd_table(case, row_order)
    rows = K.split_tile_rows(case.c_out)
    tab_d = t(tab.tab, dev)
    order_d = t(tab.order, dev) if row_order else None
    if row_order:
        assert torch.equal(K.permute_cols(t(tab.nat, dev), order_d), tab_d[:, :case.n_out])
    prefix = K.tile_prefix(tab_d[:, :case.n_out].contiguous(), rows)
    want = R.tile_prefix(tab.tab, case.n_out, rows)
    assert np.array_equal(prefix.cpu().numpy(), want)
    cut = R.stream_k_cut_tiles(want, case.c_in, case.kvol, rows)
    return tab, tab_d, order_d, prefix, cut


def _by_row(ref_tile_order, tab):
    if tab.order is None:
        return ref_tile_order
    out = np.empty_like(ref_tile_order)
    out[tab.order] = ref_tile_order
    return out


# =========================================================================== structure
@pytest.mark.parametrize("case", C.fwd_cases(), ids=lambda c: c.id)
def test_split_exact(dev, case):
    """Split forward / dgrad: all three scheduling modes, with and without a row order, three /
    two / one plane, every launch twice, flags back at zero -- bit for bit the float64 sum."""
    inst = K.split_instantiation(case.c_out)
    assert (inst["nt"], inst["waves"], inst["pingpong"], inst["passes"]) == tuple(case.inst)
    assert K.split_tile_rows(case.c_out) == 32 * case.inst[1]
    assert K.split_supported(case.c_in, case.c_out, case.kvol)
    plain = C.fwd_table(case, False)
    data = {}
    for planes, bits in ((3, 12), (2, 12), (1, 8)):
        f, w, ref, s = C.fwd_exact_data(case, plain, bits)
        assert s.max(initial=0.0) < 2 ** 24
        data[planes] = (t(f, dev), K.pack_weight_split(t(w, dev), planes, transpose=case.dgrad), ref)
    for row_order in (False, True):
        tab, tab_d, order_d, prefix, cut = _tables(dev, case, row_order)
        assert np.array_equal(tab.tab, plain.tab)
        if case.expect_cut:      # a tile summed in pieces by two stream-K ranges
            assert cut, "no tile is cut between two stream-K ranges"
        for planes, (fd, ws, ref) in data.items():
            want = f32(_by_row(ref, tab), dev)
            for mode in MODES:
                for rep in range(2):
                    out = _split(dev, case, tab_d, order_d, prefix, fd, ws, planes, mode)
                    _same(out, want, "%s planes=%d order=%s launch %d" % (mode, planes, row_order, rep))
                    _flags_zero(dev)


@pytest.mark.parametrize("case", C.bn_cases(), ids=lambda c: c.id)
def test_split_bn_stats_exact(dev, case):
    """bn_stats=True at the row edges of both tile heights: pivot, sum and sum of squares
    equal their float64 values exactly."""
    rows = K.split_tile_rows(case.c_out)
    plain = C.fwd_table(case, False)
    f, w, ref, s = C.bn_exact_data(case, plain)
    assert s.max() < 2 ** 24
    fd, ws = t(f, dev), K.pack_weight_split(t(w, dev), 3)
    n_tiles = (case.n_out + rows - 1) // rows
    want = np.zeros((n_tiles, 3, case.c_out))
    for ti in range(n_tiles):
        blk = ref[ti * rows:(ti + 1) * rows]
        d = blk - blk[0]
        want[ti] = blk[0], d.sum(0), (d * d).sum(0)
    assert np.abs(want).max() < 2 ** 24          # (and so is every partial sum of the squares)
    assert (np.abs(ref).max() * 2) ** 2 * rows < 2 ** 24
    for row_order in (False, True):
        tab, tab_d, order_d, prefix, _ = _tables(dev, case, row_order)
        for mode in MODES:
            for rep in range(2):
                out, part = _split(dev, case, tab_d, order_d, prefix, fd, ws, 3, mode, bn=True)
                _same(out, f32(_by_row(ref, tab), dev), "%s order=%s" % (mode, row_order))
                assert part.shape == (n_tiles, 3, case.c_out)
                for j, name in enumerate(("pivot", "sum", "sum of squares")):
                    _same(part[:, j], f32(want[:, j], dev), "%s %s order=%s" % (name, mode, row_order))
                _flags_zero(dev)


@pytest.mark.parametrize("case", C.f32_cases(), ids=lambda c: c.id)
def test_f32_forward_exact(dev, case):
    """msmd_spconv_fwd_f32: every tile count, staging width and row edge; static grid and the
    persistent form (row order + counter); ld > n_out with decoy padding."""
    for ld, pad in ((None, "builder"), (case.n_out + 19, "decoy")):
        for row_order in (False, True):
            tab = C.f32_table(case, row_order, ld, pad)
            f, w, ref, s = C.f32_exact_data(case, tab)
            assert s.max() < 2 ** 24
            # (this kernel reads the table by OUTPUT ROW; the order only chooses the tiling)
            nat = np.concatenate([tab.nat, tab.tab[:, case.n_out:]], 1)
            order_d = t(tab.order, dev) if row_order else None
            wp = K.pack_weight(t(w, dev))
            for rep in range(2):
                out = K.conv_forward(t(f, dev), wp, t(nat, dev), case.n_out, case.c_out,
                                     weight_flip=case.flip, row_order=order_d)
                _same(out, f32(ref, dev), "ld=%s order=%s launch %d" % (ld, row_order, rep))
                _flags_zero(dev)


@pytest.mark.parametrize("c_out", C.F32_PASS_WIDTHS)
def test_f32_column_passes_exact(dev, c_out):
    """spconv.functional._conv_f32: widths without an instantiation run as column passes."""
    from msmdfusion_amd.spconv import functional as F
    case = C.F32Case("f32-passes-c48to%d-n193-k27-random" % c_out, 48, c_out, 193, 579, 27, False,
                     "pipe1", 64)
    tab = C.f32_table(case)
    f, w, ref, s = C.f32_exact_data(case, tab)
    assert s.max() < 2 ** 24
    for krsc in (False, True):
        wd = t(w, dev)
        if krsc:
            wd = wd.permute(2, 0, 1).contiguous().view(c_out, 3, 3, 3, 48)
        out = F._conv_f32(t(f, dev), wd, krsc, False, t(tab.tab, dev), case.n_out)
        _same(out, f32(ref, dev), "krsc=%s" % krsc)


def _check_segments(seg, pairs, num, chunk_rows, kvol):
    table, n_chunks = seg
    tb = table.cpu().numpy()
    ns = n_chunks * kvol
    prefix, p0, cnt = tb[:ns + 1], tb[ns + 1:2 * ns + 1], tb[2 * ns + 1:]
    assert np.array_equal(cnt.reshape(n_chunks, kvol).sum(0), num)
    assert np.array_equal(np.diff(prefix), (cnt + 31) // 32) and prefix[0] == 0
    for c in range(n_chunks):
        for k in range(kvol):
            rows = pairs[k, 1, p0[c * kvol + k]:p0[c * kvol + k] + cnt[c * kvol + k]]
            assert ((rows >= c * chunk_rows) & (rows < (c + 1) * chunk_rows)).all()
    return (cnt == 0).reshape(n_chunks, kvol).all(1).sum()


@pytest.mark.parametrize("case", C.wgrad_cases(), ids=lambda c: c.id)
def test_wgrad_exact(dev, case):
    """The three wgrad kernels (whole-block, 64 x 64 slab, fp32) on prescribed pair lists,
    [K, Cin, Cout] and KRSC outputs, offset-major and row-chunk-major: bit for bit."""
    pr = C.wgrad_pairs(case)
    pairs_d, num_d = t(pr.pairs, dev), t(pr.num, dev)
    krsc = (case.c_out, case.kvol, 1, 1, case.c_in)
    split = case.kernel != "f32"
    assert K.wgrad_split_supported(case.c_in, case.c_out) == split
    segs = [None]
    if case.kernel == "block":
        one = K.pair_segments(pairs_d, num_d, 0)
        assert one is not None and one[1] == 1
        segs.append(one)
        if case.chunk_rows:
            seg = K.pair_segments(pairs_d, num_d, case.chunk_rows)
            assert seg[1] == (case.ld + case.chunk_rows - 1) // case.chunk_rows
            empty = _check_segments(seg, pr.pairs, pr.num, case.chunk_rows, case.kvol)
            if case.id.endswith("emptychunks"):
                assert seg[1] == K.WGRAD_MAX_CHUNKS and empty > seg[1] // 2
            segs.append(seg)
    elif split and case.kvol > 64:
        assert K.pair_segments(pairs_d, num_d, 0) is None
    for planes, bits in ((3, 12), (2, 12), (1, 8)):
        f, g, ref, s = C.wgrad_exact_data(case, pr, bits)
        assert s.max(initial=0.0) < 2 ** 24
        fd, gd, want = t(f, dev), t(g, dev), f32(ref, dev)
        want_k = want.permute(2, 0, 1).contiguous().view(krsc)
        for rep in range(2):
            if planes == 3:      # the fp32 kernel takes every width
                _same(K.conv_wgrad(fd, gd, pairs_d, num_d).flatten(1), want.flatten(1), "fp32 kernel")
                _same(K.conv_wgrad(fd, gd, pairs_d, num_d, krsc_shape=krsc).flatten(1),
                      want_k.flatten(1), "fp32 kernel, KRSC")
            if not split:
                continue
            for seg in segs:
                what = "planes=%d chunks=%s launch %d" % (planes, seg and seg[1], rep)
                dw = K.conv_wgrad_split(fd, gd, pairs_d, num_d, planes, segments=seg)
                _same(dw.flatten(1), want.flatten(1), what)
                dwk = K.conv_wgrad_split(fd, gd, pairs_d, num_d, planes, krsc_shape=krsc, segments=seg)
                _same(dwk.flatten(1), want_k.flatten(1), what + " KRSC")


# =========================================================================== arithmetic
@functools.lru_cache(maxsize=None)
def _fwd_reference(ac):
    """(table, features, weight, ref64, S, e of the float32 chain) of an arithmetic case:
    computed once, shared, never modified."""
    b = ac.base
    tab, f, w = C.arith_fwd_setup(ac)
    dgrad = getattr(b, "dgrad", False)
    ref, s = R.conv_table(f, w, tab.nat, b.n_out, b.flip, dgrad)
    e = R.normalised_error(R.conv_fwd_f32_chain(f, w, tab.nat, b.n_out, b.flip, dgrad), ref, s)
    for a in (tab.tab, tab.nat, f, w, ref, s):
        a.setflags(write=False)
    return tab, f, w, ref, s, e


def _plane_targets(conv, a, b, planes):
    """(cut, kept, d): the float64 sum over the operands cut to `planes` planes; the same
    without the plane products that Products<planes> drops by design (two planes: am * bm);
    d = the sum of |those products|, so that |kept - cut| <= d element by element."""
    cut = conv(R.cut_planes(a, planes), R.cut_planes(b, planes))[0]
    kept, d = cut, np.zeros_like(cut)
    for i, j in R.dropped_products(planes):
        o, m = conv(R.plane(a, i), R.plane(b, j))
        kept, d = kept - o, d + m
    return cut, kept, d


def _judge(what, out, planes, ref, s, e_chain, targets):
    """Three planes: against the float64 sum.  Two planes / one plane: against the float64 sum
    of the operands cut to their planes -- for two planes less the am * bm products, which that
    mode leaves out by design: measured against the plain cut sum the 40 -> 128, K = 32 case
    gave e = 9.5e-7 with the chain at 2.3e-7, and sum |am| |bm| / S <= 2^-16 = 1.5e-5 is that
    term's bound (each |m| <= 2^-8 |x|).  The float32 allowance is the same 4 x e_chain."""
    if planes == 3:
        e = R.normalised_error(out, ref, s)
    else:
        cut, kept, d = targets
        e = R.normalised_error(out, kept, s)
        print("RATIO %s planes=%d against the cut operands: e=%.3e, dropped by design <= %.3e"
              % (what, planes, R.normalised_error(out, cut, s), R.normalised_error(cut + d, cut, s)))
    print("RATIO %s planes=%d e=%.3e chain=%.3e ratio=%.2f" % (what, planes, e, e_chain, e / e_chain))
    assert e <= 4 * e_chain, (what, planes, e, e_chain)


@pytest.mark.parametrize("ac", C.arith_fwd_cases(), ids=lambda a: a.id)
def test_split_arithmetic(dev, ac):
    """Three planes: e <= 4 x the float32 chain's e (six times the accumulations, unknown order
    inside an MFMA).  Two planes / one plane: the same allowance around the float64 sum of the
    operands cut to their planes."""
    b = ac.base
    tab, f, w, ref, s, e_chain = _fwd_reference(ac)
    assert 0 < e_chain < 2.0 ** -18
    rows = K.split_tile_rows(b.c_out)
    tab_d, order_d, fd = t(tab.tab, dev), t(tab.order, dev), t(f, dev)
    prefix = K.tile_prefix(tab_d, rows)
    def conv(x, y):
        return R.conv_table(x, y, tab.nat, b.n_out, b.flip, b.dgrad)
    for planes in (3, 2, 1):
        ws = K.pack_weight_split(t(w, dev), planes, transpose=b.dgrad)
        targets = _plane_targets(conv, f, w, planes) if planes < 3 else None
        for mode in MODES:
            out = _split(dev, b, tab_d, order_d, prefix, fd, ws, planes, mode).cpu().numpy()
            _judge("split %s %s" % (ac.id, mode), out, planes, ref, s, e_chain, targets)


@pytest.mark.parametrize("ac", C.arith_f32_cases(), ids=lambda a: a.id)
def test_f32_arithmetic(dev, ac):
    b = ac.base
    tab, f, w, ref, s, e_chain = _fwd_reference(ac)
    assert 0 < e_chain < 2.0 ** -18
    out = K.conv_forward(t(f, dev), K.pack_weight(t(w, dev)), t(tab.tab, dev), b.n_out, b.c_out)
    _judge("f32 %s" % ac.id, out.cpu().numpy(), 3, ref, s, e_chain, None)


@pytest.mark.parametrize("ac", C.arith_wgrad_cases(), ids=lambda a: a.id)
def test_wgrad_arithmetic(dev, ac):
    b = ac.base
    pr, f, g = C.arith_wgrad_setup(ac)
    ref, s = R.conv_wgrad(f, g, pr.pairs, pr.num)
    e_chain = R.normalised_error(R.conv_wgrad_f32_chain(f, g, pr.pairs, pr.num), ref, s)
    assert 0 < e_chain < 2.0 ** -18
    fd, gd, pairs_d, num_d = t(f, dev), t(g, dev), t(pr.pairs, dev), t(pr.num, dev)
    runs = [("fp32", 3, lambda: K.conv_wgrad(fd, gd, pairs_d, num_d))]
    if b.kernel != "f32":
        for planes in (3, 2, 1):
            runs.append((b.kernel, planes, lambda p=planes: K.conv_wgrad_split(fd, gd, pairs_d, num_d, p)))
    def conv(x, y):
        return R.conv_wgrad(x, y, pr.pairs, pr.num)
    for name, planes, run in runs:
        targets = _plane_targets(conv, f, g, planes) if planes < 3 else None
        _judge("wgrad-%s %s" % (name, ac.id), run().cpu().numpy(), planes, ref, s, e_chain, targets)


SCALES = (-60, -20, 20, 60)


def _bits(x):
    return x.view(torch.int32)


@pytest.mark.parametrize("ac", [a for a in C.arith_fwd_cases() + C.arith_f32_cases()
                                if a.data == "normal"], ids=lambda a: a.id)
def test_forward_power_of_two_scaling(dev, ac):
    """features * 2^s with weights * 2^-s reproduce the unscaled output bit for bit: the
    scaling commutes with every rounding while nothing leaves the normal range."""
    b = ac.base
    tab, f, w, ref, s, _ = _fwd_reference(ac)
    split = isinstance(b, C.FwdCase)
    tab_d = t(tab.tab, dev)

    def run(fs, wsc, planes):
        if not split:
            return K.conv_forward(t(fs, dev), K.pack_weight(t(wsc, dev)), tab_d, b.n_out, b.c_out)
        rows = K.split_tile_rows(b.c_out)
        return _split(dev, b, tab_d, t(tab.order, dev), K.tile_prefix(tab_d, rows), t(fs, dev),
                      K.pack_weight_split(t(wsc, dev), planes, transpose=b.dgrad), planes, "streamk")
    for planes in (3, 2, 1) if split else (3,):
        base = run(f, w, planes)
        for sh in SCALES:
            out = run(f * np.float32(2.0 ** sh), w * np.float32(2.0 ** -sh), planes)
            assert torch.equal(_bits(out), _bits(base)), (planes, sh)


@pytest.mark.parametrize("ac", [a for a in C.arith_wgrad_cases() if a.data == "normal"],
                         ids=lambda a: a.id)
def test_wgrad_power_of_two_scaling(dev, ac):
    b = ac.base
    pr, f, g = C.arith_wgrad_setup(ac)
    pairs_d, num_d = t(pr.pairs, dev), t(pr.num, dev)

    def run(fs, gs, planes):
        if planes == 0:
            return K.conv_wgrad(t(fs, dev), t(gs, dev), pairs_d, num_d)
        return K.conv_wgrad_split(t(fs, dev), t(gs, dev), pairs_d, num_d, planes)
    for planes in (0,) + ((3, 2, 1) if b.kernel != "f32" else ()):
        base = run(f, g, planes)
        for sh in SCALES:
            out = run(f * np.float32(2.0 ** sh), g * np.float32(2.0 ** -sh), planes)
            assert torch.equal(_bits(out), _bits(base)), (planes, sh)


# --------------------------------------------------------------------------- non-finite values
def _poison_rows(tab, n_in):
    """(a referenced input row, an unreferenced one, bool[n_out] rows connected to the first)."""
    used = np.unique(tab.nat[tab.nat >= 0])
    hit = int(used[used.size // 2])
    free = int(np.setdiff1d(np.arange(n_in), used)[0])
    return hit, free, (tab.nat == hit).any(0)


@pytest.mark.parametrize("ac", [a for a in C.arith_fwd_cases() if a.data == "normal"],
                         ids=lambda a: a.id)
def test_split_non_finite(dev, ac):
    """One NaN (or +inf) input row changes exactly the output rows connected to it, and those
    become NaN in every element: bf16(inf) = inf leaves the plane residual inf - inf = NaN, so
    the split kernels return NaN where the fp32 kernel returns inf (include/msmd_hip.h).  All
    other rows stay bit-identical in all three scheduling modes; an unreferenced NaN row
    changes nothing."""
    b = ac.base
    tab, f, w, ref, s, _ = _fwd_reference(ac)
    hit, free, connected = _poison_rows(tab, b.n_in)
    assert connected.any() and not connected.all()
    conn = t(connected, dev)
    rows = K.split_tile_rows(b.c_out)
    tab_d, order_d = t(tab.tab, dev), t(tab.order, dev)
    prefix = K.tile_prefix(tab_d, rows)
    for planes in (3, 2, 1):
        ws = K.pack_weight_split(t(np.abs(w) + np.float32(1e-3), dev), planes, transpose=b.dgrad)
        for mode in MODES:
            clean = _split(dev, b, tab_d, order_d, prefix, t(f, dev), ws, planes, mode)
            assert torch.isfinite(clean).all()
            for value in (np.nan, np.inf):
                fp = f.copy()
                fp[free] = np.nan
                out = _split(dev, b, tab_d, order_d, prefix, t(fp, dev), ws, planes, mode)
                assert torch.equal(_bits(out), _bits(clean)), (planes, mode, "unreferenced row")
                fp[hit] = value
                out = _split(dev, b, tab_d, order_d, prefix, t(fp, dev), ws, planes, mode)
                assert torch.equal(_bits(out[~conn]), _bits(clean[~conn])), (planes, mode, value)
                if np.isinf(value) and planes == 1:      # no residual: bf16(inf) * w = inf
                    assert torch.isinf(out[conn]).all() and (out[conn] > 0).all()
                else:
                    assert torch.isnan(out[conn]).all(), (planes, mode, value)
            _flags_zero(dev)


@pytest.mark.parametrize("ac", [a for a in C.arith_f32_cases() if a.data == "normal"],
                         ids=lambda a: a.id)
def test_f32_non_finite(dev, ac):
    """The fp32 kernel: NaN rows give NaN, a +inf row under positive weights gives +inf."""
    b = ac.base
    tab, f, w, ref, s, _ = _fwd_reference(ac)
    hit, free, connected = _poison_rows(tab, b.n_in)
    conn = t(connected, dev)
    wp = K.pack_weight(t(np.abs(w) + np.float32(1e-3), dev))
    tab_d = t(tab.tab, dev)
    clean = K.conv_forward(t(f, dev), wp, tab_d, b.n_out, b.c_out)
    for value in (np.nan, np.inf):
        fp = f.copy()
        fp[free] = np.nan
        out = K.conv_forward(t(fp, dev), wp, tab_d, b.n_out, b.c_out)
        assert torch.equal(_bits(out), _bits(clean))
        fp[hit] = value
        out = K.conv_forward(t(fp, dev), wp, tab_d, b.n_out, b.c_out)
        assert torch.equal(_bits(out[~conn]), _bits(clean[~conn]))
        if np.isinf(value):
            assert torch.isinf(out[conn]).all() and (out[conn] > 0).all()
        else:
            assert torch.isnan(out[conn]).all()


@pytest.mark.parametrize("ac", [a for a in C.arith_wgrad_cases() if a.data == "normal"],
                         ids=lambda a: a.id)
def test_wgrad_non_finite(dev, ac):
    """A NaN / +inf feature row changes exactly the offsets whose pair lists hold it."""
    b = ac.base
    pr, f, g = C.arith_wgrad_setup(ac)
    g = np.abs(g) + np.float32(1e-3)
    used = np.unique(np.concatenate([pr.pairs[k, 0, :n] for k, n in enumerate(pr.num)]))
    hit = int(used[used.size // 2])
    free = int(np.setdiff1d(np.arange(b.n_in), used)[0])
    touched = np.array([(pr.pairs[k, 0, :n] == hit).any() for k, n in enumerate(pr.num)])
    assert touched.any() and not touched.all()
    tk = t(touched, dev)
    pairs_d, num_d, gd = t(pr.pairs, dev), t(pr.num, dev), t(g, dev)
    runs = [(0, lambda x: K.conv_wgrad(x, gd, pairs_d, num_d))]
    if b.kernel != "f32":
        runs += [(p, lambda x, p=p: K.conv_wgrad_split(x, gd, pairs_d, num_d, p)) for p in (3, 2, 1)]
    for planes, run in runs:
        clean = run(t(f, dev))
        assert torch.isfinite(clean).all()
        for value in (np.nan, np.inf):
            fp = f.copy()
            fp[free] = np.nan
            assert torch.equal(_bits(run(t(fp, dev))), _bits(clean)), (planes, "unreferenced row")
            fp[hit] = value
            out = run(t(fp, dev))
            assert torch.equal(_bits(out[~tk]), _bits(clean[~tk])), (planes, value)
            if np.isinf(value) and planes in (0, 1):
                assert torch.isinf(out[tk]).all() and (out[tk] > 0).all()
            else:
                assert torch.isnan(out[tk]).all(), (planes, value)
