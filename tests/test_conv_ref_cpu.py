"""The float64 restatements and case builders of the sparse-conv edge suite, checked without
a GPU: the restatements against the C oracle on geometric rulebooks (which also pins the
weight_flip convention read out of the kernel), the builders' invariants, S < 2^24 for every
integer case and a float32-chain error below 2^-18 for every arithmetic case."""

import numpy as np
import pytest

import conv_cases as C
import conv_ref as R
from msmdfusion_amd import synthetic as S
from oracle import oracle as O

U = 2.0 ** -24


def _geometry(subm):
    shape = [9, 24, 24]
    idx = S.random_voxel_indices(400, 2, shape, seed=3)
    if subm:
        oi, pr, nm, _ = O.get_indice_pairs(idx, 2, shape, 3, 1, 1, 1, True)
    else:
        oi, pr, nm, _ = O.get_indice_pairs(idx, 2, shape, 3, 2, 1, 1, False)
    return idx.shape[0], oi.shape[0], pr, nm


@pytest.mark.parametrize("subm", [True, False], ids=["subm", "strided"])
def test_restatements_equal_the_oracle(subm):
    n_in, n_out, pr, nm = _geometry(subm)
    cin, cout = 16, 24
    rng = np.random.RandomState(5)
    f = rng.randn(n_in, cin).astype(np.float32)
    w = rng.randn(27, cin, cout).astype(np.float32)
    g = rng.randn(n_out, cout).astype(np.float32)
    nbr = R.table_from_pairs(pr, nm, n_out)
    exp = O.indice_conv_fwd(f, w, pr, nm, n_out, subm=subm)
    edin, edw = O.indice_conv_bwd(f, w, g, pr, nm, subm=subm)
    # float32 rounding of a sum of T terms: T u S at the very most
    out, s = R.conv_fwd(f, w, nbr, n_out)
    assert (np.abs(out - exp) <= 27 * cin * U * s + 1e-30).all()
    chain = R.conv_fwd_f32_chain(f, w, nbr, n_out)
    assert (np.abs(out - chain) <= 27 * cin * U * s + 1e-30).all()
    din, sd = R.conv_dgrad(g, w, R.mirror_table(nbr, n_out, n_in), n_in)
    assert (np.abs(din - edin) <= 27 * cout * U * sd + 1e-30).all()
    if subm:     # the forward table read with flipped weights is the mirrored table
        din_f, sf = R.conv_dgrad(g, w, nbr, n_in, weight_flip=True)
        # (the same terms in the opposite offset order: equal to float64 rounding)
        assert np.abs(sf - sd).max() <= 1e-12 * sd.max()
        assert np.abs(din_f - din).max() <= 1e-12 * sd.max()
        assert np.array_equal(R.mirror_table(nbr, n_out, n_in), nbr[::-1])
    dw, sw = R.conv_wgrad(f, g, pr, nm)
    assert (np.abs(dw - edw) <= int(nm.max()) * U * sw + 1e-30).all()
    wch = R.conv_wgrad_f32_chain(f, g, pr, nm)
    assert (np.abs(dw - wch) <= int(nm.max()) * U * sw + 1e-30).all()


def test_bf16_planes():
    x = np.random.RandomState(0).randn(4096).astype(np.float32) * np.float32(3.7)
    assert np.array_equal(R.cut_planes(x, 3), x.astype(np.float64))      # h + m + l is exact
    h = R.bf16_round(x)
    assert (h.view(np.uint32) & 0xFFFF == 0).all() and (np.abs(x - h) <= np.abs(x) * 2.0 ** -8).all()
    assert (np.abs(R.cut_planes(x, 2) - x) <= np.abs(x) * 2.0 ** -16).all()
    planes = [R.plane(x, p).astype(np.float64) for p in range(3)]
    assert np.array_equal(planes[0] + planes[1] + planes[2], x.astype(np.float64))
    assert np.array_equal(planes[0] + planes[1], R.cut_planes(x, 2))
    assert (np.abs(planes[1]) <= np.abs(x) * 2.0 ** -8).all()      # half an ulp of 8 bits
    assert R.dropped_products(1) == () and R.dropped_products(2) == ((1, 1),)
    assert R.dropped_products(3) == ((1, 2), (2, 1), (2, 2))
    # ties to even
    tie = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], np.float32)
    assert np.array_equal(R.bf16_round(tie), np.array([1.0, 1.0 + 2.0 ** -6], np.float32))


@pytest.mark.parametrize("case", C.fwd_cases() + C.bn_cases(), ids=lambda c: c.id)
def test_forward_case_invariants(case):
    rows = 32 * case.inst[1]
    for row_order in (False, True):
        t = C.fwd_table(case, row_order)
        assert t.tab.shape == (case.kvol, case.ld or case.n_out) and t.tab.dtype == np.int32
        assert t.tab.min() >= -1 and t.tab.max() < case.n_in
        if row_order:     # tile order as K.permute_cols defines it
            assert np.array_equal(np.sort(t.order), np.arange(case.n_out))
            assert np.array_equal(t.nat[:, t.order], t.tab[:, :case.n_out])
        else:
            assert np.array_equal(t.nat, t.tab[:, :case.n_out])
        real = t.tab[:, :case.n_out]
        if t.decoy is not None:
            assert (real != t.decoy).all() and (t.tab[:, case.n_out:] == t.decoy).all()
        else:
            assert (t.tab[:, case.n_out:] == -1).all()
        if case.source == "last":
            assert set(np.unique(real)) <= {-1, case.n_in - 1}
        if case.recipe == "none" and not case.tile_recipes:
            assert (real == -1).all()
        for pos, recipe in (case.tile_recipes or {}).items():
            n_tiles = (case.n_out + rows - 1) // rows
            blk = real[:, (pos % n_tiles) * rows:(pos % n_tiles + 1) * rows] >= 0
            want = {"all": blk.all(), "none": not blk.any(),
                    "first": blk[0].all() and not blk[1:].any(),
                    "last": blk[-1].all() and not blk[:-1].any(),
                    "group": blk.any(0).sum() == min(32, blk.shape[1]) and blk.all(0).sum() == blk.any(0).sum(),
                    "random": blk.any() and not blk.all()}[recipe]
            assert want, (pos, recipe)
        if case.id.endswith("-bn"):
            f, w, ref, s = C.bn_exact_data(case, t)
            dev_ = ref - ref[0]
            assert (dev_ * dev_).sum(0).max() * 4 < 2 ** 24       # any pivot of the tile
        else:
            for bits in (12, 8):
                f, w, ref, s = C.fwd_exact_data(case, t, bits)
                assert s.max(initial=0.0) < 2 ** 24
                assert np.abs(w).max() <= 3 and np.array_equal(f, np.rint(f))
                assert np.abs(np.delete(f, t.decoy, 0) if t.decoy is not None else f).max() < 2 ** bits
        pre = R.tile_prefix(t.tab, case.n_out, rows)
        cut = R.stream_k_cut_tiles(pre, case.c_in, case.kvol, rows)
        assert bool(cut) or not case.expect_cut
    assert tuple(case.inst) == C.split_inst(case.c_out)


def test_forward_cases_cover_what_they_claim():
    cases = C.fwd_cases()
    seen = {}
    for c in cases:
        seen.setdefault((c.inst[0], c.inst[2]), set()).add(c.c_in % 32 == 0)
    assert set(seen) == {(2, False), (4, False), (6, False), (8, False), (6, True), (8, True),
                         (12, True)}
    assert all(v == {True, False} for v in seen.values())      # full and partial last k-block
    assert {c.c_in for c in cases} >= {32, 40, 64, 72, 136, 256}
    assert {c.c_out for c in cases} == {32, 36, 48, 64, 80, 96, 112, 128, 132, 144, 160, 164, 176,
                                        192, 208, 256, 272}
    for waves, rows in C.ROWS.items():
        assert {c.n_out for c in cases if c.inst[1] == waves} == set(rows)
    assert {(c.kvol, c.flip) for c in cases} >= {(k, f) for k in C.KVOLS for f in (False, True)}
    assert any(c.expect_cut for c in cases if c.inst[2]) and any(c.expect_cut for c in cases if not c.inst[2])
    assert max(c.n_out for c in cases) <= 1100 and max(c.kvol for c in cases) <= 32


@pytest.mark.parametrize("case", C.f32_cases(), ids=lambda c: c.id)
def test_f32_case_invariants(case):
    t = C.f32_table(case)
    assert t.tab.min() >= -1 and t.tab.max() < case.n_in
    f, w, ref, s = C.f32_exact_data(case, t)
    assert s.max() < 2 ** 24 and w.shape == (case.kvol, case.c_in, case.c_out)
    assert case.staging == C.f32_staging(case.c_in, case.c_out, case.kvol)


@pytest.mark.parametrize("case", C.wgrad_cases(), ids=lambda c: c.id)
def test_wgrad_case_invariants(case):
    pr = C.wgrad_pairs(case)
    assert pr.pairs.shape == (case.kvol, 2, case.ld) and np.array_equal(pr.num, case.num)
    assert pr.pairs.min() >= -1
    assert pr.pairs[:, 0].max(initial=-1) < case.n_in and pr.pairs[:, 1].max(initial=-1) < case.n_out
    for k, p in enumerate(case.num):
        o = pr.pairs[k, 1, :p]
        assert (np.diff(o) > 0).all() and (o >= 0).all() and (pr.pairs[k, 0, :p] >= 0).all()
        tail = pr.pairs[k, :, p:]
        if case.pad == "decoy":
            assert (tail[0] == case.n_in - 1).all() and (tail[1] == case.n_out - 1).all()
            assert (pr.pairs[k, 0, :p] < case.n_in - 1).all() and (o < case.n_out - 1).all()
        else:
            assert (tail == -1).all()
    if case.chunk_rows:        # the segment table's chunks must cover the output rows
        assert case.n_out <= case.ld and (case.ld + case.chunk_rows - 1) // case.chunk_rows <= 256
    assert case.kernel == C.wgrad_kernel(case.c_in, case.c_out, case.kvol)
    for bits in (12, 8):
        f, g, ref, s = C.wgrad_exact_data(case, pr, bits)
        assert s.max(initial=0.0) < 2 ** 24
        assert np.abs(g[:case.n_out - 1] if case.pad == "decoy" else g).max() <= 3


def test_wgrad_cases_cover_what_they_claim():
    cs = C.wgrad_cases()
    block = [c for c in cs if c.kernel == "block"]
    for side in (64, 80, 96, 112, 128):          # every quadrant shape on either side
        assert any(c.c_in == side for c in block) and any(c.c_out == side for c in block), side
    for side in (160, 192, 224, 256, 320):       # the multi-block sides
        assert any(side in (c.c_in, c.c_out) for c in block), side
    assert [C.wgrad_side_blocks(c) for c in (160, 192, 224, 256, 320)] == [2, 2, 2, 2, 4]
    slab = [c for c in cs if c.kernel == "slab"]
    assert {68, 100, 144, 176, 208} <= {c.c_in for c in slab} | {c.c_out for c in slab}
    assert any(c.kvol == 125 for c in slab)
    assert any(c.kernel == "f32" and max(c.c_in, c.c_out) < 64 for c in cs)
    assert {n for c in cs for n in c.num} >= set(C.NUMS)
    assert any(c.ld == 1 for c in cs) and any(sum(c.num) == 0 for c in cs)
    chunks = {(c.ld + c.chunk_rows - 1) // c.chunk_rows for c in cs if c.chunk_rows}
    assert 256 in chunks and {c.chunk_rows for c in cs if c.chunk_rows} >= {1, 100}


@pytest.mark.parametrize("ac", C.arith_fwd_cases() + C.arith_f32_cases(), ids=lambda a: a.id)
def test_arithmetic_forward_cases_are_well_conditioned(ac):
    b = ac.base
    tab, f, w = C.arith_fwd_setup(ac)
    flip, dgrad = b.flip, getattr(b, "dgrad", False)
    ref, s = R.conv_table(f, w, tab.nat, b.n_out, flip, dgrad)
    e = R.normalised_error(R.conv_fwd_f32_chain(f, w, tab.nat, b.n_out, flip, dgrad), ref, s)
    assert 0 < e < 2.0 ** -18, e


@pytest.mark.parametrize("ac", C.arith_wgrad_cases(), ids=lambda a: a.id)
def test_arithmetic_wgrad_cases_are_well_conditioned(ac):
    pr, f, g = C.arith_wgrad_setup(ac)
    ref, s = R.conv_wgrad(f, g, pr.pairs, pr.num)
    e = R.normalised_error(R.conv_wgrad_f32_chain(f, g, pr.pairs, pr.num), ref, s)
    assert 0 < e < 2.0 ** -18, e
