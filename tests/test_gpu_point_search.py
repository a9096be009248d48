"""The GMA-Conv neighbour search (csrc/points.hip, csrc/gma_nn.hip) at every edge of its
dispatch: each FPS instantiation and its upper size, the pruned kernel's hand-over taken
and not taken, ball query / nearest key / assignment at their block, chunk and group
boundaries, and the ragged one-call chain with more than one query tile.  All outputs are
integer indices with an exact reference (the oracle, pinned against numpy restatements in
tests/test_point_search_cpu.py): every comparison is np.array_equal.  The inputs and the
properties they must have live in tests/point_search_cases.py."""
import numpy as np
import pytest
import torch

import point_search_cases as C
from msmdfusion_amd import kernels as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)      # a copy: some inputs are read-only


def _np(x):
    return x.detach().cpu().numpy()


def fps_both(xyz, m, dev):
    got = K.furthest_point_sample(t(xyz, dev), m)
    assert got.dtype == torch.int32 and tuple(got.shape) == (xyz.shape[0], m)
    return _np(got), O.furthest_point_sample(xyz, m)


# ------------------------------------------------------------------ FPS, plain kernels
@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("n", C.FPS_PLAIN_N,
                         ids=["%s-n%d" % (C.fps_instantiation(n, C.FPS_PLAIN_M), n)
                              for n in C.FPS_PLAIN_N])
def test_fps_plain_instantiations(dev, n, kind):
    """One n per fps_kernel<PPT> and the largest n it takes; m = 40 is never pruned."""
    assert C.fps_instantiation(n, C.FPS_PLAIN_M).startswith("plain")
    xyz = np.stack([C.fps_cloud(n, kind, n), C.fps_cloud(n, kind, n + 1)])
    got, exp = fps_both(xyz, C.FPS_PLAIN_M, dev)
    assert not np.array_equal(exp[0], exp[1])
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("n,m", C.FPS_SMALL, ids=["plain2-n%d-m%d" % nm for nm in C.FPS_SMALL])
def test_fps_small_sets(dev, n, m, kind):
    """Every floor(log2 n) edge of the tie rank below 1024, and m > n: once every point is
    taken the reference keeps selecting index 0.  Whole rows."""
    xyz = np.stack([C.fps_cloud(n, kind, 10 * n + m), C.fps_cloud(n, kind, 10 * n + m + 1)])
    got, exp = fps_both(xyz, m, dev)
    if m > n:
        assert (exp[:, n:] == 0).all() and sorted(exp[0, :n].tolist()) == list(range(n))
    assert np.array_equal(got, exp)


# ------------------------------------------------------------------ FPS, pruned kernels
def _pruned_ids():
    out = []
    for n in C.FPS_PRUNED_N:
        for m in C.FPS_PRUNED_M:
            for order in ("coherent", "permuted"):
                side = "handover" if order == "permuted" else "finish"
                out.append(pytest.param(n, m, order,
                                        id="%s-%s-n%d-m%d" % (C.fps_instantiation(n, m), side, n, m)))
    return out


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("n,m,order", _pruned_ids())
def test_fps_pruned_instantiations(dev, n, m, order, kind):
    """fps_pruned_kernel<16|32|48> at both ends of its range, on index-coherent input (it
    finishes the element; the resume launch behind it returns at once) and on the same kind
    of input permuted (it hands over after round 95; the resume launch replays and finishes).
    Which of the two happens is the probe model's verdict, with a factor 2 to spare."""
    assert C.fps_instantiation(n, m).startswith("pruned")
    clouds = [C.fps_line(n, kind, seed, order) for seed in (0, 1)]
    for p in clouds:
        count, nb, over = C.fps_probe_refreshes(p, m)
        assert over is (order == "permuted") and C.fps_probe_margin_ok(count, nb, over), (count, nb)
    got, exp = fps_both(np.stack(clouds), m, dev)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("n,m", C.FPS_NEIGHBOURS,
                         ids=["%s-n%d-m%d" % (C.fps_instantiation(n, m), n, m)
                              for n, m in C.FPS_NEIGHBOURS])
@pytest.mark.parametrize("order", ["coherent", "permuted"])
def test_fps_beside_the_pruned_dispatch(dev, n, m, order):
    """One point too few, one sample too few, one point too many for the pruned kernel."""
    assert C.fps_instantiation(n, m).startswith("plain")
    xyz = np.stack([C.fps_line(n, "float", 2, order), C.fps_line(n, "int", 3, order)])
    got, exp = fps_both(xyz, m, dev)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("n", [6144, 24576], ids=["pruned16-mixed-n6144", "pruned48-mixed-n24576"])
def test_fps_pruned_batch_with_both_sides(dev, n):
    """Element 0 finishes in the pruned kernel, element 1 hands over: the resume launch
    returns for one and replays the other."""
    m = 260
    xyz = np.stack([C.fps_line(n, "float", 4, "coherent"), C.fps_line(n, "float", 5, "permuted")])
    sides = [C.fps_probe_refreshes(p, m) for p in xyz]
    assert [s[2] for s in sides] == [False, True]
    assert all(C.fps_probe_margin_ok(*s) for s in sides)
    got, exp = fps_both(xyz, m, dev)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


def test_fps_ragged_pruned_batch(dev):
    """One ragged call through the pruned kernel: a coherent element, an empty one, one
    point, 300 points (both far fewer than samples) and a permuted element that hands over.
    Whole rows against the oracle per element; the empty element gives the documented row of
    zeros (the oracle is not defined there).  Bit for bit the same on a second run."""
    parts, m = C.fps_ragged_parts(), C.FPS_RAGGED_M
    sizes = [p.shape[0] for p in parts]
    assert sizes == C.FPS_RAGGED_SIZES and C.fps_instantiation(max(sizes), m) == "pruned48"
    for p, order in zip(parts, C.FPS_RAGGED_ORDER):
        if order:
            count, nb, over = C.fps_probe_refreshes(p, m)
            assert over is (order == "permuted") and C.fps_probe_margin_ok(count, nb, over)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    xyz, offs_d = t(np.concatenate(parts), dev), t(offs, dev)
    got = K.furthest_point_sample_ragged(xyz, offs_d, max(sizes), m)
    again = K.furthest_point_sample_ragged(xyz, offs_d, max(sizes), m)
    assert torch.equal(got, again)
    got = _np(got)
    assert got.shape == (len(sizes), m)
    for i, p in enumerate(parts):
        if sizes[i] == 0:
            assert (got[i] == 0).all()
        else:
            assert np.array_equal(got[i], O.furthest_point_sample(p[None], m)[0]), i


# ------------------------------------------------------------------ ball query
@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("radii", C.BALL_RADII, ids=lambda r: "r%g-%g" % r)
@pytest.mark.parametrize("n,m", C.BALL_NM, ids=["n%d-m%d" % nm for nm in C.BALL_NM])
def test_ball_query_edges(dev, n, m, radii, kind):
    """B = 2 with different clouds and centres, n and m beside the group of 64 and the four
    centres of a block, nsample beside 64, an inner radius, centres without a hit."""
    C.check_ball_family(kind)
    xyz, cen = C.ball_case(n, m, kind)
    hits = [C.ball_hits_np(radii[0], radii[1], xyz[e], cen[e]) for e in range(2)]
    assert any(h.size == 0 for h in hits[0] + hits[1]), "a centre without a hit"
    if m >= 2:
        assert any(h.size for h in hits[0]) and any(h.size for h in hits[1])
    if radii[0] > 0 and m >= 3:
        assert any((xyz[e] == c).all(1).any() for e in range(2) for c in cen[e]), "d2 == 0 centre"
    for ns in C.BALL_NSAMPLE:
        exp = O.ball_query(radii[0], radii[1], ns, xyz, cen)
        got = K.ball_query(radii[0], radii[1], ns, t(xyz, dev), t(cen, dev))
        assert got.dtype == torch.int32 and tuple(got.shape) == (2, m, ns)
        assert np.array_equal(_np(got), exp), ns


# ------------------------------------------------------------------ nearest key
@pytest.mark.parametrize("nk", C.NN_NK)
@pytest.mark.parametrize("nq", C.NN_NQ)
def test_nn_search_block_and_chunk_edges(dev, nq, nk):
    q, k = C.nn_case(nq, nk)
    exp = O.nn_search(q, k, C.NN_THRESH)
    if nk == 0:
        assert (exp == -1).all()
    elif nq >= 255:
        assert (exp >= 0).any() and (exp < 0).any()
    got = K.nn_search(t(q, dev), t(k, dev), C.NN_THRESH)
    assert got.dtype == torch.int32 and tuple(got.shape) == (nq,)
    assert np.array_equal(_np(got), exp)


def test_nn_search_ties_and_threshold(dev):
    q, k, exp = C.nn_tie_case()
    assert np.array_equal(O.nn_search(q, k, C.NN_THRESH), exp)
    assert np.array_equal(_np(K.nn_search(t(q, dev), t(k, dev), C.NN_THRESH)), exp)
    q, k, thresh, exp = C.nn_thresh_case()
    assert np.array_equal(O.nn_search(q, k, thresh), exp)
    assert np.array_equal(_np(K.nn_search(t(q, dev), t(k, dev), thresh)), exp)


# ------------------------------------------------------------------ assignment
@pytest.mark.parametrize("name", sorted(C.assign_hand_cases()))
def test_nn_assign_hand_cases(dev, name):
    g, rep_nn, nq, exp = C.assign_hand_cases()[name]
    g = np.asarray(g, np.int32).reshape(-1, np.asarray(g).shape[-1])
    rep_nn = np.asarray(rep_nn, np.int32)
    assert O.nn_assign(g, rep_nn, nq).tolist() == exp
    assert _np(K.nn_assign(t(g, dev), t(rep_nn, dev), nq)).tolist() == exp


@pytest.mark.parametrize("m,ns", C.ASSIGN_RANDOM)
def test_nn_assign_random(dev, m, ns):
    g, rep_nn = C.assign_random_case(m, ns)
    assert (rep_nn < 0).any() and (rep_nn >= 0).any()
    exp = O.nn_assign(g, rep_nn, C.ASSIGN_NQ)
    assert (exp >= 0).any() and (exp < 0).any()
    assert np.array_equal(_np(K.nn_assign(t(g, dev), t(rep_nn, dev), C.ASSIGN_NQ)), exp)


# ------------------------------------------------------------------ the ragged one-call chain
def chain_run(dev, radius, max_cluster, quirks=False, n_pad=0):
    q, k = C.chain_batch()
    o2, o3, modes, bases, nq_max, nk_max = C.chain_desc_lists(q, k, 4, C.CHAIN_FPS_NUM, quirks)
    desc = K.gma_nn_chain_desc(o2, o3, modes, bases, dev)
    got = K.gma_nn_chain(t(q, dev), t(k, dev), desc, 4, t(C.chain_fps_rows(), dev),
                         C.CHAIN_FPS_NUM, nq_max, nk_max, C.THRESH, radius, max_cluster, n_pad)
    assert got.dtype == torch.long and tuple(got.shape) == (q.shape[0] + n_pad,)
    return _np(got)


@pytest.mark.parametrize("max_cluster", C.CHAIN_MAX_CLUSTER, ids=lambda v: "cap%d" % v)
@pytest.mark.parametrize("radius", C.CHAIN_RADII, ids=lambda r: "r%.7f" % r)
def test_chain_with_two_query_tiles(dev, radius, max_cluster):
    """fps_num = 1024: 700 DIRECT queries (a full tile of 512 with both query slots of a
    thread in use, and a partial one), 1024 representatives of 3000 and of 1100 queries (two
    full tiles, six ball trips), radius^2 at, above and beside an integer, and a cap that
    binds inside a trip while the ball goes on in a later one."""
    q, k = C.chain_batch()
    qs, ks = q[q[:, 0] == 2], k[k[:, 0] == 2]
    parts = {}
    C.oracle_fps_nn(qs, ks, C.CHAIN_FPS_NUM, radius, max_cluster, C.THRESH, parts)
    assert np.array_equal(parts["rep_idx"], C.chain_fps_rows()[2])
    fl = C.chain_cap_flags(qs[:, 1:], parts["rep_idx"], parts["rep_nn"], radius, max_cluster)
    assert fl["cap_in_group"] and fl["cap_in_trip"] and fl["later_trip"], fl
    exp = C.oracle_batch(q, k, 4, C.CHAIN_FPS_NUM, radius, max_cluster, C.THRESH, n_pad=3)
    for b, (some, none) in enumerate([(True, True), (False, True), (True, True), (True, True)]):
        rows = exp[:-3][q[:, 0] == b]
        assert (rows >= 0).any() == some and (rows < 0).any() == none, b
    got = chain_run(dev, radius, max_cluster, n_pad=3)
    for b in range(4):
        assert np.array_equal(got[:-3][q[:, 0] == b], exp[:-3][q[:, 0] == b]), b
    assert (got[-3:] == -1).all()


def test_chain_with_the_reference_bases(dev):
    q, k = C.chain_batch()
    cum = C.oracle_batch(q, k, 4, C.CHAIN_FPS_NUM, 6.0, 8, C.THRESH)
    ref = C.oracle_batch(q, k, 4, C.CHAIN_FPS_NUM, 6.0, 8, C.THRESH, quirks=True)
    assert not np.array_equal(cum, ref)
    assert np.array_equal(chain_run(dev, 6.0, 8), cum)
    assert np.array_equal(chain_run(dev, 6.0, 8, quirks=True), ref)
