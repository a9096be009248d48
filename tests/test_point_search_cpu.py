"""The references of tests/test_gpu_point_search.py, pinned before they are used as such:
the oracle's ball query and nearest key equal plain numpy restatements on every case of the
GPU test, the hand-built cases have the properties they are named for, and the model of the
pruned FPS kernel's hand-over rule puts every pruned input on its side of the threshold
with a factor 2 to spare.  No GPU."""
import numpy as np
import pytest

import point_search_cases as C
from oracle import oracle as O


# ------------------------------------------------------------------ ball query
@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("n,m", C.BALL_NM)
def test_oracle_ball_query_equals_numpy(n, m, kind):
    xyz, cen = C.ball_case(n, m, kind)
    assert not np.array_equal(xyz[0], xyz[1])
    for lo, hi in C.BALL_RADII:
        for ns in C.BALL_NSAMPLE:
            exp = np.stack([C.ball_query_np(lo, hi, ns, xyz[e], cen[e]) for e in range(2)])
            assert np.array_equal(O.ball_query(lo, hi, ns, xyz, cen), exp), (lo, hi, ns)


def test_ball_query_np_known_rows():
    """The restatement itself, on rows worked out by hand (d2 to the centre (0,0,0):
    0, 1, 4, 9, 25, 4)."""
    xyz = np.array([(0, 0, 0), (1, 0, 0), (0, 2, 0), (0, 0, 3), (0, 3, 4), (2, 0, 0)], np.float32)
    cen = np.array([(0, 0, 0), (50, 0, 0)], np.float32)
    assert C.ball_query_np(0, 3, 4, xyz, cen).tolist() == [[0, 1, 2, 5], [0, 0, 0, 0]]
    # d2 == min_r^2 is a hit, d2 == max_r^2 is not, and d2 == 0 is one whatever min_r is
    assert C.ball_query_np(2, 5, 5, xyz, cen).tolist() == [[0, 2, 3, 5, 0], [0, 0, 0, 0, 0]]
    assert C.ball_query_np(2, 5, 2, xyz[1:], cen).tolist() == [[1, 2], [0, 0]]


@pytest.mark.parametrize("kind", ["int", "float"])
def test_ball_family_exercises_every_edge(kind):
    """What the family is for, asserted on the inputs so that a change of them cannot lose
    it: per nsample, a centre with more hits and one with fewer; a row of zeros; a first hit
    outside the first group of 64; the nsample-th hit strictly inside a group of 64."""
    C.check_ball_family(kind)


def test_ball_case_min_radius_keeps_the_centre_itself():
    """min_radius > 0 with a centre equal to a cloud point: d2 == 0 is a hit although it is
    below min_radius^2, and it is the only hit below it."""
    xyz, cen = C.ball_case(333, 10)
    seen = 0
    for e in range(2):
        for c, h in zip(cen[e], C.ball_hits_np(2.0, 6.0, xyz[e], cen[e])):
            d2 = ((xyz[e][h] - c) ** 2).sum(1)
            own = np.flatnonzero((xyz[e] == c).all(1))
            if own.size:
                assert own[0] in h and (d2 == 0).sum() == 1 and ((d2 == 0) | (d2 >= 4)).all()
                seen += 1
    assert seen >= 4


# ------------------------------------------------------------------ nearest key
@pytest.mark.parametrize("nk", C.NN_NK)
@pytest.mark.parametrize("nq", C.NN_NQ)
def test_oracle_nn_search_equals_numpy(nq, nk):
    q, k = C.nn_case(nq, nk)
    exp = C.nn_search_np(q, k, C.NN_THRESH)
    got = O.nn_search(q, k, C.NN_THRESH)
    assert got.shape == (nq,) and np.array_equal(got, exp)
    if nk == 0:
        assert (got == -1).all()
    elif nq >= 255:
        assert (got >= 0).sum() >= nq // 2 and (got < 0).any()
        assert nk < 2049 or ((got >= 1024).any() and (got < 1024).any())   # winners in two chunks


def test_nn_constructed_cases():
    q, k, exp = C.nn_tie_case()
    d2 = ((q[:, None].astype(np.int64) - k[None]) ** 2).sum(-1)
    assert d2[0, 1023] == d2[0, 1024] == d2[0].min() == 9
    assert d2[1, 1100] == d2[1, 1500] == d2[1, 1900] == d2[1].min() == 16
    assert np.array_equal(C.nn_search_np(q, k, C.NN_THRESH), exp)
    assert np.array_equal(O.nn_search(q, k, C.NN_THRESH), exp)
    q, k, thresh, exp = C.nn_thresh_case()
    d2 = ((q[:, None].astype(np.int64) - k[None]) ** 2).sum(-1)
    assert d2[0].min() == 25 and d2[1].min() == 24 and thresh * thresh == 25
    assert np.array_equal(C.nn_search_np(q, k, thresh), exp)
    assert np.array_equal(O.nn_search(q, k, thresh), exp)


# ------------------------------------------------------------------ assignment
@pytest.mark.parametrize("name", sorted(C.assign_hand_cases()))
def test_oracle_nn_assign_hand_cases(name):
    g, rep_nn, nq, exp = C.assign_hand_cases()[name]
    g = np.asarray(g, np.int32).reshape(-1, np.asarray(g).shape[-1])
    assert O.nn_assign(g, np.asarray(rep_nn, np.int32), nq).tolist() == exp


@pytest.mark.parametrize("m,ns", C.ASSIGN_RANDOM)
def test_assign_random_cases_cover_the_rule(m, ns):
    g, rep_nn = C.assign_random_case(m, ns)
    assert (rep_nn < 0).any() and (rep_nn >= 0).any() and g.min() >= 0 and g.max() < C.ASSIGN_NQ
    # the highest valid representative wins, restated: walk the representatives downwards
    exp = np.full((C.ASSIGN_NQ,), -1, np.int32)
    for r in range(m - 1, -1, -1):
        if rep_nn[r] >= 0:
            rows = g[r][exp[g[r]] == -1]
            exp[rows] = rep_nn[r]
    assert np.array_equal(O.nn_assign(g, rep_nn, C.ASSIGN_NQ), exp)
    if (m, ns) == (300, 65):
        # a point whose highest ball is dead and which a lower, live one assigns
        top = np.full((C.ASSIGN_NQ,), -1)
        for r in range(m):
            top[g[r]] = r
        assert ((top >= 0) & (rep_nn[top] < 0) & (exp >= 0)).any()


# ------------------------------------------------------------------ FPS hand-over model
def test_probe_model_on_the_line():
    """7 000 points on a line: far below the threshold in index order, every bucket in
    every round (63 rounds x 28 buckets) after a permutation."""
    for order, want in (("coherent", False), ("permuted", True)):
        count, nb, over = C.fps_probe_refreshes(C.fps_line(7000, "float", 0, order), 260)
        assert nb == 28 and over is want and C.fps_probe_margin_ok(count, nb, over), (order, count)
        assert count < 28 * 8 if order == "coherent" else count > 28 * 56
    assert C.fps_probe_refreshes(C.fps_line(7000, "float", 0, "permuted"), 192)[2] is False


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("n", C.FPS_PRUNED_N)
def test_probe_model_classifies_every_pruned_input(n, kind):
    for order in ("coherent", "permuted"):
        for seed in (0, 1):
            count, nb, over = C.fps_probe_refreshes(C.fps_line(n, kind, seed, order), 260)
            assert over is (order == "permuted"), (order, count, nb)
            assert C.fps_probe_margin_ok(count, nb, over), (order, count, nb)


def test_probe_model_classifies_the_ragged_elements():
    parts = C.fps_ragged_parts()
    assert [p.shape[0] for p in parts] == C.FPS_RAGGED_SIZES
    for p, order in zip(parts, C.FPS_RAGGED_ORDER):
        if order:
            count, nb, over = C.fps_probe_refreshes(p, C.FPS_RAGGED_M)
            assert over is (order == "permuted") and C.fps_probe_margin_ok(count, nb, over)


def test_fps_instantiation_names():
    """The ids of the FPS cases name all eleven instantiations."""
    names = {C.fps_instantiation(n, C.FPS_PLAIN_M) for n in C.FPS_PLAIN_N}
    assert names == {"plain%d" % p for p in (2, 4, 8, 16, 20, 22, 24, 0)}
    assert [C.fps_instantiation(n, 193) for n in C.FPS_PRUNED_N] == \
        ["pruned16", "pruned16", "pruned32", "pruned32", "pruned48", "pruned48"]
    assert [C.fps_instantiation(n, m) for n, m in C.FPS_NEIGHBOURS] == ["plain8", "plain8", "plain0"]
    assert C.fps_instantiation(max(C.FPS_RAGGED_SIZES), C.FPS_RAGGED_M) == "pruned48"


def test_oracle_fps_more_samples_than_points():
    """The reference's loop keeps selecting index 0 once every point is taken."""
    assert O.furthest_point_sample(C.fps_cloud(3, "float", 1)[None], 7)[0].tolist()[3:] == [0] * 4
    assert O.furthest_point_sample(C.fps_cloud(1, "int", 1)[None], 5)[0].tolist() == [0] * 5


# ------------------------------------------------------------------ the chain's batch
def test_chain_batch_has_the_shape_it_is_named_for():
    q, k = C.chain_batch()
    o2, o3, modes, bases, nq_max, nk_max = C.chain_desc_lists(q, k, 4, C.CHAIN_FPS_NUM)
    assert np.diff(o2).tolist() == [700, 50, 3000, 1100] and np.diff(o3).tolist() == [1500, 0, 1300, 600]
    assert modes == [1, 0, 2, 2] and bases == [0, 1500, 1500, 2800] and (nq_max, nk_max) == (1024, 1500)
    assert C.chain_desc_lists(q, k, 4, C.CHAIN_FPS_NUM, quirks=True)[3] == [0, 1500, 0, 1300]
    assert 700 > C.CHAIN_TILE and 0 < 700 % C.CHAIN_TILE < 256     # full tile + partial one
    assert -(-3000 // C.CHAIN_TRIP) == 6


@pytest.mark.parametrize("radius", C.CHAIN_RADII, ids=lambda r: "r%.3f" % r)
def test_chain_batch_makes_the_cap_bind_inside_a_trip(radius):
    """Per radius and cap: a live representative whose ball is cut inside a group of 64 rows,
    one cut between two groups of a trip, and one with further members in a later trip; and
    sample 3 has dead and live representatives."""
    q, k = C.chain_batch()
    r2 = np.float32(radius) * np.float32(radius)
    assert r2 in (36, 42.25, 6.25, 20) or 0 < abs(float(r2) - 20) < 1e-5
    for ns in C.CHAIN_MAX_CLUSTER:
        parts = {}
        qs, ks = q[q[:, 0] == 2], k[k[:, 0] == 2]
        C.oracle_fps_nn(qs, ks, C.CHAIN_FPS_NUM, radius, ns, C.THRESH, parts)
        assert np.array_equal(parts["rep_idx"], C.chain_fps_rows()[2])
        fl = C.chain_cap_flags(qs[:, 1:], parts["rep_idx"], parts["rep_nn"], radius, ns)
        assert fl["cap_in_group"] and fl["cap_in_trip"] and fl["later_trip"], (ns, fl)
    parts = {}
    C.oracle_fps_nn(q[q[:, 0] == 3], k[k[:, 0] == 3], C.CHAIN_FPS_NUM, radius, 8, C.THRESH, parts)
    assert (parts["rep_nn"] < 0).any() and (parts["rep_nn"] >= 0).any()
