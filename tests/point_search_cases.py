"""Inputs of the neighbour-search tests (FPS, ball query, nearest key, assignment, the
ragged one-call chain), shared by tests/test_point_search_cpu.py and
tests/test_gpu_point_search.py so that both see identical data, and three restatements in
plain numpy float32 that do not go through the oracle's C: ball_query_np, nn_search_np and
fps_probe_refreshes (the hand-over rule of fps_pruned_kernel, csrc/points.hip).

Everything here is numpy only; the oracle is used where the issue is the oracle's own
sequence (the FPS samples of the probe model, the composition of fps_NN_fast)."""
import functools

import numpy as np

from msmdfusion_amd import synthetic as S
from oracle import oracle as O

F32 = np.float32


# ------------------------------------------------------------------ numpy restatements
def _d2_f32(c, xyz):
    """(cx-x)^2 + (cy-y)^2 + (cz-z)^2, every operation rounded to float32, left to right."""
    d = c[None].astype(F32) - xyz.astype(F32)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def ball_hits_np(min_r, max_r, xyz, centres):
    """Per centre the indices of all its hits, ascending: d2 == 0 or min_r^2 <= d2 < max_r^2."""
    lo, hi = F32(min_r) * F32(min_r), F32(max_r) * F32(max_r)
    out = []
    for c in np.asarray(centres, F32):
        d2 = _d2_f32(c, np.asarray(xyz, F32))
        out.append(np.flatnonzero((d2 == 0) | ((d2 >= lo) & (d2 < hi))))
    return out


def ball_query_np(min_r, max_r, nsample, xyz, centres):
    """One batch element: xyz [n,3], centres [m,3] -> [m,nsample] int32.  The first hit
    pre-fills the row, the first nsample hits follow in index order; no hit = zeros."""
    out = np.zeros((len(centres), nsample), np.int32)
    for row, h in zip(out, ball_hits_np(min_r, max_r, xyz, centres)):
        if h.size:
            row[:] = h[0]
            row[:min(h.size, nsample)] = h[:nsample]
    return out


def nn_search_np(q, k, thresh):
    """float32 sqrt of the float32 sum of squares, first minimum, -1 unless d < thresh."""
    q, k = np.asarray(q, np.int32).reshape(-1, 3), np.asarray(k, np.int32).reshape(-1, 3)
    out = np.full((q.shape[0],), -1, np.int32)
    if k.shape[0] == 0:
        return out
    kf = k.astype(F32)
    for i, qi in enumerate(q.astype(F32)):
        d = qi[None] - kf
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        assert dist.dtype == F32
        j = int(np.argmin(dist))
        if dist[j] < F32(thresh):
            out[i] = j
    return out


FPS_BUCKET = 256                 # points.hip: 64 lanes x kFpsSlotsPerBucket
FPS_PROBE0, FPS_PROBE1 = 32, 96  # points.hip: kFpsProbe0, kFpsProbe1
FPS_PRUNED_MIN_N, FPS_PRUNED_MAX_N, FPS_PRUNED_MIN_M = 6144, 48 * 512, 2 * FPS_PROBE1 + 1


def fps_probe_refreshes(points, m):
    """The hand-over rule of fps_pruned_kernel, from its comment: buckets of 256 consecutive
    points; in round j the previous sample refreshes a bucket when the float32 distance from
    it to the bucket's bounding box is below the bucket's largest running distance before
    the round; the refreshes of rounds 33..95 are counted and the element is handed to the
    plain kernel when 2 * count > nbuckets * 64.  -> (count, nbuckets, hands_over).
    The sample sequence is the oracle's (the kernel's, if the kernel is right).  The kernel
    probes only when m > 192."""
    p = np.ascontiguousarray(points, F32)
    n = p.shape[0]
    nb = -(-n // FPS_BUCKET)
    if m < FPS_PRUNED_MIN_M:
        return 0, nb, False
    idx = O.furthest_point_sample(p[None], FPS_PROBE1)[0]
    pad = nb * FPS_BUCKET - n
    lo = np.concatenate([p, np.full((pad, 3), np.inf, F32)]).reshape(nb, FPS_BUCKET, 3).min(1)
    hi = np.concatenate([p, np.full((pad, 3), -np.inf, F32)]).reshape(nb, FPS_BUCKET, 3).max(1)
    run = np.full((n,), 1e10, F32)
    count = 0
    for j in range(1, FPS_PROBE1):
        s = p[idx[j - 1]]
        if j > FPS_PROBE0:
            e = np.maximum(np.maximum(lo - s[None], s[None] - hi), F32(0))
            bound = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            top = np.concatenate([run, np.full((pad,), -1, F32)]).reshape(nb, FPS_BUCKET).max(1)
            count += int((bound < top).sum())
        run = np.minimum(_d2_f32(s, p), run)
    return count, nb, 2 * count > nb * (FPS_PROBE1 - FPS_PROBE0)


def fps_probe_margin_ok(count, nb, hands_over):
    """A factor 2 to spare on the input's side of the threshold nb * 32.  Below it: twice the
    count still does not hand over.  Above it the count itself cannot double (at most 63
    refreshes per bucket against a threshold of 32), so the spare is measured in what the
    pruning saved: twice the skipped refreshes still hand over."""
    rounds = FPS_PROBE1 - FPS_PROBE0 - 1          # 33..95
    limit = nb * (FPS_PROBE1 - FPS_PROBE0)        # hands over when 2 * count > limit
    if hands_over:
        skipped = nb * rounds - count
        return 2 * (nb * rounds - 2 * skipped) > limit
    return 2 * (2 * count) <= limit


# ------------------------------------------------------------------ FPS inputs
def fps_instantiation(n_max, m):
    """The kernel launch_fps (points.hip) picks, as the ids of the FPS cases name it."""
    ppl = -(-n_max // 512)
    if n_max >= FPS_PRUNED_MIN_N and ppl <= 48 and m >= FPS_PRUNED_MIN_M:
        return "pruned%d" % (16 if ppl <= 16 else 32 if ppl <= 32 else 48)
    ppt = -(-n_max // 1024)
    for p in (2, 4, 8, 16, 20, 22, 24):
        if ppt <= p:
            return "plain%d" % p
    return "plain0"


FPS_PLAIN_N = [2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 20480, 20481, 22528, 22529,
               24576, 24577]
FPS_PLAIN_M = 40
FPS_SMALL = [(1, 1), (1, 5), (2, 2), (2, 4), (3, 3), (3, 7), (63, 40), (64, 40), (65, 40),
             (1023, 40), (1024, 40), (1025, 40)]
FPS_PRUNED_N = [6144, 8192, 8193, 16384, 16385, 24576]
FPS_PRUNED_M = [193, 260]
FPS_NEIGHBOURS = [(6143, 260), (8192, 192), (24577, 260)]
FPS_RAGGED_SIZES = [7000, 0, 1, 300, 24576]
FPS_RAGGED_ORDER = ["coherent", None, None, None, "permuted"]
FPS_RAGGED_M = 260


def fps_cloud(n, kind, seed):
    """[n,3] float32: small-integer voxel coordinates (ties dominate) or non-integer ones."""
    rng = np.random.RandomState(seed)
    if kind == "int":
        return np.stack([rng.randint(0, 41, n), rng.randint(0, 200, n), rng.randint(0, 200, n)],
                        -1).astype(F32)
    assert kind == "float"
    return (rng.rand(n, 3) * [41.0, 200.0, 200.0]).astype(F32)


def fps_line(n, kind, seed, order):
    """Points along a line, 0.5 apart, with jitter in the other two axes: in index order the
    buckets are short segments (the pruning pays), permuted every bucket spans the line (the
    kernel hands over).  kind "int": four points per integer x, integer jitter -- ties."""
    rng = np.random.RandomState(seed)
    i = np.arange(n)
    if kind == "int":
        p = np.stack([i // 4, rng.randint(0, 4, n), rng.randint(0, 4, n)], -1).astype(F32)
    else:
        assert kind == "float"
        p = np.stack([0.5 * i, rng.rand(n) * 2.0, rng.rand(n) * 2.0], -1).astype(F32)
    if order == "permuted":
        p = p[rng.permutation(n)]
    else:
        assert order == "coherent"
    return np.ascontiguousarray(p)


def fps_ragged_parts():
    parts = []
    for i, (n, order) in enumerate(zip(FPS_RAGGED_SIZES, FPS_RAGGED_ORDER)):
        parts.append(fps_line(n, "float", 70 + i, order) if order else fps_cloud(n, "int", 70 + i))
    return parts


# ------------------------------------------------------------------ ball query inputs
BALL_NM = [(1, 1), (63, 3), (64, 4), (65, 5), (333, 10), (1000, 7)]
BALL_NSAMPLE = [1, 3, 64, 65, 130]
BALL_RADII = [(0.0, 4.0), (2.0, 6.0), (0.0, 1.0)]
BALL_GRID = {333: (6, 30, 30), 1000: (6, 20, 20)}    # 1000 points: dense, balls above 130 rows


def ball_case(n, m, kind="int", seed=0):
    """-> xyz [2,n,3], centres [2,m,3] float32, two different elements.  The cloud is n
    distinct cells of a 6x30x30 grid (6x20x20 for the 1000 points); element 0 is sorted along y (centres deep in the cloud
    have their first hit late), element 1 is in random order.  Centre i of element e is, by
    (i + e) mod 3: a point of the cloud; a point 100 units from one (no hit: a zeros row);
    a point one cell beside one (any distance, usually not a cloud point).  The last centre
    of element 0 is the LAST point of its cloud (first hit >= 64 under radius 1)."""
    rng = np.random.RandomState(1000 * n + m + seed)
    d, h, w = BALL_GRID.get(n, BALL_GRID[333])
    xyz, cen = [], []
    for e in range(2):
        lin = rng.permutation(d * h * w)[:n]
        p = np.stack([lin // (h * w), (lin // w) % h, lin % w], -1).astype(F32)
        if kind == "float":
            p = (p * F32(0.7) + rng.rand(n, 3).astype(F32) * F32(0.3)).astype(F32)
        if e == 0:
            p = p[np.argsort(p[:, 1], kind="stable")]
        c = p[rng.randint(0, n, m)].copy()
        for i in range(m):
            how = (i + e) % 3
            if how == 1:
                c[i, 2] += 100
            elif how == 2:
                c[i, 1] += 1
        if e == 0 and m >= 3:
            c[m - 1] = p[n - 1]
        xyz.append(p)
        cen.append(c)
    return np.stack(xyz), np.stack(cen)


def ball_flags(hits, nsample):
    """What the hit lists of one call exercise (hits: ball_hits_np of every centre)."""
    full = [h for h in hits if h.size >= nsample]
    return {
        "overfull": any(h.size > nsample for h in hits),
        "underfull": any(0 < h.size < nsample for h in hits),
        "empty": any(h.size == 0 for h in hits),
        "late_first": any(h.size and h[0] >= 64 for h in hits),
        "cap_mid_group": any(h[nsample - 1] % 64 not in (0, 63) for h in full),
    }


@functools.lru_cache(maxsize=None)
def ball_family_flags(kind="int"):
    """{(n, m, radii, nsample): flags} over the whole family, both elements pooled."""
    out = {}
    for n, m in BALL_NM:
        xyz, cen = ball_case(n, m, kind)
        for radii in BALL_RADII:
            hits = ball_hits_np(radii[0], radii[1], xyz[0], cen[0]) + \
                ball_hits_np(radii[0], radii[1], xyz[1], cen[1])
            for ns in BALL_NSAMPLE:
                out[(n, m, radii, ns)] = ball_flags(hits, ns)
    return out


def check_ball_family(kind="int"):
    """Asserts that the family reaches every edge it is there for."""
    fam = ball_family_flags(kind)
    for ns in BALL_NSAMPLE:
        some = lambda f: [key for key, fl in fam.items() if key[3] == ns and fl[f]]
        assert some("overfull"), ns
        assert some("underfull") or ns == 1, ns
        assert some("cap_mid_group"), ns
        assert some("late_first") and some("empty"), ns
        # first hit past the first group under a min_radius > 0 too
        assert any(key[2][0] > 0 for key in some("late_first")), ns
    # n = 333: both sides of the cap at a middle nsample, the issue's own check
    assert fam[(333, 10, (0.0, 4.0), 3)]["overfull"] and fam[(333, 10, (0.0, 4.0), 64)]["underfull"]
    # every case has a centre without a hit (with one centre per element: element 1's)
    assert all(fl["empty"] for key, fl in fam.items())


# ------------------------------------------------------------------ nearest key inputs
NN_NQ = [0, 1, 255, 256, 257]
NN_NK = [0, 1, 1023, 1024, 1025, 2049]
NN_EXTENT = (41, 1440, 1440)
NN_THRESH = 13.3


def nn_case(nq, nk, seed=0):
    """Random keys over the whole extent; every other query sits within a few cells of a key
    (found), the rest anywhere (mostly nothing within the threshold)."""
    rng = np.random.RandomState(7 * nq + 13 * nk + seed)
    ext = np.array(NN_EXTENT)
    k = (rng.rand(nk, 3) * ext).astype(np.int32)
    q = (rng.rand(nq, 3) * ext).astype(np.int32)
    if nk:
        near = k[rng.randint(0, nk, nq)] + rng.randint(-4, 5, (nq, 3))
        near = np.clip(near, 0, ext - 1).astype(np.int32)
        q[::2] = near[::2]
    if nq:
        q[-1] = ext - 1            # the far corner: coordinates up to (40, 1439, 1439)
    return q, k


def nn_filler(n, start=0):
    """n distinct keys far (> 100 cells) from the queries of the constructed cases."""
    i = np.arange(start, start + n)
    return np.stack([i % 40, 700 + i // 40, 900 + 0 * i], 1).astype(np.int32)


def nn_tie_case():
    """-> q, k, expected.  Query 0: keys 1023 and 1024 (last of chunk 0, first of chunk 1)
    at d2 = 9, the lower index wins across chunks.  Query 1: keys 1100, 1500, 1900 of one
    chunk at d2 = 16: 1100.  Query 2: the very last key.  Query 3: nothing near."""
    nk = 2049
    k = nn_filler(nk)
    k[1023], k[1024] = (10, 50, 53), (10, 53, 50)
    k[1100], k[1500], k[1900] = (10, 100, 104), (10, 104, 100), (14, 100, 100)
    k[nk - 1] = (10, 150, 151)
    assert np.unique(k, axis=0).shape[0] == nk
    q = np.array([(10, 50, 50), (10, 100, 100), (10, 150, 150), (10, 300, 300)], np.int32)
    return q, k, np.array([1023, 1100, nk - 1, -1], np.int32)


def nn_thresh_case():
    """-> q, k, thresh, expected: d == thresh is not a hit (d2 = 25 at thresh 5), the next
    smaller d2 = 24 is."""
    k = nn_filler(300)
    k[7] = (13, 54, 50)
    k[9] = (12, 102, 104)
    q = np.array([(10, 50, 50), (10, 100, 100)], np.int32)
    return q, k, 5.0, np.array([-1, 9], np.int32)


# ------------------------------------------------------------------ assignment inputs
def assign_hand_cases():
    """name -> (group_idx [m,ns], rep_nn [m], nq, expected [nq])."""
    e = np.zeros((0, 3), np.int32)
    return {
        "higher-valid-wins": ([[0, 1, 2], [2, 3, 3]], [10, 20], 5, [10, 10, 20, 20, -1]),
        "higher-dead-assigns-nothing": ([[0, 1, 2], [2, 3, 3]], [10, -1], 5, [10, 10, 10, -1, -1]),
        "lower-dead": ([[0, 1, 2], [2, 3, 3]], [-1, 20], 5, [-1, -1, 20, 20, -1]),
        "no-ball": ([[1, 1, 1]], [7], 3, [-1, 7, -1]),
        "m0": (e, np.zeros((0,), np.int32), 4, [-1, -1, -1, -1]),
        "prefill-duplicates": ([[4, 4, 4, 4], [4, 0, 4, 4], [1, 1, 1, 1]], [5, 6, -1],
                               6, [6, -1, -1, -1, 6, -1]),
    }


ASSIGN_RANDOM = [(300, 1), (31, 8), (300, 65)]
ASSIGN_NQ = 5000


def assign_random_case(m, ns):
    """Rows as ball_query leaves them: `c` hits then the first hit repeated."""
    rng = np.random.RandomState(100 * m + ns)
    g = np.zeros((m, ns), np.int32)
    for r in range(m):
        c = rng.randint(1, ns + 1)
        h = np.sort(rng.choice(ASSIGN_NQ, c, replace=False))
        g[r] = h[0]
        g[r, :c] = h
    rep_nn = rng.randint(-1, 500, m).astype(np.int32)
    rep_nn[rng.rand(m) < 0.2] = -1            # one representative in five is dead
    return g, rep_nn


# ------------------------------------------------------------------ fps_NN_fast, composed
GRID = [41, 120, 120]
FPS_NUM, RADIUS, MAX_CLUSTER, THRESH = 64, 6, 8, 13.3


def oracle_fps_nn(query, key, fps_num, radius, max_cluster, thresh, parts=None):
    """fps_NN_fast (sparse_multimodal_encoder_painting.py:276-323) with oracle pieces, as
    tests/test_gpu_fusion.py composes it."""
    nq = query.shape[0]
    if nq <= fps_num:
        return O.nn_search(query[:, 1:], key[:, 1:], thresh)
    q = query[:, 1:].astype(np.float32)[None]
    rep_idx = O.furthest_point_sample(q, fps_num)[0]
    rep = query[rep_idx, 1:]
    rep_nn = O.nn_search(rep, key[:, 1:], thresh)
    grp = O.ball_query(0, radius, max_cluster, q, rep.astype(np.float32)[None])[0]
    if parts is not None:
        parts.update(rep_idx=rep_idx, rep_nn=rep_nn, grp=grp)
    return O.nn_assign(grp, rep_nn, nq)


def oracle_batch(q, k, batch, fps_num=FPS_NUM, radius=RADIUS, max_cluster=MAX_CLUSTER,
                 thresh=THRESH, quirks=False, n_pad=0):
    """The per-sample loop of grouped_sparse_conv (:349-369): cumulative bases, or the
    reference's own (the previous sample's count) with quirks."""
    out = np.full((q.shape[0] + n_pad,), -1, np.int64)
    c3 = [int((k[:, 0] == b).sum()) for b in range(batch)]
    o3 = np.cumsum([0] + c3)
    for b in range(batch):
        rows = np.flatnonzero(q[:, 0] == b)
        kb = k[k[:, 0] == b]
        if rows.size == 0 or kb.shape[0] == 0:
            continue
        nn = oracle_fps_nn(q[rows], kb, fps_num, radius, max_cluster, thresh).astype(np.int64)
        base = (c3[b - 1] if b else 0) if quirks else o3[b]
        out[rows] = np.where(nn >= 0, nn + base, nn)
    return out


def with_batch(zyx, b):
    zyx = np.asarray(zyx, np.int32).reshape(-1, 3)
    return np.concatenate([np.full((zyx.shape[0], 1), b, np.int32), zyx], 1)


def cloud(n, b, seed, extent=GRID, clustered=True):
    rows = S.random_voxel_indices(n, 1, extent, seed=seed, clustered=clustered)
    assert rows.shape[0] == n
    rows[:, 0] = b
    return rows


# ------------------------------------------------------------------ the chain, called directly
CHAIN_FPS_NUM = 1024
# float32 radius^2: 36, 42.25, 6.25, exactly 20 (float32(sqrt 20)^2 rounds to it), and the
# float32 neighbours of sqrt 20 on both sides: 19.999996 and 20.000004
_R20 = np.float32(np.sqrt(20.0))
CHAIN_RADII = [6.0, 6.5, 2.5, float(np.sqrt(20.0)), float(np.nextafter(_R20, F32(0))),
               float(np.nextafter(_R20, F32(9)))]
CHAIN_MAX_CLUSTER = [1, 8, 70]
CHAIN_TILE, CHAIN_TRIP, CHAIN_GROUP = 512, 512, 64     # gma_nn.hip: kChainTile, 64*kBallUnroll


@functools.lru_cache(maxsize=None)
def chain_batch():
    """-> q [n,4], k [nk,4] (b,z,y,x) int32, four samples.
    0: 700 queries / 1500 keys, DIRECT at fps_num 1024 (two query tiles, the second partial).
    1: 50 queries / no key: SKIP.
    2: 3000 queries / 1300 keys, CLUSTERED: 952 clustered rows and a full 8x16x16 block of
       2048, all in random row order -- balls of up to 81 rows at radius 2.5, spread over the
       six trips of 512 rows.
    3: 1100 queries / 600 keys in one corner of the grid: dead representatives."""
    rng = np.random.RandomState(5)
    lo, ext = np.array([16, 50, 60]), np.array([8, 16, 16])
    blk = np.stack(np.meshgrid(*[np.arange(e) for e in ext], indexing="ij"), -1).reshape(-1, 3) + lo
    rest = cloud(2000, 2, 14)[:, 1:]
    inside = ((rest >= lo) & (rest < lo + ext)).all(1)
    s2 = np.concatenate([rest[~inside][:3000 - blk.shape[0]], blk])
    assert s2.shape[0] == 3000 and np.unique(s2, axis=0).shape[0] == 3000
    s2 = with_batch(s2[rng.permutation(3000)], 2)
    q = np.concatenate([cloud(700, 0, 11), cloud(50, 1, 12), s2, cloud(1100, 3, 13)])
    k = np.concatenate([cloud(1500, 0, 21), cloud(1300, 2, 22),
                        cloud(600, 3, 23, extent=[41, 60, 60])])
    q.setflags(write=False)
    k.setflags(write=False)
    return q, k


def chain_desc_lists(q, k, batch, fps_num, quirks=False):
    """The descriptor of msmd_gma_nn_chain, by hand: query offsets, key offsets, modes
    (0 SKIP, 1 DIRECT, 2 CLUSTERED), bases; and nq_max, nk_max."""
    c2 = [int((q[:, 0] == b).sum()) for b in range(batch)]
    c3 = [int((k[:, 0] == b).sum()) for b in range(batch)]
    o2, o3 = np.cumsum([0] + c2).tolist(), np.cumsum([0] + c3).tolist()
    modes = [0 if not (c2[b] and c3[b]) else 1 if c2[b] <= fps_num else 2 for b in range(batch)]
    bases = [(c3[b - 1] if b else 0) if quirks else o3[b] for b in range(batch)]
    nq_max = max([fps_num if m == 2 else c2[b] if m == 1 else 0 for b, m in enumerate(modes)])
    nk_max = max([c3[b] if m else 0 for b, m in enumerate(modes)])
    return o2, o3, modes, bases, nq_max, nk_max


@functools.lru_cache(maxsize=None)
def chain_fps_rows(fps_num=CHAIN_FPS_NUM):
    """int32 [4, fps_num]: the oracle's representatives of the CLUSTERED samples, zeros
    elsewhere -- the chain is tested on its own, behind a known FPS."""
    q, k = chain_batch()
    _, _, modes, _, _, _ = chain_desc_lists(q, k, 4, fps_num)
    out = np.zeros((4, fps_num), np.int32)
    for b, mode in enumerate(modes):
        if mode == 2:
            out[b] = O.furthest_point_sample(q[q[:, 0] == b][None, :, 1:].astype(F32), fps_num)[0]
    out.setflags(write=False)
    return out


def chain_cap_flags(qs, rep_idx, rep_nn, radius, nsample):
    """For the rows `qs` [n,3] of one CLUSTERED sample: is there a live representative
    (rep_nn >= 0) whose ball (d2 < float32 radius^2) ...
    cap_in_group: has its nsample-th and (nsample+1)-th member in one group of 64 rows;
    cap_in_trip:  has them in one trip of 512 rows but in different groups;
    later_trip:   has its nsample-th member in one trip and further members in a later one."""
    r2 = F32(radius) * F32(radius)
    q64 = qs.astype(np.int64)
    flags = dict(cap_in_group=False, cap_in_trip=False, later_trip=False)
    for r in np.flatnonzero(rep_nn >= 0):
        d2 = ((q64 - q64[rep_idx[r]]) ** 2).sum(1)
        h = np.flatnonzero(d2.astype(F32) < r2)
        if h.size <= nsample:
            continue
        a, b = h[nsample - 1], h[nsample]
        flags["cap_in_group"] |= a // CHAIN_GROUP == b // CHAIN_GROUP
        flags["cap_in_trip"] |= a // CHAIN_TRIP == b // CHAIN_TRIP and a // CHAIN_GROUP != b // CHAIN_GROUP
        flags["later_trip"] |= h[-1] // CHAIN_TRIP > a // CHAIN_TRIP
    return flags
