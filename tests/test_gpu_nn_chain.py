"""The GMA neighbour search behind FPS as one ragged call (kernels.gma_nn_chain,
csrc/gma_nn.hip) against the oracle composed as the reference composes fps_NN_fast
(sparse_multimodal_encoder_painting.py:276-323, per sample :349-369).  The outputs are
integer row indices: everything is compared bit for bit."""
import numpy as np
import pytest
import torch

from msmdfusion_amd import kernels as K
from point_search_cases import (FPS_NUM, GRID, MAX_CLUSTER, RADIUS, THRESH, cloud, oracle_batch,
                                oracle_fps_nn, with_batch)

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def enc(dev):
    from msmdfusion_amd.multimodal_encoder import SparseMultiModalEncoderPaint
    return SparseMultiModalEncoderPaint(in_channels_2D=(64,) * 4, padding=(1, 1, [0, 1, 1], 0)).to(dev)


@pytest.fixture()
def calls(monkeypatch):
    """Counts the calls of the one-call entry: a test of it must not pass through the
    per-sample path, nor the fallback test through the entry."""
    seen = []
    real = K.gma_nn_chain

    def counted(*a, **kw):
        seen.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(K, "gma_nn_chain", counted)
    return seen


def run(enc, dev, q, k, batch, fps_num=FPS_NUM, radius=RADIUS, max_cluster=MAX_CLUSTER,
        thresh=THRESH, n_pad=0, bound=max(GRID)):
    got = enc.nearest_3d_of_only_2d(torch.from_numpy(q).to(dev), torch.from_numpy(k).to(dev), batch,
                                    fps_num, radius, max_cluster, thresh, coord_bound=bound,
                                    n_pad=n_pad)
    assert got.dtype == torch.long and got.shape == (q.shape[0] + n_pad,)
    return _np(got)


def ragged_batch():
    """(a) 700 queries / 1500 keys, clustered; (b) 40 / 900, direct; (c) no query;
    (d) 300 queries / no key.  (a)'s keys fill a corner of the grid only, so that some
    representatives find no key within the threshold."""
    q = np.concatenate([cloud(700, 0, 11), cloud(40, 1, 12), cloud(300, 3, 13)])
    k = np.concatenate([cloud(1500, 0, 21, extent=[41, 60, 60]), cloud(900, 1, 22),
                        cloud(500, 2, 23)])
    return q, k


def test_ragged_batch_with_every_mode(enc, dev, calls):
    q, k = ragged_batch()
    exp = oracle_batch(q, k, 4)
    parts = {}
    a = oracle_fps_nn(q[q[:, 0] == 0], k[k[:, 0] == 0], FPS_NUM, RADIUS, MAX_CLUSTER, THRESH, parts)
    assert (a >= 0).any() and (a < 0).any(), "sample (a) needs valid and unassigned rows"
    assert (parts["rep_nn"] < 0).any() and (parts["rep_nn"] >= 0).any(), "needs a dead representative"
    # the first-nsample cap binds: some ball holds more points than it may keep
    qa = q[q[:, 0] == 0][:, 1:].astype(np.int64)
    assert (((qa[:, None] - qa[None]) ** 2).sum(-1) < RADIUS ** 2).sum(1).max() > MAX_CLUSTER
    got = run(enc, dev, q, k, 4)
    assert calls == [1]
    for b in range(4):
        assert np.array_equal(got[q[:, 0] == b], exp[q[:, 0] == b]), b
    assert (got[q[:, 0] == 1] >= 1500).all() and (got[q[:, 0] == 3] == -1).all()
    old = enc._nearest_3d_per_sample(torch.from_numpy(q).to(dev), torch.from_numpy(k).to(dev), 4,
                                     FPS_NUM, RADIUS, MAX_CLUSTER, THRESH)
    assert np.array_equal(got, _np(old))


def filler(n, start):
    """n distinct keys far (> 100 voxels) from the queries of the edge tests."""
    i = np.arange(start, start + n)
    return np.stack([i % 40, 250 + i // 40, 300 + 0 * i], 1)


@pytest.mark.parametrize("nk", [K.NN_CHAIN_KEYS + 1, 2 * K.NN_CHAIN_KEYS])
def test_key_chunk_edges_and_ties(enc, dev, calls, nk):
    chunk = K.NN_CHAIN_KEYS
    keys = filler(nk, 0)
    queries = [(10, 50, 50), (10, 100, 100), (10, 150, 150)]
    keys[0] = (10, 50, 53)            # d2 = 9 from query 0 ...
    keys[chunk] = (10, 53, 50)        # ... and so is this one, in the second chunk: 0 wins
    for i, kz in zip((5, 100, 200), [(10, 100, 104), (10, 104, 100), (14, 100, 100)]):
        keys[i] = kz                  # three keys of one chunk at d2 = 16 from query 1: 5 wins
    keys[nk - 1] = (10, 150, 151) if nk - 1 != chunk else keys[nk - 1]   # the last key of all
    assert np.unique(keys, axis=0).shape[0] == nk
    q, k = with_batch(queries, 0), with_batch(keys, 0)
    exp = oracle_batch(q, k, 1, fps_num=2048)
    assert exp[0] == 0 and exp[1] == 5 and (exp[2] == nk - 1 or nk - 1 == chunk)
    got = run(enc, dev, q, k, 1, fps_num=2048, bound=512)
    assert calls == [1] and np.array_equal(got, exp)


def test_threshold_edge(enc, dev, calls):
    keys = filler(300, 0)
    keys[7] = (13, 54, 50)            # d2 = 25 from query 0: sqrt = 5.0 is not < 5.0
    keys[9] = (12, 102, 104)          # d2 = 24 from query 1
    q, k = with_batch([(10, 50, 50), (10, 100, 100)], 0), with_batch(keys, 0)
    exp = oracle_batch(q, k, 1, fps_num=2048, thresh=5.0)
    assert exp.tolist() == [-1, 9]
    got = run(enc, dev, q, k, 1, fps_num=2048, thresh=5.0, bound=512)
    assert calls == [1] and np.array_equal(got, exp)


def offsets_batch():
    q = np.concatenate([cloud(200, 0, 31), cloud(150, 1, 32), cloud(180, 2, 33)])
    k = np.concatenate([cloud(900, 0, 41), cloud(700, 1, 42), cloud(800, 2, 43)])
    return q, k


def test_cumulative_and_reference_offsets(enc, dev, calls):
    q, k = offsets_batch()
    cum, ref = oracle_batch(q, k, 3), oracle_batch(q, k, 3, quirks=True)
    rows2 = q[:, 0] == 2
    assert np.array_equal(cum[~rows2], ref[~rows2]) and not np.array_equal(cum[rows2], ref[rows2])
    assert np.array_equal(run(enc, dev, q, k, 3), cum)
    enc.reference_quirks = True
    try:
        assert np.array_equal(run(enc, dev, q, k, 3), ref)
    finally:
        enc.reference_quirks = False
    assert calls == [1, 1]


def test_pad_rows(enc, dev, calls):
    q, k = offsets_batch()
    exp = oracle_batch(q, k, 3, n_pad=2)
    got = run(enc, dev, q, k, 3, n_pad=2)
    assert calls == [1] and np.array_equal(got, exp) and (got[-2:] == -1).all()


def test_scratch_reuse_on_one_stream(enc, dev, calls):
    """A large problem, then a small one with other contents, back to back on one
    stream: the second result is right only if every call initialises its slots."""
    q, k = ragged_batch()
    q2 = np.concatenate([cloud(90, 0, 51), cloud(30, 1, 52)])
    k2 = np.concatenate([cloud(400, 0, 61, extent=[41, 60, 60]), cloud(300, 1, 62)])
    exp, exp2 = oracle_batch(q, k, 4), oracle_batch(q2, k2, 2)
    assert (exp2 >= 0).any() and (exp2 < 0).any()
    got = run(enc, dev, q, k, 4)
    got2 = run(enc, dev, q2, k2, 2)
    assert calls == [1, 1]
    assert np.array_equal(got, exp) and np.array_equal(got2, exp2)


def test_threshold_outside_the_precondition_takes_the_per_sample_path(enc, dev, calls):
    q, k = offsets_batch()
    exp = oracle_batch(q, k, 3, thresh=3000.0, n_pad=1)
    got = run(enc, dev, q, k, 3, thresh=3000.0, n_pad=1)
    assert calls == [] and np.array_equal(got, exp)
    assert (got >= 0).sum() > (oracle_batch(q, k, 3) >= 0).sum() and got[-1] == -1
