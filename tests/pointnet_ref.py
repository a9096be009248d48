"""numpy float32 restatement of the PointNet++ ops (helper, not a test module): the operation
order csrc/pointnet.hip documents, so GPU results can be compared bit for bit.

    gather / group      plain indexing
    three_nn            d = (dx*dx + dy*dy) + dz*dz, the three smallest by (d, index)
    three_interpolate   (w0*f0 + w1*f1) + w2*f2
    knn                 lexicographic (d2, index) sort, first k
    fps_with_dist       running minimum against row `old`; ties by the reference block
                        reduction's order (bit-reversed k mod block, then k div block)
    scatter_bwd         the backward of gather / group / three_interpolate: a loop over the
                        destinations in ascending position, adding w * g to the source's
                        float32 accumulator with a Kahan compensation term
"""
import numpy as np

F32 = np.float32


def gather_points(feat, idx):
    """feat (B, C, N), idx (B, M) -> (B, C, M)."""
    return np.stack([feat[b][:, idx[b]] for b in range(feat.shape[0])])


def group_points(feat, idx):
    """feat (B, C, N), idx (B, P, S) -> (B, C, P, S)."""
    b, p, s = idx.shape
    return gather_points(feat, idx.reshape(b, p * s)).reshape(b, feat.shape[1], p, s)


def sq_dist(a, b):
    """a (n, 3), b (m, 3) float32 -> (n, m) float32, (dx*dx + dy*dy) + dz*dz."""
    a, b = a.astype(F32), b.astype(F32)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def three_nn(unknown, known):
    """unknown (B, N, 3), known (B, M, 3) -> SQUARED dist (B, N, 3) float32, idx int32."""
    bsz, n, _ = unknown.shape
    m = known.shape[1]
    dist = np.full((bsz, n, 3), np.inf, F32)
    idx = np.zeros((bsz, n, 3), np.int32)
    for b in range(bsz):
        if m == 0:
            continue
        d = sq_dist(unknown[b], known[b])
        order = np.argsort(d, axis=1, kind="stable")[:, :3]
        t = order.shape[1]
        idx[b, :, :t] = order
        dist[b, :, :t] = np.take_along_axis(d, order, axis=1)
    return dist, idx


def three_interpolate(feat, idx, weight):
    """feat (B, C, M), idx / weight (B, N, 3) -> (B, C, N)."""
    out = []
    for b in range(feat.shape[0]):
        f = feat[b].astype(F32)
        w = weight[b].astype(F32)
        f0, f1, f2 = f[:, idx[b, :, 0]], f[:, idx[b, :, 1]], f[:, idx[b, :, 2]]
        out.append((w[None, :, 0] * f0 + w[None, :, 1] * f1) + w[None, :, 2] * f2)
    return np.stack(out).astype(F32)


def knn(k, xyz, center_xyz):
    """xyz (B, N, 3), center_xyz (B, P, 3) -> int64 (B, k, P), by (d2, index)."""
    out = []
    for b in range(xyz.shape[0]):
        d = sq_dist(center_xyz[b], xyz[b])
        out.append(np.argsort(d, axis=1, kind="stable")[:, :k].T)
    return np.stack(out).astype(np.int64)


def _bitrev(v, bits):
    r = 0
    for i in range(bits):
        r |= ((v >> i) & 1) << (bits - 1 - i)
    return r


def fps_tie_rank(n):
    """rank[k] of the reference block reduction for n points (smaller wins a tie)."""
    bits = min(int(np.floor(np.log2(n))), 10)
    bs = 1 << bits
    k = np.arange(n)
    rev = np.array([_bitrev(int(v), bits) for v in range(bs)], dtype=np.int64)
    return (rev[k % bs] << 21) | (k // bs)


def fps_with_dist(dist, m):
    """dist (B, N, N) float32 -> int32 (B, m)."""
    bsz, n, _ = dist.shape
    rank = fps_tie_rank(n)
    out = np.zeros((bsz, m), np.int32)
    for b in range(bsz):
        temp = np.full(n, 1e10, F32)
        old = 0
        for j in range(1, m):
            temp = np.minimum(dist[b, old].astype(F32), temp)
            cand = np.nonzero(temp > -1)[0]
            if cand.size == 0:
                old = 0
            else:
                best = temp[cand].max()
                tied = cand[temp[cand] == best]
                old = int(tied[np.argmin(rank[tied])])
            out[b, j] = old
    return out


def fps_from_xyz(xyz, m):
    """Coordinate-form FPS through the same tie order (d = (dx*dx + dy*dy) + dz*dz)."""
    return fps_with_dist(np.stack([sq_dist(p, p) for p in xyz]), m)


def scatter_bwd(grad_out, idx, n, weight=None, div=1, dtype=F32):
    """grad_out (B, C, ...) with M / div positions per (b, c); idx (B, ...) with M entries per
    batch element; weight (B, ...) like idx or None.  -> (B, C, n): for j ascending, the term
    w[j] * g[:, j // div] is added to acc[:, idx[j]] in `dtype`, compensated:
    y = term - comp; t = acc + y; comp = (t - acc) - y; acc = t."""
    bsz, c = grad_out.shape[:2]
    g = grad_out.reshape(bsz, c, -1).astype(dtype)
    ii = idx.reshape(bsz, -1)
    w = None if weight is None else weight.reshape(bsz, -1).astype(dtype)
    out = np.zeros((bsz, c, n), dtype)
    for b in range(bsz):
        acc = np.zeros((n, c), dtype)            # row per source: contiguous updates
        comp = np.zeros((n, c), dtype)
        gb = np.ascontiguousarray(g[b].T)
        for j in range(ii.shape[1]):
            s = ii[b, j]
            if 0 <= s < n:
                v = gb[j // div]
                y = (v if w is None else w[b, j] * v) - comp[s]
                t = acc[s] + y
                comp[s] = (t - acc[s]) - y
                acc[s] = t
        out[b] = acc.T
    return out
