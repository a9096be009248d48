"""numpy restatements the transposed-conv / max-pool tests check against.

deconv_pairs: getValidOutPosTranspose + getIndicePairsDeConv
(mmdet3d/ops/spconv/include/spconv/geometry.h:87-140, 196-245) with dilation 1, in the
reference's raw first-touch output order (canonicalise with oracle.canonical_rulebook).
maxpool_fwd / maxpool_bwd: SparseMaxPoolForwardFunctor / SparseMaxPoolBackwardFunctor
(src/maxpool.cc:20-62) driven per offset as pool_ops.h:34,71 drives them."""
import itertools

import numpy as np


def deconv_output_size(in_shape, ksize, stride, padding, output_padding=(0, 0, 0)):
    """ops.py:33-43."""
    return [(int(in_shape[i]) - 1) * stride[i] - 2 * padding[i] + ksize[i] + output_padding[i]
            for i in range(3)]


def deconv_pairs(indices, out_shape, ksize, stride, padding):
    """-> (out_indices[M,4], indice_pairs[K,2,N], indice_num[K])"""
    idx = np.asarray(indices, np.int64).reshape(-1, 4)
    n = idx.shape[0]
    kvol = int(np.prod(ksize))
    pairs = np.full((kvol, 2, max(n, 1)), -1, np.int32)
    num = np.zeros((kvol,), np.int32)
    grid, outs = {}, []
    for j in range(n):
        b = int(idx[j, 0])
        lowers = [int(idx[j, 1 + d]) * stride[d] - padding[d] for d in range(3)]
        for kz, ky, kx in itertools.product(range(ksize[0]), range(ksize[1]), range(ksize[2])):
            val = (lowers[0] + kz, lowers[1] + ky, lowers[2] + kx)
            if any(v < 0 or v >= out_shape[d] for d, v in enumerate(val)):
                continue
            offset = (kz * ksize[1] + ky) * ksize[2] + kx
            key = (b,) + val
            if key not in grid:
                grid[key] = len(outs)
                outs.append(key)
            pairs[offset, 0, num[offset]] = j
            pairs[offset, 1, num[offset]] = grid[key]
            num[offset] += 1
    out = np.asarray(outs, np.int32).reshape(-1, 4)
    return out, pairs[:, :, :n], num


def maxpool_fwd(feat, pairs, num, n_out):
    feat = np.asarray(feat, np.float32)
    out = np.zeros((n_out, feat.shape[1]), np.float32)
    for k in range(pairs.shape[0]):
        for p in range(int(num[k])):
            i, o = pairs[k, 0, p], pairs[k, 1, p]
            take = out[o] < feat[i]
            out[o][take] = feat[i][take]
    return out


def maxpool_bwd(feat, out, dout, pairs, num):
    feat = np.asarray(feat, np.float32)
    din = np.zeros_like(feat)
    for k in range(pairs.shape[0]):
        for p in range(int(num[k])):
            i, o = pairs[k, 0, p], pairs[k, 1, p]
            hit = out[o] == feat[i]
            din[i][hit] += dout[o][hit]
    return din


def random_voxels(rng, batch, shape, per_batch):
    """Unique (b, z, y, x) rows, in random order."""
    rows = []
    for b in range(batch):
        cells = rng.choice(int(np.prod(shape)), size=min(per_batch, int(np.prod(shape))),
                           replace=False)
        z, rem = np.divmod(cells, shape[1] * shape[2])
        y, x = np.divmod(rem, shape[2])
        rows.append(np.stack([np.full_like(z, b), z, y, x], 1))
    idx = np.concatenate(rows).astype(np.int32)
    return idx[rng.permutation(idx.shape[0])]
