"""Float64 restatements of the sparse convolution, from the table forms the kernels take.

    forward / dgrad   out[o] = sum_k x[nbr[k, o]] @ M(W[kw]),  kw = K - 1 - k with weight_flip,
                      M = transpose for dgrad  (csrc/spconv_split.hip: `kw = flip ? kvol - 1 - k
                      : k`; the packer's bit 0 stores W[k]^T, so a dgrad call is the forward
                      kernel on `d_out` with the transposed image)
    wgrad             dW[k] = sum_{p < num[k]} f[pairs[k, 0, p]]^T (x) g[pairs[k, 1, p]]

Each also returns the "weight of the sum" S, the same sum over |a| |b|: the scale an
accumulation error is measured against (max |out - ref| / S), and -- on integer data -- the
bound under which every float32 partial sum in any order is exact (S < 2^24).
Nothing here is the code under test: plain numpy loops over offsets."""

import numpy as np


# --------------------------------------------------------------------------- tables
def _weights(w, flip, transpose):
    """[K, a, b] weight as the kernel applies it per table row k: [K, contraction, outputs]."""
    w = np.asarray(w)
    if flip:
        w = w[::-1]
    return w.transpose(0, 2, 1) if transpose else w


def conv_table(x, w, nbr, n_out, weight_flip=False, transpose=False):
    """-> (out float64 [n_out, outputs], S float64 same shape).  nbr is [K, ld >= n_out];
    only its first n_out columns are the table."""
    x64 = np.asarray(x, np.float64)
    wk = _weights(w, weight_flip, transpose).astype(np.float64)
    nbr = np.asarray(nbr)
    out = np.zeros((n_out, wk.shape[2]))
    s = np.zeros_like(out)
    ax, aw = np.abs(x64), np.abs(wk)
    for k in range(nbr.shape[0]):
        src = nbr[k, :n_out]
        m = src >= 0
        if m.any():
            out[m] += x64[src[m]] @ wk[k]
            s[m] += ax[src[m]] @ aw[k]
    return out, s


def conv_fwd(feat, w, nbr, n_out, weight_flip=False):
    return conv_table(feat, w, nbr, n_out, weight_flip, False)


def conv_dgrad(d_out, w, table, n_in, weight_flip=False):
    """d_in from the MIRRORED table (table[k, i] = output row fed by input row i through
    offset k; weight_flip off) or from a SubM FORWARD table with weight_flip on."""
    return conv_table(d_out, w, table, n_in, weight_flip, True)


def mirror_table(nbr, n_out, n_in):
    """Input-side table of a forward table whose offsets each use an input row at most once."""
    nbr = np.asarray(nbr)
    out = np.full((nbr.shape[0], n_in), -1, np.int32)
    for k in range(nbr.shape[0]):
        src = nbr[k, :n_out]
        o = np.nonzero(src >= 0)[0]
        assert np.unique(src[o]).size == o.size, "an offset reads an input row twice"
        out[k, src[o]] = o
    return out


def conv_wgrad(feat, d_out, pairs, num):
    """-> (dW float64 [K, c_in, c_out], S)."""
    f, g = np.asarray(feat, np.float64), np.asarray(d_out, np.float64)
    pairs, num = np.asarray(pairs), np.asarray(num)
    dw = np.zeros((pairs.shape[0], f.shape[1], g.shape[1]))
    s = np.zeros_like(dw)
    for k in range(pairs.shape[0]):
        p = int(num[k])
        if p:
            i, o = pairs[k, 0, :p], pairs[k, 1, :p]
            dw[k] = f[i].T @ g[o]
            s[k] = np.abs(f[i]).T @ np.abs(g[o])
    return dw, s


def table_from_pairs(pairs, num, n_out):
    pairs, num = np.asarray(pairs), np.asarray(num)
    nbr = np.full((pairs.shape[0], n_out), -1, np.int32)
    for k in range(pairs.shape[0]):
        p = int(num[k])
        nbr[k, pairs[k, 1, :p]] = pairs[k, 0, :p]
    return nbr


# --------------------------------------------------------------------------- the yardstick
def _fma32(acc, a, b):
    """float32(acc + a * b) with one rounding (a * b of two float32 is exact in float64; the
    second rounding float64 -> float32 of the sum is innocuous to 2^-29 of an ulp)."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def conv_fwd_f32_chain(x, w, nbr, n_out, weight_flip=False, transpose=False):
    """The same forward sum accumulated in float32, one fused multiply-add per term in
    ascending (offset, channel) order: what a scalar float32 loop returns."""
    x = np.asarray(x, np.float32)
    wk = np.ascontiguousarray(_weights(w, weight_flip, transpose), np.float32)
    nbr = np.asarray(nbr)
    acc = np.zeros((n_out, wk.shape[2]), np.float32)
    for k in range(nbr.shape[0]):
        src = nbr[k, :n_out]
        m = np.nonzero(src >= 0)[0]
        if not m.size:
            continue
        rows = x[src[m]]
        a = acc[m]
        for c in range(wk.shape[1]):
            a = _fma32(a, rows[:, c:c + 1], wk[k, c][None, :])
        acc[m] = a
    return acc


def conv_wgrad_f32_chain(feat, d_out, pairs, num):
    """dW accumulated in float32 over each offset's pairs in list order."""
    f, g = np.asarray(feat, np.float32), np.asarray(d_out, np.float32)
    pairs, num = np.asarray(pairs), np.asarray(num)
    dw = np.zeros((pairs.shape[0], f.shape[1], g.shape[1]), np.float32)
    for k in range(pairs.shape[0]):
        a = dw[k]
        for p in range(int(num[k])):
            a = _fma32(a, f[pairs[k, 0, p]][:, None], g[pairs[k, 1, p]][None, :])
        dw[k] = a
    return dw


def normalised_error(got, ref, s):
    """max |got - ref| / S over the outputs with S > 0 (0.0 when there is none)."""
    m = s > 0
    if not m.any():
        return 0.0
    return float((np.abs(np.asarray(got, np.float64) - ref)[m] / s[m]).max())


# --------------------------------------------------------------------------- bf16 planes
def bf16_round(x):
    """float32 -> nearest bf16 (ties to even), returned as float32 (finite inputs)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def plane(x, p):
    """Plane p (0 = h, 1 = m, 2 = l) of split8's error-free splitting, float32."""
    r = np.ascontiguousarray(x, np.float32)
    for _ in range(p):
        r = r - bf16_round(r)
    return bf16_round(r)


# csrc/spconv_split.hip: Products<NP> -- the (plane of a, plane of b) products a kernel keeps
KEPT_PRODUCTS = {1: ((0, 0),), 2: ((0, 0), (0, 1), (1, 0)),
                 3: ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))}


def dropped_products(planes):
    """The plane products of (sum of `planes` planes)^2 that Products<planes> leaves out."""
    return tuple((i, j) for i in range(planes) for j in range(planes)
                 if (i, j) not in KEPT_PRODUCTS[planes])


def cut_planes(x, planes):
    """x cut to the sum of its leading `planes` bf16 planes (h, m, l of split8), float64."""
    r = np.ascontiguousarray(x, np.float32)
    tot = np.zeros(r.shape, np.float64)
    for _ in range(planes):
        h = bf16_round(r)
        tot += h
        r = r - h          # exact in float32
    return tot


# --------------------------------------------------------------------------- stream-K tables
SK_C1 = 12            # csrc/spconv_split.hip: kSkC1Default
SK_MIN_RANKS = 64     # kSkMinRanks
SK_OVH_UNITS = 8      # launch_fwd_split: ovh_units


def tile_prefix(tab, n_out, rows):
    """msmd_rulebook_tile_prefix: prefix sums of the tiles' cost -- per active offset SK_C1 +
    the 32-row groups it keeps busy (positions past the end repeat the last row), 1 for an
    empty tile."""
    tab = np.asarray(tab)[:, :n_out]
    w = []
    for t0 in range(0, n_out, rows):
        pos = np.minimum(np.arange(t0, t0 + rows), n_out - 1)
        act = (tab[:, pos] >= 0).reshape(tab.shape[0], rows // 32, 32).any(2)
        groups = act.sum(1)
        w.append(max(int((SK_C1 + groups[groups > 0]).sum()), 1))
    return np.concatenate([[0], np.cumsum(w)]).astype(np.int32)


def stream_k_cut_tiles(prefix, c_in, kvol, rows):
    """Tiles that two stream-K ranges certainly share (a range boundary falls after the
    tile's first offset starts and no later than where its last one can start), from the
    kernel's own arithmetic: S = max(ceil(W / ranges), c0 + 64) units per range with tile t at
    [prefix[t] + c0 (t + 1), prefix[t + 1] + c0 (t + 1))."""
    prefix = np.asarray(prefix, np.int64)
    n_tiles = prefix.size - 1
    kbt = (c_in + 31) // 32
    c0 = ((SK_OVH_UNITS + kbt - 1) // kbt) * (SK_C1 + 2)
    n_ranges = min(n_tiles * kvol, 512 if rows == 128 else 256)
    total = int(prefix[-1]) + c0 * n_tiles
    seg = max(-(-total // n_ranges), c0 + SK_MIN_RANKS)
    cut = []
    for t in range(n_tiles):
        start = int(prefix[t]) + c0 * (t + 1)
        last = start + int(prefix[t + 1] - prefix[t]) - (SK_C1 + rows // 32)
        b = (start // seg + 1) * seg         # first boundary past the tile's first offset
        if start < b <= last:
            cut.append(t)
    return cut
