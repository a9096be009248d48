"""Synthetic neighbour tables, pair lists, data and the case tables of the sparse-conv edge
suite (tests/test_gpu_conv_edges.py, tests/test_conv_ref_cpu.py).  The kernels only ever see
tables, so no voxel geometry is involved: a table is built position by position, tile by
tile, with a mask recipe per tile.  No index lies outside [-1, n_in)."""

import zlib
from collections import namedtuple

import numpy as np

import conv_ref as R

RECIPES = ("all", "first", "last", "none", "group", "random")


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


# --------------------------------------------------------------------------- tables
Table = namedtuple("Table", "tab nat order n_out n_in ld kvol decoy")
# tab   [K, ld]     the table in the order the kernel tiles it (tile order under `order`)
# nat   [K, n_out]  the same table by output row: nat[k, order[p]] = tab[k, p]
# order [n_out] | None   output row at tile position p
# decoy row of the features no real entry refers to (padding refers to it), or None


def tile_mask(recipe, kvol, rows, rng, group=1):
    """[K, rows] bool: which (offset, position) of one tile is connected."""
    m = np.zeros((kvol, rows), bool)
    if recipe == "all":
        m[:] = True
    elif recipe == "first":
        m[0] = True
    elif recipe == "last":
        m[kvol - 1] = True
    elif recipe == "group":            # one 32-row group of the tile, every offset
        g = min(group, rows // 32 - 1)
        m[:, 32 * g:32 * g + 32] = True
    elif recipe == "random":
        m = rng.rand(kvol, rows) < rng.uniform(0.1, 0.7, size=(kvol, 1))
    elif recipe != "none":
        raise ValueError(recipe)
    return m


def make_table(n_out, n_in, kvol, tile_rows, recipe="all", tile_recipes=None, ld=None,
               source="random", pad="builder", row_order=False, seed=0):
    """recipe: mask recipe of every tile; tile_recipes {tile: recipe} overrides single tiles
    (negative tile numbers count from the last).  source: "random" input rows, or "last"
    (every connected entry is row n_in - 1).  pad: what columns n_out .. ld hold -- "builder":
    -1, as the rulebook builders leave them; "decoy": the (valid) index of a feature row that
    no real entry uses.  row_order: a random permutation of the output rows."""
    key = (n_out, n_in, kvol, tile_rows, recipe, sorted((tile_recipes or {}).items()), ld, source,
           pad, seed)
    rng = _rng("table", key)           # (the same `tab` with and without a row order)
    ld = n_out if ld is None else ld
    assert ld >= n_out and n_in >= 1
    n_tiles = (n_out + tile_rows - 1) // tile_rows
    per_tile = {(t % n_tiles if n_tiles else t): r for t, r in (tile_recipes or {}).items()}
    decoy = n_in - 1 if pad == "decoy" else None
    hi = n_in - 1 if decoy is not None else n_in       # real entries stay below the decoy
    assert hi >= 1
    tab = np.full((kvol, ld), -1, np.int32)
    for t in range(n_tiles):
        p0 = t * tile_rows
        # (the connected group must exist in a short last tile too)
        m = tile_mask(per_tile.get(t, recipe), kvol, tile_rows, rng, 1 if p0 + 64 <= n_out else 0)
        m = m[:, :min(tile_rows, n_out - p0)]
        src = (np.full(m.shape, hi - 1) if source == "last"
               else rng.randint(0, hi, size=m.shape)).astype(np.int32)
        tab[:, p0:p0 + m.shape[1]] = np.where(m, src, -1)
    if decoy is not None:
        tab[:, n_out:] = decoy
    order = _rng("order", key).permutation(n_out).astype(np.int32) if row_order else None
    nat = tab[:, :n_out].copy()
    if order is not None:
        nat = np.empty_like(nat)
        nat[:, order] = tab[:, :n_out]
    return Table(tab, nat, order, n_out, n_in, ld, kvol, decoy)


# --------------------------------------------------------------------------- pair lists
Pairs = namedtuple("Pairs", "pairs num n_in n_out ld decoy_in decoy_out")


def make_pairs(num, n_in, n_out, ld, pad="builder", seed=0, rows=None):
    """pairs[K, 2, ld] with num[k] pairs per offset in ascending output row (distinct rows per
    offset, as msmd_rulebook_pairs writes them and msmd_rulebook_pair_segments relies on).
    Slots past num[k]: -1 ("builder", what msmd_rulebook_pairs leaves) or the indices of a
    decoy input row and a decoy output row that no pair uses.  rows: the output rows to draw
    from (default all)."""
    num = np.asarray(num, np.int32)
    rng = _rng("pairs", num.tolist(), n_in, n_out, ld, pad, seed)
    decoy = pad == "decoy"
    hi_in, hi_out = (n_in - 1, n_out - 1) if decoy else (n_in, n_out)
    pool = np.arange(hi_out) if rows is None else np.asarray(rows)
    assert num.max(initial=0) <= min(ld, pool.size) and hi_in >= 1 and pool.max(initial=0) < hi_out
    pairs = np.full((num.size, 2, ld), -1, np.int32)
    if decoy:
        pairs[:, 0], pairs[:, 1] = n_in - 1, n_out - 1
    for k, p in enumerate(num):
        pairs[k, 1, :p] = np.sort(rng.choice(pool, size=p, replace=False))
        pairs[k, 0, :p] = rng.randint(0, hi_in, size=p)
    return Pairs(pairs, num, n_in, n_out, ld, n_in - 1 if decoy else None,
                 n_out - 1 if decoy else None)


# --------------------------------------------------------------------------- data
DECOY_VALUE = 3.0e30     # what a decoy row holds: one stray read of it changes any sum


def int_rows(n, c, bits, key):
    """Integers of at most `bits` significant bits, both signs, as float32."""
    rng = _rng("int", n, c, key)
    x = rng.randint(-(1 << 12) + 1, 1 << 12, size=(n, c))
    return (np.sign(x) * (np.abs(x) >> (12 - bits))).astype(np.float32)


def small_ints(shape, key, lim=3):
    return _rng("small", shape, key).randint(-lim, lim + 1, size=shape).astype(np.float32)


def bits_for(s12_max, want=12):
    """Feature bits (<= want) that keep S below 2^24, given S's maximum for 12-bit features
    (dropping a low bit at least halves every |feature|, floor division included)."""
    bits = 12
    while bits > 1 and (s12_max / (1 << (12 - bits)) >= (1 << 24) or bits > want):
        bits -= 1
    return bits


# --------------------------------------------------------------------------- forward cases
FwdCase = namedtuple("FwdCase", "id c_in c_out n_out n_in kvol flip dgrad recipe tile_recipes ld "
                                "source pad inst expect_cut")
# inst = (nt, waves, pingpong, passes) K.split_instantiation(c_out) must report


def split_inst(c_out):
    """The dispatch of csrc/spconv_split.hip (fwd_waves, fwd_passes, the instantiation)."""
    nt_total = (c_out + 15) // 16
    waves = 8 if c_out >= 161 else 4
    passes = 1 if waves == 8 and nt_total in (11, 12) else (nt_total + 7) // 8
    per = (nt_total + passes - 1) // passes
    if waves == 8:
        nt = 12 if per > 8 else 8 if per > 6 else 6
    else:
        nt = 8 if per > 6 else 6 if per > 4 else 4 if per > 2 else 2
    return nt, waves, waves == 8, passes


def _fwd(c_in, c_out, n_out, kvol=27, flip=False, dgrad=False, recipe="all", tile_recipes=None,
         n_in=None, ld=None, source="random", pad="builder", tag=None):
    nt, waves, pp, passes = split_inst(c_out)
    n_in = 3 * n_out if n_in is None else n_in
    mask = recipe if not tile_recipes else "+".join(
        "%s@%s" % (r, {0: "first", -1: "last"}.get(t, "mid")) for t, r in sorted(tile_recipes.items()))
    cid = "split-%s-%s%dx%d-c%dto%d-n%d-k%d%s-%s" % (
        "dgrad" if dgrad else "fwd", "pp" if pp else "nt", nt, passes, c_in, c_out, n_out, kvol,
        "flip" if flip else "", mask)
    if tag:
        cid += "-" + tag
    n_tiles = (n_out + 32 * waves - 1) // (32 * waves)
    expect_cut = (n_tiles > 1 and kvol >= 8 and recipe in ("all", "random", "group"))
    return FwdCase(cid, c_in, c_out, n_out, n_in, kvol, flip, dgrad, recipe, tile_recipes, ld,
                   source, pad, (nt, waves, pp, passes), expect_cut)


# every instantiation with a full and with a partial last k-block (c_in % 32 == 0 / != 0)
SPLIT_WIDTHS = [(32, 32), (40, 32), (64, 48), (40, 36), (72, 64), (32, 80), (136, 96), (64, 112),
                (40, 128), (256, 132), (72, 144), (32, 160), (136, 164), (64, 176), (40, 192),
                (256, 208), (72, 256), (64, 272), (136, 272)]
ROWS = {4: (1, 127, 128, 129, 385), 8: (1, 255, 256, 257, 769)}
KVOLS = (1, 2, 8, 27, 31, 32)
EDGE_LAYERS = ((64, 64), (72, 192))       # one 4-wave and one ping-pong layer for the sweeps


def _multi(c_out):
    return ROWS[split_inst(c_out)[1]][-1]


def fwd_cases():
    cs = []
    for i, (ci, co) in enumerate(SPLIT_WIDTHS):          # instantiations; dgrad every other
        cs.append(_fwd(ci, co, _multi(co), flip=bool(i & 1), dgrad=bool(i & 1)))
    for ci, co in EDGE_LAYERS:
        waves = split_inst(co)[1]
        for n in ROWS[waves][:-1]:                       # row edges
            cs.append(_fwd(ci, co, n))
        for kvol in KVOLS:                               # kernel volumes, flip off and on
            for flip in (False, True):
                if kvol == 27 and not flip:
                    continue                             # (the instantiation sweep's case)
                cs.append(_fwd(ci, co, _multi(co), kvol=kvol, flip=flip, dgrad=flip and kvol % 2 == 1,
                               recipe="random" if kvol >= 8 else "all"))
        n = _multi(co)
        cs.append(_fwd(ci, co, n, n_in=1, tag="nin1"))
        cs.append(_fwd(ci, co, n, source="last", tag="lastrow"))
        cs.append(_fwd(ci, co, n, ld=n + 37, tag="ld"))
        cs.append(_fwd(ci, co, n, ld=n + 37, pad="decoy", kvol=32, recipe="random", tag="decoy"))
        for recipe in RECIPES:                           # every recipe in every tile position
            for pos in (0, 1, -1):
                if recipe == "all":
                    cs.append(_fwd(ci, co, n, recipe="random", tile_recipes={pos: "all"}))
                else:
                    cs.append(_fwd(ci, co, n, tile_recipes={pos: recipe}))
        cs.append(_fwd(ci, co, n, recipe="none", tag="empty"))
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return cs


def fwd_table(case, row_order):
    waves = case.inst[1]
    return make_table(case.n_out, case.n_in, case.kvol, 32 * waves, case.recipe, case.tile_recipes,
                      case.ld, case.source, case.pad, row_order, seed=case.id)


def fwd_weight(case, lim=3):
    """The weight as the packer takes it: [K, c_in, c_out], or for dgrad the layer's own
    [K, c_out(layer's inputs), c_in] -- packed with transpose."""
    shape = (case.kvol, case.c_out, case.c_in) if case.dgrad else (case.kvol, case.c_in, case.c_out)
    return small_ints(shape, case.id, lim)


def fwd_exact_data(case, tab, want_bits=12):
    """(features, weight, ref float64, S) with S.max() < 2^24 by construction; a decoy row
    holds DECOY_VALUE."""
    w = fwd_weight(case)
    f12 = int_rows(case.n_in, case.c_in, 12, case.id)
    if tab.decoy is not None:
        f12[tab.decoy] = 0
    _, s12 = R.conv_table(f12, w, tab.nat, case.n_out, case.flip, case.dgrad)
    bits = bits_for(s12.max(initial=0.0), want_bits)
    f = int_rows(case.n_in, case.c_in, bits, case.id)
    if tab.decoy is not None:
        f[tab.decoy] = 0
    ref, s = R.conv_table(f, w, tab.nat, case.n_out, case.flip, case.dgrad)
    if tab.decoy is not None:
        f[tab.decoy] = DECOY_VALUE
    return f, w, ref, s


# bn_stats: the four row edges of both tile heights; tiny integers (squares below 2^24)
def bn_cases():
    return [_fwd(ci, co, n, kvol=2, tag="bn") for ci, co in ((32, 64), (40, 192))
            for n in ROWS[split_inst(co)[1]][1:]]


def bn_exact_data(case, tab):
    f = small_ints((case.n_in, case.c_in), case.id + "f", 1)
    w = small_ints((case.kvol, case.c_in, case.c_out), case.id + "w", 1)
    ref, s = R.conv_table(f, w, tab.nat, case.n_out)
    return f, w, ref, s


# --------------------------------------------------------------------------- fp32 forward
F32Case = namedtuple("F32Case", "id c_in c_out n_out n_in kvol flip staging tile_rows")


def f32_staging(c_in, c_out, kvol):
    """launch_fwd / dispatch_fwd_pipe of csrc/spconv.hip: the staging form a layer runs."""
    nt = (c_out + 15) // 16
    if c_in % 16 == 0 and c_out % 4 == 0 and kvol <= 32:
        t = c_in // 16
        return "pipe4" if nt <= 8 and t % 4 == 0 else "pipe2" if t % 2 == 0 else "pipe1"
    return "vec4" if c_in % 4 == 0 else "scalar"


def f32_cases():
    cs = []

    def add(ci, co, n, kvol=27, flip=False):
        rows = 128 if (co + 15) // 16 < 4 else 64
        cs.append(F32Case("f32-%s-t%d-c%dto%d-n%d-k%d%s-random" % (
            f32_staging(ci, co, kvol), (co + 15) // 16, ci, co, n, kvol, "flip" if flip else ""),
            ci, co, n, 3 * n, kvol, flip, f32_staging(ci, co, kvol), rows))
    # every tile count, last tile full and 4 wide; every staging width across them
    cins = (64, 32, 16, 48, 20, 5, 7, 64)
    for i, t in enumerate((1, 2, 3, 4, 5, 6, 8, 12)):
        n = 385 if t < 4 else 193
        add(cins[i], 16 * t, n)
        add(cins[(i + 3) % 8], 16 * t - 12, n, flip=True)
    # (12 tiles at c_in = 64 is the two-chunk staging: more than 8 tiles decline four chunks)
    add(16, 18, 129)                 # c_out % 4 != 0 declines the pipelined form
    for n in (1, 127, 128, 129):      # row edges of the 128-row form ...
        add(32, 32, n, kvol=32)
    for n in (1, 63, 64, 65):         # ... and of the 64-row form
        add(48, 128, n, kvol=1 if n == 1 else 31)
    assert {c.staging for c in cs} == {"pipe4", "pipe2", "pipe1", "vec4", "scalar"}
    assert len({c.id for c in cs}) == len(cs)
    return cs


F32_PASS_WIDTHS = (100, 136, 208)      # spconv.functional._conv_f32 cuts these into passes


# --------------------------------------------------------------------------- wgrad cases
WgradCase = namedtuple("WgradCase", "id kernel c_in c_out kvol num n_in n_out ld pad chunk_rows rows")
NUMS = (0, 1, 31, 32, 33, 255, 256, 257)
WGRAD_MAX_TILES = 8


def wgrad_side_blocks(c):
    """side_blocks of csrc/spconv_wgrad_block.hip: blocks a side is cut into, 0 = declined."""
    if c < 64 or c % 16:
        return 0
    t = c // 16
    for nb in range(1, t // 4 + 1):
        if t % nb == 0 and 4 <= t // nb <= WGRAD_MAX_TILES:
            return nb
    return 0


def wgrad_kernel(c_in, c_out, kvol):
    if c_in < 64 or c_out < 64 or c_in % 4 or c_out % 4:
        return "f32"
    if wgrad_side_blocks(c_in) and wgrad_side_blocks(c_out) and kvol <= 64:
        return "block"
    return "slab"


def _nums(kind, kvol):
    if kind == "mix":
        return [NUMS[(k * 3 + 1) % 8] for k in range(kvol)]
    if kind == "zero":
        return [0] * kvol
    if kind == "first":
        return [257] + [0] * (kvol - 1)
    if kind == "last":
        return [0] * (kvol - 1) + [33]
    if kind == "steps":                     # one 32-pair step (or less) per offset
        return [1 + (k * 7) % 32 for k in range(kvol)]
    if kind == "short":                     # all lists together below one 256-pair range
        return [(k % 3 == 0) * (1 + k % 5) for k in range(kvol)]
    if kind == "one":
        return [k % 2 for k in range(kvol)]
    raise ValueError(kind)


def wgrad_cases():
    cs = []

    def add(ci, co, kind="mix", kvol=27, n_out=300, ld=None, pad="builder", chunk_rows=None,
            rows=None, tag=None):
        num = _nums(kind, kvol)
        # (ld >= n_out, as every rulebook has it: the segment tables chunk rows [0, ld))
        ld = max(max(num), 1, n_out) if ld is None else ld
        n_in = 2 * n_out + 3
        kern = wgrad_kernel(ci, co, kvol)
        shape = "%dx%d" % (wgrad_side_blocks(ci), wgrad_side_blocks(co)) if kern == "block" else ""
        cid = "wgrad-%s%s-c%dto%d-n%d-k%d-%s" % (kern, shape, ci, co, n_out, kvol, kind)
        if chunk_rows:
            cid += "-chunk%d" % chunk_rows
        if tag:
            cid += "-" + tag
        cs.append(WgradCase(cid, kern, ci, co, kvol, num, n_in, n_out, ld, pad, chunk_rows, rows))
    # whole-block kernel: every consumer quadrant shape on each side, then the multi-block sides
    for ci, co in ((64, 80), (80, 96), (96, 112), (112, 128), (128, 64)):
        add(ci, co)
    for ci, co in ((160, 64), (64, 192), (224, 96), (112, 256), (320, 64), (64, 160), (192, 224)):
        add(ci, co)
    # slab kernel: the widths the block kernel declines, and kernel volume 125
    for ci, co in ((68, 100), (144, 64), (64, 176), (208, 68), (100, 144)):
        add(ci, co)
    add(64, 64, kind="short", kvol=125)
    # fp32 kernel below 64 channels (every slab side: 1, 2 and 4 tiles)
    for ci, co in ((16, 32), (5, 16), (32, 48), (48, 20), (64, 32)):
        add(ci, co)
    # pair lists
    for kern_w in ((64, 64), (128, 128), (68, 64), (32, 32)):
        for kind in ("zero", "first", "last", "steps", "short"):
            add(*kern_w, kind=kind)
        add(*kern_w, kind="one", n_out=1, ld=1, tag="ld1")
        add(*kern_w, pad="decoy", ld=300, tag="decoy")
    # row-chunk segment tables (block kernel)
    add(64, 64, chunk_rows=1, n_out=256, ld=256, kind="steps", tag="maxchunks")
    add(96, 128, chunk_rows=100, n_out=300, ld=300)
    add(128, 64, chunk_rows=100, n_out=300, ld=333, pad="decoy", tag="decoy")
    add(64, 80, chunk_rows=4, n_out=1024, ld=1024, kind="steps", rows=np.arange(600, 640),
        tag="emptychunks")
    add(160, 64, chunk_rows=7, n_out=300, ld=300)
    assert len({c.id for c in cs}) == len(cs)
    return cs


def wgrad_pairs(case):
    return make_pairs(case.num, case.n_in, case.n_out, case.ld, case.pad, seed=case.id,
                      rows=case.rows)


def wgrad_exact_data(case, pr, want_bits=12):
    g = small_ints((case.n_out, case.c_out), case.id + "g")
    f12 = int_rows(case.n_in, case.c_in, 12, case.id)
    _, s12 = R.conv_wgrad(f12, g, pr.pairs, pr.num)
    f = int_rows(case.n_in, case.c_in, bits_for(s12.max(initial=0.0), want_bits), case.id)
    ref, s = R.conv_wgrad(f, g, pr.pairs, pr.num)
    if pr.decoy_in is not None:
        f[pr.decoy_in] = DECOY_VALUE
        g[pr.decoy_out] = DECOY_VALUE
    return f, g, ref, s


# --------------------------------------------------------------------------- arithmetic cases
ArithCase = namedtuple("ArithCase", "id base data")
ARITH_DATA = ("normal", "rowscale", "offset1000")


def arith_data(kind, n, c, key):
    """unit normal; rows scaled by 2^s, s uniform in [-20, 20]; channels offset by 1000 sigma."""
    rng = _rng("arith", kind, n, c, key)
    x = rng.randn(n, c)
    if kind == "rowscale":
        x = x * np.exp2(rng.randint(-20, 21, size=(n, 1)))
    elif kind == "offset1000":
        x = x + 1000.0
    return x.astype(np.float32)


def arith_weight(kind, shape, key, col_axis):
    rng = _rng("arithw", kind, shape, key)
    w = rng.randn(*shape) / np.sqrt(shape[0] * shape[1])
    if kind == "rowscale":             # the weight's output columns scaled likewise
        sh = [1, 1, 1]
        sh[col_axis] = shape[col_axis]
        w = w * np.exp2(rng.randint(-20, 21, size=sh))
    return w.astype(np.float32)


def arith_fwd_cases():
    base = [_fwd(64, 64, 385, recipe="random"), _fwd(72, 192, 769, recipe="random"),
            _fwd(40, 128, 385, kvol=32, flip=True, recipe="random"),
            _fwd(136, 272, 257, kvol=8, dgrad=True, flip=True, recipe="random"),
            # few terms per output: the chain's own error is smallest here, so a lost plane
            # (2^-17 per product) stands out most
            _fwd(32, 48, 129, kvol=1, recipe="random"), _fwd(40, 176, 257, kvol=2, recipe="random")]
    return [ArithCase("%s-%s" % (b.id, d), b, d) for b in base for d in ARITH_DATA]


def arith_f32_cases():
    base = [F32Case("f32-pipe2-t2-c32to32-n385-k27-random", 32, 32, 385, 1155, 27, False, "pipe2", 128),
            F32Case("f32-pipe4-t8-c64to128-n193-k27-random", 64, 128, 193, 579, 27, False, "pipe4", 64),
            F32Case("f32-scalar-t1-c7to16-n385-k27-random", 7, 16, 385, 1155, 27, False, "scalar", 128)]
    return [ArithCase("%s-%s" % (b.id, d), b, d) for b in base for d in ARITH_DATA]


def arith_wgrad_cases():
    cs = {c.id: c for c in wgrad_cases()}
    base = [cs["wgrad-block1x1-c64to80-n300-k27-mix"], cs["wgrad-block2x2-c192to224-n300-k27-mix"],
            cs["wgrad-slab-c68to100-n300-k27-mix"], cs["wgrad-f32-c32to48-n300-k27-mix"]]
    return [ArithCase("%s-%s" % (b.id, d), b, d) for b in base for d in ARITH_DATA]


def f32_table(case, row_order=False, ld=None, pad="builder"):
    return make_table(case.n_out, case.n_in, case.kvol, case.tile_rows, "random", ld=ld, pad=pad,
                      row_order=row_order, seed=case.id)


def f32_exact_data(case, tab):
    fc = _fwd(32, 32, 1)._replace(id=case.id, c_in=case.c_in, c_out=case.c_out, n_out=case.n_out,
                                  n_in=case.n_in, kvol=case.kvol, flip=case.flip)
    return fwd_exact_data(fc, tab)


def arith_fwd_setup(ac):
    """(table, features, weight) of a forward / dgrad / fp32 arithmetic case."""
    b = ac.base
    if isinstance(b, F32Case):
        tab = f32_table(b)
        shape, col, dgrad = (b.kvol, b.c_in, b.c_out), 2, False
    else:
        tab = fwd_table(b, row_order=True)
        dgrad = b.dgrad
        shape, col = ((b.kvol, b.c_out, b.c_in), 1) if dgrad else ((b.kvol, b.c_in, b.c_out), 2)
    return tab, arith_data(ac.data, b.n_in, b.c_in, ac.id), arith_weight(ac.data, shape, ac.id, col)


def arith_wgrad_setup(ac):
    b = ac.base
    pr = wgrad_pairs(b)
    return (pr, arith_data(ac.data, b.n_in, b.c_in, ac.id + "f"),
            arith_data(ac.data, b.n_out, b.c_out, ac.id + "g"))
