"""SparseConvTensor and rulebook cache.

Mirrors the spconv-2.x type the reference call sites construct and mutate
(legacy twin mmdet3d/ops/spconv/structure.py:21-69):
SparseConvTensor(features, indices, spatial_shape, batch_size) with
.features/.indices/.spatial_shape/.batch_size/.indice_dict, .replace_feature(),
.dense(), .find_indice_pair(), assignable .indices (MSMDFusion.py:322-323).
"""
from typing import List, Optional

import os
import threading

import numpy as np
import torch

from .. import kernels as K
from .functional import ConvNeeds, conv_needs, dense as _dense


_PLAN = threading.local()
_UNSET = object()       # "not computed yet" (None is a result: an empty table has no order)
# MSMD_PLAN_BATCH=0: every table planned at once by its own prepare() (A/B, tests)
PLAN_BATCHING = os.environ.get("MSMD_PLAN_BATCH", "1") != "0"
# MSMD_SUBM_BATCH=0: SubM tables built at once even inside a plan_batch (plans stay batched)
SUBM_BATCHING = os.environ.get("MSMD_SUBM_BATCH", "1") != "0"
PLAN_SCOPE = os.environ.get("MSMD_PLAN_SCOPE", "call")


class plan_batch:
    """`with plan_batch():` -- IndiceData.prepare() calls inside (SparseConvTensor.plan, the
    fusion stack's stage planning) record what each table's kernels will need; the exit of
    the OUTERMOST context computes all of it in one K.rulebook_plan_many call on the current
    stream.  Nothing in an index pass reads a plan (the feature pass does), so the ~21 tables
    of an LC step are planned together at the end of fusion.prepare(): 8 launches instead of
    ~280, 3 ms less on the index queue.  Per thread (the prefetch worker and
    the step thread plan independently); results are those of the table-by-table calls."""

    LEVELS = {"call": 0, "stage": 1, "all": 2}

    def __init__(self, level="call"):
        """level: how much of an index pass this context spans -- "call" (one
        SparseConvTensor.plan), "stage" (an encoder / one fusion stage), "all" (a whole
        prepare()).  MSMD_PLAN_SCOPE names the widest level that batches (default call: on a
        GPU-bound step a launch set spanning more displaces the conv kernels)."""
        self.jobs = {}
        self.subm_jobs = []
        self.outer = None
        self.level = self.LEVELS[level]

    def __enter__(self):
        self.outer = getattr(_PLAN, "batch", None)
        self.active = PLAN_BATCHING and self.level <= self.LEVELS.get(PLAN_SCOPE, 0)
        if self.outer is None and self.active:
            _PLAN.batch = self
        return self

    def __exit__(self, exc_type, exc, tb):
        if self.outer is None and self.active:
            _PLAN.batch = None
            if exc_type is None:
                self.flush()
            else:       # tables never filled: a rulebook that survives the error must not be used
                for j in self.subm_jobs:        # (cached_rulebook rebuilds a poisoned entry)
                    j["rb"].nbr_fwd = None
                    j["rb"].pending = False
                self.subm_jobs, self.jobs = [], {}
        return False

    def job(self, rb, side):
        if self.outer is not None:
            return self.outer.job(rb, side)
        key = (id(rb), side)
        j = self.jobs.get(key)
        if j is None:
            j = self.jobs[key] = dict(rb=rb, side=side, tile_rows=set(), want_order=False,
                                      want_pairs=False, want_segments=False)
        return j

    def subm(self, rb, batch_size):
        """A SubM rulebook whose table is to be filled at the exit (build_rulebook)."""
        if self.outer is not None:
            return self.outer.subm(rb, batch_size)
        self.subm_jobs.append(dict(rb=rb, indices=rb.indices, batch_size=batch_size,
                                   spatial_shape=rb.spatial_shape, ksize=rb.ksize,
                                   nbr=rb.nbr_fwd))

    def flush(self):
        subm, self.subm_jobs = self.subm_jobs, []
        try:
            K.rulebook_subm_many(subm)          # the tables first: the plans read them
        except Exception:
            for j in subm:                      # never filled: must not be used
                j["rb"].nbr_fwd = None
                j["rb"].pending = False
            self.jobs = {}
            raise
        for j in subm:
            j["rb"].pending = False
        jobs, todo = list(self.jobs.values()), []
        self.jobs = {}
        for j in jobs:
            rb, fwd, side = j["rb"], j["side"] == "fwd", getattr(j["rb"], j["side"])
            rows = {r for r in j["tile_rows"] if r not in side._prefix}
            want_table = bool(j["tile_rows"]) and side._tiled is _UNSET
            if rows and not want_table:             # a further height of a table already tiled
                for r in rows:
                    side.prefix(r)
                rows = set()
            want_pairs = fwd and j["want_pairs"] and rb._pairs is None
            want_seg = fwd and j["want_segments"] and rb._pair_segments is False
            if want_seg and rb._pairs is not None:
                rb.pair_segments()
                want_seg = False
            want_order = j["want_order"] and side._order is _UNSET
            if not (rows or want_table or want_pairs or want_seg or want_order):
                continue
            todo.append((rb, j["side"], dict(nbr=side.nbr, tile_rows=rows, want_order=want_order,
                                             want_table=want_table, want_pairs=want_pairs,
                                             want_segments=want_seg,
                                             ld=max(rb.n_in, rb.n_out, 1))))
        for (rb, side, job), res in zip(todo, K.rulebook_plan_many([t[2] for t in todo])):
            rb._planned(side, res, job["want_order"])
            if job["want_segments"] and res["segments"] is None:
                rb.pair_segments()              # chunked segment tables (MSMD_WGRAD_CHUNK_ROWS)


class _TableSide:
    """One neighbour table of a rulebook (nbr [K, n]: the output-stationary table of the
    forward pass or of dgrad) and what the conv kernels derive from it, each computed once:
    the tiling order of its rows (similar neighbour masks adjacent, tiles heaviest first),
    the table in that order, and the stream-K work table per tile height."""

    def __init__(self, nbr):
        self.nbr = nbr
        self._order = self._tiled = _UNSET
        self._prefix = {}

    def order(self):
        if self._order is _UNSET:
            self._order = K.rulebook_tiling(self.nbr, want_table=False)[0]
        return self._order

    def tiling(self):
        """(table, row_order) the split-bf16 kernel tiles a pass by: the table in mask-sorted
        tile order (column p belongs to row order[p]).
        SubM rulebooks serve 8 launches per step (4 convs x forward/dgrad), a strided
        conv's tables one launch each -- but those need it most: a stride-2 output
        row has ~5 of the 27 offsets and its neighbours in linear order all have
        different ones, so a 128-row tile in natural order walks every offset
        (issued / useful work 5.4 forward, 8.1 backward on the bench workload;
        1.8 / 1.0 sorted -- tools/order_sim.py).  The sort + permute (~100 us) runs
        in the index pass, off the feature pass."""
        if self._tiled is _UNSET:
            self._order, self._tiled = K.rulebook_tiling(self.nbr)
        return self._tiled, self._order

    def prefix(self, rows):
        """Stream-K work table of the tiling (K.tile_prefix) for tiles of `rows` rows
        (K.split_tile_rows of the layer's width): with it every workgroup of the split
        kernel takes the same share of the launch."""
        if rows not in self._prefix:
            self._prefix[rows] = K.tile_prefix(self.tiling()[0], rows)
        return self._prefix[rows]

    def take(self, res, keep_order):
        """Adopt one K.rulebook_plan / K.rulebook_plan_many result for this table."""
        if res["tiled"] is not None:
            self._order, self._tiled = res["order"], res["tiled"]
        elif keep_order and self._order is _UNSET:
            self._order = res["order"]
        self._prefix.update(res["prefix"])


class IndiceData:
    """One rulebook (spconv-2.x ImplicitGemmIndiceData's role,
    bug_fix/conv.py:416-436): the output-stationary neighbour tables plus,
    built lazily for the weight gradient, the reference-format pair lists."""

    def __init__(self, out_indices, indices, nbr_fwd, nbr_bwd, is_subm, spatial_shape,
                 out_spatial_shape, ksize, stride, padding, dilation, algo=None):
        self.out_indices = out_indices
        self.indices = indices
        self.fwd = _TableSide(nbr_fwd)          # [K, n_out]
        # [K, n_in]; a SubM rulebook's dgrad reads the forward table (with flipped weights)
        self.bwd = self.fwd if is_subm else _TableSide(nbr_bwd)
        self.is_subm = is_subm
        self.spatial_shape = spatial_shape
        self.out_spatial_shape = out_spatial_shape
        self.ksize, self.stride, self.padding, self.dilation = ksize, stride, padding, dilation
        self.algo = algo
        # True between build_rulebook() inside a plan_batch() and that context's exit: the
        # SubM table is allocated but not filled yet -- nothing may read it (table() checks)
        self.pending = False
        self._pairs = None              # (forward table only, like the segment table)
        self._pair_segments = False     # not computed yet (None = chunking off)
        self._inverted = None

    @property
    def nbr_fwd(self):
        return self.fwd.nbr

    @nbr_fwd.setter
    def nbr_fwd(self, nbr):
        self.fwd.nbr = nbr

    @property
    def nbr_bwd(self):
        return None if self.is_subm else self.bwd.nbr

    @nbr_bwd.setter
    def nbr_bwd(self, nbr):
        assert not self.is_subm, "a SubM rulebook has no input-side table of its own"
        self.bwd.nbr = nbr

    def inverted(self):
        """The rulebook of the inverse conv paired with this one (bug_fix/conv.py:350-362): the
        same pairs read the other way round -- the tables swapped (nbr_bwd is complete, so the
        inverse's forward and weight-gradient pairs are all there), input and output index sets
        and shapes swapped.  Tiling, order, prefix and pair caches of its own; built once."""
        if self.is_subm:
            raise RuntimeError("inverse conv can only be used with standard conv and pool ops.")
        if self.nbr_bwd is None:
            raise RuntimeError("this rulebook was built without its input-side table (nbr_bwd): "
                               "an inverse conv cannot use it")
        if self._inverted is None:
            self._inverted = IndiceData(self.indices, self.out_indices, self.nbr_bwd, self.nbr_fwd,
                                        False, list(self.out_spatial_shape),
                                        list(self.spatial_shape), self.ksize, self.stride,
                                        self.padding, self.dilation, self.algo)
        return self._inverted

    def check_ready(self):
        """Raise if the table cannot be read yet / any more (deferred fill still pending, or
        the launch set that should have filled it failed)."""
        if self.pending:
            raise RuntimeError("this SubM rulebook's table is filled when the enclosing "
                               "spconv.plan_batch() closes; it cannot be used inside it")
        if self.nbr_fwd is None:
            raise RuntimeError("this rulebook's table was never filled (its plan_batch() "
                               "failed); build it again")

    @property
    def n_in(self):
        return self.indices.shape[0]

    @property
    def n_out(self):
        return self.out_indices.shape[0]

    def pairs(self):
        """(indice_pairs[K,2,ld], indice_num[K]) -- spconv_ops.h:55-59 format."""
        if self._pairs is None:
            self._pairs = K.rulebook_pairs(self.nbr_fwd, ld=max(self.n_in, self.n_out, 1))
        return self._pairs

    def pair_segments(self):
        """Row-chunk segment table of the pair lists for the whole-block wgrad kernel
        (kernels.pair_segments), or None when chunking is off."""
        if self._pair_segments is False:
            self._pair_segments = K.pair_segments(*self.pairs())
        return self._pair_segments

    def prepare(self, need_grad, c_in=None, c_out=None):
        """Compute everything derived from the table now -- the pair lists when a
        weight gradient will be needed and, for a conv of c_in -> c_out channels,
        the tiling order / tile-ordered table its kernels will ask for (conv_needs) -- so
        that the feature pass enqueues no index work and never waits on the host.
        Inside `plan_batch()` the work is only recorded; the batch's exit runs it for
        all tables together (K.rulebook_plan_many: one launch set)."""
        kvol = self.nbr_fwd.shape[0]
        needs = ConvNeeds(None, None, False, need_grad, False, 0) if c_in is None else \
            conv_needs(c_in, c_out, kvol, self.n_in, self.n_out, need_grad, self.is_subm)
        asks, want_segments = [a for a in (needs.fwd, needs.bwd) if a], needs.want_segments
        batch = getattr(_PLAN, "batch", None)
        if batch is not None and (asks or need_grad) and kvol <= 31 and \
                self.n_out > 0 and self.n_in > 0:
            fwd = batch.job(self, "fwd")
            fwd["want_pairs"] |= need_grad
            fwd["want_segments"] |= want_segments
            for side, kernel, rows in asks:
                j = batch.job(self, side)
                if kernel == "split":
                    j["tile_rows"].add(rows)
                j["want_order"] |= kernel == "ordered"
            return self
        # one library call for what the split kernels want from each table (tiling
        # order, table in tile order, stream-K prefix, pair lists) instead of four:
        # the index pass is bound by host time
        for side in dict.fromkeys(a[0] for a in asks):
            rows = {r for s, kernel, r in asks if s == side and kernel == "split"}
            table = getattr(self, side)
            if rows and kvol <= 31 and table.nbr.shape[1] > 0 and table._tiled is _UNSET:
                want_pairs = side == "fwd" and need_grad and self._pairs is None
                self._planned(side, K.rulebook_plan(table.nbr, rows, want_pairs,
                                                    ld=max(self.n_in, self.n_out, 1)), False)
        if need_grad:
            self.pairs()
            if want_segments:
                self.pair_segments()
        for side, kernel, rows in asks:     # whatever is still missing (K > 31, empty tables)
            if kernel == "split":
                getattr(self, side).prefix(rows)
            elif kernel == "ordered":
                getattr(self, side).order()
        return self

    def _planned(self, side, res, keep_order):
        """Take one K.rulebook_plan / K.rulebook_plan_many result for the table of `side`."""
        getattr(self, side).take(res, keep_order)
        if res["pairs"] is not None:
            self._pairs = res["pairs"]
        if res.get("segments") is not None:
            self._pair_segments = res["segments"]


def build_rulebook(indices, batch_size, spatial_shape, ksize, stride, padding, dilation, subm,
                   algo=None, transposed=False, output_padding=(0, 0, 0)):
    if any(d != 1 for d in dilation):
        raise NotImplementedError("only dilation 1 is built (all reference configs use it)")
    if transposed:
        if subm:
            raise ValueError("a SubM conv cannot be transposed")
        out_idx, nbr_fwd, nbr_bwd, out_shape = K.rulebook_deconv(
            indices, batch_size, spatial_shape, ksize, stride, padding, output_padding)
        return IndiceData(out_idx, indices, nbr_fwd, nbr_bwd, False, list(spatial_shape),
                          list(out_shape), ksize, stride, padding, dilation, algo)
    if subm:
        if any(k % 2 == 0 for k in ksize):
            raise NotImplementedError("SubM needs odd kernel sizes")
        batch = getattr(_PLAN, "batch", None)
        # inside plan_batch(): the table is filled when the context closes, together with
        # every other SubM table of the index pass (K.rulebook_subm_many).  Only tables whose
        # prepare() is deferred too (K <= 31, not empty): nothing may read one before the exit.
        defer = batch is not None and SUBM_BATCHING and indices.shape[0] > 0 and \
            K.kernel_volume(ksize) <= 31 and indices.dtype == torch.int32 and \
            indices.is_contiguous()
        nbr = K.subm_table(indices, ksize) if defer else \
            K.rulebook_subm(indices, batch_size, spatial_shape, ksize)
        rb = IndiceData(indices, indices, nbr, None, True, list(spatial_shape),
                        list(spatial_shape), ksize, [1, 1, 1], [k // 2 for k in ksize],
                        dilation, algo)
        if defer:
            rb.pending = True
            batch.subm(rb, batch_size)
        return rb
    out_idx, nbr_fwd, nbr_bwd, out_shape = K.rulebook_conv(indices, batch_size, spatial_shape,
                                                           ksize, stride, padding)
    return IndiceData(out_idx, indices, nbr_fwd, nbr_bwd, False, list(spatial_shape),
                      list(out_shape), ksize, stride, padding, dilation, algo)


def rulebook_key(indices, spatial_shape, ksize, stride, padding, dilation, subm,
                 transposed=False, output_padding=(0, 0, 0)):
    """Key of a rulebook in SparseConvTensor._rb_cache (see there)."""
    key = (indices.data_ptr(), indices.shape[0], tuple(spatial_shape), tuple(ksize),
           tuple(stride), tuple(padding), tuple(dilation), bool(subm))
    if transposed:
        key += ("transposed", tuple(int(v) for v in K._expand3(output_padding)))
    return key


def _changes_set_otherwise(layer):
    """A transposed or inverse conv or a pool: a layer that changes the voxel set other than
    as a strided conv does."""
    return bool(getattr(layer, "transposed", False) or getattr(layer, "inverse", False)
                or getattr(layer, "is_pool", False))


class SparseConvTensor:

    def __init__(self, features: torch.Tensor, indices: torch.Tensor,
                 spatial_shape: List[int], batch_size: int, grid=None, voxel_num=None,
                 indice_dict: Optional[dict] = None, benchmark: bool = False):
        assert features.dim() == 2 and indices.dim() == 2
        assert indices.dtype == torch.int32, "indices must be int32 (b,z,y,x)"
        assert features.shape[0] == indices.shape[0], \
            f"{features.shape[0]} feature rows for {indices.shape[0]} voxels"
        self._features = features
        self.indices = indices
        self.spatial_shape = [int(s) for s in spatial_shape]
        self.batch_size = int(batch_size)
        self.indice_dict = {} if indice_dict is None else indice_dict
        self.grid = grid
        self.voxel_num = voxel_num
        self.benchmark = benchmark
        self.benchmark_record = {}
        self._timer = None
        self.thrust_allocator = None
        # rulebooks keyed by geometry + the identity of the indices tensor:
        # a rulebook depends on nothing else, so every SubM conv over the same
        # voxel set shares one (the reference rebuilds it for each of the 16
        # indice_key=None convs of SparseEncoder).  Results are identical.
        self._rb_cache = {}

    # spconv 2.x forbids `x.features = ...` (hence replace_feature); the legacy
    # type allowed it.  Both spellings work here.
    @property
    def features(self):
        return self._features

    @features.setter
    def features(self, val):
        self._features = val
        self.__dict__.pop("bn_stats", None)

    def replace_feature(self, feature: torch.Tensor):
        assert feature.shape[0] == self.indices.shape[0], \
            f"{feature.shape[0]} feature rows for {self.indices.shape[0]} voxels"
        new = self.shadow_copy()
        new._features = feature
        return new

    def shadow_copy(self):
        """A second handle on the same data (callers go on to re-point .indices /
        .features one after the other, so no row-count check here)."""
        new = SparseConvTensor.__new__(SparseConvTensor)
        new.__dict__.update(self.__dict__)
        # (the BatchNorm partials a conv leaves on ITS output describe those features only)
        new.__dict__.pop("bn_stats", None)
        return new

    @property
    def spatial_size(self):
        return int(np.prod(self.spatial_shape))

    @property
    def sparity(self):
        return self.indices.shape[0] / np.prod(self.spatial_shape) / self.batch_size

    def find_indice_pair(self, key) -> Optional[IndiceData]:
        if key is None:
            return None
        return self.indice_dict.get(key)

    def cached_rulebook(self, ksize, stride, padding, dilation, subm, transposed=False,
                        output_padding=(0, 0, 0)):
        # after voxel_modality_split the tensors carry 5-column indices
        # (b,mix,z,y,x: MSMDFusion.py:322-323); spconv asserts on ndim there too
        assert self.indices.shape[1] == 4, \
            f"sparse conv needs (b,z,y,x) indices, got {self.indices.shape[1]} columns"
        ident = rulebook_key(self.indices, self.spatial_shape, ksize, stride, padding, dilation,
                             subm, transposed, output_padding)
        hit = self._rb_cache.get(ident)
        # (an entry whose deferred fill failed is rebuilt, not handed out again)
        if hit is not None and hit.indices is self.indices and hit.nbr_fwd is not None:
            return hit
        rb = build_rulebook(self.indices, self.batch_size, self.spatial_shape, list(ksize),
                            list(stride), list(padding), list(dilation), subm,
                            transposed=transposed, output_padding=K._expand3(output_padding))
        self._rb_cache[ident] = rb
        return rb

    def seed_rulebook(self, conv, out_indices, nbr_fwd, nbr_bwd, out_shape):
        """File the rulebook of the plain strided `conv` over this tensor's voxel set -- its
        output set and tables computed elsewhere (the chains that count several output sets
        with one host read) -- where cached_rulebook() will look it up."""
        rb = IndiceData(out_indices, self.indices, nbr_fwd, nbr_bwd, False,
                        list(self.spatial_shape), list(out_shape), list(conv.kernel_size),
                        list(conv.stride), list(conv.padding), list(conv.dilation), None)
        self._rb_cache[rulebook_key(self.indices, self.spatial_shape, conv.kernel_size,
                                    conv.stride, conv.padding, conv.dilation, False)] = rb
        return rb

    def seed_strided_chain(self, convs):
        """The strided convs of `convs` (execution order) as ONE chain: when every conv
        between two of them keeps the voxel set (SubM), each strided conv's input set is the
        previous one's output set, and all their output sets can be counted on the device
        back to back with a single host read (kernels.rulebook_conv_chain) instead of one
        read per conv.  The rulebooks land in the shared cache under the keys plan() /
        forward() will look up; results are those of the level-by-level path.  The chain ends
        at the first layer that changes the voxel set otherwise (a transposed or inverse conv,
        a pool): those are left to plan()."""
        strided = []
        for c in convs:
            if _changes_set_otherwise(c):
                break
            if not c.subm and not getattr(c, "conv1x1", False):
                strided.append(c)
        if len(strided) < 2 or os.environ.get("MSMD_CONV_CHAIN", "1") != "1" or \
                any(d != 1 for c in strided for d in c.dilation):
            return
        geoms = [(list(c.kernel_size), list(c.stride), list(c.padding)) for c in strided]
        t = self
        for c, (out_idx, nbr_fwd, nbr_bwd, out_shape) in zip(
                strided, K.rulebook_conv_chain(t.indices, t.batch_size, t.spatial_shape, geoms)):
            t.seed_rulebook(c, out_idx, nbr_fwd, nbr_bwd, out_shape)
            t = t.shadow_copy()         # (shares the cache) the next conv's input set
            t.indices, t.spatial_shape = out_idx, list(out_shape)

    def plan(self, convs, need_grad, strided_outputs=None):
        """Index-only pre-pass: build (or fetch) the rulebook of every sparse
        layer in `convs` (execution order: spconv.sparse_convs(block)), following the
        voxel set through the ones that change it -- strided and transposed convs and
        max-pools to their output sets, an inverse conv back to its couple's input set.
        Rulebooks depend on indices only, never on features, so
        the whole chain -- including its host reads of output-voxel counts --
        runs before the first feature kernel; the feature pass then finds every
        rulebook in the shared cache.  `strided_outputs` (a list) receives the
        (indices, spatial_shape) after every set-changing layer, in order."""
        t = self
        with plan_batch():
            for conv in convs:
                if getattr(conv, "conv1x1", False):
                    continue
                if getattr(conv, "inverse", False):
                    # the couple: planned earlier (this call or an earlier one on this chain),
                    # or already in the tensor's indice_dict.  Without it the forward pass
                    # raises; nothing further can be planned.
                    couple = t.__dict__.get("_plan_keys", {}).get(conv.indice_key) or \
                        t.find_indice_pair(conv.indice_key)
                    if couple is None or couple.is_subm or couple.nbr_bwd is None:
                        break
                    rb = couple.inverted()
                else:
                    rb = t.find_indice_pair(conv.indice_key) if conv.subm else None
                    if rb is None:
                        rb = t.cached_rulebook(conv.kernel_size, conv.stride, conv.padding,
                                               conv.dilation, conv.subm,
                                               transposed=getattr(conv, "transposed", False),
                                               output_padding=getattr(conv, "output_padding",
                                                                      (0, 0, 0)))
                if not getattr(conv, "is_pool", False):     # (a pool reads nbr_bwd only)
                    rb.prepare(need_grad, conv.in_channels, conv.out_channels)
                if not conv.subm:
                    keys = t.__dict__.get("_plan_keys", {})
                    t = t.shadow_copy()
                    if conv.indice_key is not None and not getattr(conv, "inverse", False):
                        t._plan_keys = dict(keys, **{conv.indice_key: rb})
                    t.indices = rb.out_indices
                    t._features = t._features.new_empty((rb.out_indices.shape[0], 0))
                    t.spatial_shape = rb.out_spatial_shape
                    if strided_outputs is not None:
                        strided_outputs.append((rb.out_indices, list(rb.out_spatial_shape)))
        return t

    def dense(self, channels_first: bool = True):
        """[B,C,D,H,W] (structure.py:55-64); channels_last returns the permuted
        view of the same buffer."""
        assert self.indices.shape[1] == 4, \
            f"dense() needs (b,z,y,x) indices, got {self.indices.shape[1]} columns"
        out = _dense(self._features, self.indices, self.batch_size, self.spatial_shape)
        if channels_first:
            return out
        nd = len(self.spatial_shape)
        return out.permute(0, *range(2, nd + 2), 1).contiguous()
