"""The bitmap set builder behind the strided, transposed and union rulebooks (csrc/voxel_set.hpp,
rulebook.hip, dense.hip) without a GPU: that the union set and the strided builder size one
workspace layout, that the chain sizes are the sums of kernels.py's 256-byte regions, and the
status code of every rejected call.  Every call here is refused before anything is enqueued:
the device addresses are made up and never dereferenced."""
import ctypes as C

import pytest

from msmdfusion_amd import kernels as K
from msmdfusion_amd._lib import int3, lib

INVALID_ARG, WORKSPACE, UNSUPPORTED, RANGE = -1, -2, -3, -5    # msmd_status


# ((3, [5, 7, 3]): 315 cells, no multiple of the bitmap's 32-cell words)
@pytest.mark.parametrize("batch,shape", [(1, [1, 1, 1]), (1, [41, 16, 16]), (3, [5, 7, 3]),
                                         (2, [41, 1440, 1440])])
def test_union_and_strided_sets_share_one_workspace_layout(batch, shape):
    """add_conv_chain sizes a union region with the conv query, lets the chain call carve it and
    hands the same bytes to msmd_sparse_add_fill."""
    conv = lib.msmd_rulebook_conv_workspace_bytes(batch, int3(shape))
    assert conv > 0 and conv % 256 == 0
    assert lib.msmd_sparse_add_workspace_bytes(batch, int3(shape)) == conv


def test_chain_workspaces_are_sums_of_level_regions():
    batch = 2
    geo = K._StridedGeometry([41, 64, 64], [(3, 2, 1)] * 3)
    assert geo.in_shape == [[41, 64, 64], [21, 32, 32], [11, 16, 16]]
    assert geo.out_shape == [[21, 32, 32], [11, 16, 16], [6, 8, 8]]
    assert list(geo.f_out) == [21, 32, 32, 11, 16, 16, 6, 8, 8]
    conv = [K._region_bytes(batch, s) for s in geo.out_shape]
    union = [0] + [K._region_bytes(batch, s) for s in geo.in_shape[1:]]
    assert all(v % 256 == 0 for v in conv + union)
    assert lib.msmd_rulebook_conv_chain_workspace_bytes(batch, 3, geo.f_out) == sum(conv)
    assert lib.msmd_rulebook_add_conv_chain_workspace_bytes(batch, 3, geo.f_in, geo.f_out) \
        == sum(conv) + sum(union)


# ---- rejection codes ---------------------------------------------------------------------------
# The codes below were recorded by running this table against the library as it was before the
# set builder moved into voxel_set.hpp, on a machine without a GPU.  One case could only be
# recorded there: `broken_chain` is refused at level 1, and the library as it was had enqueued
# level 0 -- on these made-up addresses -- by then.  msmd_rulebook_add_conv_count_chain now
# checks every level before its first launch, and the case depends on that: the code is the
# recorded one, and nothing is enqueued.
IDX, CNT, WS = 0x10000, 0x20000, 0x30000    # made-up device addresses (WS is 256-aligned)
HUGE = 1 << 62
SHAPE = [4, 6, 6]
KS, ST, PD = [3, 3, 3], [2, 2, 2], [1, 1, 1]
# a two-level chain from [8, 12, 12]
CH_IN = [[8, 12, 12], [4, 6, 6]]
CH_OUT = [[4, 6, 6], [2, 3, 3]]


def _arr(v):
    """None stays a null pointer; a list of rows or of ints becomes a flat int array."""
    if v is None:
        return None
    flat = [int(x) for r in v for x in r] if isinstance(v[0], (list, tuple)) else list(v)
    return (C.c_int * len(flat))(*flat)


def _count(fn):
    def call(indices=IDX, n=4, batch=1, shape=SHAPE, ks=KS, st=ST, pd=PD, n_out=CNT, ws=None,
             ws_bytes=0):
        return fn(indices, n, batch, _arr(shape), _arr(ks), _arr(st), _arr(pd), n_out, ws,
                  ws_bytes, None)
    return call


def _fill(fn):
    def call(indices=IDX, n=4, batch=1, shape=SHAPE, ks=KS, st=ST, pd=PD, n_out=3, ws=None,
             ws_bytes=0):
        return fn(indices, n, batch, _arr(shape), _arr(ks), _arr(st), _arr(pd), n_out, IDX, IDX,
                  IDX, ws, ws_bytes, None)
    return call


def _conv_chain(indices=IDX, n=4, batch=1, levels=2, shape=CH_OUT, ks=(KS, KS), st=(ST, ST),
                pd=(PD, PD), n_out=CNT, ws=None, ws_bytes=0):
    return lib.msmd_rulebook_conv3d_count_chain(indices, n, batch, levels, _arr(shape), _arr(ks),
                                                _arr(st), _arr(pd), n_out, ws, ws_bytes, None)


def _add_chain(n=4, batch=1, levels=2, in_shape=CH_IN, shape=CH_OUT, ks=(KS, KS), st=(ST, ST),
               pd=(PD, PD), n_out=CNT, ws=None, ws_bytes=0):
    extra = (C.c_void_p * 2)(IDX, IDX)
    return lib.msmd_rulebook_add_conv_count_chain(extra, _arr([n, 4]), batch, levels,
                                                  _arr(in_shape), _arr(shape), _arr(ks), _arr(st),
                                                  _arr(pd), n_out, ws, ws_bytes, None)


def _add_count(n=4, batch=1, shape=SHAPE, n_out=CNT, ws=None, ws_bytes=0):
    return lib.msmd_sparse_add_count(IDX, n, IDX, 4, batch, _arr(shape), n_out, ws, ws_bytes, None)


def _add_fill(n=4, batch=1, shape=SHAPE, ws=None, ws_bytes=0):
    return lib.msmd_sparse_add_fill(None, IDX, n, None, IDX, 4, 0, batch, _arr(shape), 3, IDX,
                                    None, IDX, IDX, ws, ws_bytes, None)


_ONE = lib.msmd_rulebook_conv_workspace_bytes(1, int3(SHAPE))
_CONV_CHAIN = lib.msmd_rulebook_conv_chain_workspace_bytes(1, 2, _arr(CH_OUT))
_ADD_CHAIN = lib.msmd_rulebook_add_conv_chain_workspace_bytes(1, 2, _arr(CH_IN), _arr(CH_OUT))

# The single calls check the workspace last, so every case of theirs keeps the null workspace of
# the defaults: a call that passed the check under test would still be refused.  The chain calls
# check the workspace before the geometry: their geometry cases carry a (made-up) workspace and
# put the bad value where it is met before the first launch.
_GEOMETRY = dict(
    null_stride=(dict(st=None), INVALID_ARG),
    null_padding=(dict(pd=None), INVALID_ARG),
    negative_n=(dict(n=-1), INVALID_ARG),
    null_count=(dict(n_out=None), INVALID_ARG),
    zero_extent=(dict(shape=[4, 0, 6]), INVALID_ARG),
    kernel_volume=(dict(ks=[17, 17, 17]), UNSUPPORTED),
    too_many_cells=(dict(shape=[70000] * 3), RANGE),
)


def _cases(need, *names, **more):
    cases = {k: _GEOMETRY[k] for k in names}
    cases["null_workspace"] = (dict(), WORKSPACE)
    cases["short_workspace"] = (dict(ws=WS, ws_bytes=need - 1), WORKSPACE)
    cases.update(more)
    return cases


_COUNT_CASES = _cases(_ONE, *_GEOMETRY)
_FILL_CASES = _cases(_ONE, *(k for k in _GEOMETRY if k != "null_count"))
_SET_CASES = ("negative_n", "zero_extent", "too_many_cells")


def _chain_cases(need, rows):
    """The geometry cases of a chain call: the bad value sits in level 0."""
    big = dict(ws=WS, ws_bytes=HUGE)
    return _cases(
        need, "null_stride", "null_padding", "negative_n", "null_count",
        zero_extent=(dict(shape=[[4, 0, 6], CH_OUT[1]], **big), INVALID_ARG),
        kernel_volume=(dict(ks=([17, 17, 17], KS), **big), UNSUPPORTED),
        too_many_cells=(dict(shape=[[70000] * 3, CH_OUT[1]], **big), RANGE),
        unaligned_workspace=(dict(ws=WS + 16, ws_bytes=HUGE), WORKSPACE),
        no_levels=(dict(levels=0), INVALID_ARG), **rows)


ENTRY_POINTS = {
    "conv3d_count": (_count(lib.msmd_rulebook_conv3d_count), _COUNT_CASES),
    "conv3d_fill": (_fill(lib.msmd_rulebook_conv3d_fill), _FILL_CASES),
    "deconv3d_count": (_count(lib.msmd_rulebook_deconv3d_count), _COUNT_CASES),
    "deconv3d_fill": (_fill(lib.msmd_rulebook_deconv3d_fill), _FILL_CASES),
    "conv3d_count_chain": (_conv_chain, _chain_cases(_CONV_CHAIN, {})),
    "add_conv_count_chain": (_add_chain, _chain_cases(_ADD_CHAIN, dict(
        # (the row counts of this call are checked per level, behind the workspace)
        negative_n=(dict(n=-1, ws=WS, ws_bytes=HUGE), INVALID_ARG),
        zero_input_extent=(dict(in_shape=[[8, 0, 12], CH_IN[1]], ws=WS, ws_bytes=HUGE),
                           INVALID_ARG),
        # level 1's input grid is not level 0's output grid (see the note above)
        broken_chain=(dict(in_shape=[CH_IN[0], [4, 6, 7]], ws=WS, ws_bytes=HUGE), INVALID_ARG)))),
    "sparse_add_count": (_add_count, _cases(_ONE, "null_count", *_SET_CASES)),
    "sparse_add_fill": (_add_fill, _cases(_ONE, *_SET_CASES)),
}


@pytest.mark.parametrize("entry", list(ENTRY_POINTS))
def test_rejection_codes(entry):
    call, cases = ENTRY_POINTS[entry]
    got = {name: call(**args) for name, (args, _) in cases.items()}
    assert got == {name: code for name, (_, code) in cases.items()}
