"""Host logic between the index pass and the sparse-conv launches (no GPU): the rulebook
cache key and its seeding, that IndiceData.prepare() starts from the same needs
(functional.conv_needs) inside and outside a plan_batch, that its immediate path makes a
pinned list of library calls, and that a SubM rulebook has one table side."""
import types

import pytest
import torch

from msmdfusion_amd.spconv import core
from msmdfusion_amd.spconv.functional import conv_needs

K3S2P1 = types.SimpleNamespace(kernel_size=[3, 3, 3], stride=[2, 2, 2], padding=[1, 1, 1],
                               dilation=[1, 1, 1])


def _tensor(shape=(8, 8, 8)):
    idx = torch.zeros((10, 4), dtype=torch.int32)
    idx[:, 3] = torch.arange(10, dtype=torch.int32) % 8
    idx[:, 2] = torch.arange(10, dtype=torch.int32) // 8
    return core.SparseConvTensor(torch.zeros((10, 4)), idx, list(shape), 1)


def test_seeded_rulebooks_are_found(monkeypatch):
    def no_build(*a, **k):
        raise AssertionError("build_rulebook reached")
    monkeypatch.setattr(core, "build_rulebook", no_build)
    t = _tensor()
    out_idx = torch.zeros((3, 4), dtype=torch.int32)
    tables = torch.zeros((27, 3), dtype=torch.int32), torch.zeros((27, 10), dtype=torch.int32)
    rb = t.seed_rulebook(K3S2P1, out_idx, *tables, [4, 4, 4])
    assert t.cached_rulebook([3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1], False) is rb
    assert rb.indices is t.indices and rb.out_indices is out_idx and not rb.is_subm
    assert rb.spatial_shape == [8, 8, 8] and rb.out_spatial_shape == [4, 4, 4]
    assert (rb.nbr_fwd is tables[0]) and (rb.nbr_bwd is tables[1])
    # the same indices tensor on a grid of another shape: another key, a miss
    other = _tensor((8, 8, 16))
    other.indices = t.indices
    other._rb_cache = t._rb_cache
    with pytest.raises(AssertionError, match="build_rulebook reached"):
        other.cached_rulebook([3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1], False)
    g = (t.indices, [8, 8, 8], [3, 3, 3])
    keys = [core.rulebook_key(*g, [1, 1, 1], [1, 1, 1], [1, 1, 1], True),
            core.rulebook_key(*g, [1, 1, 1], [1, 1, 1], [1, 1, 1], False),
            core.rulebook_key(*g, [2, 2, 2], [1, 1, 1], [1, 1, 1], False),
            core.rulebook_key(*g, [2, 2, 2], [1, 1, 1], [1, 1, 1], False, transposed=True),
            core.rulebook_key(*g, [2, 2, 2], [1, 1, 1], [1, 1, 1], False, transposed=True,
                              output_padding=1)]
    assert len(set(keys)) == len(keys)
    assert "transposed" in keys[3] and "transposed" not in keys[2]
    assert keys[0] == (t.indices.data_ptr(), 10, (8, 8, 8), (3, 3, 3), (1, 1, 1), (1, 1, 1),
                       (1, 1, 1), True)


# ---- the routing table -----------------------------------------------------------------------
N = 300                     # rows of every table: 3 tiles of 128 rows, 2 of 256
WORK = ("rulebook_plan", "rulebook_plan_many", "rulebook_tiling", "tile_prefix",
        "rulebook_pairs", "pair_segments")


def _install_fakes(monkeypatch):
    """Recording fakes of the library calls prepare() and plan_batch make.  Tables carry their
    side in their values (forward 0, input side 1) and the fakes' tile-ordered tables keep it,
    so every call is recorded with the side it works on."""
    log = []

    def side(nbr):
        return "bwd" if int(nbr.reshape(-1)[0]) else "fwd"

    def prefix(nbr, rows):
        return torch.zeros(((nbr.shape[1] + rows - 1) // rows + 1,), dtype=torch.int32)

    def pairs(nbr, ld):
        return (torch.zeros((nbr.shape[0], 2, ld), dtype=torch.int32),
                torch.zeros((nbr.shape[0],), dtype=torch.int32))

    def rulebook_plan(nbr, tile_rows=(), want_pairs=False, ld=None):
        # (ld only sizes the pair lists: the library does not read it without them)
        log.append(("rulebook_plan", side(nbr), sorted(tile_rows), bool(want_pairs),
                    ld if want_pairs else None))
        return dict(order=torch.zeros((nbr.shape[1],), dtype=torch.int32), tiled=nbr.clone(),
                    prefix={r: prefix(nbr, r) for r in tile_rows},
                    pairs=pairs(nbr, ld) if want_pairs else None)

    def rulebook_plan_many(jobs):
        log.append(("rulebook_plan_many", len(jobs)))
        out = []
        for j in jobs:
            nbr, seg = j["nbr"], bool(j.get("want_segments"))
            table = bool(j.get("want_table")) or bool(j.get("tile_rows"))
            out.append(dict(order=torch.zeros((nbr.shape[1],), dtype=torch.int32),
                            tiled=nbr.clone() if table else None,
                            prefix={r: prefix(nbr, r) for r in j.get("tile_rows") or ()},
                            pairs=pairs(nbr, j["ld"]) if j.get("want_pairs") or seg else None,
                            segments=(torch.zeros((3 * nbr.shape[0] + 1,), dtype=torch.int32), 1)
                            if seg else None))
        return out

    def rulebook_tiling(nbr, want_table=True):
        log.append(("rulebook_tiling", side(nbr), bool(want_table)))
        return (torch.zeros((nbr.shape[1],), dtype=torch.int32),
                nbr.clone() if want_table else None)

    def tile_prefix(nbr, rows):
        log.append(("tile_prefix", side(nbr), rows))
        return prefix(nbr, rows)

    def rulebook_pairs(nbr, ld=None):
        log.append(("rulebook_pairs", side(nbr), ld))
        return pairs(nbr, ld)

    def pair_segments(prs, num):
        log.append(("pair_segments",))
        return torch.zeros((3 * prs.shape[0] + 1,), dtype=torch.int32), 1

    def asked(name, fn):        # the predicates: recorded too, but they launch nothing
        def f(*a):
            log.append((name,) + a)
            return fn(*a)
        return f
    fakes = dict(rulebook_plan=rulebook_plan, rulebook_plan_many=rulebook_plan_many,
                 rulebook_tiling=rulebook_tiling, tile_prefix=tile_prefix,
                 rulebook_pairs=rulebook_pairs, pair_segments=pair_segments,
                 rulebook_subm_many=lambda jobs: None,
                 split_tile_rows=asked("split_tile_rows", lambda c: 256 if c <= 64 else 128),
                 split_supported=asked("split_supported", lambda ci, co, kvol=27:
                                       ci >= 32 and co >= 32 and ci % 8 == 0),
                 wgrad_split_supported=asked("wgrad_split_supported", lambda ci, co:
                                             ci % 64 == 0 and co % 64 == 0))
    for name, f in fakes.items():
        monkeypatch.setattr(core.K, name, f)
    monkeypatch.delenv("MSMD_CONV_PLANES", raising=False)
    monkeypatch.setattr(core, "PLAN_BATCHING", True)
    monkeypatch.setattr(core, "PLAN_SCOPE", "call")
    return log


@pytest.fixture
def lib(monkeypatch):
    return _install_fakes(monkeypatch)


def _rulebook(subm, kvol=27):
    idx = torch.zeros((N, 4), dtype=torch.int32)
    out_idx = idx if subm else torch.zeros((N, 4), dtype=torch.int32)
    return core.IndiceData(out_idx, idx, torch.zeros((kvol, N), dtype=torch.int32),
                           None if subm else torch.ones((kvol, N), dtype=torch.int32), subm,
                           [8, 8, 8], [8, 8, 8], [3, 3, 3], [1, 1, 1], [1, 1, 1], [1, 1, 1])


def _state(rb):
    """What has ended up on a rulebook, per side: (tiled?, order?, prefix heights), then
    pair lists? and segment table?."""
    def side(s):
        return (s._tiled is not core._UNSET, s._order is not core._UNSET, sorted(s._prefix))
    return (side(rb.fwd), None if rb.is_subm else side(rb.bwd), rb._pairs is not None,
            rb._pair_segments is not False)


# Per (c_in, c_out): the state the kernels' routing asks for -- split forward / split dgrad
# (64 -> 64; 64 -> 192 with 128-row forward and 256-row dgrad tiles), ordered fp32 forward /
# plain dgrad (16 -> 64), plain both ways (5 -> 16) -- and the library calls of the IMMEDIATE
# path.  The call lists were recorded by running this test body against the commit before
# IndiceData got its table sides (there through the then _order_* / _tiled_* / _prefix_*
# fields): they pin "the same library calls as before".  Pinned are the calls that launch or
# allocate (WORK); the predicates are asked once by conv_needs now, where each copy of the
# decision used to ask them again.
KERNELS = {(64, 64): ("split", "split"), (16, 64): ("ordered", "plain"),
           (5, 16): ("plain", "plain"), (64, 192): ("split", "split")}      # forward, dgrad
NONE, ORDER = (False, False, []), (False, True, [])


def TILED(*heights):
    return (True, True, list(heights))


PLAN, PAIRS, SEG = "rulebook_plan", ("rulebook_pairs", "fwd", N), ("pair_segments",)
ORDER_FWD = ("rulebook_tiling", "fwd", False)
EXPECTED = {
    # (c_in, c_out, need_grad, subm): ((forward side, input side, pairs?, segments?), calls)
    (64, 64, False, True): ((TILED(256), None, False, False), [(PLAN, "fwd", [256], False, None)]),
    (16, 64, False, True): ((ORDER, None, False, False), [ORDER_FWD]),
    (5, 16, False, True): ((NONE, None, False, False), []),
    (64, 192, False, True): ((TILED(128), None, False, False),
                             [(PLAN, "fwd", [128], False, None)]),
    (64, 64, True, True): ((TILED(256), None, True, True), [(PLAN, "fwd", [256], True, N), SEG]),
    (16, 64, True, True): ((ORDER, None, True, False), [PAIRS, ORDER_FWD]),
    (5, 16, True, True): ((NONE, None, True, False), [PAIRS]),
    (64, 192, True, True): ((TILED(128, 256), None, True, True),
                            [(PLAN, "fwd", [128, 256], True, N), SEG]),
    (64, 64, False, False): ((TILED(256), NONE, False, False),
                             [(PLAN, "fwd", [256], False, None)]),
    (16, 64, False, False): ((ORDER, NONE, False, False), [ORDER_FWD]),
    (5, 16, False, False): ((NONE, NONE, False, False), []),
    (64, 192, False, False): ((TILED(128), NONE, False, False),
                              [(PLAN, "fwd", [128], False, None)]),
    (64, 64, True, False): ((TILED(256), TILED(256), True, True),
                            [(PLAN, "fwd", [256], True, N), (PLAN, "bwd", [256], False, None),
                             SEG]),
    (16, 64, True, False): ((ORDER, NONE, True, False), [PAIRS, ORDER_FWD]),
    (5, 16, True, False): ((NONE, NONE, True, False), [PAIRS]),
    (64, 192, True, False): ((TILED(128), TILED(256), True, True),
                             [(PLAN, "fwd", [128], True, N), (PLAN, "bwd", [256], False, None),
                              SEG]),
}
K125_CALLS = [PAIRS, SEG, ("rulebook_tiling", "fwd", True), ("tile_prefix", "fwd", 256),
              ("rulebook_tiling", "bwd", True), ("tile_prefix", "bwd", 256)]


@pytest.mark.parametrize("subm", [True, False])
@pytest.mark.parametrize("need_grad", [False, True])
@pytest.mark.parametrize("c_in,c_out", [(64, 64), (16, 64), (5, 16), (64, 192)])
def test_both_paths_start_from_the_same_needs(lib, c_in, c_out, need_grad, subm):
    now = _rulebook(subm).prepare(need_grad, c_in, c_out)
    calls = [c for c in lib if c[0] in WORK]
    del lib[:]
    with core.plan_batch():
        batched = _rulebook(subm)
        assert batched.prepare(need_grad, c_in, c_out) is batched
        assert not [c for c in lib if c[0] in WORK]             # only recorded so far
    many = [c for c in lib if c[0] in WORK]
    assert [c[0] for c in many] == ["rulebook_plan_many"], many
    needs = conv_needs(c_in, c_out, 27, N, N, need_grad, subm)
    assert needs.fwd[1] == KERNELS[c_in, c_out][0] and needs.fwd[0] == "fwd"
    assert needs.bwd == (None if not need_grad else
                         ("fwd" if subm else "bwd", KERNELS[c_in, c_out][1],
                          256 if KERNELS[c_in, c_out][1] == "split" else None))
    state, expected_calls = EXPECTED[(c_in, c_out, need_grad, subm)]
    assert _state(now) == _state(batched) == state
    assert calls == expected_calls


def test_a_k125_table_never_batches(lib):
    """K > 31: the library's one-call plans do not cover it; inside a plan_batch too the
    lazy getters run at once."""
    with core.plan_batch():
        batched = _rulebook(False, kvol=125).prepare(True, 64, 64)
        inside = [c for c in lib if c[0] in WORK]
    # (nothing was left for the exit: its launch set is empty)
    assert [c for c in lib if c[0] in WORK] == inside + [("rulebook_plan_many", 0)]
    del lib[:]
    now = _rulebook(False, kvol=125).prepare(True, 64, 64)
    assert [c for c in lib if c[0] in WORK] == inside == K125_CALLS
    assert _state(now) == _state(batched) == (TILED(256), TILED(256), True, True)


def test_a_subm_rulebook_has_one_side(lib):
    rb = _rulebook(True)
    assert rb.bwd is rb.fwd and rb.nbr_bwd is None
    strided = _rulebook(False)
    assert strided.bwd is not strided.fwd and strided.bwd.nbr is strided.nbr_bwd
    rb.fwd.tiling()
    got = rb.bwd.prefix(128)
    assert rb.fwd._prefix[128] is got
    assert [c for c in lib if c[0] in WORK] == [("rulebook_tiling", "fwd", True),
                                                ("tile_prefix", "fwd", 128)]
    # ... and a poisoned table is seen through both spellings
    rb.nbr_fwd = None
    assert rb.fwd.nbr is None
    with pytest.raises(RuntimeError, match="never filled"):
        rb.check_ready()
