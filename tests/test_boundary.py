"""The drop-in boundary, checked without a GPU: libmsmd_hip.so loads, exports
every symbol include/msmd_hip.h declares, the ctypes table mirrors the header,
argument validation works on the host side, and the product package never
touches the oracle."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "msmd_hip.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(msmd_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        args = [a.strip() for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
        decls[m.group(1)] = len(args)
    return decls


def test_library_exports_every_declared_symbol():
    from msmdfusion_amd import _lib
    decls = _declared()
    assert len(decls) >= 28
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r" T (msmd_\w+)", nm))
    assert set(decls) <= exported, sorted(set(decls) - exported)
    assert exported <= set(decls), "undeclared exports: %s" % sorted(exported - set(decls))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in decls:
        assert getattr(lib, name) is not None


def test_ctypes_table_mirrors_header():
    from msmdfusion_amd import _lib
    decls = _declared()
    assert set(_lib.SIGNATURES) == set(decls)
    for name, (_, argtypes) in _lib.SIGNATURES.items():
        assert len(argtypes) == decls[name], name
    assert _lib.lib.msmd_abi_version() == _lib.ABI_VERSION
    assert _lib.lib.msmd_status_string(0) == b"ok"
    assert b"workspace" in _lib.lib.msmd_status_string(-2)


def test_descriptor_structs_mirror_the_header(tmp_path):
    """The ctypes mirrors of the descriptor structs the *_many entry points take from the host
    (msmd_plan_desc, msmd_subm_desc) have the header's size and field offsets (gcc)."""
    import ctypes as C
    from msmdfusion_amd import kernels as K
    fields = {"msmd_plan_desc": (K._PlanDesc, ["nbr", "kvol", "n_rows", "order", "tiled",
                                               "prefix128", "prefix256", "indice_pairs",
                                               "indice_num", "segtab", "ld"]),
              "msmd_subm_desc": (K._SubmDesc, ["indices", "n", "batch_size", "spatial_shape",
                                               "ksize", "method", "nbr"])}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "msmd_hip.h"', 'int main(void) {']
    for name, (_, fs) in fields.items():
        src.append('printf("%s %%zu", sizeof(%s));' % (name, name))
        for f in fs:
            src.append('printf(" %%zu", offsetof(%s, %s));' % (name, f))
        src.append('printf("\\n");')
    src.append("return 0; }")
    c = tmp_path / "descs.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "descs"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    for line in filter(None, out):
        name, size, *offs = line.split()
        cls, fs = fields[name]
        assert C.sizeof(cls) == int(size), name
        assert [getattr(cls, f).offset for f in fs] == [int(o) for o in offs], name


def test_host_side_argument_validation():
    """Bad arguments are rejected before anything is enqueued (no GPU needed)."""
    from msmdfusion_amd._lib import float_arr, int3, lib
    assert lib.msmd_hard_voxelize(None, 10, 5, float_arr([0.1] * 3), float_arr([0, 0, 0, 1, 1, 1]),
                                  10, 100, None, None, None, None, None, None, 0, None) == -1
    assert lib.msmd_rulebook_subm3d(None, -1, 1, int3([4, 4, 4]), int3([3, 3, 3]), None, None, 0,
                                    None) == -1
    # 70000^3 cells cannot be indexed with 32-bit linear ids
    assert lib.msmd_rulebook_subm3d(None, 0, 1, int3([70000] * 3), int3([3, 3, 3]), None, None, 0,
                                    None) == -5
    assert lib.msmd_spconv_fwd_f32(None, 0, 16, None, None, 0, 10, 27, 0, None, None, None, 16,
                                   None) == -1
    # c_out = 7*16 has no built kernel
    assert lib.msmd_spconv_fwd_f32(ctypes.c_void_p(256), 1, 16, ctypes.c_void_p(256),
                                   ctypes.c_void_p(256), 1, 1, 27, 0, None, None,
                                   ctypes.c_void_p(256), 112, None) == -3
    assert lib.msmd_rulebook_row_masks(None, 100, 0, None, None, None) == -3
    assert lib.msmd_bn_act_fwd_f32(None, None, 10, 6, None, None, None, None, 1, 0.1, 1e-3, 1,
                                   None, None, None, None, 0, None) != 0
    assert lib.msmd_voxelize_workspace_bytes(30000, 120000, 10) > 120000 * 10 * 4
    assert lib.msmd_spconv_packed_weight_elems(27, 5, 16) == 27 * 1 * 1 * 256
    assert lib.msmd_device_ok() in (0, 1)


def test_planning_calls_refuse_bad_arguments_host_side():
    """msmd_rulebook_tiling / _plan / _pairs / _plan_many validate everything before the first
    launch.  The codes are the ones the table-by-table implementation returned (recorded
    there; msmd_rulebook_plan's two pair-list checks ran after its tiling launches there and
    returned the same code): the single-table calls are launch sets of one table now."""
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd._lib import lib
    p, big = ctypes.c_void_p(256), 1 << 24        # (never dereferenced: every call is refused)
    INVALID, WORKSPACE, UNSUPPORTED, RANGE = -1, -2, -3, -5
    plan = lib.msmd_rulebook_plan
    assert plan(p, 27, 0, 128, p, p, None, None, None, 0, None, p, big, None) == INVALID   # no rows
    assert plan(p, 27, 10, 128, None, p, None, None, None, 0, None, p, big, None) == INVALID
    assert plan(p, 27, 10, 128, p, None, None, None, None, 0, None, p, big, None) == INVALID
    assert plan(p, 40, 10, 128, p, p, None, None, None, 0, None, p, big, None) == UNSUPPORTED
    assert plan(p, 27, 10, 128, p, p, None, None, p, 10, None, p, big, None) == INVALID   # no num
    assert plan(p, 27, 10, 128, p, p, None, None, p, 9, p, p, big, None) == INVALID       # ld < n
    assert plan(p, 27, 10, 128, p, p, None, None, None, 0, None, p, 0, None) == WORKSPACE
    assert plan(p, 27, 10, 128, p, p, None, None, None, 0, None, ctypes.c_void_p(260), big,
                None) == WORKSPACE
    tiling = lib.msmd_rulebook_tiling
    assert tiling(p, 0, 10, 128, p, p, p, big, None) == UNSUPPORTED
    assert tiling(p, 32, 10, 128, p, p, p, big, None) == UNSUPPORTED
    assert tiling(p, 27, -1, 128, p, p, p, big, None) == INVALID
    assert tiling(p, 27, 10, 0, p, p, p, big, None) == INVALID
    assert tiling(p, 27, 10, 128, None, p, p, big, None) == INVALID
    assert tiling(None, 27, 0, 128, None, None, None, 0, None) == 0                       # empty: ok
    assert tiling(p, 27, 10, 128, p, None, p, 0, None) == WORKSPACE
    pairs = lib.msmd_rulebook_pairs
    assert pairs(p, 0, 10, p, 10, p, p, big, None) == INVALID
    assert pairs(p, 125, 10, p, 10, None, p, big, None) == INVALID
    assert pairs(p, 125, 10, p, -1, p, p, big, None) == INVALID
    assert pairs(p, 125, 10, None, 10, p, p, big, None) == INVALID
    assert pairs(p, 4096, 1 << 20, p, 1 << 20, p, p, big, None) == RANGE
    assert pairs(p, 125, 10, p, 10, p, p, 0, None) == WORKSPACE
    many = lib.msmd_rulebook_plan_many

    def desc(**kw):
        d = (K._PlanDesc * 1)()
        for k, v in dict(dict(nbr=256, kvol=27, n_rows=10, order=256, ld=10), **kw).items():
            setattr(d[0], k, v)
        return d
    assert many(desc(), -1, p, big, None) == INVALID
    assert many(None, 1, p, big, None) == INVALID
    assert many(None, 0, None, 0, None) == 0
    assert many(desc(), 1, None, big, None) == WORKSPACE
    assert many(desc(), 1, p, 0, None) == WORKSPACE
    assert many(desc(kvol=40), 1, p, big, None) == UNSUPPORTED
    assert many(desc(n_rows=-1), 1, p, big, None) == INVALID
    assert many(desc(nbr=None), 1, p, big, None) == INVALID
    assert many(desc(order=None, tiled=256), 1, p, big, None) == INVALID       # a table needs an order
    assert many(desc(prefix128=256), 1, p, big, None) == INVALID               # a prefix needs a table
    assert many(desc(indice_pairs=256), 1, p, big, None) == INVALID            # pairs need counts
    assert many(desc(indice_pairs=256, indice_num=256, ld=9), 1, p, big, None) == INVALID
    assert many(desc(segtab=256), 1, p, big, None) == INVALID                  # segments need pairs
    assert many(desc(kvol=31, n_rows=1 << 27, ld=1 << 27), 1, p, big, None) == RANGE


def test_many_calls_refuse_a_bad_descriptor_of_a_later_launch_set_host_side():
    """msmd_hard_voxelize_many, msmd_rulebook_subm3d_many and msmd_rows_where_eq_many check
    every descriptor of the call, and the first two the workspace against the largest launch
    set, before the first fill or launch: a bad entry in a LATER launch set (12, 16 and 16
    entries per set) is refused with nothing enqueued -- here, where there is no device to
    enqueue on.  The single calls are the one-descriptor case and return their codes as before
    (test_host_side_argument_validation)."""
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd._lib import float_arr, int3, lib
    INVALID, WORKSPACE, RANGE = -1, -2, -5
    p, big = ctypes.c_void_p(256), 1 << 30        # (never dereferenced: every call is refused)

    vox = (K._VoxDesc * 13)()
    for d in vox:
        d.points, d.num_points, d.num_features = 256, 100, 5
        d.voxel_size[:] = [0.1] * 3
        d.coors_range[:] = [0, 0, 0, 1, 1, 1]
        d.max_points, d.max_voxels = 10, 50
        d.coors = d.num_points_per_voxel = d.voxel_num = 256
    many = lib.msmd_hard_voxelize_many
    assert lib.msmd_hard_voxelize_many_workspace_bytes(vox, 13) > 0
    assert many(vox, 13, p, 0, None) == WORKSPACE
    assert many(vox, 13, ctypes.c_void_p(260), big, None) == WORKSPACE
    vox[12].max_points = 0
    assert many(vox, 13, p, big, None) == INVALID
    vox[12].max_points = 10
    vox[12].voxel_size[:] = [1e-4] * 3                    # 10^12 cells
    assert many(vox, 13, p, big, None) == RANGE
    vox[12].voxel_size[:] = [10.0] * 3                    # a grid of 0 cells
    assert many(vox, 13, p, big, None) == INVALID
    assert many(None, 1, p, big, None) == INVALID and many(vox, 0, p, big, None) == INVALID
    one = lib.msmd_hard_voxelize
    args = (float_arr([0.1] * 3), float_arr([0, 0, 0, 1, 1, 1]), 10, 50, None, p, p, None, p)
    assert one(p, 100, 5, *args, p, 0, None) == WORKSPACE
    assert one(p, 100, 5, *args, p, lib.msmd_voxelize_workspace_bytes(100, 50, 10) - 1,
               None) == WORKSPACE
    assert one(p, 100, 2, *args, p, big, None) == INVALID
    assert one(p, 100, 5, float_arr([1e-4] * 3), *args[1:], p, big, None) == RANGE

    subm = (K._SubmDesc * 17)()
    for d in subm:
        d.indices, d.n, d.batch_size, d.nbr = 256, 100, 1, 256
        d.spatial_shape[:] = [8, 64, 64]
        d.ksize[:] = [3, 3, 3]
        d.method = 1
    many = lib.msmd_rulebook_subm3d_many
    assert lib.msmd_rulebook_subm3d_many_workspace_bytes(subm, 17) > 0
    assert many(subm, 17, p, 0, None) == WORKSPACE
    subm[16].method = 2
    assert many(subm, 17, p, big, None) == INVALID
    subm[16].method = 1
    subm[16].spatial_shape[:] = [1, 32768, 32768]        # 2^24 bricks: no bitmap index
    assert many(subm, 17, p, big, None) == RANGE
    subm[16].spatial_shape[:] = [70000] * 3
    assert many(subm, 17, p, big, None) == RANGE
    subm[16].spatial_shape[:] = [8, 64, 64]
    subm[16].n = -1
    assert many(subm, 17, p, big, None) == INVALID
    assert many(None, 0, None, 0, None) == 0
    shape, ks = int3([8, 64, 64]), int3([3, 3, 3])
    for one, need in ((lib.msmd_rulebook_subm3d, lib.msmd_rulebook_subm_workspace_bytes(100)),
                      (lib.msmd_rulebook_subm3d_bitmap,
                       lib.msmd_rulebook_subm_bitmap_workspace_bytes(100, 1, shape))):
        assert need > 0
        assert one(p, 100, 1, shape, ks, p, p, need - 1, None) == WORKSPACE
        assert one(p, 100, 1, shape, ks, p, ctypes.c_void_p(260), big, None) == WORKSPACE
        assert one(None, 0, 1, shape, ks, None, None, 0, None) == 0      # empty: before the workspace
        assert one(p, 100, 1, shape, ks, None, p, big, None) == INVALID
    assert lib.msmd_rulebook_subm3d_bitmap(p, 100, 1, int3([1, 32768, 32768]), ks, p, p, big,
                                           None) == RANGE

    n = 17
    flags, rows = (ctypes.c_void_p * n)(*[256] * n), (ctypes.c_void_p * n)(*[256] * n)
    ints = lambda v: (ctypes.c_int * n)(*[v] * n)          # noqa: E731
    strides, lens, values, caps = ints(1), ints(100), ints(1), ints(10)
    many = lib.msmd_rows_where_eq_many
    strides[16] = 0
    assert many(flags, strides, lens, values, rows, caps, n, p, big, None) == INVALID
    strides[16] = 1
    assert many(flags, strides, lens, values, rows, caps, n, p, 0, None) == WORKSPACE


def test_product_never_touches_the_oracle():
    """oracle/ is test infrastructure: nothing under msmdfusion_amd/ may import
    or call it, and the package has no CPU fallback branches."""
    pkg = os.path.join(ROOT, "msmdfusion_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f
                assert "libmsmd_oracle" not in text and "msmd_oracle" not in text, f


def test_kernels_refuse_cpu_tensors():
    import torch
    from msmdfusion_amd import kernels as K
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.rulebook_subm(torch.zeros((4, 4), dtype=torch.int32), 1, [4, 4, 4], 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.hard_voxelize(torch.zeros((4, 5)), [0.1] * 3, [0, 0, 0, 1, 1, 1], 10, 100)


def test_synthetic_generators_are_seeded_and_shaped():
    import numpy as np
    from msmdfusion_amd import synthetic as S
    a, b = S.lidar_sweep(3), S.lidar_sweep(3)
    assert np.array_equal(a, b) and a.dtype == np.float32 and a.shape[1] == 5
    assert 25000 < a.shape[0] < 32000
    v = S.virtual_points(1)
    assert v.shape == (49980, 64) and np.isfinite(v).all()
    idx = S.random_voxel_indices(500, 2, [5, 30, 30], seed=0)
    assert np.unique(idx, axis=0).shape[0] == idx.shape[0]
    assert (idx.min(0) >= 0).all() and (idx.max(0) < [2, 5, 30, 30]).all()


def test_configs_match_the_reference_dicts():
    """msmdfusion_amd/configs.py restates the hot-path sections of the two
    reference configs; tests/golden/reference_configs.json holds the values
    dumped from the reference files (make_config_fixture.py)."""
    import json
    from msmdfusion_amd import configs as C
    fx = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_configs.json")))
    norm = lambda o: json.loads(json.dumps(o))   # tuples -> lists
    assert norm(C.MSMDFUSION_LC) == fx["MSMDFusion_nusc_voxel_LC"]
    assert norm(C.TRANSFUSION_L) == fx["transfusion_nusc_voxel_L"]


def test_hot_path_builds_from_the_configs():
    """Registry strings + constructor arguments of the unchanged config dicts
    build the modules, with the reference's parameter names (state-dict keys)."""
    from msmdfusion_amd import configs as C
    vox, vfe, enc, mm = C.build_hot_path(C.MSMDFUSION_LC)
    assert type(enc).__name__ == "SparseEncoder" and type(mm).__name__ == "SparseMultiModalEncoderPaint"
    assert type(vfe).__name__ == "HardSimpleVFE" and vox.max_num_points == 10
    keys = set(enc.state_dict().keys())
    for k in ("conv_input.0.weight", "conv_input.1.running_mean",
              "encoder_layers.encoder_layer1.0.conv1.weight",
              "encoder_layers.encoder_layer1.2.0.weight",
              "encoder_layers.encoder_layer4.1.bn2.weight", "conv_out.0.weight"):
        assert k in keys, k
    assert tuple(enc.state_dict()["conv_input.0.weight"].shape) == (16, 3, 3, 3, 5)      # KRSC
    assert tuple(enc.state_dict()["conv_out.0.weight"].shape) == (128, 3, 1, 1, 128)
    mk = set(mm.state_dict().keys())
    assert any(k.startswith("downscale_blocks") for k in mk)
    assert any(k.startswith("aggregation_blocks") for k in mk)
    _, _, enc_l, mm_l = C.build_hot_path(C.TRANSFUSION_L)
    assert mm_l is None and set(enc_l.state_dict().keys()) == keys


def test_tiling_rank_table_matches_its_derivation():
    """kRank27 (csrc/tiling_key.hpp), the bit each 3x3x3 offset gets in the tiling sort key,
    is the rank of the offset under (|dz|+|dy|+|dx|, |dz|, |dy|): centre lowest, then the
    face, edge and corner neighbours -- the order tools/order_sim.py evaluates."""
    import re
    src = open(os.path.join(ROOT, "msmdfusion_amd", "csrc", "tiling_key.hpp")).read()
    m = re.search(r"kRank27\[27\]\s*=\s*\{([^}]*)\}", src)
    assert m, "kRank27 not found"
    table = [int(x) for x in m.group(1).replace("\n", " ").split(",")]
    assert sorted(table) == list(range(27))

    def cls(k):     # offset k = (kz*3 + ky)*3 + kx  (spconv geometry.h:62-73)
        dz, dy, dx = k // 9 - 1, (k // 3) % 3 - 1, k % 3 - 1
        return (abs(dz) + abs(dy) + abs(dx), abs(dz), abs(dy))
    by_rank = sorted(range(27), key=cls)
    want = [0] * 27
    for bit, k in enumerate(by_rank):
        want[k] = bit
    assert table == want
    assert table[13] == 0 and max(table[k] for k in (0, 2, 6, 8, 18, 20, 24, 26)) == 26


def test_batchnorm_partials_belong_to_one_tensor_object():
    """A conv in front of a BatchNorm1d is marked (SparseSequential / SparseBasicBlock) so that
    its kernel leaves the BN's statistics partials on ITS output tensor object; whatever
    replaces that tensor's features must not inherit them (stale sums would silently become
    another layer's batch statistics)."""
    import torch
    from torch import nn
    from msmdfusion_amd import spconv
    from msmdfusion_amd.sparse_block import make_sparse_convmodule
    idx = torch.tensor([[0, 1, 2, 3], [0, 1, 2, 4]], dtype=torch.int32)
    x = spconv.SparseConvTensor(torch.zeros(2, 8), idx, [8, 8, 8], 1)
    x.bn_stats = torch.ones(1, 2, 8)
    assert getattr(x.replace_feature(torch.ones(2, 8)), "bn_stats", None) is None
    assert getattr(x.shadow_copy(), "bn_stats", None) is None
    x.features = torch.ones(2, 8)
    assert getattr(x, "bn_stats", None) is None
    seq = make_sparse_convmodule(8, 16, 3, "k", norm_cfg=dict(type="BN1d"), conv_type="SubMConv3d")
    seq._compile()
    conv = next(m for m in seq.children() if isinstance(m, spconv.SparseConvolution))
    assert conv.emit_bn_stats is True
    # ... only while the norm will use batch statistics: in eval mode the sums would be
    # computed and dropped (the conv is re-marked from the norm's mode at every forward)
    seq.eval()
    seq._compile()
    assert conv.emit_bn_stats is False
    bn = next(m for m in seq.children() if isinstance(m, nn.BatchNorm1d))
    assert not spconv.modules.wants_batch_stats(bn) and spconv.modules.wants_batch_stats(bn.train())
    plain = spconv.SparseSequential(spconv.SubMConv3d(8, 8, 3, indice_key="a"), nn.ReLU())
    plain._compile()
    assert next(iter(plain.children())).emit_bn_stats is False


def test_deferred_batch_counters_apply_once_at_exit():
    """BatchNorm batch counters: immediate outside the context (torch's behaviour), collected
    and applied together when distributed.TrainStep's `deferred_batch_counters()` closes."""
    import torch
    from msmdfusion_amd.spconv import functional as Fsp
    a, b = torch.zeros((), dtype=torch.long), torch.zeros((), dtype=torch.long)
    Fsp.count_batch(a)
    assert int(a) == 1
    with Fsp.deferred_batch_counters():
        Fsp.count_batch(a)
        Fsp.count_batch(b)
        Fsp.count_batch(a)
        assert int(a) == 1 and int(b) == 0          # nothing applied yet
        with Fsp.deferred_batch_counters():         # nested: the outer one flushes
            Fsp.count_batch(b)
        assert int(b) == 0
    assert int(a) == 3 and int(b) == 2
    Fsp.count_batch(b)
    assert int(b) == 3
