"""msmd_primitive_index / msmd_primitive_targets_f32 against the restated reference loop
(tests/primitive_ref.py).  Discrete outputs (point_mask, the class column, which rows are
written) must be exact; float outputs stay within 4 x the float32 restatement's own error
against the float64 restatement, per output tensor of a case.  Every generated case re-checks
the margin assertions on the restatement first: a case that violates them fails."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import primitive_cases as PC  # noqa: E402
import primitive_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = ("z", "xy", "line")


def _corners(sample):
    from msmdfusion_amd.head_loss import DepthBoxes
    return DepthBoxes(sample["boxes"], with_yaw=sample["with_yaw"]).corners.contiguous()


def _batch(samples, dev):
    """-> the flat device tensors the kernels take, and the per-sample CPU lists."""
    corners = [s.get("corners", None) if s.get("corners", None) is not None else _corners(s)
               for s in samples]
    p_off = np.cumsum([0] + [s["points"].shape[0] for s in samples])
    b_off = np.cumsum([0] + [c.shape[0] for c in corners])
    width = samples[0]["points"].shape[1]
    flat = dict(
        points=torch.cat([s["points"] for s in samples]).reshape(-1, width).contiguous().to(dev),
        sem=torch.cat([s["sem"] for s in samples]).to(dev),
        inst=torch.cat([s["inst"] for s in samples]).to(dev),
        corners=torch.cat(corners).reshape(-1, 8, 3).contiguous().to(dev),
        p_off=torch.tensor(p_off, dtype=torch.int32, device=dev),
        b_off=torch.tensor(b_off, dtype=torch.int32, device=dev))
    return flat, corners


def _kernel(flat, mode, cfg, with_yaw, num_classes, label_bound=None, index=None):
    from msmdfusion_amd import kernels as K
    if index is None:
        index = K.primitive_index(flat["sem"], flat["inst"], flat["p_off"], num_classes,
                                  label_bound=label_bound)
    return K.primitive_targets(flat["points"], flat["sem"], flat["p_off"], flat["corners"],
                               flat["b_off"], index, mode, with_yaw, cfg, label_bound=label_bound)


def _check(samples, cfg, dev, modes=MODES, label_bound=None, margins=True):
    flat, corners = _batch(samples, dev)
    with_yaw, classes = samples[0]["with_yaw"], samples[0]["num_classes"]
    lists = ([s["points"] for s in samples], [s["sem"] for s in samples],
             [s["inst"] for s in samples], corners)
    results = {}
    for mode in modes:
        t32, t64 = R.Trace(), R.Trace()
        r32 = R.batch_targets_ref(*lists, with_yaw, mode, classes, cfg, torch.float32,
                                  label_bound, t32)
        r64 = R.batch_targets_ref(*lists, with_yaw, mode, classes, cfg, torch.float64,
                                  label_bound, t64)
        if margins:
            R.assert_margins(t32, t64, cfg)
        mask, offset, sem = [t.cpu() for t in _kernel(flat, mode, cfg, with_yaw, classes,
                                                      label_bound)]
        assert sem.shape[1] == 4 + R.NUM_DIMS[mode]
        assert torch.equal(mask, r32[0]), mode
        assert torch.equal(sem[:, -1], r32[2][:, -1]), mode
        written = (r32[2] != 0).any(1) | (r32[1] != 0).any(1)
        assert torch.equal((sem != 0).any(1) | (offset != 0).any(1), written), mode
        for name, got, a, b in (("offset", offset, r32[1], r64[1]),
                                ("sem", sem[:, :-1], r32[2][:, :-1], r64[2][:, :-1])):
            bound = 4 * float((a.double() - b).abs().max()) if a.numel() else 0.0
            err = float((got.double() - b).abs().max()) if a.numel() else 0.0
            print("%s %s: err %.3e bound %.3e, %d rows on" % (mode, name, err, bound,
                                                              int(mask.sum())))
            assert err <= bound, (mode, name, err, bound)
        results[mode] = (mask, offset, sem, r32)
    return results


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2051])
def test_sizes_per_sample(dev, n):
    sizes = [] if n < 63 else ([n] if n < 257 else [n // 4, n // 8, 9, 3])
    sample = PC.make_sample(10 + n, n, sizes)
    out = _check([sample], PC.SMALL_CFG, dev)
    if n >= 63:
        assert all(float(out[m][0].sum()) > 0 for m in MODES)


@pytest.mark.parametrize("with_yaw", [True, False])
def test_ragged_batch_with_an_empty_middle_sample(dev, with_yaw):
    a = PC.make_sample(1, 300, [120, 80, 40], with_yaw=with_yaw)
    empty = PC.make_sample(2, 0, [], with_yaw=with_yaw)
    b = PC.make_sample(3, 129, [100], with_yaw=with_yaw)
    _check([a], PC.SMALL_CFG, dev)
    _check([a, b], PC.SMALL_CFG, dev)
    out = _check([a, empty, b], PC.SMALL_CFG, dev)
    assert float(out["line"][0].sum()) > 0


@pytest.mark.parametrize("count", [0, 1, 4, 33])
def test_instance_counts(dev, count):
    """0 (background only), 1, 4 and 33 instances (more than one bitmap word of labels);
    eight yaws including 0 and +-pi/2."""
    sample = PC.make_sample(20 + count, 40 * count + 50, [40] * count, label_stride=2)
    out = _check([sample], PC.SMALL_CFG, dev)
    if count == 0:
        assert all(float(out[m][0].sum()) == 0 for m in MODES)


def test_list_lengths_straddle_the_chunk(dev):
    from msmdfusion_amd._lib import lib
    chunk = lib.msmd_primitive_point_chunk()
    sizes = [chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    _check([PC.make_sample(5, sum(sizes) + 77, sizes)], PC.SMALL_CFG, dev)
    _check([PC.make_sample(6, sum(sizes) + 77, sizes, with_yaw=False)], PC.SMALL_CFG, dev)


def test_one_instance_owns_every_point(dev):
    _check([PC.make_sample(7, 700, [700])], PC.SMALL_CFG, dev)


def test_rank_is_not_the_label_and_a_rank_beyond_the_boxes(dev):
    """Labels 2, 5, 8, 11: the box of label 5 is corners[1].  With the last box missing the
    fourth instance gets no targets and the others keep theirs."""
    full = PC.make_sample(8, 400, [90, 90, 90, 90])
    ref = _check([full], PC.SMALL_CFG, dev)
    short = dict(full, boxes=full["boxes"][:3])
    out = _check([short], PC.SMALL_CFG, dev)
    last = full["inst"] == 11
    for mode in MODES:
        assert float(ref[mode][0][last].sum()) > 0 and float(out[mode][0][last].sum()) == 0
        assert torch.equal(ref[mode][2][~last], out[mode][2][~last])


def test_labels_outside_the_bound_take_no_part(dev):
    sample = PC.make_sample(9, 300, [80, 80, 80])
    sample["inst"][sample["inst"] == 5] = 100              # >= label_bound 64
    sample["inst"][sample["inst"] == 8] = -1
    sample["boxes"] = sample["boxes"][[0]]
    out = _check([sample], PC.SMALL_CFG, dev, label_bound=64)
    keep = sample["inst"] == 2
    for mode in MODES:
        assert float(out[mode][0][keep].sum()) > 0 and float(out[mode][0][~keep].sum()) == 0


def test_counts_at_and_one_above_the_thresholds(dev):
    """Bottom face with exactly num_point points (off) and top with num_point + 1 (on); edges
    with exactly num_point_line (off) and num_point_line + 1 (on)."""
    cfg = PC.SMALL_CFG
    n, l = cfg["num_point"], cfg["num_point_line"]
    fn = PC.exact_count_levels([(n, l, n + 1, l + 1), (n + 1, l + 1, n, l)])
    for with_yaw in (True, False):
        sample = PC.make_sample(11, 200, [60, 60], with_yaw=with_yaw, level_fn=fn,
                                yaws=(0.4, -0.9))
        out = _check([sample], cfg, dev)
        mask, _, sem, _ = out["z"]
        assert int(mask[sample["inst"] == 2].sum()) == n + 1
        assert int(mask[sample["inst"] == 5].sum()) == n + 1


def test_the_config_thresholds_at_100_and_101(dev):
    cfg = PC.CONFIG_CFG
    fn = PC.exact_count_levels([(100, 10, 101, 11)])
    sample = PC.make_sample(12, 400, [330], level_fn=fn, yaws=(1.2,))
    out = _check([sample], cfg, dev)
    assert int(out["z"][0].sum()) == 101


def test_variance_test_fails_on_a_bimodal_face(dev):
    sample = PC.make_sample(13, 300, [120, 120], bimodal=(0,))
    out = _check([sample], PC.VAR_CFG, dev, modes=("z",))
    plain = _check([sample], PC.SMALL_CFG, dev, modes=("z",))
    first = sample["inst"] == 2
    assert float(plain["z"][0][first].sum()) > float(out["z"][0][first].sum())


def test_a_point_near_a_corner_is_written_by_the_last_primitive(dev):
    """Level (0, 0, 0): on the bottom and left faces, and on three lines; the value the
    reference leaves is that of the last primitive in its write order."""
    def fn(r, rng, m, ks):
        lev = np.stack([PC.random_levels(rng, m, ks[a]) for a in range(3)], axis=1)
        lev[:6] = 0
        return lev
    for with_yaw in (True, False):
        _check([PC.make_sample(14, 150, [120], level_fn=fn, with_yaw=with_yaw)],
               PC.SMALL_CFG, dev)


def test_nan_points_and_a_nan_box_switch_off_only_their_instance(dev):
    clean = PC.make_sample(15, 400, [100, 100, 100])
    ref = _check([clean], PC.SMALL_CFG, dev)
    bad = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in clean.items()}
    row = int(torch.nonzero(bad["inst"] == 2)[0])
    bad["points"][row, :3] = float("nan")
    bad["boxes"][2] = float("nan")
    out = _check([bad], PC.SMALL_CFG, dev)
    mid = (clean["inst"] == 5) & (clean["sem"] != clean["num_classes"])
    for mode in MODES:
        mask, offset, sem, _ = out[mode]
        assert float(mask[~mid].sum()) == 0 and bool(torch.isfinite(sem).all())
        assert torch.equal(sem[mid], ref[mode][2][mid]) and float(mask[mid].sum()) > 0


def _big_batch(dev, b=8, n=40000, instances=32):
    samples = [PC.make_sample(100 + s, n, [900] * instances) for s in range(b)]
    return _batch(samples, dev)[0]


def test_one_index_serves_the_three_modes_and_runs_are_bitwise_equal(dev):
    from msmdfusion_amd import kernels as K
    flat = _big_batch(dev)
    shared = K.primitive_index(flat["sem"], flat["inst"], flat["p_off"], 18)
    for mode in MODES:
        one = _kernel(flat, mode, PC.CONFIG_CFG, True, 18, index=shared)
        own = _kernel(flat, mode, PC.CONFIG_CFG, True, 18)
        again = _kernel(flat, mode, PC.CONFIG_CFG, True, 18, index=shared)
        assert float(one[0].sum()) > 0
        for a, b, c in zip(one, own, again):
            assert torch.equal(a, b) and torch.equal(a, c)


def test_no_host_read_and_no_hidden_allocation(dev):
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd._lib import lib
    sample = PC.make_sample(16, 2051, [500, 300, 200])
    flat, _ = _batch([sample], dev)
    _kernel(flat, "z", PC.SMALL_CFG, True, 18)                 # warm: module load
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        index = K.primitive_index(flat["sem"], flat["inst"], flat["p_off"], 18)
        outs = [_kernel(flat, mode, PC.SMALL_CFG, True, 18, index=index) for mode in MODES]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    stated = lib.msmd_primitive_index_workspace_bytes(1, 2051, K.PRIMITIVE_MAX_LABELS)
    assert index.numel() == stated
    expect = sum((t.numel() * t.element_size() + 511) // 512 * 512
                 for t in [index] + [t for o in outs for t in o])
    assert peak <= expect, (peak, expect)


def test_cpu_tensors_and_bad_arguments_are_refused(dev):
    from msmdfusion_amd import kernels as K
    sample = PC.make_sample(17, 100, [60])
    flat, _ = _batch([sample], dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.primitive_index(flat["sem"].cpu(), flat["inst"].cpu(), flat["p_off"].cpu(), 18)
    index = K.primitive_index(flat["sem"], flat["inst"], flat["p_off"], 18)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.primitive_targets(flat["points"].cpu(), flat["sem"], flat["p_off"], flat["corners"],
                            flat["b_off"], index, "z", True, PC.SMALL_CFG)
    with pytest.raises(ValueError, match="mode"):
        K.primitive_targets(flat["points"], flat["sem"], flat["p_off"], flat["corners"],
                            flat["b_off"], index, "yz", True, PC.SMALL_CFG)
    with pytest.raises(ValueError, match="label_bound"):
        K.primitive_index(flat["sem"], flat["inst"], flat["p_off"], 18, label_bound=4096)
