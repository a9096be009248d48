#!/usr/bin/env python
"""Generates tests/golden/pointnet_ops_vectors.npz from the NUMBERS in the reference's own op
tests (tests/test_models/test_common_modules/test_pointnet_ops.py): test_fps_with_dist (the
in-file case), test_knn, test_grouping_points, test_gather_points, test_three_interpolate and
test_three_nn.

mmdet3d cannot be imported here, and nothing of it is: the test file is parsed (ast) and the
literal argument of every `torch.tensor([...])` assigned to a name is evaluated as data.  What
a test computes instead of writing down (the knn expectation: topk of the float32 distance
matrix; the FPS distance matrix) is recomputed here by the test's own formula on CPU.  The
.npz holds arrays only, keyed `<test>__<name>`.  Build container only (/root/reference).
"""
import ast
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/tests/test_models/test_common_modules/test_pointnet_ops.py"
OUT = os.path.join(ROOT, "tests", "golden", "pointnet_ops_vectors.npz")
TESTS = ("test_fps_with_dist", "test_knn", "test_grouping_points", "test_gather_points",
         "test_three_interpolate", "test_three_nn")
INT_NAMES = ("idx", "expected_idx")


def _tensor_literal(node):
    """The list literal inside torch.tensor([...])[.int()][.cuda()], or None."""
    while isinstance(node, ast.Call):
        f = node.func
        if isinstance(f, ast.Attribute) and f.attr == "tensor" and node.args:
            try:
                return ast.literal_eval(node.args[0])
            except ValueError:
                return None
        node = f.value if isinstance(f, ast.Attribute) else None
    return None


def main():
    tree = ast.parse(open(REF).read())
    out = {}
    for fn in tree.body:
        if not isinstance(fn, ast.FunctionDef) or fn.name not in TESTS:
            continue
        for st in ast.walk(fn):
            if isinstance(st, ast.Assign) and len(st.targets) == 1 and \
                    isinstance(st.targets[0], ast.Name):
                lit = _tensor_literal(st.value)
                key = "%s__%s" % (fn.name[5:], st.targets[0].id)
                if lit is not None and key not in out:
                    dtype = np.int32 if st.targets[0].id in INT_NAMES else np.float32
                    out[key] = np.asarray(lit, dtype=dtype)
    # test_knn:107-110,119-122 -- the expectation is computed, not written down
    xyz, new_xyz = torch.from_numpy(out["knn__xyz"]), torch.from_numpy(out["knn__new_xyz"])

    def topk5(centres, pts):
        a = centres.unsqueeze(2).repeat(1, 1, pts.shape[1], 1)
        b = pts.unsqueeze(1).repeat(1, centres.shape[1], 1, 1)
        dist = ((a - b) * (a - b)).sum(-1)
        return dist.topk(k=5, dim=2, largest=False)[1].transpose(2, 1).numpy().astype(np.int64)
    out["knn__expected_idx"] = topk5(new_xyz, xyz)
    out["knn__expected_idx_self"] = topk5(xyz, xyz)
    # test_fps_with_dist:390-391
    p = torch.from_numpy(out["fps_with_dist__xyz"])
    out["fps_with_dist__xyz_square_dist"] = \
        ((p.unsqueeze(dim=1) - p.unsqueeze(dim=2)) ** 2).sum(-1).numpy()
    np.savez_compressed(OUT, **out)
    for k in sorted(out):
        print(k, out[k].shape, out[k].dtype)


if __name__ == "__main__":
    main()
