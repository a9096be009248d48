"""`knn_ext` -- the pybind module of mmdet3d/ops/knn (src/knn.cpp:26-62) on the C ABI: one
batch element per call, coordinate-major inputs, 1-BASED int64 indices (knn.py subtracts 1).
Only 3 coordinates are built (the reference takes any `dim`; its callers pass xyz)."""
import torch

from .. import kernels as K
from ._pointnet_common import check_input


def knn_wrapper(ref, ref_nb, query, query_nb, ind, k):
    """ind[k, query_nb] (int64) <- 1 + index of the j-th nearest of ref[3, ref_nb] to every
    column of query[3, query_nb], ordered by (squared distance, index)."""
    dev = check_input(ref=ref, query=query, ind=ind)
    if ref.dtype != torch.float32 or query.dtype != torch.float32:
        raise RuntimeError("ref and query must be float32")
    if tuple(ref.shape) != (3, ref_nb) or tuple(query.shape) != (3, query_nb):
        raise RuntimeError("ref / query must be [3, ref_nb] / [3, query_nb]")
    if ind.dtype != torch.int64 or tuple(ind.shape) != (k, query_nb):
        raise RuntimeError("ind must be int64 [k, query_nb]")
    with torch.cuda.device(dev):
        idx = K.knn(k, ref.t().contiguous()[None], query.t().contiguous()[None])
        torch.add(idx[0], 1, out=ind)
