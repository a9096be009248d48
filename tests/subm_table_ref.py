"""The SubM neighbour table from a dense numpy grid: the reference of the SubM rulebook tests,
independent of the hash index, the bitmap index and the C oracle (test_oracle_cpu pins it to
the C oracle on the duplicate-free cases).  Shared by the CPU and the GPU tests."""
import numpy as np

from msmdfusion_amd import synthetic as S

# (rows, batch, grid, kernel, index method): hash and bitmap mixed, different grids, kernel
# sizes and batch sizes.  Case 0 repeats 37 coordinates (subm_case_indices).
CASES = [(5000, 2, [11, 64, 64], 3, "hash"), (5000, 2, [11, 64, 64], 3, "bitmap"),
         (1, 1, [5, 8, 8], 3, "bitmap"), (130, 3, [7, 30, 30], [3, 3, 1], "hash"),
         (2600, 2, [11, 64, 64], [1, 3, 3], "bitmap"), (9000, 4, [21, 90, 90], 3, None),
         (700, 1, [41, 200, 200], 3, None), (3000, 2, [3, 100, 100], [3, 5, 3], "bitmap")]
N_DUPLICATES = 37


def case_indices(i):
    n_vox, batch, shape = CASES[i][:3]
    idx = S.random_voxel_indices(n_vox, batch, shape, seed=i)
    if i == 0:                       # duplicate coordinates: the last row wins
        idx = np.concatenate([idx, idx[:N_DUPLICATES]])
    return idx


def subm_table(idx, batch, shape, ksize):
    """exp[k, o] = the row at (b_o, z_o - kz // 2 + kz', ...) or -1, k in (kz, ky, kx) order.
    Of rows that repeat a coordinate the LAST one is found (numpy's rule for repeated indices
    in an assignment, the kernels' documented duplicate rule), by every row of the coordinate."""
    ks = [int(ksize)] * 3 if isinstance(ksize, int) else [int(v) for v in ksize]
    idx = np.asarray(idx, np.int64).reshape(-1, 4)
    n = idx.shape[0]
    grid = np.full([batch] + list(shape), -1, np.int32)
    grid[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = np.arange(n, dtype=np.int32)
    exp = np.full((ks[0] * ks[1] * ks[2], n), -1, np.int32)
    k = 0
    for kz in range(ks[0]):
        for ky in range(ks[1]):
            for kx in range(ks[2]):
                z = idx[:, 1] - ks[0] // 2 + kz
                y = idx[:, 2] - ks[1] // 2 + ky
                x = idx[:, 3] - ks[2] // 2 + kx
                ok = (z >= 0) & (z < shape[0]) & (y >= 0) & (y < shape[1]) & (x >= 0) & (x < shape[2])
                exp[k, ok] = grid[idx[ok, 0], z[ok], y[ok], x[ok]]
                k += 1
    return exp
