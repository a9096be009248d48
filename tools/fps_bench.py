#!/usr/bin/env python
"""Times furthest point sampling (2048 samples) on LC-shaped inputs: the voxel
coordinates of synthetic virtual points at stage 0 (0.075 m) and stage 1
(0.15 m), in first-touch order (what hard voxelization emits) and shuffled (the
pruned kernel's worst case), and checks every result against the oracle.

    python tools/fps_bench.py

Search-chain mode: HIP-event time of the neighbour search BEHIND FPS (nearest key of the
representatives, ball query, assignment, batch offsets, pad rows) at the four stages of the
LC batch bench.py runs, through the per-sample entries and through the one-call entry
(kernels.gma_nn_chain), alone on the chip; both results are checked to be equal.

    python tools/fps_bench.py --chain [table.txt]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msmdfusion_amd import kernels as K  # noqa: E402
from msmdfusion_amd import synthetic as S  # noqa: E402
from oracle import oracle as O  # noqa: E402


def voxel_coords(seed, scale, n_pts):
    p = S.virtual_points(seed, n=n_pts)[:, :3]
    vs = np.array(S.VOXEL_SIZE) * scale
    c = np.floor((p - np.array(S.POINT_CLOUD_RANGE[:3])) / vs).astype(np.int64)[:, ::-1]  # z,y,x
    _, first = np.unique(c, axis=0, return_index=True)
    return np.ascontiguousarray(c[np.sort(first)], dtype=np.float32)


def main():
    dev = torch.device("cuda:0")
    for name, scale, n_pts in [("stage0", 1, 50000), ("stage0-big", 1, 56000), ("stage1", 2, 50000)]:
        a, b = voxel_coords(0, scale, n_pts), voxel_coords(1, scale, n_pts)
        n = min(a.shape[0], b.shape[0])
        for order in ("first-touch", "shuffled"):
            xyz = np.stack([a[:n], b[:n]])
            if order == "shuffled":
                rng = np.random.RandomState(0)
                xyz = np.stack([x[rng.permutation(n)] for x in xyz])
            t = torch.from_numpy(xyz).to(dev)
            got = K.furthest_point_sample(t, 2048)
            torch.cuda.synchronize()
            ok = np.array_equal(got.cpu().numpy(), O.furthest_point_sample(xyz, 2048))
            ts = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                K.furthest_point_sample(t, 2048)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            print("%-10s %-11s n=%5d x2  %.3f ms  (%.2f us/round)  oracle-exact=%s"
                  % (name, order, n, min(ts), min(ts) / 2047 * 1e3, ok), flush=True)


def chain_old(q_bzyx, k_bzyx, c2, c3, rep_all, fps_num, radius, mcs, thresh, n_pad):
    """What SparseMultiModalEncoderPaint._nearest_3d_per_sample enqueues behind its FPS call."""
    out = torch.full((q_bzyx.shape[0],), -1, dtype=torch.long, device=q_bzyx.device)
    q_zyx, k_zyx = q_bzyx[:, 1:].contiguous(), k_bzyx[:, 1:].contiguous()
    o2, o3 = np.cumsum([0] + list(c2)), np.cumsum([0] + list(c3))
    for b in range(len(c2)):
        if not (c2[b] and c3[b]):
            continue
        q, k = q_zyx[o2[b]:o2[b + 1]], k_zyx[o3[b]:o3[b + 1]]
        if c2[b] <= fps_num:
            nn_idx = K.nn_search(q, k, thresh).long()
        else:
            q_f = q.float().unsqueeze(0)
            rep = q[rep_all[b].long()]
            rep_nn = K.nn_search(rep, k, thresh)
            group = K.ball_query(0, radius, mcs, q_f, rep.float().unsqueeze(0))[0]
            nn_idx = K.nn_assign(group, rep_nn, c2[b]).long()
        out[o2[b]:o2[b + 1]] = torch.where(nn_idx >= 0, nn_idx + int(o3[b]), nn_idx)
    return torch.cat([out, out.new_full((n_pad,), -1)]) if n_pad else out


def event_us(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), min(ts)


def chain_main(out_path=None):
    import bench
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = bench.FusionBackbone().to(dev)
    ids = range(bench.WORKLOADS["lc"]["spg"])
    clouds = [torch.from_numpy(S.lidar_sweep(i)).to(dev) for i in ids]
    virtual = [torch.from_numpy(S.virtual_points(i)).to(dev) for i in ids]
    with torch.no_grad():
        prep = model.det.prepare(clouds, virtual, nn_side_stream=False)
    path, batch = model.path, len(clouds)
    lines = ["search chain behind FPS, LC batch (%d samples), alone on the chip; us per stage, "
             "median (min) of 20" % batch,
             "VALU estimate: pairs x 10 ops / (256 CU x 64 lanes x 2.4 GHz)",
             "%-6s %-16s %-14s %10s %16s %16s %10s" % ("stage", "queries", "keys", "pairs",
                                                       "per-sample us", "one call us", "VALU us")]
    for i, plan in enumerate(prep["plans"]):
        c2, c3 = plan["counts_host"]
        fps_num, radius = path.fps_num_list[i], path.radius_list[i]
        mcs, thresh = path.max_cluster_samples_list[i], path.dist_thresh_list[i]
        q, k, n_pad = plan["o2_bzyx"], plan["idx3"], plan["n_pad"]
        o2, o3 = np.cumsum([0] + list(c2)).tolist(), np.cumsum([0] + list(c3)).tolist()
        modes = [K.NN_CHAIN_SKIP if not (a and b) else K.NN_CHAIN_DIRECT if a <= fps_num
                 else K.NN_CHAIN_CLUSTERED for a, b in zip(c2, c3)]
        desc = K.gma_nn_chain_desc(o2, o3, modes, o3[:-1], dev)
        rep_all = torch.zeros((batch, fps_num), dtype=torch.int32, device=dev)
        for b in range(batch):
            if modes[b] == K.NN_CHAIN_CLUSTERED:
                rep_all[b] = K.furthest_point_sample(
                    q[o2[b]:o2[b + 1], 1:].float()[None], fps_num)[0]
        searchers = [fps_num if m == K.NN_CHAIN_CLUSTERED else a if m == K.NN_CHAIN_DIRECT else 0
                     for a, m in zip(c2, modes)]
        nk_max = max(b if m != K.NN_CHAIN_SKIP else 0 for b, m in zip(c3, modes))

        def old():
            return chain_old(q, k, c2, c3, rep_all, fps_num, radius, mcs, thresh, n_pad)

        def new():
            return K.gma_nn_chain(q, k, desc, batch, rep_all, fps_num, max(searchers), nk_max,
                                  thresh, radius, mcs, n_pad)
        assert torch.equal(old(), new()), "stage %d: the two chains disagree" % i
        t_old, t_new = event_us(old), event_us(new)
        pairs = sum(s * b for s, b in zip(searchers, c3))
        lines.append("%-6d %-16s %-14s %10d %9.1f (%5.1f) %9.1f (%5.1f) %10.1f" % (
            i, "/".join(map(str, c2)), "/".join(map(str, c3)), pairs, t_old[0], t_old[1],
            t_new[0], t_new[1], pairs * 10 / (256 * 64 * 2.4e3)))
    text = "\n".join(lines)
    print(text, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--chain":
        chain_main(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        main()
