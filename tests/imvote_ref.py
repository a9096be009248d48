"""Restatements for the ImVoteNet tests (not collected): VoteFusion in matrix form, in any
dtype, with a stable-sort top-k (equal scores to the lower box index); sample_valid_seeds as
the reference's loop (imvotenet.py:12-49); and the seed generator that makes the uv rounding
well defined (seeds back-projected from chosen pixels and depths)."""
import os

import numpy as np
import torch

from msmdfusion_amd import fusion_layers as FL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "vote_fusion_vectors.npz")
EPS = 1e-6


def vote_fusion_ref(imgs, bboxes, seeds, img_metas, calibs, num_classes, k, dtype=torch.float64):
    """VoteFusion.forward (vote_fusion.py:40-212) as [S, Nb] matrices in `dtype`.  Differences
    from the reference, all invisible where it is well defined: the top-k is a stable sort, a
    class outside [0, num_classes) has no semantic cue, a pixel outside img_shape has a zero
    texture cue, the empty branch writes 5 + num_classes rows.  -> (feat [B, C, K S], mask
    [B, K S], details per sample: dict(uv, in_box [S, K], chosen [S, K]))."""
    feats, masks, details = [], [], []
    for i, (img, bx, seed, meta) in enumerate(zip(imgs, bboxes, seeds, img_metas)):
        seed, bx = seed.to(dtype), bx.to(dtype)
        rt = torch.as_tensor(calibs["Rt"][i]).to(seed)
        kmat = torch.as_tensor(calibs["K"][i]).to(seed)
        s, nb = seed.shape[0], bx.shape[0]
        xyz = FL.apply_3d_transformation(seed, "DEPTH", meta, reverse=True)
        cam = FL.convert_point_depth_cam(xyz, rt, to_cam=True)
        uv = (FL.points_cam2img(cam, kmat) - 1).round()
        resc = FL.coord_2d_transform(meta, uv, True).round()
        cues = seed.new_zeros((s, k, 5 + num_classes))
        score = seed.new_zeros((s, max(nb, k)))
        inb = torch.zeros((s, max(nb, k)), dtype=torch.bool, device=seed.device)
        if nb:
            b0 = FL.bbox_2d_transform(meta, bx, False)
            inb[:, :nb] = (uv[:, None, 0] > b0[None, :, 0]) & (uv[:, None, 0] < b0[None, :, 2]) & \
                (uv[:, None, 1] > b0[None, :, 1]) & (uv[:, None, 1] < b0[None, :, 3])
            score[:, :nb] = inb[:, :nb].to(dtype) + bx[None, :, 4]
            mid = torch.stack([(b0[:, 0] + b0[:, 2]) / 2, (b0[:, 1] + b0[:, 3]) / 2], -1)
            delta = (mid[None] - uv[:, None]) * cam[:, None, 2:3] / kmat[0, 0]       # [S, Nb, 2]
            vote = torch.cat([delta, torch.zeros_like(delta[..., :1])], -1).view(-1, 3)
            vote = FL.convert_point_depth_cam(vote, rt, to_cam=False)
            vote = FL.apply_3d_transformation(vote, "DEPTH", meta, reverse=False).view(s, nb, 3)
            ray = seed[:, None] + vote
            ray = ray / torch.sqrt((ray ** 2).sum(-1) + EPS).unsqueeze(-1)
            xz = ray[..., [0, 2]] / (ray[..., [1]] + EPS) * seed[:, None, [1]] - seed[:, None, [0, 2]]
            sem = seed.new_zeros((s, nb, num_classes))
            cls = bx[:, 5].long()
            ok = (cls >= 0) & (cls < num_classes)
            sem[:, ok, cls[ok]] = bx[ok, 4]
            allc = torch.cat([xz, ray, sem], -1) * inb[:, :nb, None].to(dtype)
            order = torch.sort(score, dim=1, descending=True, stable=True)[1][:, :k]
            chosen_score = score.gather(1, order)
            real = order < nb
            g = allc.gather(1, order.clamp(max=nb - 1)[..., None].expand(-1, -1, allc.shape[-1]))
            cues = g * real[..., None].to(dtype)
            mask = chosen_score.floor() != 0
            chosen_inb = inb.gather(1, order)
        else:
            order = torch.arange(k, device=seed.device).expand(s, k)
            mask = torch.zeros((s, k), dtype=torch.bool, device=seed.device)
            mask[:, 0] = True
            chosen_inb = torch.zeros((s, k), dtype=torch.bool, device=seed.device)
        h, w = meta["img_shape"][:2]
        x, y = resc[:, 0], resc[:, 1]
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        xi, yi = x.clamp(0, w - 1).long(), y.clamp(0, h - 1).long()
        xi, yi = torch.where(inside, xi, torch.zeros_like(xi)), torch.where(inside, yi,
                                                                            torch.zeros_like(yi))
        pix = img.float()[:, yi, xi]
        tex = (pix / pix.new_tensor(255.)).to(dtype) * inside.to(dtype)     # [3, S], true division
        feat = torch.cat([cues.permute(2, 1, 0).reshape(5 + num_classes, k * s),
                          tex[:, None, :].expand(3, k, s).reshape(3, k * s)], 0)
        feats.append(feat)
        masks.append(mask.t().reshape(-1))
        details.append(dict(uv=uv, in_box=chosen_inb, chosen=order))
    return torch.stack(feats), torch.stack(masks), details


def sample_valid_seeds_loop(mask, num_sampled_seed, generator=None):
    """imvotenet.py:12-49, sample by sample (nonzero / unique / randperm)."""
    device = mask.device
    out = mask.new_zeros((mask.shape[0], num_sampled_seed), dtype=torch.int64)
    for b in range(mask.shape[0]):
        valid = torch.nonzero(mask[b]).squeeze(-1)
        if len(valid) < num_sampled_seed:
            t1 = torch.arange(num_sampled_seed, device=device)
            uniques, counts = torch.cat((t1, valid % num_sampled_seed)).unique(return_counts=True)
            difference = uniques[counts == 1]
            rand = torch.randperm(len(difference), device=device,
                                  generator=generator)[:num_sampled_seed - len(valid)]
            cur = torch.cat((valid, difference[rand]))
        else:
            rand = torch.randperm(len(valid), device=device, generator=generator)[:num_sampled_seed]
            cur = valid[rand]
        out[b] = cur
    return out


# ---- inputs on which the rounding is well defined ----------------------------------------------
def make_case(seed, s, nbs, num_classes, img_hw=(36, 50), pad_hw=(48, 64), flows=None,
              scaled=None, flips=None):
    """A batch (numpy / python): seeds [B, S, 3] back-projected from integer pixels (u - 1 within
    0.25 of an integer; scale factors 1 or (1.2, 1.25) with rows whose rescaled pixel would sit on
    a half redrawn), boxes with distinct confidences whose edges are off the pixel grid, images,
    calibration and metas.  Forward coordinate >= 0.5."""
    rng = np.random.RandomState(seed)
    b = len(nbs)
    flows = flows or [[], ["HF", "R", "S", "T"], ["R", "S", "T", "HF"]]
    metas, rts, ks, boxes, seeds, pics = [], [], [], [], [], []
    oh, ow = img_hw
    for i in range(b):
        sc = (1.2, 1.25) if (scaled[i] if scaled else i % 2 == 0) else (1.0, 1.0)
        m = dict(img_shape=[int(oh * sc[1]), int(ow * sc[0]), 3], ori_shape=[oh, ow, 3],
                 scale_factor=[sc[0], sc[1], sc[0], sc[1]])
        if flips[i] if flips else i % 3 == 0:
            m["flip"] = True
        flow = flows[i % len(flows)]
        if flow:
            a = rng.uniform(0.15, 0.35) * rng.choice([-1, 1])
            m.update(transformation_3d_flow=list(flow),
                     pcd_rotation=[[np.cos(a), np.sin(a), 0], [-np.sin(a), np.cos(a), 0],
                                   [0, 0, 1.0]],
                     pcd_scale_factor=float(rng.uniform(0.9, 1.1)),
                     pcd_trans=rng.uniform(-0.2, 0.2, 3).tolist(), pcd_horizontal_flip=True)
        a1, a2 = rng.uniform(-0.08, 0.08, 2)
        rx = np.array([[1, 0, 0], [0, np.cos(a1), -np.sin(a1)], [0, np.sin(a1), np.cos(a1)]])
        rz = np.array([[np.cos(a2), -np.sin(a2), 0], [np.sin(a2), np.cos(a2), 0], [0, 0, 1]])
        rt, f = rx @ rz, rng.uniform(38.0, 44.0)
        k = np.array([[f, 0, ow / 2 + rng.uniform(-1, 1)], [0, f, oh / 2 + rng.uniform(-1, 1)],
                      [0, 0, 1.0]])
        n = nbs[i]
        bx = np.zeros((n, 6))
        conf = rng.permutation(np.linspace(0.08, 0.93, max(n, 1)))[:n]
        for j in range(n):
            w, h = rng.randint(12, ow - 6), rng.randint(10, oh - 4)
            l, t = rng.randint(0, ow - w) + 0.37, rng.randint(0, oh - h) + 0.41
            bx[j] = [l, t, l + w + 0.2, t + h + 0.15, conf[j], rng.randint(0, num_classes)]
        bx[:, [0, 2]] *= sc[0]
        bx[:, [1, 3]] *= sc[1]
        if m.get("flip", False):
            bx[:, [0, 2]] = m["img_shape"][1] - bx[:, [2, 0]]
        # pixels: y rows whose rescaled coordinate is a half-integer (v * 1.25) are left out
        vs = np.array([v for v in range(2, oh - 2) if abs((v * sc[1]) % 1 - 0.5) > 1e-3])
        us = np.array([u for u in range(2, ow - 2) if abs((u * sc[0]) % 1 - 0.5) > 1e-3])
        out = np.zeros((s, 3), np.float32)
        todo = np.arange(s)
        d2c = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]]) @ rt.T
        fwd = FL.flow_matrix(m, reverse=False, coords_type="DEPTH")
        while todo.size:
            c = todo.size
            u = rng.choice(us, c) + 1 + rng.uniform(-0.25, 0.25, c)
            v = rng.choice(vs, c) + 1 + rng.uniform(-0.25, 0.25, c)
            z = rng.uniform(1.0, 4.0, c)
            cam = (np.linalg.inv(k) @ np.stack([u, v, np.ones(c)])) * z
            depth = (np.linalg.inv(d2c) @ cam).T
            out[todo] = (depth @ fwd[:3, :3].T + fwd[:3, 3]).astype(np.float32)
            todo = todo[out[todo, 1] < 0.5]
        img = np.zeros((3,) + tuple(pad_hw), np.float32)
        ih, iw = m["img_shape"][:2]
        img[:, :ih, :iw] = rng.randint(0, 256, (3, ih, iw))
        metas.append(m), rts.append(rt), ks.append(k), boxes.append(bx.astype(np.float32))
        seeds.append(out), pics.append(img)
    return dict(seeds=np.stack(seeds), boxes=boxes, metas=metas, Rt=np.stack(rts), K=np.stack(ks),
                imgs=np.stack(pics), num_classes=num_classes)


def to_torch(case, device="cpu", dtype=torch.float32):
    t = lambda a: torch.from_numpy(np.asarray(a)).to(device=device, dtype=dtype)   # noqa: E731
    return (t(case["imgs"]), [t(x) for x in case["boxes"]], t(case["seeds"]), case["metas"],
            dict(Rt=t(case["Rt"]), K=t(case["K"])))


def load_golden():
    return np.load(GOLDEN)
