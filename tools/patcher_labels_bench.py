#!/usr/bin/env python3
"""Label serializers, tree deserializers (csrc/patcher_labels.hip) and the deserializers' adjoints (csrc/patcher_labels_bwd.hip) on the GPU: each
op at two shapes,
    3-D  the basic_ct/sap shape: B = 2, 64^3, fixed_length 512, p = 4, 4 classes
    2-D  B = 8, 512^2, fixed_length 1024, p = 8, 4 classes
against (a) a per-leaf torch statement of the same rule on the same GPU (the reference's loop shape: one leaf per iteration) and (b) the bytes
the op must move at the measured HBM copy rate (6.29 TB/s).  The trees come from the GPU builders on synthetic contour maps.

Timing: device events around `reps` back-to-back calls after warm-up, three windows per op (min and max are printed: the spread); the torch
loop is timed once over the whole batch (host clock around a device synchronise).  The deserializers' zero fill is stated separately, twice: the
same call with count = 0 (the fill and a grid whose workgroups all return at once) and a fill of the output's bytes alone (tensor.zero_()).  One JSON line per op and shape.
Each adjoint (ops.*_deserialize_bwd, planar dout into the model layout) is stated against the forward call of the same shape, against
backward() of the per-leaf F.interpolate loop (the graph is built outside the clock) and against its bytes at the copy rate.  Last, the whole
SAP training step (forward, loss, backward, optimizer) of the smoke configuration (64 x 64, patch 8, fixed_length 16, 3 classes, batch 4) with
the loss on the token grid and with `loss_at_full_resolution`.

    python tools/patcher_labels_bench.py [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd"))
from UCF_VIT._hip import ops  # noqa: E402

HBM = 6.29e12           # bytes / s, measured float4 copy
DEV = "cuda"


def timed(fn, reps):
    """ms per call: three windows of `reps` calls -> (median, min, max)"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(3):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        t.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(t) / reps)
    return sorted(out)[1], min(out), max(out)


def once(fn):
    fn()                                                   # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def contours(shape, rng):
    """a few sphere / circle outlines, like object contours -> uint8 0 / 255, and the label map they bound (4 classes)"""
    grid = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    edges, labels = np.zeros(shape, bool), np.zeros(shape, np.uint8)
    for k in range(6):
        c = [rng.integers(0, n) for n in shape]
        r = rng.integers(shape[0] // 16, shape[0] // 3)
        d = np.sqrt(sum((g - v) ** 2 for g, v in zip(grid, c)))
        edges |= np.abs(d - r) < 1.0
        labels[d < r] = 1 + k % 3
    return edges.astype(np.uint8) * 255, labels


def nearest_floor(j, n_src, n_dst):
    return torch.clamp((j * n_src) // n_dst, max=n_src - 1)


def nearest_grid(j, n_src, n_dst):
    if n_src < 2 or n_dst < 2:
        return torch.zeros_like(j)
    num, den = j * (n_src - 1), n_dst - 1
    i = torch.clamp(num // den, max=n_src - 2)
    return torch.where(2 * (num - i * den) <= den, i, i + 1)


def torch_labels(dim, labels, nodes, count, p, nc):
    """per leaf, as the reference loops: the nearest rule by index tensors, then one F.one_hot over the sequence"""
    B, S = nodes.shape[:2]
    idx = torch.zeros((B, S) + (p,) * dim, dtype=torch.int64, device=DEV)
    k = torch.arange(p, device=DEV)
    nd, ct = nodes.tolist(), count.tolist()
    for b in range(B):
        for s in range(min(ct[b], S)):
            q = nd[b][s]
            if dim == 2:
                x1, x2, y1, y2 = q
                if x2 - x1 <= 0 or y2 - y1 <= 0:
                    continue
                idx[b, s] = labels[b][(y1 + nearest_floor(k, y2 - y1, p))[:, None], (x1 + nearest_floor(k, x2 - x1, p))[None, :]]
            else:
                x1, x2, y1, y2, z1, z2 = q
                if x2 - x1 <= 0 or y2 - y1 <= 0 or z2 - z1 <= 0:
                    continue
                idx[b, s] = labels[b][(z1 + nearest_grid(k, z2 - z1, p))[:, None, None], (y1 + nearest_grid(k, y2 - y1, p))[None, :, None],
                                      (x1 + nearest_grid(k, x2 - x1, p))[None, None, :]]
    return idx, F.one_hot(idx.reshape(B, -1), nc).permute(0, 2, 1).float().contiguous()


def torch_deserialize(dim, seq, nodes, count, size, p):
    """seq [B, C, S, P] -> [B, C, *size]: per leaf F.interpolate (bicubic, half-pixel centres, A = -0.75 / trilinear, aligned corners)"""
    B, C, S, _ = seq.shape
    out = torch.zeros((B, C) + tuple(size), dtype=torch.float32, device=DEV)
    nd, ct = nodes.tolist(), count.tolist()
    for b in range(B):
        for s in range(min(ct[b], S)):
            q = nd[b][s]
            patch = seq[b, :, s].reshape(1, C, *([p] * dim))
            if dim == 2:
                x1, x2, y1, y2 = q
                if x2 - x1 <= 0 or y2 - y1 <= 0:
                    continue
                out[b, :, y1:y2, x1:x2] = F.interpolate(patch, size=(y2 - y1, x2 - x1), mode="bicubic", align_corners=False)[0]
            else:
                x1, x2, y1, y2, z1, z2 = q
                if x2 - x1 <= 0 or y2 - y1 <= 0 or z2 - z1 <= 0:
                    continue
                out[b, :, z1:z2, y1:y2, x1:x2] = F.interpolate(patch, size=(z2 - z1, y2 - y1, x2 - x1), mode="trilinear", align_corners=True)[0]
    return out


def torch_backward_ms(dim, seq, nodes, count, shape, p, g):
    """backward() of the per-leaf loop alone, ms: the second of two runs, each on a graph built before the clock starts"""
    ms = None
    for _ in range(2):
        leaf = seq.clone().requires_grad_(True)
        full = torch_deserialize(dim, leaf, nodes, count, shape, p)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        full.backward(g)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
    return ms, leaf.grad


def sap_step(reps):
    """ms per training step of the tiny SAP of the smoke configuration, loss on the token grid / at full resolution"""
    import yaml
    sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd", "training_scripts"))
    import _common
    import train_sap_simple as T
    from UCF_VIT.simple.arch import SAP
    from UCF_VIT.utils.fused_attn import FusedAttn
    from UCF_VIT.utils.misc import configure_optimizer
    conf = yaml.safe_load(open(os.path.join(ROOT, "ucf-vit_amd", "configs", "catsdogs_vit_tiny_smoke.yaml")))
    conf["model"]["net"]["init_args"].update(tile_size=[64, 64], patch_size=8, embed_dim=96, depth=2, num_heads=3, adaptive_patching=True, fixed_length=16,
                                             use_adaptive_pos_emb=True)
    conf["data"].update(num_classes=3, batch_size=4)
    margs, a, d = _common.model_args(conf)
    nc, L, m = d["num_classes"], margs["fixed_length"], conf["model"]
    sqrt_len = _common.sqrt_len_of(L, margs["twoD"])
    torch.manual_seed(0)
    model = SAP(num_classes=nc, sqrt_len=sqrt_len, sqrt_len_method=True, class_token=False, weight_init='skip', FusedAttn_option=FusedAttn.HIP,
                **margs).to(DEV)
    model.set_compute_dtype(torch.float32)
    opt = configure_optimizer(model, 1e-3, float(m["beta_1"]), float(m["beta_2"]), float(m["weight_decay"]))
    loader = _common.SyntheticSeqLoader(d["batch_size"], margs["in_chans"], margs["img_size"], margs["patch_size"], L, nc, 1, DEV, 1234, labels_from_image=True)
    seq, seq_ps, (seq_label, label_map, nodes, count) = next(iter(loader))
    seq = seq / 255.0
    common = (d["dict_in_variables"][d["dataset"]], model, margs["patch_size"], margs["twoD"], nc, sqrt_len, seq_ps, margs["in_chans"])

    def step(full):
        loss, _ = T.training_step_full_resolution(seq, label_map, nodes, count, *common, L) if full else T.training_step_adaptive(seq, seq_label, *common)
        loss.backward()
        opt.step()
        opt.zero_grad()
    out = {"op": "sap_training_step", "shape": "B=4 64^2 L=16 p=8 nc=3 embed 96 depth 2, fp32"}
    for name, full in (("token_grid_loss", False), ("loss_at_full_resolution", True)):
        ms = timed(lambda: step(full), reps)
        out[name + "_ms"], out[name + "_ms_min_max"] = round(ms[0], 4), [round(ms[1], 4), round(ms[2], 4)]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    reps = ap.parse_args().reps
    rng = np.random.Generator(np.random.PCG64(0))
    for dim, B, n, L, p, nc in ((3, 2, 64, 512, 4, 4), (2, 8, 512, 1024, 8, 4)):
        shape = (n,) * dim
        maps, labs = zip(*[contours(shape, rng) for _ in range(B)])
        edges, labels = torch.from_numpy(np.stack(maps)).to(DEV), torch.from_numpy(np.stack(labs)).to(DEV)
        nodes, _, count, _ = ops.quadtree_build(edges, L) if dim == 2 else ops.octree_build(edges, L)
        ser = ops.quadtree_serialize_labels if dim == 2 else ops.octree_serialize_labels
        des = ops.quadtree_deserialize if dim == 2 else ops.octree_deserialize
        P, npix = p ** dim, n ** dim
        size = shape if dim == 2 else n
        ext = (nodes[..., 1] - nodes[..., 0]).clamp_min(0)
        tag = {"shape": f"B={B} {n}^{dim} L={L} p={p} nc={nc}", "valid_leaves": int(count.sum().item()), "largest_leaf": int(ext.max().item()),
               "smallest_leaf": int(ext[ext > 0].min().item())}
        # ---- label serializer: indices + one-hot
        idx, oh = ser(labels, nodes, count, p, nc)
        ms = timed(lambda: ser(labels, nodes, count, p, nc), reps)
        t_ms, (t_idx, t_oh) = once(lambda: torch_labels(dim, labels.long(), nodes, count, p, nc))
        must = B * L * P * (1 + 8 + 4 * nc) + nodes.numel() * 4
        print(json.dumps({"op": f"{'quadtree' if dim == 2 else 'octree'}_serialize_labels", **tag, "ms": round(ms[0], 4), "ms_min_max": [round(ms[1], 4), round(ms[2], 4)],
                          "torch_per_leaf_ms": round(t_ms, 2), "speedup": round(t_ms / ms[0], 1), "bytes_must_move": must,
                          "ms_at_hbm_rate": round(must / HBM * 1e3, 5), "equal_to_torch": bool(torch.equal(idx, t_idx) and torch.equal(oh, t_oh))}), flush=True)
        # ---- deserializer: logits per class in the model layout -> planar image
        seq = torch.randn((B, nc, L, P), device=DEV)
        zero = torch.zeros_like(count)
        for mode in ("bicubic" if dim == 2 else "trilinear", "nearest"):
            full = des(seq, nodes, count, size, p, mode=mode, channels_last=False)
            ms = timed(lambda: des(seq, nodes, count, size, p, mode=mode, channels_last=False), reps)
            fill = timed(lambda: des(seq, nodes, zero, size, p, mode=mode, channels_last=False), reps)
            blank = torch.empty_like(full)
            memset = timed(lambda: blank.zero_(), reps)                                   # a fill of the output's bytes alone
            must = B * nc * (L * P + npix) * 4 + nodes.numel() * 4
            rec = {"op": f"{'quadtree' if dim == 2 else 'octree'}_deserialize[{mode}]", **tag, "ms": round(ms[0], 4), "ms_min_max": [round(ms[1], 4), round(ms[2], 4)],
                   "zero_fill_and_empty_grid_ms": round(fill[0], 4), "zero_fill_and_empty_grid_share": round(fill[0] / ms[0], 3),
                   "fill_of_the_output_alone_ms": round(memset[0], 4), "fill_alone_share": round(memset[0] / ms[0], 3), "bytes_must_move": must,
                   "ms_at_hbm_rate": round(must / HBM * 1e3, 5)}
            if mode != "nearest":
                t_ms, t_full = once(lambda: torch_deserialize(dim, seq, nodes, count, shape, p))
                rec.update(torch_per_leaf_ms=round(t_ms, 2), speedup=round(t_ms / ms[0], 1), max_abs_diff_to_torch=float((full - t_full).abs().max().item()))
            print(json.dumps(rec), flush=True)
            # ---- its adjoint: planar gradient of the image plane -> the model layout
            bwd = ops.quadtree_deserialize_bwd if dim == 2 else ops.octree_deserialize_bwd
            g = torch.randn_like(full)
            dseq = bwd(g, nodes, count, seq, p, mode=mode, channels_last=False)
            bms = timed(lambda: bwd(g, nodes, count, seq, p, mode=mode, channels_last=False), reps)
            must = B * nc * (L * P + npix) * 4 + nodes.numel() * 4
            rec = {"op": f"{'quadtree' if dim == 2 else 'octree'}_deserialize_bwd[{mode}]", **tag, "ms": round(bms[0], 4),
                   "ms_min_max": [round(bms[1], 4), round(bms[2], 4)], "forward_ms": round(ms[0], 4), "over_forward": round(bms[0] / ms[0], 2),
                   "bytes_must_move": must, "ms_at_hbm_rate": round(must / HBM * 1e3, 5),
                   "same_bits_twice": bool(torch.equal(dseq, bwd(g, nodes, count, seq, p, mode=mode, channels_last=False)))}
            if mode != "nearest":
                t_ms, t_grad = torch_backward_ms(dim, seq, nodes, count, shape, p, g)
                rec.update(torch_per_leaf_backward_ms=round(t_ms, 2), speedup=round(t_ms / bms[0], 1),
                           max_abs_diff_to_torch=float((dseq - t_grad).abs().max().item()))
            print(json.dumps(rec), flush=True)
    sap_step(reps)


if __name__ == "__main__":
    main()
