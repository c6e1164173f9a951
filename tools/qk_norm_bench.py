#!/usr/bin/env python3
"""The QK-norm kernels (csrc/qk_norm.hip) at the ViT-L stream, qkv [665 x 197, 3 x 16 x 64] bf16, and at the ViT-B geometry
([256 x 197, 3 x 12 x 64]), against the bytes they must move and against the LayerNorm kernels at [rows, 1024] / [rows, 768] in the same
process, and what qk_norm costs one ViT-L Block (forward + backward, batch 665, N 197, bf16) against the same Block without it.

  python tools/qk_norm_bench.py [reps=100] [block_reps=10] [rounds=5]

Must-move bytes, in D-wide token matrices of the dtype (D = H dh; Q and K together are two of them):
  qk_norm_fwd (eval)   reads 2, writes 2 in place                               = 4
  qk_norm_fwd (train)  reads 2, writes 2 in place, writes 2 saved (+ statistics) = 6
  qk_norm_bwd          reads 2 (dqkv) + 2 (saved), writes 2 (+ statistics)      = 6     with and without the two sets of partial sums
  layernorm_fwd        reads 1, writes 1                                        = 2
  layernorm_bwd        reads 2 (dy, x), writes 1                                = 3
Every case is timed `rounds` times (`reps` launches each): the figure is the median, the spread (min, max) is printed with it, and the
achieved bandwidth is must-move bytes over the median.  Fractions are of the 6.29 TB/s a float4 copy reaches on an MI355X
(profiles/layer_scale.md).  The in-place kernels are timed on the buffer they keep rewriting: a LayerNorm of a LayerNorm is as much
work as the first.

Block: HF.BlockFn with the four parameters and without, in one process, `rounds` alternating windows of `block_reps` forward + backward
passes each; median window and spread.  Times are HIP-event times after a warm-up of every shape.  One JSON line per case on stdout."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd"))
from UCF_VIT._hip import functional as HF  # noqa: E402
from UCF_VIT._hip import ops  # noqa: E402
from UCF_VIT.simple import building_blocks as BB  # noqa: E402

DEV = "cuda"
B, N, D, HEADS = 665, 197, 1024, 16
GEOMETRIES = {"vit_l": (665 * 197, 16, 64), "vit_b": (256 * 197, 12, 64)}
STREAM_TBPS = 6.29


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def kernels(geom, reps, rounds):
    rows, H, dh = GEOMETRIES[geom]
    Dm = H * dh
    g = torch.Generator(device=DEV).manual_seed(0)
    qkv = torch.randn((rows, 3 * Dm), generator=g, device=DEV).to(torch.bfloat16)
    dqkv = torch.randn((rows, 3 * Dm), generator=g, device=DEV).to(torch.bfloat16)
    par = [(1.0 + 0.3 * torch.randn(dh, generator=g, device=DEV)).contiguous() for _ in range(4)]
    saved, mean, rstd = ops.qk_norm_fwd(qkv.clone(), *par, H, dh, 1e-6)
    pg, cs = torch.empty((4, dh), device=DEV), torch.empty(2 * Dm, device=DEV)
    x = torch.randn((rows, Dm), generator=g, device=DEV).to(torch.bfloat16)
    dy = torch.randn((rows, Dm), generator=g, device=DEV).to(torch.bfloat16)
    lw, lb = torch.ones(Dm, device=DEV, dtype=torch.bfloat16), torch.zeros(Dm, device=DEV, dtype=torch.bfloat16)
    _, lmean, lrstd = ops.layernorm_fwd(x, lw, lb, 1e-6)
    mat = rows * Dm * 2
    cases = [
        ("qk_norm_fwd/eval", None, lambda: ops.qk_norm_fwd(qkv, *par, H, dh, 1e-6, save=False), 4 * mat),
        ("qk_norm_fwd/train", None, lambda: ops.qk_norm_fwd(qkv, *par, H, dh, 1e-6), 6 * mat + 2 * rows * 2 * H * 4),
        ("qk_norm_bwd", None, lambda: ops.qk_norm_bwd(dqkv, saved, par[0], par[2], mean, rstd, H, dh), 6 * mat + 2 * rows * 2 * H * 4),
        ("qk_norm_bwd+sums", None, lambda: ops.qk_norm_bwd(dqkv, saved, par[0], par[2], mean, rstd, H, dh, param_grads=pg, c_colsum=cs),
         6 * mat + 2 * rows * 2 * H * 4),
        ("layernorm_fwd", "qk_norm_fwd", lambda: ops.layernorm_fwd(x, lw, lb, 1e-6), 2 * mat),
        ("layernorm_bwd", "qk_norm_bwd", lambda: ops.layernorm_bwd(dy, x, lw, lmean, lrstd), 3 * mat),
    ]
    for name, sibling_of, fn, must in cases:
        _timed(fn, 3)
        ts = [_timed(fn, reps) for _ in range(rounds)]
        t = statistics.median(ts)
        print(json.dumps({"kernel": name, "geometry": geom, "sibling_of": sibling_of, "shape": [rows, H, dh], "dtype": "bfloat16",
                          "ms": round(t, 4), "min_max_ms": [round(min(ts), 4), round(max(ts), 4)], "must_move_bytes": must,
                          "must_move_TBps": round(must / t / 1e9, 3),
                          "TBps_min_max": [round(must / max(ts) / 1e9, 3), round(must / min(ts) / 1e9, 3)],
                          "frac_of_stream_6.29": round(must / t / 1e9 / STREAM_TBPS, 3)}), flush=True)


def block(block_reps, rounds):
    torch.manual_seed(0)
    blk = BB.Block(D, HEADS, qkv_bias=True, qk_norm=True, norm_layer=lambda d: BB.LayerNorm(d, eps=1e-6)).to(DEV)
    BB.set_compute_dtype(blk, torch.bfloat16)
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn((B, N, D), generator=g, device=DEV).to(torch.bfloat16).requires_grad_(True)
    gy = torch.randn((B, N, D), generator=g, device=DEV).to(torch.bfloat16)
    a, m = blk.attn, blk.mlp
    args = (x, blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias, blk.norm2.weight, blk.norm2.bias,
            m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, HEADS, 1e-6, torch.bfloat16, None, False)
    qk = (a.q_norm.weight, a.q_norm.bias, a.k_norm.weight, a.k_norm.bias, 1e-6)

    def step(with_qk):
        y = HF.BlockFn.apply(*args, None, None, None, None, None, True, *qk) if with_qk else HF.BlockFn.apply(*args)
        y.backward(gy)
        HF.flush_wgrads()
        x.grad = None
        for p in blk.parameters():
            p.grad = None

    t = {False: [], True: []}
    for with_qk in (False, True):
        _timed(lambda: step(with_qk), 2)                             # warm-up of both variants
    for _ in range(rounds):
        for with_qk in (False, True):
            t[with_qk].append(_timed(lambda: step(with_qk), block_reps))
    m0, m1 = statistics.median(t[False]), statistics.median(t[True])
    print(json.dumps({"block": "ViT-L fwd+bwd", "batch": B, "tokens": N, "dim": D, "dtype": "bfloat16", "rounds": rounds, "reps": block_reps,
                      "plain_ms": round(m0, 3), "plain_min_max_ms": [round(min(t[False]), 3), round(max(t[False]), 3)],
                      "qk_norm_ms": round(m1, 3), "qk_norm_min_max_ms": [round(min(t[True]), 3), round(max(t[True]), 3)],
                      "extra_ms": round(m1 - m0, 3), "extra_frac": round(m1 / m0 - 1.0, 4)}), flush=True)


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    for geom in GEOMETRIES:
        kernels(geom, arg(1, 100), arg(3, 5))
    block(arg(2, 10), arg(3, 5))
