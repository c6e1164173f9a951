#!/usr/bin/env python3
"""The LayerScale kernels (csrc/layer_scale.hip) at the ViT-L stream, [665 x 197, 1024] bf16, against the bytes they must move and
against their siblings in the same process, and what LayerScale costs one ViT-L Block (forward + backward, batch 665, N 197, bf16)
against the same Block without it.

  python tools/layer_scale_bench.py [reps=100] [block_reps=10] [rounds=5]

Three variants of every kernel: plain (gamma alone), with the drop-path scale s (drop_prob 0.1: a dropped sample's rows are not read)
and with the dropout mask p = 0.1.  Must-move bytes: forward reads res and the branch and writes out (three matrices; two with
res == NULL); backward reads dy and the branch and writes dbranch.  The siblings move one matrix less in backward (no branch).
  layer_scale_add      | drop_path_add (s) / dropout_add (p)
  layer_scale_add/nores| drop_path_scale (s) / dropout (p)
  layer_scale_grad+sums| drop_path_scale+colsum (s) / dropout+colsum (p)            both sums, folded by ucfvit_reduce_rows
Every case is timed `rounds` times (`reps` launches each): the figure is the median, the spread (min, max) is printed with it, and
the achieved bandwidth is must-move bytes over the median.  Fractions are of the 6.29 TB/s a float4 copy reaches on an MI355X.

Block: HF.BlockFn with gammas and without, in one process, `rounds` alternating windows of `block_reps` forward + backward passes
each; median window and spread.  Times are HIP-event times after a warm-up of every shape.  One JSON line per case on stdout."""
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
STREAM_TBPS = 6.29
P, SEED = 0.1, 0x0123456789ABCDEF


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


def _draw(drop_prob, seed):
    keep = 1.0 - drop_prob
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.empty(B, device=DEV).bernoulli_(keep, generator=g) / keep


def kernels(reps, rounds):
    g = torch.Generator(device=DEV).manual_seed(0)
    rows = B * N
    res = torch.randn((rows, D), generator=g, device=DEV).to(torch.bfloat16)
    x = torch.randn((rows, D), generator=g, device=DEV).to(torch.bfloat16)
    dy = torch.randn((rows, D), generator=g, device=DEV).to(torch.bfloat16)
    out = torch.empty_like(x)
    gamma = (0.5 + 0.3 * torch.randn(D, generator=g, device=DEV)).contiguous()
    cs, gs = torch.empty(D, device=DEV), torch.empty(D, device=DEV)
    rb = D * 2
    s = _draw(0.1, 1)
    kept = int((s != 0).sum().item()) * N
    ls = dict(rows_per_sample=N, out=out)
    cases = [
        # variant, kernel, sibling-of, fn, must-move bytes
        ("plain", "layer_scale_add", None, lambda: ops.layer_scale_add(res, x, gamma, **ls), 3 * rows * rb),
        ("plain", "layer_scale_add/nores", None, lambda: ops.layer_scale_add(None, x, gamma, **ls), 2 * rows * rb),
        ("plain", "layer_scale_grad+sums", None, lambda: ops.layer_scale_grad(dy, x, gamma, c_colsum=cs, c_gamma=gs, **ls), 3 * rows * rb),
        ("plain", "layer_scale_grad", None, lambda: ops.layer_scale_grad(dy, None, gamma, **ls), 2 * rows * rb),
        ("s", "layer_scale_add", None, lambda: ops.layer_scale_add(res, x, gamma, s=s, **ls), (2 * rows + kept) * rb),
        ("s", "drop_path_add", "layer_scale_add", lambda: ops.drop_path_add(res, x, s, N, out=out), (2 * rows + kept) * rb),
        ("s", "layer_scale_add/nores", None, lambda: ops.layer_scale_add(None, x, gamma, s=s, **ls), (rows + kept) * rb),
        ("s", "drop_path_scale", "layer_scale_add/nores", lambda: ops.drop_path_scale(x, s, N, out=out), (rows + kept) * rb),
        ("s", "layer_scale_grad+sums", None, lambda: ops.layer_scale_grad(dy, x, gamma, s=s, c_colsum=cs, c_gamma=gs, **ls),
         (rows + 2 * kept) * rb),
        ("s", "drop_path_scale+colsum", "layer_scale_grad+sums", lambda: ops.drop_path_scale(dy, s, N, out=out, c_colsum=cs),
         (rows + kept) * rb),
        ("p", "layer_scale_add", None, lambda: ops.layer_scale_add(res, x, gamma, p=P, seed=SEED, **ls), 3 * rows * rb),
        ("p", "dropout_add", "layer_scale_add", lambda: ops.dropout_add(res, x, P, SEED, out=out), 3 * rows * rb),
        ("p", "layer_scale_add/nores", None, lambda: ops.layer_scale_add(None, x, gamma, p=P, seed=SEED, **ls), 2 * rows * rb),
        ("p", "dropout", "layer_scale_add/nores", lambda: ops.dropout(x, P, SEED, out=out), 2 * rows * rb),
        ("p", "layer_scale_grad+sums", None, lambda: ops.layer_scale_grad(dy, x, gamma, p=P, seed=SEED, c_colsum=cs, c_gamma=gs, **ls),
         3 * rows * rb),
        ("p", "dropout+colsum", "layer_scale_grad+sums", lambda: ops.dropout(dy, P, SEED, out=out, c_colsum=cs), 2 * rows * rb),
    ]
    for variant, name, sibling_of, fn, must in cases:
        _timed(fn, 3)
        ts = [_timed(fn, reps) for _ in range(rounds)]
        t = statistics.median(ts)
        print(json.dumps({"kernel": name, "variant": variant, "sibling_of": sibling_of, "shape": [rows, D], "dtype": "bfloat16",
                          "ms": round(t, 4), "min_max_ms": [round(min(ts), 4), round(max(ts), 4)], "must_move_bytes": must,
                          "must_move_TBps": round(must / t / 1e9, 3),
                          "TBps_min_max": [round(must / max(ts) / 1e9, 3), round(must / min(ts) / 1e9, 3)],
                          "frac_of_stream_6.29": round(must / t / 1e9 / STREAM_TBPS, 3)}), flush=True)


def block(block_reps, rounds):
    torch.manual_seed(0)
    blk = BB.Block(D, HEADS, qkv_bias=True, init_values=0.1, norm_layer=lambda d: BB.LayerNorm(d, eps=1e-6)).to(DEV)
    BB.set_compute_dtype(blk, torch.bfloat16)
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn((B, N, D), generator=g, device=DEV).to(torch.bfloat16).requires_grad_(True)
    gy = torch.randn((B, N, D), generator=g, device=DEV).to(torch.bfloat16)
    a, m = blk.attn, blk.mlp
    args = (x, blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias, blk.norm2.weight, blk.norm2.bias,
            m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, HEADS, 1e-6, torch.bfloat16, None, False)

    def step(with_ls):
        y = HF.BlockFn.apply(*args, None, None, None, blk.ls1.gamma, blk.ls2.gamma) if with_ls else HF.BlockFn.apply(*args)
        y.backward(gy)
        HF.flush_wgrads()
        x.grad = None
        for p in blk.parameters():
            p.grad = None

    t = {False: [], True: []}
    for with_ls in (False, True):
        _timed(lambda: step(with_ls), 2)                             # warm-up of both variants
    for _ in range(rounds):
        for with_ls in (False, True):
            t[with_ls].append(_timed(lambda: step(with_ls), block_reps))
    m0, m1 = statistics.median(t[False]), statistics.median(t[True])
    print(json.dumps({"block": "ViT-L fwd+bwd", "batch": B, "tokens": N, "dim": D, "dtype": "bfloat16", "rounds": rounds, "reps": block_reps,
                      "plain_ms": round(m0, 3), "plain_min_max_ms": [round(min(t[False]), 3), round(max(t[False]), 3)],
                      "layer_scale_ms": round(m1, 3), "layer_scale_min_max_ms": [round(min(t[True]), 3), round(max(t[True]), 3)],
                      "extra_ms": round(m1 - m0, 3), "extra_frac": round(m1 / m0 - 1.0, 4)}), flush=True)


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    kernels(arg(1, 100), arg(3, 5))
    block(arg(2, 10), arg(3, 5))
