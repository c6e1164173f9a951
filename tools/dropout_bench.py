#!/usr/bin/env python3
"""The dropout kernels (csrc/dropout.hip) at the ViT-L stream and MLP widths, [665 x 197, 1024] and [665 x 197, 4096] bf16, against the
bytes they must move and against the stochastic-depth kernels (csrc/drop_path.hip) at the same shapes, which move the same bytes without
a mask: the gap is what Philox4x32-10 costs.  Then what proj_drop = 0.1 costs one ViT-L Block (forward + backward, batch 665, N 197, bf16).

  python tools/dropout_bench.py [reps=100] [block_reps=10] [rounds=5]

Kernels (p = 0.1, no drop-path scale; the drop-path kernels with every sample kept):
  dropout_add / drop_path_add          out = res + m * branch / keep, in place over the branch: reads res and the branch, writes every row
  dropout / drop_path_scale            out = m * x / keep: reads and writes every row
  dropout+colsum / scale+colsum        the same with the fp32 column-sum partials and their ucfvit_reduce_rows fold (the bias-gradient route)
Bandwidth fractions are of the 6.29 TB/s a float4 copy reaches on an MI355X (8.0 TB/s is the HBM3E specification).

Block: HF.BlockFn with the dropout argument (p = 0.1, three fixed seeds) and without, in one process, `rounds` alternating windows of
`block_reps` forward + backward passes each; the figure is the median window and the spread is printed with it.  Times are HIP-event
times after a warm-up of every shape.  One JSON line per case on stdout."""
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
P, SEED = 0.1, 0x9E3779B97F4A7C15
STREAM_TBPS, SPEC_TBPS = 6.29, 8.0


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


def kernels(reps, width):
    g = torch.Generator(device=DEV).manual_seed(0)
    rows = B * N
    res = torch.randn((rows, width), generator=g, device=DEV).to(torch.bfloat16)
    x = torch.randn((rows, width), generator=g, device=DEV).to(torch.bfloat16)
    out = torch.empty_like(x)
    cs = torch.empty(width, device=DEV)
    one = torch.ones(B, device=DEV)
    row_bytes = width * 2
    pairs = [("add", lambda: ops.dropout_add(res, x, P, SEED), lambda: ops.drop_path_add(res, x, one, N), 3 * rows * row_bytes),
             ("scale", lambda: ops.dropout(x, P, SEED, out=out), lambda: ops.drop_path_scale(x, one, N, out=out), 2 * rows * row_bytes),
             ("scale+colsum", lambda: ops.dropout(x, P, SEED, out=out, c_colsum=cs),
              lambda: ops.drop_path_scale(x, one, N, out=out, c_colsum=cs), 2 * rows * row_bytes)]
    for name, drop, plain, must in pairs:
        keep0 = x.clone() if name == "add" else None              # add runs in place: the timed loop feeds on its own output, restore after
        t = {}
        for which, fn in (("dropout", drop), ("drop_path", plain)):
            t[which] = _timed(fn, reps)
            if keep0 is not None:
                x.copy_(keep0)
        print(json.dumps({"kernel": name, "shape": [rows, width], "dtype": "bfloat16", "p": P,
                          "dropout_ms": round(t["dropout"], 4), "drop_path_ms": round(t["drop_path"], 4),
                          "philox_extra_ms": round(t["dropout"] - t["drop_path"], 4), "ratio": round(t["dropout"] / t["drop_path"], 3),
                          "must_move_bytes": must, "dropout_TBps": round(must / t["dropout"] / 1e9, 3),
                          "drop_path_TBps": round(must / t["drop_path"] / 1e9, 3),
                          "dropout_frac_of_stream_6.29": round(must / t["dropout"] / 1e9 / STREAM_TBPS, 3),
                          "dropout_frac_of_spec_8.0": round(must / t["dropout"] / 1e9 / SPEC_TBPS, 3)}), flush=True)


def block(block_reps, rounds):
    torch.manual_seed(0)
    blk = BB.Block(D, HEADS, qkv_bias=True, norm_layer=lambda d: BB.LayerNorm(d, eps=1e-6)).to(DEV)
    BB.set_compute_dtype(blk, torch.bfloat16)
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn((B, N, D), generator=g, device=DEV).to(torch.bfloat16).requires_grad_(True)
    gy = torch.randn((B, N, D), generator=g, device=DEV).to(torch.bfloat16)
    a, m = blk.attn, blk.mlp
    args = (x, blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias, blk.norm2.weight, blk.norm2.bias,
            m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, HEADS, 1e-6, torch.bfloat16, None, False)
    drop = (P, SEED, SEED + 1, SEED + 2)

    def step(with_drop):
        y = HF.BlockFn.apply(*args, None, None, drop) if with_drop else HF.BlockFn.apply(*args)
        y.backward(gy)
        HF.flush_wgrads()
        x.grad = None
        for p in blk.parameters():
            p.grad = None

    t = {False: [], True: []}
    for with_drop in (False, True):
        _timed(lambda: step(with_drop), 2)                           # warm-up of both variants
    for _ in range(rounds):
        for with_drop in (False, True):
            t[with_drop].append(_timed(lambda: step(with_drop), block_reps))
    m0, m1 = statistics.median(t[False]), statistics.median(t[True])
    print(json.dumps({"block": "ViT-L fwd+bwd", "batch": B, "tokens": N, "dim": D, "dtype": "bfloat16", "rounds": rounds, "reps": block_reps,
                      "proj_drop_0_ms": round(m0, 3), "proj_drop_0_min_max_ms": [round(min(t[False]), 3), round(max(t[False]), 3)],
                      "proj_drop_0.1_ms": round(m1, 3), "proj_drop_0.1_min_max_ms": [round(min(t[True]), 3), round(max(t[True]), 3)],
                      "extra_ms": round(m1 - m0, 3), "extra_frac": round(m1 / m0 - 1.0, 4)}), flush=True)


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    kernels(arg(1, 100), D)
    kernels(arg(1, 100), 4 * D)
    block(arg(2, 10), arg(3, 5))
