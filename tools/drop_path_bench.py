#!/usr/bin/env python3
"""The stochastic-depth kernels (csrc/drop_path.hip) at the ViT-L stream, [665 x 197, 1024] bf16, against the bytes they must move, and
what drop path costs one ViT-L Block (forward + backward, batch 665, N 197, bf16) against the same Block without it.

  python tools/drop_path_bench.py [reps=100] [block_reps=10] [rounds=5]

Kernels, with all samples kept and with drop_prob = 0.1 (a dropped sample's branch is not read):
  add            out = res + s * branch, in place over the branch: reads res and the kept rows of the branch, writes every row
  scale          out = s * x: reads the kept rows, writes every row
  scale+colsum   the same with the fp32 column-sum partials and their ucfvit_reduce_rows fold (the bias-gradient route)
Bandwidth fractions are of the 6.29 TB/s a float4 copy reaches on an MI355X (8.0 TB/s is the HBM3E specification).

Block: HF.BlockFn with scales of drop_prob = 0.1 (drawn once, fixed) and without, in one process, `rounds` alternating windows of
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


def _draw(drop_prob, seed):
    keep = 1.0 - drop_prob
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.empty(B, device=DEV).bernoulli_(keep, generator=g) / keep


def kernels(reps):
    g = torch.Generator(device=DEV).manual_seed(0)
    rows = B * N
    res = torch.randn((rows, D), generator=g, device=DEV).to(torch.bfloat16)
    x = torch.randn((rows, D), generator=g, device=DEV).to(torch.bfloat16)
    out = torch.empty_like(x)
    cs = torch.empty(D, device=DEV)
    row_bytes = D * 2
    for drop_prob in (0.0, 0.1):
        s = _draw(drop_prob, 1)
        kept = int((s != 0).sum().item()) * N
        cases = [("add", lambda: ops.drop_path_add(res, x, s, N), (rows + kept + rows) * row_bytes),
                 ("scale", lambda: ops.drop_path_scale(x, s, N, out=out), (kept + rows) * row_bytes),
                 ("scale+colsum", lambda: ops.drop_path_scale(x, s, N, out=out, c_colsum=cs), (kept + rows) * row_bytes)]
        for name, fn, must in cases:
            keep0 = x.clone() if name == "add" else None          # add runs in place: the timed loop feeds on its own output, restore after
            t = _timed(fn, reps)
            if keep0 is not None:
                x.copy_(keep0)
            print(json.dumps({"kernel": name, "shape": [rows, D], "dtype": "bfloat16", "drop_prob": drop_prob, "kept_rows": kept,
                              "ms": round(t, 4), "must_move_bytes": must, "must_move_TBps": round(must / t / 1e9, 3),
                              "frac_of_stream_6.29": round(must / t / 1e9 / STREAM_TBPS, 3),
                              "frac_of_spec_8.0": round(must / t / 1e9 / SPEC_TBPS, 3)}), flush=True)


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
    s1, s2 = _draw(0.1, 3), _draw(0.1, 4)

    def step(with_drop):
        y = HF.BlockFn.apply(*args, s1, s2) if with_drop else HF.BlockFn.apply(*args)
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
                      "drop_path_0_ms": round(m0, 3), "drop_path_0_min_max_ms": [round(min(t[False]), 3), round(max(t[False]), 3)],
                      "drop_path_0.1_ms": round(m1, 3), "drop_path_0.1_min_max_ms": [round(min(t[True]), 3), round(max(t[True]), 3)],
                      "extra_ms": round(m1 - m0, 3), "extra_frac": round(m1 / m0 - 1.0, 4)}), flush=True)


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    kernels(arg(1, 100))
    block(arg(2, 10), arg(3, 5))
