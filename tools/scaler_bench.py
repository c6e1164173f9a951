#!/usr/bin/env python3
"""Cost of the loss scaler's kernels on flat buffers of the ViT-L parameter count (HIP events, warm-up, median of --reps launches):

  1. ucfvit_adamw           from --baseline-lib (another build of the library, e.g. the parent commit's) if given, else from this build
  2. ucfvit_adamw_scaled    clean flag
  3. ucfvit_grad_nonfinite  (a pure read of the gradient buffer)
  4. ucfvit_adamw_scaled    flag set: a skipped step

and whether (1) and (2) leave bit-identical p, m, v and shadow from the same state (scale 1, first step).  One JSON line on stdout.

    python tools/scaler_bench.py [--n 304000000] [--reps 30] [--grad-dtype fp32|bf16] [--baseline-lib path/to/libucfvit_hip.so]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd"))

from UCF_VIT._hip import lib, ops  # noqa: E402


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
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
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=304_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--grad-dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--baseline-lib", default=None)
    a = ap.parse_args()
    n = a.n // 64 * 64
    dev = "cuda"
    gdt = torch.float32 if a.grad_dtype == "fp32" else torch.bfloat16
    gb = 2 if a.grad_dtype == "bf16" else 4
    L = lib.load()
    base = L
    if a.baseline_lib:
        base = ctypes.CDLL(a.baseline_lib)
        base.ucfvit_adamw.restype, base.ucfvit_adamw.argtypes = lib.SIGNATURES["ucfvit_adamw"]
    hp = dict(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.05)
    stream = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731

    def buffers(seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        p = torch.randn(n, generator=g, device=dev)
        grad = (torch.randn(n, generator=g, device=dev) * 1e-2).to(gdt)
        return p, grad, torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.empty(n, dtype=torch.bfloat16, device=dev)

    def plain(library, p, g, m, v, sh, step=1):
        rc = library.ucfvit_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), sh.data_ptr(), n, hp["lr"], hp["b1"], hp["b2"],
                                  hp["eps"], hp["wd"], 1.0 - hp["b1"] ** step, 1.0 - hp["b2"] ** step, 1.0, ops.dt(g), stream())
        assert rc == 0, rc

    def scaled(p, g, m, v, sh, st):
        ops.adamw_scaled(p, g, m, v, sh, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], st)

    from UCF_VIT._hip.grad_scaler import HipGradScaler
    clean = HipGradScaler(init_scale=1.0, backoff_factor=1.0, growth_interval=10 ** 6).device_state()
    fired = clean.clone()
    fired[lib.GS_FOUND_INF] = 1.0

    # --- same state, first step: baseline ucfvit_adamw, this build's ucfvit_adamw and ucfvit_adamw_scaled must agree bit for bit
    outs = []
    for which in ("baseline", "plain", "scaled"):
        p, g, m, v, sh = buffers(1)
        if which == "scaled":
            scaled(p, g, m, v, sh, clean)
        else:
            plain(base if which == "baseline" else L, p, g, m, v, sh)
        outs.append([t.view(torch.int16 if t.element_size() == 2 else torch.int32) for t in (p, m, v, sh)])
        if which == "baseline":
            keep = outs[0]
            outs[0] = [t.clone() for t in keep]
    same_plain = all(torch.equal(x, y) for x, y in zip(outs[0], outs[1]))
    same_scaled = all(torch.equal(x, y) for x, y in zip(outs[0], outs[2]))
    del outs, keep

    t1 = timed(lambda: plain(base, p, g, m, v, sh, 7), a.reps)
    t2 = timed(lambda: scaled(p, g, m, v, sh, clean), a.reps)
    t3 = timed(lambda: ops.grad_nonfinite(g, clean), a.reps)
    before = p[:1024].clone()
    t4 = timed(lambda: scaled(p, g, m, v, sh, fired), a.reps)
    assert torch.equal(before, p[:1024]) and clean[lib.GS_FOUND_INF].item() == 0.0
    adamw_bytes = n * (6 * 4 + gb + 2)             # p, m, v read and written, g read, shadow written
    out = dict(device=torch.cuda.get_device_name(0), n=n, grad_dtype=a.grad_dtype, reps=a.reps,
               baseline_lib=bool(a.baseline_lib), adamw_us=t1, adamw_scaled_us=t2, grad_nonfinite_us=t3, adamw_scaled_skipped_us=t4,
               adamw_GBps=adamw_bytes / t1[0] * 1e-3, adamw_scaled_GBps=adamw_bytes / t2[0] * 1e-3, grad_nonfinite_GBps=n * gb / t3[0] * 1e-3,
               scaled_over_plain=t2[0] / t1[0], plain_bits_equal_baseline=same_plain, scaled_bits_equal_baseline=same_scaled)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
