#!/usr/bin/env python3
"""Cost of gradient clipping by global norm at the ViT-L parameter count (HIP events, warm-up; every figure is the median of --rounds medians
of --reps launches, with the smallest and largest of those medians: the spread the comparisons are read against).

Kernels, on one flat buffer of --n elements, fp32 or bf16 gradients:
  grad_nonfinite        the pass the fused one replaces (the yardstick: same bytes, same process, same box)
  grad_sqnorm           without and with the loss scaler's state
  grad_clip_coef        the fold of the partial sums
  adamw / adamw_clipped and adamw_scaled / adamw_clipped with the scaler's state (the yardstick of each is its unclipped sibling)
  torch                 torch.nn.utils.clip_grad_norm_ on the same flat buffer (fp32 only: it rewrites the gradient), then ucfvit_adamw
Rounds of the members of a comparison are interleaved, so a drift of the box lands on all of them.

Optimizer, on a ViT-L/16 whose parameters live in one HipParamStore (two flat runs): HipAdamW.step / HipGradScaler.step + update with and
without max_grad_norm.  --skip-step leaves this part out.  One JSON line on stdout.

    python tools/grad_clip_bench.py [--n 304000000] [--reps 20] [--rounds 5] [--grad-dtype fp32|bf16] [--skip-step]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd"))

from UCF_VIT._hip import lib, ops  # noqa: E402


def median_us(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def compare(fns, reps, rounds, warmup=3):
    """{name: (median of the round medians, smallest, largest)} in microseconds, rounds interleaved over the names"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    meds = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            meds[k].append(median_us(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in meds.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=304_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--grad-dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    n = a.n // 64 * 64
    dev = "cuda"
    gdt = torch.float32 if a.grad_dtype == "fp32" else torch.bfloat16
    gb = 2 if a.grad_dtype == "bf16" else 4
    hp = (1e-3, 0.9, 0.95, 1e-8, 0.05)
    out = dict(device=torch.cuda.get_device_name(0), n=n, grad_dtype=a.grad_dtype, reps=a.reps, rounds=a.rounds)

    from UCF_VIT._hip.grad_scaler import HipGradScaler
    gs = HipGradScaler(init_scale=1.0, backoff_factor=1.0, growth_interval=10 ** 6).device_state()
    gen = torch.Generator(device=dev).manual_seed(1)
    p = torch.randn(n, generator=gen, device=dev)
    g = (torch.randn(n, generator=gen, device=dev) * 1e-2).to(gdt)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    sh = torch.empty(n, dtype=torch.bfloat16, device=dev)
    count = ops.grad_sqnorm_partials(n, gdt)
    ws = torch.zeros(count, dtype=torch.float64, device=dev)
    gc = torch.zeros(lib.GC_STATE_FLOATS, device=dev)
    gc[lib.GC_MAX_NORM] = 1.0

    # --- the reduction pass against the pass it replaces
    r = compare({"grad_nonfinite": lambda: ops.grad_nonfinite(g, gs),
                 "grad_sqnorm": lambda: ops.grad_sqnorm(g, ws),
                 "grad_sqnorm_scaled": lambda: ops.grad_sqnorm(g, ws, 1.0, gs),
                 "grad_clip_coef": lambda: ops.grad_clip_coef(ws, count, gc)}, a.reps, a.rounds)
    out.update({k + "_us": t for k, t in r.items()})
    out["read_GBps"] = {k: n * gb / r[k][0] * 1e-3 for k in ("grad_nonfinite", "grad_sqnorm", "grad_sqnorm_scaled")}
    out["sqnorm_over_nonfinite"] = r["grad_sqnorm"][0] / r["grad_nonfinite"][0]
    out["sqnorm_scaled_over_nonfinite"] = r["grad_sqnorm_scaled"][0] / r["grad_nonfinite"][0]
    out["partials"] = count
    out["norm"], out["coef"] = gc[lib.GC_NORM].item(), gc[lib.GC_COEF].item()

    # --- AdamW against AdamW with the coefficient (the moments drift over the repetitions: the traffic does not depend on the values)
    r = compare({"adamw": lambda: ops.adamw(p, g, m, v, sh, *hp, 7),
                 "adamw_clipped": lambda: ops.clipped_adamw(p, g, m, v, sh, None, *hp, 7, None, gc),
                 "adamw_scaled": lambda: ops.adamw_scaled(p, g, m, v, sh, *hp, gs),
                 "adamw_clipped_scaled": lambda: ops.clipped_adamw(p, g, m, v, sh, None, *hp, 7, None, gc, gs)}, a.reps, a.rounds)
    out.update({k + "_us": t for k, t in r.items()})
    out["adamw_GBps"] = n * (6 * 4 + gb + 2) / r["adamw"][0] * 1e-3             # p, m, v read and written, g read, shadow written
    out["clipped_over_adamw"] = r["adamw_clipped"][0] / r["adamw"][0]
    out["clipped_scaled_over_adamw_scaled"] = r["adamw_clipped_scaled"][0] / r["adamw_scaled"][0]

    # --- the torch statement on the same flat buffer: clip_grad_norm_ (a norm pass, then a read and a write of the gradient), then AdamW
    if gdt == torch.float32:
        holder = torch.nn.Parameter(p)              # clip_grad_norm_ wants parameters: p's storage, carrying the flat gradient
        holder.grad = g

        def torch_way():
            torch.nn.utils.clip_grad_norm_([holder], 1.0)
            ops.adamw(p, g, m, v, sh, *hp, 7)

        def hip_way():
            ops.grad_sqnorm(g, ws)
            ops.grad_clip_coef(ws, count, gc)
            ops.clipped_adamw(p, g, m, v, sh, None, *hp, 7, None, gc)

        r = compare({"torch_clip_then_adamw": torch_way, "sqnorm_coef_clipped_adamw": hip_way}, a.reps, a.rounds)
        out.update({k + "_us": t for k, t in r.items()})
        out["torch_over_hip"] = r["torch_clip_then_adamw"][0] / r["sqnorm_coef_clipped_adamw"][0]
    del p, g, m, v, sh

    # --- a full optimizer step on a ViT-L-sized store
    if not a.skip_step:
        from UCF_VIT._hip.params import ensure_store
        from UCF_VIT.simple.arch import VIT
        from UCF_VIT.utils.misc import configure_optimizer
        model = VIT(img_size=[224, 224], patch_size=16, in_chans=3, num_classes=1000, embed_dim=1024, depth=24, num_heads=16,
                    weight_init='skip').to(dev)
        if gdt == torch.bfloat16:
            model.set_compute_dtype(torch.bfloat16)      # the bf16 shadow is written by the same pass
        st = ensure_store(model)
        st.flat_g.copy_(torch.randn(st.total, generator=gen, device=dev) * 1e-2)
        for q, o in zip(st.params, st.offsets):
            q.grad = st.grad_view(q, o, q.numel())
        if gdt == torch.bfloat16:
            st.refresh_shadow()
        steps = {}
        for name, clip, scaled in (("step", None, False), ("step_clipped", 1.0, False), ("step_scaled", None, True),
                                   ("step_scaled_clipped", 1.0, True)):
            opt = configure_optimizer(model, 1e-3, 0.9, 0.95, 0.05, max_grad_norm=clip)
            sc = HipGradScaler(init_scale=1.0, backoff_factor=1.0, growth_interval=10 ** 6) if scaled else None

            def one(opt=opt, sc=sc):
                if sc is None:
                    opt.step()
                else:
                    sc.step(opt)
                    sc.update()
            steps[name] = one
        r = compare(steps, a.reps, a.rounds)
        out.update({k + "_us": t for k, t in r.items()})
        out["store_elements"] = st.total
        out["step_clipped_over_step"] = r["step_clipped"][0] / r["step"][0]
        out["step_scaled_clipped_over_step_scaled"] = r["step_scaled_clipped"][0] / r["step_scaled"][0]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
