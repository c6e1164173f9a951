#!/usr/bin/env python3
"""The DDPM kernels (csrc/diffusion.hip, the time-token kernels of csrc/elementwise.hip) against the bytes they must move, and the
DiffusionVIT training step and sampler at the reference's imagenet/diffusion shape (256 x 256, patch 16, 768 / 12 / 12, decoder
512 / 8 / 16, 1000 time steps) in bf16.

  python tools/diffusion_bench.py kernels [reps=50] [rounds=5]
  python tools/diffusion_bench.py step [batch=32] [reps=10] [rounds=5] [--tree DIR]
  python tools/diffusion_bench.py sample [batch=8] [steps=20] [--sampler ddim --steps S]
  python tools/diffusion_bench.py ema [n=304000000] [reps=20] [rounds=5]

Must-move bytes:
  q_sample         reads x0 and eps, writes x_t (fp32)                                           = 3 images
  ddpm_step        reads x, z and pred (bf16, half an image's bytes), writes x (fp32)            = 3.5 images
  ddim_step        the same (without z at eta = 0: 2.5 images)
  tokens_fwd       reads and writes the token matrix (bf16)                                      = 2 matrices (+ pos, L2-resident)
  time_tokens_fwd  the same + the [B, D] time rows
  tokens_bwd       reads dout, writes dpatches                                                   = 2 matrices (+ dpos)
  time_tokens_bwd  the same + the chunk partials (fp32 [N / 8][B][D], written and read) + dtemb
  tokens_bwd + sum the yardstick of the fused backward: tokens_bwd and a second pass over dout for the per-sample sums (ucfvit_colsum
                   per sample is not batched, so the second pass is timed as one more read of dout by tokens_bwd without dpatches)
Every case is timed `rounds` times, `reps` launches each, the cases of one comparison alternating inside a round: the figure is the median
with (min ... max); the bandwidth is must-move bytes over the median, as a fraction of the 6.29 TB/s a float4 copy reaches on an MI355X
(profiles/layer_scale.md).  HIP-event times after a warm-up of every case.  One JSON line per case on stdout.

step: forward + backward + HipAdamW step of the model wrapped in the same noising and loss, `--tree DIR` takes the package from another
checkout (the parent commit, whose DiffusionVIT runs its glue on torch: the noising is then torch's, the loss HF.patch_mse in both).

sample: the ancestral sampler over a `steps`-step schedule, or with `--sampler ddim --steps S` the strided sampler, S steps of the 1000-step
schedule (eta 0, no clamp).

ema: the optimiser pass over n fp32 parameters with fp32 gradients and the bf16 shadow written: adamw (reads p, g, m, v, writes p, m, v and
the shadow: 30 B per parameter), adamw_ema (+ the average read and written: 38 B), and adamw followed by ema.lerp_(p, rate) as a pass of its
own (+ p and the average read, the average written: 42 B)."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else ROOT
OPTS = ("--tree", "--sampler", "--steps")
ARGS = [a for i, a in enumerate(sys.argv[1:], 1) if a not in OPTS and sys.argv[i - 1] not in OPTS]
sys.path.insert(0, os.path.join(TREE, "ucf-vit_amd"))
from UCF_VIT._hip import functional as HF  # noqa: E402
from UCF_VIT._hip import ops  # noqa: E402

DEV = "cuda"
STREAM_TBPS = 6.29
MODEL_KW = dict(img_size=[256, 256], patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, class_token=False, linear_decoder=False,
                decoder_depth=8, decoder_embed_dim=512, decoder_num_heads=16, mlp_ratio_decoder=4.0, time_steps=1000, weight_init='skip')


def _timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def compare(cases, reps, rounds):
    """cases: name -> (fn, must-move bytes or None); alternating inside every round"""
    for fn, _ in cases.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(rounds):
        for k, (fn, _) in cases.items():
            ms[k].append(_timed(fn, reps))
    for k, (_, nbytes) in cases.items():
        med, lo, hi = statistics.median(ms[k]), min(ms[k]), max(ms[k])
        rec = dict(case=k, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
        if nbytes:
            rec.update(MB=round(nbytes / 1e6, 1), TBps=round(nbytes / med / 1e9, 3), of_copy=round(nbytes / med / 1e9 / STREAM_TBPS, 3))
        print(json.dumps(rec), flush=True)


def kernels(reps, rounds):
    g = torch.Generator(device=DEV).manual_seed(0)
    T = 1000
    sa, sb = torch.rand(T, device=DEV, generator=g), torch.rand(T, device=DEV, generator=g)
    for B in (32, 256):
        shape = (B, 3, 256, 256)
        x0, eps, z = (torch.randn(shape, device=DEV, generator=g) for _ in range(3))
        out = torch.empty_like(x0)
        t = torch.randint(0, T, (B,), device=DEV, generator=g)
        pred = torch.randn((B, 256, 768), device=DEV, generator=g).to(torch.bfloat16)
        img = x0.numel() * 4
        compare({f"q_sample B={B}": (lambda: ops.ddpm_q_sample(x0, eps, t, sa, sb, out=out), 3 * img),
                 f"ddpm_step B={B}": (lambda: ops.ddpm_step(x0, pred, z, 16, 1.01, 0.09, 0.14, out=out), 3 * img + pred.numel() * 2),
                 f"ddim_step B={B}": (lambda: ops.ddim_step(x0, pred, z, 16, 0.8, 0.6, 1.25, 1.0 / 0.6, 0.85, 0.5, 0.14, out=out),
                                      3 * img + pred.numel() * 2),
                 f"ddim_step clip B={B}": (lambda: ops.ddim_step(x0, pred, z, 16, 0.8, 0.6, 1.25, 1.0 / 0.6, 0.85, 0.5, 0.14, clip=1.0, out=out),
                                           3 * img + pred.numel() * 2),
                 f"ddim_step no z B={B}": (lambda: ops.ddim_step(x0, pred, None, 16, 0.8, 0.6, 1.25, 1.0 / 0.6, 0.85, 0.5, 0.0, out=out),
                                           2 * img + pred.numel() * 2)}, reps, rounds)
        del x0, eps, z, out, pred
    B, L, D = 256, 256, 768
    patches = torch.randn((B * L, D), device=DEV, generator=g).to(torch.bfloat16)
    pos = torch.randn((L, D), device=DEV, generator=g).to(torch.bfloat16)
    temb = torch.randn((B, D), device=DEV, generator=g).to(torch.bfloat16)
    dout = torch.randn((B, L, D), device=DEV, generator=g).to(torch.bfloat16)
    mat = B * L * D * 2
    ws = ops._l.load().ucfvit_time_tokens_bwd_workspace(B, L, D, 0)
    compare({"tokens_fwd": (lambda: ops.tokens_fwd(patches, None, pos, B, L, D), 2 * mat),
             "time_tokens_fwd": (lambda: ops.time_tokens_fwd(patches, None, pos, temb, B, L, D), 2 * mat + B * D * 2)}, reps, rounds)
    dpos = torch.empty((L, D), device=DEV)
    compare({"tokens_bwd": (lambda: ops.tokens_bwd(dout, B, L, D, False, True, dpos=dpos), 2 * mat),
             "time_tokens_bwd": (lambda: ops.time_tokens_bwd(dout, B, L, D, False, True, dpos=dpos), 2 * mat + 2 * ws + B * D * 4),
             "tokens_bwd + second read of dout": (lambda: (ops.tokens_bwd(dout, B, L, D, False, True, dpos=dpos),
                                                           ops.tokens_bwd(dout, B, L, D, False, True, dpos=dpos, want_patches=False)), 3 * mat)},
            reps, rounds)


def _model():
    from UCF_VIT.simple.arch import DiffusionVIT
    from UCF_VIT.utils.fused_attn import FusedAttn
    from UCF_VIT.utils.misc import configure_optimizer
    torch.manual_seed(0)
    m = DiffusionVIT(FusedAttn_option=FusedAttn.HIP, **MODEL_KW).to(DEV)
    m.set_compute_dtype(torch.bfloat16)
    return m, configure_optimizer(m, 1e-4, 0.9, 0.95, 1e-5)


def step(batch, reps, rounds):
    m, opt = _model()
    m.train()
    g = torch.Generator(device=DEV).manual_seed(1)
    x0 = torch.rand((batch, 3, 256, 256), device=DEV, generator=g)
    native = hasattr(HF, "q_sample")
    if native:
        from UCF_VIT.ddpm.ddpm import DDPM_Scheduler
        sched = DDPM_Scheduler(1000).to(DEV)
    else:                                                          # the parent commit: the reference script's torch noising
        beta = torch.linspace(1e-4, 0.02, 1000)
        alpha = torch.cumprod(1 - beta, dim=0)

    def one():
        t = torch.randint(0, 1000, (batch,), device=DEV, generator=g)
        e = torch.randn(x0.shape, device=DEV, generator=g)
        if native:
            x_t = sched.q_sample(x0, t, e)
        else:
            a = alpha[t.cpu()].view(batch, 1, 1, 1).to(DEV)
            x_t = torch.sqrt(a) * x0 + torch.sqrt(1 - a) * e
        loss = HF.patch_mse(m(x_t, t, ["red", "green", "blue"]), e, 16)
        loss.backward()
        opt.step()
        opt.zero_grad()

    for _ in range(3):
        one()
    torch.cuda.synchronize()
    ms = [_timed(one, reps) for _ in range(rounds)]
    med = statistics.median(ms)
    print(json.dumps(dict(case="train step", tree=os.path.basename(os.path.abspath(TREE)), native_glue=native, batch=batch, ms=round(med, 2),
                          ms_min=round(min(ms), 2), ms_max=round(max(ms), 2), images_per_s=round(batch / med * 1e3, 1),
                          peak_GB=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))), flush=True)


def sample(batch, steps, ddim_steps=None):
    from UCF_VIT.ddpm.ddpm import DDPM_Scheduler
    m, _ = _model()
    sched = DDPM_Scheduler(1000 if ddim_steps else steps).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(2)
    shape = (batch, 3, 256, 256)
    run = (lambda: sched.sample_ddim(m, shape, None, num_steps=ddim_steps, generator=g)) if ddim_steps else (lambda: sched.sample(m, shape, None, generator=g))
    run()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    run()
    e.record()
    torch.cuda.synchronize()
    ms = s.elapsed_time(e)
    if ddim_steps:
        print(json.dumps(dict(case="sample ddim", batch=batch, steps=ddim_steps, ms_per_step=round(ms / ddim_steps, 3),
                              s_per_image=round(ms / batch / 1e3, 4))), flush=True)
        return
    print(json.dumps(dict(case="sample", batch=batch, steps=steps, ms_per_step=round(ms / steps, 3),
                          s_per_image_at_1000_steps=round(ms / steps * 1000 / batch / 1e3, 3))), flush=True)


def ema(n, reps, rounds):
    g = torch.Generator(device=DEV).manual_seed(3)
    p, gr = torch.randn(n, device=DEV, generator=g), torch.randn(n, device=DEV, generator=g) * 1e-3
    m, v, avg = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), p.clone()
    sh = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    hp = (1e-4, 0.9, 0.95, 1e-8, 1e-5)
    rate = ops.ema_rate(0.9999)

    def pair():
        ops.adamw(p, gr, m, v, sh, *hp, 10)
        avg.lerp_(p, rate)

    compare({f"adamw n={n}": (lambda: ops.adamw(p, gr, m, v, sh, *hp, 10), 30 * n),
             f"adamw_ema n={n}": (lambda: ops.adamw_ema(p, gr, m, v, sh, avg, *hp, 10, rate), 38 * n),
             f"adamw + lerp_ n={n}": (pair, 42 * n)}, reps, rounds)


if __name__ == "__main__":
    mode = ARGS[0] if ARGS else "kernels"
    nums = [int(a) for a in ARGS[1:]]
    if mode == "kernels":
        kernels(*(nums + [50, 5][len(nums):]))
    elif mode == "step":
        step(*(nums + [32, 10, 5][len(nums):]))
    elif mode == "sample":
        sampler = sys.argv[sys.argv.index("--sampler") + 1] if "--sampler" in sys.argv else "ddpm"
        if sampler not in ("ddpm", "ddim"):
            raise SystemExit(__doc__)
        ddim_steps = (int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 50) if sampler == "ddim" else None
        sample(*(nums + [8, 20][len(nums):]), ddim_steps=ddim_steps)
    elif mode == "ema":
        ema(*(nums + [304_000_000, 20, 5][len(nums):]))
    else:
        raise SystemExit(__doc__)
