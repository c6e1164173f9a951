#!/usr/bin/env python3
"""UNETR with the resampling decoder (the reference's basic_ct/unetr geometry: 64^3 tile, patch 4, adaptive patching, 9^3 tokens,
embed_dim 768, feature_size 16, depth 12, B = 2): the align-corners trilinear resampling kernels of csrc/resample.hip and the whole train step.

  python tools/resample_bench.py kernels [reps=20]     resample forward / backward launches, HIP-event time and GB/s from shapes:
                                                        the decoder's 72^3 -> 64^3 x 16 (+ the 16-channel skip) and 144^3 -> 128^3 x 32
  python tools/resample_bench.py step [rounds=5] [steps=5] [modes=hip,torch]
                                                        train step (forward + Dice/CE + backward) with the decoder on the HIP kernels
                                                        against the same model with force_torch_decoder, alternated round by round
Run the kernel-trace profile (rocprofv3 --kernel-trace --stats) on `step 1 3 hip` and on `kernels 5`, each in a run of its own.
One JSON line per measurement on stdout."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd"))
from UCF_VIT._hip import ops  # noqa: E402

DEV = "cuda"
CASES = [  # B, input extent, output extent, C, skip channels, label
    (2, (72, 72, 72), (64, 64, 64), 16, 16, "decoder2 (reference geometry): 16 ch resampled into the 32-ch concatenation"),
    (2, (144, 144, 144), (128, 128, 128), 32, 0, "larger: 144^3 -> 128^3 x 32"),
]


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


def kernels(reps):
    g = torch.Generator(device=DEV).manual_seed(0)
    for B, src, dst, C, Cs, label in CASES:
        vi, vo = B * src[0] * src[1] * src[2], B * dst[0] * dst[1] * dst[2]
        x = torch.randn((B, *src, C), generator=g, device=DEV).bfloat16()
        skip = torch.randn((B, *dst, Cs), generator=g, device=DEV).bfloat16() if Cs else None
        cat = torch.empty((B, *dst, C + Cs), dtype=torch.bfloat16, device=DEV)
        dcat = torch.randn((B, *dst, C + Cs), generator=g, device=DEV).bfloat16()
        t_f = _timed(lambda: ops.resample_trilinear(x, dst, out=cat[..., :C], skip=skip), reps)
        t_b = _timed(lambda: ops.resample_trilinear_bwd(dcat[..., :C], src), reps)
        # algorithmic bytes: forward reads x once and (skip) the skip map, writes the rows of the concatenation; backward reads the C
        # channels of dy once and writes dx once (re-reads of neighbouring taps are cache hits)
        b_f = 2 * (vi * C + vo * Cs + vo * (C + Cs))
        b_b = 2 * (vo * C + vi * C)
        print(json.dumps({"case": label, "B": B, "src": src, "dst": dst, "C": C, "Cs": Cs, "fwd_ms": round(t_f, 4), "bwd_ms": round(t_b, 4),
                          "fwd_GBps": round(b_f / t_f / 1e6, 1), "bwd_GBps": round(b_b / t_b / 1e6, 1), "fwd_bytes": b_f, "bwd_bytes": b_b}),
              flush=True)


def _model():
    from UCF_VIT.simple.arch import UNETR
    from UCF_VIT.utils.fused_attn import FusedAttn
    torch.manual_seed(0)
    m = UNETR(img_size=[64, 64, 64], patch_size=4, in_chans=1, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, twoD=False,
              default_vars=["ct_res1"], single_channel=True, adaptive_patching=True, fixed_length=729, use_adaptive_pos_emb=True, num_classes=4,
              class_token=False, linear_decoder=False, feature_size=16, skip_connection=True, sqrt_len=9, sqrt_len_method=True,
              FusedAttn_option=FusedAttn.HIP).to(DEV)
    m.set_compute_dtype(torch.bfloat16)
    return m


def step(rounds, steps, modes):
    from UCF_VIT._hip import functional as HF
    m = _model()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 1, 64, 64, 64, generator=g).to(DEV)
    x_seq = torch.rand(2, 1, 36, 36, 36, generator=g).to(DEV)
    seq_ps = (torch.rand(2, 729, 4, generator=g) * 64).to(DEV)
    lab = torch.randint(0, 4, (2, 64, 64, 64), generator=g).to(DEV)

    def one(mode):
        m.allow_torch_decoder = m.force_torch_decoder = mode == "torch"
        for p in m.parameters():
            p.grad = None
        loss = HF.dice_ce(m(x, ["ct_res1"], seq_ps, x_seq), lab)
        loss.backward()
        HF.flush_wgrads()
        return loss

    for mode in modes:                       # warm-up: code objects, MIOpen algorithm choice, allocator
        for _ in range(2):
            one(mode)
    torch.cuda.synchronize()
    times = {mode: [] for mode in modes}
    for _ in range(rounds):
        for mode in modes:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(steps):
                one(mode)
            e.record()
            torch.cuda.synchronize()
            times[mode].append(s.elapsed_time(e) / steps)
    for mode in modes:
        t = sorted(times[mode])
        print(json.dumps({"step": "unetr basic_ct geometry B=2 depth 12", "decoder": mode, "median_ms": round(t[len(t) // 2], 3),
                          "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3), "rounds_ms": [round(v, 3) for v in times[mode]]}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    if what == "kernels":
        kernels(int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    elif what == "step":
        step(int(sys.argv[2]) if len(sys.argv) > 2 else 5, int(sys.argv[3]) if len(sys.argv) > 3 else 5,
             (sys.argv[4] if len(sys.argv) > 4 else "hip,torch").split(","))
    else:
        raise SystemExit(__doc__)
