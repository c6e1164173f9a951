#!/usr/bin/env python3
"""The 2-D UNETR decoder on the HIP kernels (csrc/conv2d.hip) at the reference 2-D tile: 256 x 256, patch 16 (a 16 x 16 token grid), embed_dim 768,
feature_size 16.  One process, every shape warmed, HIP events around repeated launches.

  python tools/conv2d_bench.py layers [B=64] [reps=20]
        every distinct 3x3 layer of the decoder (Cin, Cout, extent): forward, data gradient and weight gradient on the HIP kernels and through
        torch.nn.functional.conv2d / aten.convolution_backward in bf16 channels_last ON THE SAME TENSORS, alternated launch group by launch
        group; with the bytes and MACs each pass must move (from the shapes): forward and data gradient read the input once and write the
        output once, 2 V (Cin + Cout) bytes, the weight gradient reads both, all three 9 V Cin Cout MACs.  `bound_us` is the larger of
        bytes / 8.0 TB/s (HBM3E, spec) and 2 MACs / 2.5 PF (bf16 MFMA, dense, spec); `of_bound` = bound_us / measured.
  python tools/conv2d_bench.py pointwise [B=64] [reps=20]
        the pointwise layers through the 1x1x1 kernels over the factorisation of the pixels (conv.pointwise_dims), at an extent the tiles
        divide (256 x 256) and at one they do not (250 x 250), with the padded-voxel ratio the factorisation leaves
  python tools/conv2d_bench.py step [B=64] [rounds=5] [steps=3] [depth=12]
        one train step (forward + Dice/CE + backward) of the 2-D UNETR with the HIP decoder against the same model with force_torch_decoder
        (torch's fp32 N C H W convolutions, the path such a model took before), alternated round by round
One JSON line per measurement on stdout."""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd"))
from UCF_VIT._hip import conv as HC  # noqa: E402
from UCF_VIT._hip import ops  # noqa: E402

DEV = "cuda"
HBM_BPS, MFMA_FLOPS = 8.0e12, 2.5e15
# (Cin, Cout, extent, where): the 3x3 layers of UNETR(img 256 x 256, patch 16, feature_size 16); the input image arrives zero-padded to 8 channels
LAYERS = [(8, 16, 256, "encoder1 conv1"), (16, 16, 256, "encoder1 / decoder2 conv2"), (32, 16, 256, "decoder2 conv1 (concatenation)"),
          (32, 32, 128, "encoder2 / decoder3 conv2"), (64, 32, 128, "decoder3 conv1"), (32, 32, 64, "encoder2 first block"),
          (64, 64, 64, "encoder3 / decoder4 conv2"), (128, 64, 64, "decoder4 conv1"), (128, 128, 32, "decoder5 conv2"), (256, 128, 32, "decoder5 conv1")]


def _timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3          # us


def _ab(fns, reps, rounds=3):
    """the median over `rounds` of each function's time, the functions alternated round by round (all warmed first)"""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            t[k].append(_timed(f, reps))
    return {k: sorted(v)[len(v) // 2] for k, v in t.items()}


def layers(B, reps):
    g = torch.Generator(device=DEV).manual_seed(0)
    for cin, cout, n, where in LAYERS:
        V = B * n * n
        x = torch.randn((B, n, n, cin), generator=g, device=DEV).bfloat16()
        dy = torch.randn((B, n, n, cout), generator=g, device=DEV).bfloat16()
        w = (torch.randn((cout, cin, 3, 3), generator=g, device=DEV) * (2.0 / (9 * cin)) ** 0.5)
        wp, wd = HC.pack_conv2d_weight(w), (HC.pack_conv2d_weight_dgrad(w) if cin % 16 == 0 else None)
        xt, dyt = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)            # the same memory as channels_last N C H W tensors
        wt = w.bfloat16().contiguous(memory_format=torch.channels_last)
        assert xt.is_contiguous(memory_format=torch.channels_last)
        bwd = lambda mask: torch.ops.aten.convolution_backward(dyt, xt, wt, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, mask)
        fns = {"fwd_hip": lambda: ops.conv2d_fwd(x, wp, cout), "fwd_torch": lambda: F.conv2d(xt, wt, padding=1),
               "wgrad_hip": lambda: ops.conv2d_wgrad(x, dy), "wgrad_torch": lambda: bwd([False, True, False])}
        if wd is not None:
            fns["dgrad_hip"] = lambda: ops.conv2d_fwd(dy, wd, cin)
            fns["dgrad_torch"] = lambda: bwd([True, False, False])
        t = _ab(fns, reps)
        nbytes, macs = 2 * V * (cin + cout), 9 * V * cin * cout
        bound = max(nbytes / HBM_BPS, 2 * macs / MFMA_FLOPS) * 1e6
        out = {"layer": where, "B": B, "extent": n, "cin": cin, "cout": cout, "bytes": nbytes, "macs": macs, "bound_us": round(bound, 1),
               "bound_by": "hbm" if nbytes / HBM_BPS > 2 * macs / MFMA_FLOPS else "mfma"}
        for k, v in t.items():
            out[k + "_us"] = round(v, 1)
        for p in ("fwd", "dgrad", "wgrad"):
            if p + "_hip" in t:
                out[p + "_of_bound"] = round(bound / t[p + "_hip"], 3)
                out[p + "_TFLOPs"] = round(2 * macs / t[p + "_hip"] / 1e6, 1)
                out[p + "_GBps"] = round(nbytes / t[p + "_hip"] / 1e3, 1)
                out[p + "_torch_over_hip"] = round(t[p + "_torch"] / t[p + "_hip"], 2)
        print(json.dumps(out), flush=True)
        del x, dy, xt, dyt


def pointwise(B, reps):
    g = torch.Generator(device=DEV).manual_seed(1)
    for n in (256, 250):
        for cin, cout, what in ((32, 16, "residual 1x1 projection 32 -> 16"), (16, 64, "transposed convolution's mixing 16 -> 4 x 16")):
            x = torch.randn((B, n, n, cin), generator=g, device=DEV).bfloat16()
            dy = torch.randn((B, n, n, cout), generator=g, device=DEV).bfloat16()
            w2 = torch.randn((cout, cin), generator=g, device=DEV) * 0.1
            t = _ab({"fwd": lambda: HC._pointwise_fwd(x, w2, None, cout), "wgrad": lambda: HC._pointwise_wgrad(x, dy)}, reps)
            V = B * n * n
            print(json.dumps({"pointwise": what, "B": B, "extent": n, "dims_fwd": HC.pointwise_dims(n * n), "waste_fwd": round(HC.pointwise_waste(n * n), 3),
                              "dims_wgrad": HC.pointwise_dims(n * n, (2, 4, 32)), "waste_wgrad": round(HC.pointwise_waste(n * n, (2, 4, 32)), 3),
                              "fwd_us": round(t["fwd"], 1), "wgrad_us": round(t["wgrad"], 1), "fwd_GBps": round(2 * V * (cin + cout) / t["fwd"] / 1e3, 1),
                              "wgrad_GBps": round(2 * V * (cin + cout) / t["wgrad"] / 1e3, 1)}), flush=True)


def step(B, rounds, steps, depth):
    from UCF_VIT._hip import functional as HF
    from UCF_VIT.simple.arch import UNETR
    from UCF_VIT.utils.fused_attn import FusedAttn
    torch.manual_seed(0)
    m = UNETR(img_size=[256, 256], patch_size=16, in_chans=1, embed_dim=768, depth=depth, num_heads=12, mlp_ratio=4, twoD=True, num_classes=4,
              class_token=False, linear_decoder=False, feature_size=16, skip_connection=True, FusedAttn_option=FusedAttn.HIP).to(DEV)
    m.set_compute_dtype(torch.bfloat16)
    assert m.hip_decoder()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 1, 256, 256, generator=g).to(DEV)
    lab = torch.randint(0, 4, (B, 256, 256), generator=g).to(DEV)

    def one(mode):
        m.allow_torch_decoder = m.force_torch_decoder = mode == "torch"
        for p in m.parameters():
            p.grad = None
        loss = HF.dice_ce(m(x, None), lab)
        loss.backward()
        HF.flush_wgrads()
        return loss

    modes = ("hip", "torch")
    losses = {}
    for mode in modes:                       # warm-up: code objects, MIOpen algorithm choice, allocator
        for _ in range(2):
            losses[mode] = one(mode).item()
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
    med = {}
    for mode in modes:
        t = sorted(times[mode])
        med[mode] = t[len(t) // 2]
        print(json.dumps({"step": f"unetr 2-D 256x256 patch 16 embed 768 fs 16 depth {depth} B={B}", "decoder": mode, "loss": round(losses[mode], 5),
                          "median_ms": round(med[mode], 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3), "images_per_s": round(B * 1e3 / med[mode], 1),
                          "rounds_ms": [round(v, 3) for v in times[mode]]}), flush=True)
    print(json.dumps({"step_torch_over_hip": round(med["torch"] / med["hip"], 3)}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "layers"
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    if what == "layers":
        layers(arg(2, 64), arg(3, 20))
    elif what == "pointwise":
        pointwise(arg(2, 64), arg(3, 20))
    elif what == "step":
        step(arg(2, 64), arg(3, 5), arg(4, 3), arg(5, 12))
    else:
        raise SystemExit(__doc__)
