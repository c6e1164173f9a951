#!/usr/bin/env python3
"""SAP segmentation head + DiceBLoss: this tree (HF.SapHeadFn + HF.DiceBCEFn, csrc/sap_head.hip) against the code they replaced, in one process.

  python tools/sap_head_bench.py head [iters=20] [warmup=5]
        the basic_ct/sap head: B = 2, 512 tokens, embed_dim 768, patch 4 in 3-D, 4 classes, bf16 compute.  Head forward + DiceBLoss +
        backward (gradients of the tokens, the neck, the header), HIP-event time per iteration, median over `iters` after `warmup`.
  python tools/sap_head_bench.py step [iters=20] [warmup=5]
        the whole forward + loss + backward of SAP at the shape of the train_sap_simple.py smoke run of tests/test_hip_models.py (64 x 64
        pseudo image, patch 8, embed_dim 96, depth 2, 3 classes, B = 4, fp32), images/s with either head + loss.

"parent" is the project's own former path, restated here in plain torch: tokens cast to fp32 and reshaped to the grid, nn.ConvTranspose (MIOpen),
nn.Conv 1x1, and DiceBLoss as a chain of torch element-wise ops.  The two variants share weights and inputs and alternate iteration by
iteration, so clock and box differences hit both alike.  One JSON line per measurement on stdout."""
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd"))
from UCF_VIT._hip import functional as HF  # noqa: E402
from UCF_VIT.utils.metrics import DiceBLoss  # noqa: E402

DEV = "cuda"


def parent_mask_head(x, neck, header, s, nd):
    B, _, D = x.shape
    x = x.float().reshape(B, *([s] * nd), D).movedim(-1, 1)
    return header(neck(x))


def parent_diceb_loss(inputs, targets, weight=0.5, smooth=1):
    pred = torch.flatten(torch.sigmoid(inputs.float())[:, 1:])
    true = torch.flatten(targets[:, 1:].float())
    inter = (pred * true).sum()
    dice_loss = 1 - (2. * inter + smooth) / (pred.sum() + true.sum() + smooth)
    bce = torch.nn.functional.binary_cross_entropy(pred, true, reduction='mean')
    return weight * bce + (1 - weight) * dice_loss


def _alternate(variants, iters, warmup):
    """variants: {name: callable}; -> {name: sorted per-iteration ms}"""
    times = {k: [] for k in variants}
    for it in range(warmup + iters):
        for name, fn in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[name].append(s.elapsed_time(e))
    return {k: sorted(v) for k, v in times.items()}


def head(iters, warmup):
    B, s, D, p, nd, C = 2, 8, 768, 4, 3, 4
    torch.manual_seed(0)
    neck = nn.ConvTranspose3d(D, 256, kernel_size=p, stride=p, bias=False).to(DEV)
    header = nn.Conv3d(256, C, 1).to(DEV)
    params = [neck.weight, header.weight, header.bias]
    x = torch.randn(B, s ** nd, D, device=DEV).bfloat16().requires_grad_(True)
    cls = torch.randint(0, C, (B, 1) + (s * p,) * nd, device=DEV)
    target = torch.zeros((B, C) + (s * p,) * nd, device=DEV).scatter_(1, cls, 1.0)
    loss_fn = DiceBLoss(num_class=C)

    def clear():
        x.grad = None
        for q in params:
            q.grad = None

    def new():
        clear()
        loss_fn(HF.SapHeadFn.apply(x, neck.weight, header.weight, header.bias, p, s, nd, torch.bfloat16), target).backward()

    def parent():
        clear()
        parent_diceb_loss(parent_mask_head(x, neck, header, s, nd), target).backward()

    t = _alternate({"new": new, "parent": parent}, iters, warmup)
    med = {k: v[len(v) // 2] for k, v in t.items()}
    print(json.dumps({"case": "basic_ct/sap head: B=2 S=512 D=768 p=4 3-D C=4 bf16, head fwd + DiceBLoss + bwd", "iters": iters, "warmup": warmup,
                      "new_ms": round(med["new"], 4), "parent_ms": round(med["parent"], 4), "ratio": round(med["parent"] / med["new"], 2),
                      "new_min_max_ms": [round(t["new"][0], 4), round(t["new"][-1], 4)],
                      "parent_min_max_ms": [round(t["parent"][0], 4), round(t["parent"][-1], 4)]}), flush=True)


def step(iters, warmup):
    from UCF_VIT.simple.arch import SAP
    from UCF_VIT.utils.fused_attn import FusedAttn
    B, C = 4, 3
    torch.manual_seed(0)
    m = SAP(img_size=[64, 64], patch_size=8, in_chans=3, num_classes=C, embed_dim=96, depth=2, num_heads=3, adaptive_patching=True, fixed_length=16,
            sqrt_len=4, twoD=True, use_adaptive_pos_emb=True, sqrt_len_method=True, class_token=False, weight_init='skip',
            FusedAttn_option=FusedAttn.HIP).to(DEV)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, 32, 32, generator=g).to(DEV)
    seq_ps = (torch.rand(B, 16, 3, generator=g) * 64).to(DEV)
    cls = torch.randint(0, C, (B, 1, 32, 32), generator=g).to(DEV)
    target = torch.zeros(B, C, 32, 32, device=DEV).scatter_(1, cls, 1.0)
    loss_fn = DiceBLoss(num_class=C)
    hip_head = m.mask_head

    def run(parent):
        for q in m.parameters():
            q.grad = None
        m.mask_head = (lambda t: parent_mask_head(t, m.neck, m.mask_header, 4, 2)) if parent else hip_head
        out = m(x, ["red", "green", "blue"], seq_ps)
        (parent_diceb_loss(out, target) if parent else loss_fn(out, target)).backward()
        HF.flush_wgrads()

    t = _alternate({"new": lambda: run(False), "parent": lambda: run(True)}, iters, warmup)
    med = {k: v[len(v) // 2] for k, v in t.items()}
    print(json.dumps({"case": "SAP forward + DiceBLoss + backward at the train_sap_simple.py smoke shape (B=4, 64x64, patch 8, D=96, depth 2, fp32)",
                      "new_ms": round(med["new"], 4), "parent_ms": round(med["parent"], 4),
                      "new_images_per_s": round(B / med["new"] * 1e3, 1), "parent_images_per_s": round(B / med["parent"] * 1e3, 1)}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "head"
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    if what == "head":
        head(iters, warmup)
    elif what == "step":
        step(iters, warmup)
    else:
        raise SystemExit(__doc__)
