"""Generates the qk_norm fixtures from the REFERENCE implementation (run only in the build container, on the CPU):

    cd tests/golden && python make_golden_qknorm.py

Like make_golden_layerscale.py it imports the reference with the stand-ins of _ref_standins.py and records data only:
op_attn_qknorm.npz (a bare Attention with qk_norm, eps 1e-5), op_block_qknorm.npz (a Block with qk_norm and init_values, eps 1e-6; its
gradients for a full output gradient and for one that is zero outside the class row) and
model_vit_qknorm.npz (the small VIT of model_vit_small.npz with qk_norm=True).  The weights and biases of q_norm / k_norm come from
det_tensor: of order 1, different per element and between q and k (the default 1, 0 would hide a swapped or missing parameter)."""
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_standins  # noqa: E402

_ref_standins.install()
from det_weights import det_state_dict, det_tensor  # noqa: E402

from UCF_VIT.simple.arch import VIT  # noqa: E402  (reference)
from UCF_VIT.simple.building_blocks import Attention, Block  # noqa: E402
from UCF_VIT.utils.fused_attn import FusedAttn  # noqa: E402

torch.set_num_threads(4)
torch.manual_seed(0)


def npz(name, **arrs):
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    np.savez_compressed(os.path.join(HERE, name), **out)
    print(name, {k: v.shape for k, v in out.items()})


def qk_params(sd, seed, dh):
    """q_norm / k_norm weights around 1 and biases around 0, all different"""
    n = 0
    for k in sorted(sd):
        if ".q_norm." in "." + k or ".k_norm." in "." + k:
            n += 1
            sd[k] = det_tensor((dh,), seed * 1000 + 700 + n, 0.3, 0.9 if k.endswith("weight") else 0.1)
    assert n and n % 4 == 0
    return sd


def run(mod, x, seed):
    y = mod(x)
    gy = det_tensor(y.shape, seed)
    y.backward(gy)
    rec = {"x": x, "y": y, "gy": gy, "gx": x.grad}
    rec.update({"w." + k: v for k, v in mod.state_dict().items()})
    rec.update({"g." + k: p.grad for k, p in mod.named_parameters()})
    return rec


B, N, D, H = 2, 17, 64, 2
# ------------------------------------------------------------------ the bare Attention (nn.LayerNorm default eps 1e-5)
att = Attention(D, fused_attn=FusedAttn.NONE, num_heads=H, qkv_bias=True, qk_norm=True)
att.load_state_dict(qk_params(det_state_dict(att, 71), 71, D // H))
assert att.q_norm.eps == 1e-5 and {"q_norm.weight", "q_norm.bias", "k_norm.weight", "k_norm.bias"} <= set(att.state_dict())
npz("op_attn_qknorm.npz", **run(att, det_tensor((B, N, D), 72).requires_grad_(True), 73))

# ------------------------------------------------------------------ the Block
blk = Block(D, H, fused_attn=FusedAttn.NONE, qkv_bias=True, qk_norm=True, init_values=0.5, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
sd = qk_params(det_state_dict(blk, 74), 74, D // H)
sd["ls1.gamma"] = det_tensor((D,), 74 * 1000 + 901, 0.3, 0.5)
sd["ls2.gamma"] = det_tensor((D,), 74 * 1000 + 902, 0.3, 0.5)
blk.load_state_dict(sd)
assert blk.attn.q_norm.eps == 1e-6
rec = run(blk, det_tensor((B, N, D), 75).requires_grad_(True), 76)
# the same Block with an output gradient that is zero outside the class row (token 0): what a model whose head reads only the class token
# sends back through its last Block
blk.zero_grad()
xc = rec["x"].detach().clone().requires_grad_(True)
gyc = torch.zeros_like(rec["gy"])
gyc[:, 0] = rec["gy"][:, 0]
blk(xc).backward(gyc)
rec["gx_cls"] = xc.grad
rec.update({"gcls." + k: p.grad for k, p in blk.named_parameters()})
npz("op_block_qknorm.npz", **rec)

# ------------------------------------------------------------------ the model
vit_kw = dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=D, depth=2, num_heads=H, qk_norm=True,
              FusedAttn_option=FusedAttn.NONE)
model = VIT(**vit_kw)
model.load_state_dict(qk_params(det_state_dict(model, 77), 77, D // H))
model.train()
xm = det_tensor((2, 3, 32, 32), 78)
labels = torch.tensor([1, 3])
logits = model(xm, ["red", "green", "blue"])
loss = torch.nn.CrossEntropyLoss()(logits, labels)
loss.backward()
rec = dict(x=xm, logits=logits, loss=loss, labels=labels)
rec.update({"w." + k: v for k, v in model.state_dict().items() if "q_norm" in k or "k_norm" in k})
for k, p in model.named_parameters():
    rec["g." + k] = p.grad if p.grad is not None else torch.zeros_like(p)
assert any(k.endswith("attn.q_norm.weight") for k, _ in model.named_parameters())
npz("model_vit_qknorm.npz", **rec)
print("done")
