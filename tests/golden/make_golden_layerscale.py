"""Generates the LayerScale fixtures from the REFERENCE implementation (run only in the build container, on the CPU):

    cd tests/golden && python make_golden_layerscale.py

Like make_golden.py it imports the reference with the stand-ins of _ref_standins.py (whose LayerScale is timm's definition, x * gamma)
and records data only: op_block_layerscale.npz (a Block with init_values, gammas of order 1 that differ per column) and
model_vit_layerscale.npz (the small VIT of model_vit_small.npz with init_values=0.1)."""
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
from UCF_VIT.simple.building_blocks import Block  # noqa: E402
from UCF_VIT.utils.fused_attn import FusedAttn  # noqa: E402

torch.set_num_threads(4)
torch.manual_seed(0)


def npz(name, **arrs):
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    np.savez_compressed(os.path.join(HERE, name), **out)
    print(name, {k: v.shape for k, v in out.items()})


# ------------------------------------------------------------------ the Block
B, N, D, H = 2, 17, 64, 2
SEED = 61
blk = Block(D, H, fused_attn=FusedAttn.NONE, qkv_bias=True, init_values=0.5, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
sd = det_state_dict(blk, SEED)
sd["ls1.gamma"] = det_tensor((D,), SEED * 1000 + 901, 0.3, 0.5)       # of order 1, different per column
sd["ls2.gamma"] = det_tensor((D,), SEED * 1000 + 902, 0.3, 0.5)
blk.load_state_dict(sd)
assert {"ls1.gamma", "ls2.gamma"} <= set(blk.state_dict())
x = det_tensor((B, N, D), 62).requires_grad_(True)
y = blk(x)
gy = det_tensor(y.shape, SEED + 50)
y.backward(gy)
rec = {"x": x, "y": y, "gy": gy, "gx": x.grad}
rec.update({"w." + k: v for k, v in blk.state_dict().items()})
rec.update({"g." + k: p.grad for k, p in blk.named_parameters()})
npz("op_block_layerscale.npz", **rec)

# ------------------------------------------------------------------ the model
vit_kw = dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=D, depth=2, num_heads=H, init_values=0.1,
              FusedAttn_option=FusedAttn.NONE)
model = VIT(**vit_kw)
model.load_state_dict(det_state_dict(model, 63))
model.train()
xm = det_tensor((2, 3, 32, 32), 64)
labels = torch.tensor([1, 3])
logits = model(xm, ["red", "green", "blue"])
loss = torch.nn.CrossEntropyLoss()(logits, labels)
loss.backward()
rec = dict(x=xm, logits=logits, loss=loss, labels=labels)
for k, p in model.named_parameters():
    rec["g." + k] = p.grad if p.grad is not None else torch.zeros_like(p)
assert any(k.endswith("ls1.gamma") for k, _ in model.named_parameters())
npz("model_vit_layerscale.npz", **rec)
print("done")
