"""Generates the diffusion fixtures from the REFERENCE implementation (run only in the build container, on the CPU):

    cd tests/golden && python make_golden_diffusion.py

Like make_golden_qknorm.py it imports the reference with the stand-ins of _ref_standins.py and records data only:
ddpm_schedule.npz (beta and alpha of the reference DDPM_Scheduler(1000)), model_diffusion_small.npz (DiffusionVIT, 32x32, patch 8, 3
channels, D 64, depth 2, 2 heads, decoder 1 x 32 x 1 head, 10 time steps, class_token=False as the reference's training script builds it)
and model_diffusion_3d_linear.npz (twoD=False, 16x8x8 so that the axes differ, patch 4, 1 channel, depth 1, D 96 and 3
heads because the 3-D sincos table needs D % 3 == 0, linear_decoder=True; sized so that the file stays near the other model fixtures): the weights that do not follow from det_state_dict and the
seed, the state_dict's key list, input, t = [1, 7], the output in eval(), and the parameter and input gradients for a det_tensor output gradient.

The reference's forward_features calls self._pos_embed(x) without seq_ps (a TypeError); the generator binds seq_ps=None on the instance,
so every number below is the reference's own arithmetic.  The time-MLP weights and decoder_pos_embed come from det_tensor, of order 1
and different per element: the default values (weights of 0.05, a sincos table that a test could rebuild) would hide a missing add."""
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

from UCF_VIT.simple.arch import DiffusionVIT  # noqa: E402  (reference)
from UCF_VIT.ddpm.ddpm import DDPM_Scheduler  # noqa: E402
from UCF_VIT.utils.fused_attn import FusedAttn  # noqa: E402

torch.set_num_threads(4)
torch.manual_seed(0)


def npz(name, **arrs):
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    np.savez_compressed(os.path.join(HERE, name), **out)
    print(name, {k: v.shape for k, v in out.items()})


sch = DDPM_Scheduler(1000)
npz("ddpm_schedule.npz", beta=sch.beta, alpha=sch.alpha)


def record(name, kw, x, seed):
    # weight_init='skip': VIT.__init__ would call the subclass's init_weights before decoder_pos_embed exists (as for the MAE fixtures);
    # DiffusionVIT.__init__ calls it again at its end
    model = DiffusionVIT(FusedAttn_option=FusedAttn.NONE, weight_init='skip', **kw)
    sd = det_state_dict(model, seed)
    n = 0
    for k in sorted(sd):
        if k.startswith("timeEmbeddingMap."):
            n += 1
            sd[k] = det_tensor(sd[k].shape, seed * 1000 + 800 + n, 0.3 if k.endswith("weight") else 0.5)
    assert n == 4
    if "decoder_pos_embed" in sd:
        sd["decoder_pos_embed"] = det_tensor(sd["decoder_pos_embed"].shape, seed * 1000 + 900, 0.5)
    model.load_state_dict(sd)
    model._pos_embed = partial(model._pos_embed, seq_ps=None)      # the call the reference's forward_features means to make
    model.eval()
    x = x.requires_grad_(True)
    t = torch.tensor([1, 7])
    y = model(x, t, ["v"] * kw["in_chans"])
    gy = det_tensor(y.shape, seed + 1)
    y.backward(gy)
    rec = dict(x=x, t=t, y=y, gy=gy, gx=x.grad, seed=np.int64(seed), sd_keys=np.array(list(model.state_dict()), dtype=np.str_))
    # the weights that are not det_state_dict(model, seed): the tests rebuild the rest from the seed, as for the other model fixtures
    rec.update({"w." + k: v for k, v in model.state_dict().items() if k.startswith("timeEmbeddingMap.") or k == "decoder_pos_embed"})
    for k, p in model.named_parameters():
        rec["g." + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    npz(name, **rec)


record("model_diffusion_small.npz",
       dict(img_size=[32, 32], patch_size=8, in_chans=3, embed_dim=64, depth=2, num_heads=2, class_token=False, linear_decoder=False,
            decoder_depth=1, decoder_embed_dim=32, decoder_num_heads=1, mlp_ratio_decoder=4.0, time_steps=10),
       det_tensor((2, 3, 32, 32), 91), 92)
record("model_diffusion_3d_linear.npz",
       dict(img_size=[16, 8, 8], patch_size=4, in_chans=1, embed_dim=96, depth=1, num_heads=3, class_token=False, linear_decoder=True,
            decoder_depth=1, decoder_embed_dim=32, decoder_num_heads=1, mlp_ratio_decoder=4.0, time_steps=10, twoD=False),
       det_tensor((2, 1, 16, 8, 8), 94), 95)
print("done")
