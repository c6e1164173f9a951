"""Generates tests/golden/model_sap_3d.npz from the REFERENCE implementation; run only in the build container:

    cd tests/golden && python make_golden_sap3d.py

Same recipe as make_golden_adaptive.py (reference imported with the _ref_standins stand-ins, deterministic PCG64 weights and inputs): the
reference's SAP in 3-D, built as train_sap_simple.py builds it for adaptively patched input, is fed the pseudo volume x [B, 1, 8, 8, 8] and
seq_ps [B, 8, 4]; its output map, the value of the reference's OWN DiceBLoss on deterministic targets and every parameter gradient are
recorded.  embed_dim is 96 with 3 heads (as model_vit_sqrtlen_3d.npz): the reference's SAP fills its 3-D sincos table in the constructor
even with weight_init='skip', and that table needs embed_dim % 6 == 0, so the reference cannot build this model at 64.  Half of the voxels
carry hard one-hot targets, the other half soft targets in [0, 1] (DiceBLoss takes either).  The neck's gradient alone is 6 MiB, so it is
stored as a strided sample plus its norm and one projection.  Data only; no reference source text is stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_standins  # noqa: E402

_ref_standins.install()
# the reference's utils/metrics.py imports torchvision at module level and never uses it in DiceBLoss: an empty stand-in, as for timm / monai
import types  # noqa: E402
for _n in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional"):
    sys.modules.setdefault(_n, types.ModuleType(_n))
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
from det_weights import det_state_dict, det_tensor, proj_vector  # noqa: E402

from UCF_VIT.simple.arch import SAP  # noqa: E402  (reference)
from UCF_VIT.utils.fused_attn import FusedAttn  # noqa: E402
from UCF_VIT.utils.metrics import DiceBLoss  # noqa: E402  (reference)

torch.set_num_threads(4)
torch.manual_seed(0)

B, S, NC = 2, 8, 4
BIG, STRIDE = 1 << 18, 11
KW = dict(img_size=[16, 16, 16], patch_size=4, in_chans=1, num_classes=NC, embed_dim=96, depth=1, num_heads=3, adaptive_patching=True,
          fixed_length=S, sqrt_len=2, twoD=False, use_adaptive_pos_emb=True, sqrt_len_method=True, class_token=False, weight_init='skip',
          FusedAttn_option=FusedAttn.NONE)


def seq_ps_of(seed):
    """(x, y, z, size) of each token as the octree patcher emits them: integer voxel positions and power-of-two sizes"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pos = rng.integers(0, 16, (B, S, 3)).astype(np.float32)
    size = (2 ** rng.integers(1, 4, (B, S, 1))).astype(np.float32)
    return torch.from_numpy(np.concatenate([pos, size], axis=2))


def targets_of(shape, seed):
    """voxels with an even linear index: one-hot over the classes; the others: independent uniform values in [0, 1] per class"""
    rng = np.random.Generator(np.random.PCG64(seed))
    b, nc = shape[0], shape[1]
    vox = int(np.prod(shape[2:]))
    cls = rng.integers(0, nc, (b, vox))
    hard = np.zeros((b, nc, vox), dtype=np.float32)
    np.put_along_axis(hard, cls[:, None, :], 1.0, axis=1)
    soft = rng.random((b, nc, vox)).astype(np.float32)
    even = (np.arange(vox) % 2 == 0)[None, None, :]
    return torch.from_numpy(np.where(even, hard, soft).reshape(shape))


model = SAP(**KW)
model.load_state_dict(det_state_dict(model, 81, keep=()))
model.train()
x, seq_ps = det_tensor((B, 1, 8, 8, 8), 80), seq_ps_of(82)
out = model(x, ["ct"], seq_ps)
targets = targets_of(out.shape, 83)
loss = DiceBLoss(num_class=NC)(out, targets)
loss.backward()
rec = dict(x=x, seq_ps=seq_ps, targets=targets, out=out, loss=loss)
for i, (k, p) in enumerate(model.named_parameters()):
    g = p.grad if p.grad is not None else torch.zeros_like(p)
    if g.numel() <= BIG:
        rec["g." + k] = g
    else:
        # the neck's gradient (96 x 256 x 4^3 floats = 6 MiB) is over the size limit of a committed file: every STRIDE-th element (11 is
        # coprime to every extent, so every d, k and offset index occurs), the 2-norm and the projection on a fixed random direction
        rec["gs." + k] = g.reshape(-1)[::STRIDE].clone()
        rec["gn." + k] = g.double().norm()
        rec["gp." + k] = (g.double() * proj_vector(g.shape, i).double()).sum()
out_np = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in rec.items()}
np.savez_compressed(os.path.join(HERE, "model_sap_3d.npz"), **out_np)
print("model_sap_3d.npz", {k: v.shape for k, v in out_np.items() if not k.startswith("g.")}, loss.item())
