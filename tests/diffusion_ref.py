"""float64 restatements for the tests/test_diffusion_*.py files: the four DDPM kernels of include/ucfvit_hip.h in numpy, and the
DiffusionVIT forward pass in torch float64 (autograd gives its backward).  Written from the header's contracts and the reference's
formulas, not from the kernels.  The dropout mask is tests/dropout_ref.py's."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import dropout_ref as DR


# ------------------------------------------------------------------------------------------------ kernels (numpy, float64)
def q_sample(x0, eps, t, sqrt_ab, sqrt_1mab):
    """-> (a x0, b eps) in float64 with the fp32 table entries of the clamped step, per sample; their sum is the result"""
    T = len(sqrt_ab)
    tc = np.clip(np.asarray(t, dtype=np.int64), 0, T - 1)
    shp = (-1,) + (1,) * (x0.ndim - 1)
    a = np.asarray(sqrt_ab, dtype=np.float32)[tc].astype(np.float64).reshape(shp)
    b = np.asarray(sqrt_1mab, dtype=np.float32)[tc].astype(np.float64).reshape(shp)
    return a * x0.astype(np.float64), b * eps.astype(np.float64)


def time_tokens_terms(patches, cls, pos, temb):
    """-> (a, pos, temb) broadcast to [B, N, D] in float64: the three terms of (a + pos) + temb; a = cat(cls, patches)"""
    B, L, D = patches.shape
    a = patches.astype(np.float64)
    if cls is not None:
        a = np.concatenate([np.broadcast_to(cls.astype(np.float64).reshape(1, 1, D), (B, 1, D)), a], axis=1)
    N = a.shape[1]
    p = np.zeros((B, N, D)) if pos is None else np.broadcast_to(pos.astype(np.float64).reshape(1, N, D), (B, N, D))
    return a, p, np.broadcast_to(temb.astype(np.float64).reshape(B, 1, D), (B, N, D))


def time_tokens_bwd(dout, pre):
    """-> (dpatches, dpos, dcls, dtemb) in float64"""
    d = dout.astype(np.float64)
    return d[:, pre:], d.sum(0), d[:, 0].sum(0) if pre else None, d.sum(1)


def relu_dropout(x, p, seed):
    """-> (keep mask bool [rows, D] (all True at p == 0), f as the kernel forms it, y = f m relu(x) in float64)"""
    rows, D = x.shape
    if p == 0.0:
        keep, f = np.ones((rows, D), dtype=bool), 1.0
    else:
        keep, f = DR.keep_mask(seed, rows, D, p), DR.inv_keep(p)
    x64 = x.astype(np.float64)
    on = keep & (x64 > 0)
    return keep, f, np.where(on, f * np.where(on, x64, 0.0), 0.0)


def relu_dropout_bwd(x, dy, p, seed):
    keep, f, _ = relu_dropout(x, p, seed)
    on = keep & (x.astype(np.float64) > 0)
    return np.where(on, f * np.where(on, dy.astype(np.float64), 0.0), 0.0)


def unpatchify(pred, C, dims, p):
    """the reference's unpatchify (utils/misc.py): pred [B, L, p^nd C] -> [B, C, *dims]"""
    B = pred.shape[0]
    if len(dims) == 2:
        h, w = dims[0] // p, dims[1] // p
        return np.einsum("nhwpqc->nchpwq", pred.reshape(B, h, w, p, p, C)).reshape(B, C, *dims)
    h, w, d = dims[0] // p, dims[1] // p, dims[2] // p
    return np.einsum("nhwdpqrc->nchpwqdr", pred.reshape(B, h, w, d, p, p, p, C)).reshape(B, C, *dims)


def ddpm_step(x, pred, z, p, c1, c2, sigma):
    """-> (result, bound terms |c1| (|x| + |c2 e|) + |sigma z|) in float64; c1, c2, sigma are the fp32 values the kernel receives"""
    C, dims = x.shape[1], x.shape[2:]
    e = unpatchify(pred.astype(np.float64), C, dims, p)
    c1, c2, sigma = (float(np.float32(v)) for v in (c1, c2, sigma))
    x64 = x.astype(np.float64)
    noise = sigma * z.astype(np.float64) if z is not None else np.zeros_like(x64)
    return c1 * (x64 - c2 * e) + noise, abs(c1) * (np.abs(x64) + np.abs(c2 * e)) + np.abs(noise)


# ------------------------------------------------------------------------------------------------ the model (torch, float64)
def time_table(time_steps, D):
    """the reference's SinusoidalEmbeddings table: its fp32 torch calls, then exact in float64"""
    t = torch.arange(time_steps).unsqueeze(1).float()
    freq = torch.exp(torch.arange(0, D, 2).float() * -(math.log(10000.0) / D))
    table = torch.zeros(time_steps, D)
    table[:, 0::2] = torch.sin(t * freq)
    table[:, 1::2] = torch.cos(t * freq)
    return table.double()


def _ln(x, P, name, eps):
    return F.layer_norm(x, x.shape[-1:], P[name + ".weight"], P[name + ".bias"], eps)


def _block(x, P, pre, H):
    B, N, D = x.shape
    dh = D // H
    qkv = F.linear(_ln(x, P, pre + "norm1", 1e-6), P[pre + "attn.qkv.weight"], P[pre + "attn.qkv.bias"]).reshape(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    att = torch.softmax((qkv[0] * dh ** -0.5) @ qkv[1].transpose(-2, -1), dim=-1) @ qkv[2]
    x = x + F.linear(att.transpose(1, 2).reshape(B, N, D), P[pre + "attn.proj.weight"], P[pre + "attn.proj.bias"])
    h = F.gelu(F.linear(_ln(x, P, pre + "norm2", 1e-6), P[pre + "mlp.fc1.weight"], P[pre + "mlp.fc1.bias"]))
    return x + F.linear(h, P[pre + "mlp.fc2.weight"], P[pre + "mlp.fc2.bias"])


def model64(P, kw, x, t, dropout=None):
    """DiffusionVIT.forward in float64.  P: name -> float64 tensor (the state_dict's entries); kw: the constructor keywords; t: int64 [B];
    dropout: None (eval) or (p, seed) of the time MLP's hidden layer (train)."""
    p, D = kw["patch_size"], kw["embed_dim"]
    conv = F.conv2d if kw.get("twoD", True) else F.conv3d
    tok = conv(x, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=p).flatten(2).transpose(1, 2)
    tok = tok + P["pos_embed"]
    h = F.linear(time_table(kw["time_steps"], D)[t], P["timeEmbeddingMap.linear1.weight"], P["timeEmbeddingMap.linear1.bias"])
    h = torch.relu(h)
    if dropout is not None:
        keep = torch.from_numpy(DR.keep_mask(dropout[1], h.shape[0], h.shape[1], dropout[0]))
        h = torch.where(keep, h * DR.inv_keep(dropout[0]), torch.zeros_like(h))
    temb = F.linear(h, P["timeEmbeddingMap.linear2.weight"], P["timeEmbeddingMap.linear2.bias"])
    tok = tok + temb[:, None, :]
    for i in range(kw["depth"]):
        tok = _block(tok, P, f"blocks.{i}.", kw["num_heads"])
    tok = _ln(tok, P, "norm", 1e-6)
    if not kw["linear_decoder"]:
        tok = F.linear(tok, P["decoder_embed.weight"], P["decoder_embed.bias"]) + P["decoder_pos_embed"]
        for i in range(kw["decoder_depth"]):
            tok = _block(tok, P, f"decoder_blocks.{i}.", kw["decoder_num_heads"])
        tok = _ln(tok, P, "decoder_norm", 1e-5)      # nn.LayerNorm(decoder_embed_dim): torch's default eps, not the models' 1e-6
    return F.linear(tok, P["decoder_pred.weight"], P["decoder_pred.bias"])


SMALL_KW = dict(img_size=[32, 32], patch_size=8, in_chans=3, embed_dim=64, depth=2, num_heads=2, class_token=False, linear_decoder=False,
                decoder_depth=1, decoder_embed_dim=32, decoder_num_heads=1, mlp_ratio_decoder=4.0, time_steps=10)
LINEAR3D_KW = dict(img_size=[16, 8, 8], patch_size=4, in_chans=1, embed_dim=96, depth=1, num_heads=3, class_token=False, linear_decoder=True,
                   decoder_depth=1, decoder_embed_dim=32, decoder_num_heads=1, mlp_ratio_decoder=4.0, time_steps=10, twoD=False)
FIXTURES = {"model_diffusion_small.npz": SMALL_KW, "model_diffusion_3d_linear.npz": LINEAR3D_KW}


def fixture_state_dict(model, g):
    """the fixture's weights: det_state_dict(model, seed) with the recorded overrides (time MLP, decoder_pos_embed)"""
    from det_weights import det_state_dict
    sd = det_state_dict(model, int(g["seed"]))
    for k, v in g.items():
        if k.startswith("w."):
            assert k[2:] in sd and sd[k[2:]].shape == v.shape, k
            sd[k[2:]] = v.clone()
    return sd
