"""float64 restatement of the Block with LayerScale, shared by the tests/test_layer_scale_*.py files (plain torch, runs anywhere):

    x1 = x  + s1[b] * mp * (gamma1 * proj(attn(norm1(x))))          y = x1 + s2[b] * m2 * (gamma2 * fc2(m1 * gelu(fc1(norm2(x1)))))

gamma1 / gamma2 are P["ls1.gamma"] / P["ls2.gamma"] (absent: 1); s1 / s2 are per-sample drop-path scales (None: 1); mp / m1 / m2 are the
dropout masks with 1 / keep folded in (None: 1).  tests/test_layer_scale_cpu.py pins it to the reference fixture op_block_layerscale.npz
without a GPU, so the GPU tests that compare against it compare against the reference's Block."""
import torch
import torch.nn.functional as F


def p64(named, device=None):
    """{name: float64 leaf} from an iterable of (name, tensor)"""
    return {k: v.detach().to(device or v.device).double().requires_grad_(True) for k, v in named}


def attn64(h, P, H, pre="attn."):
    Bn, N, D = h.shape
    qkv = (h @ P[pre + "qkv.weight"].T + P[pre + "qkv.bias"]).view(Bn, N, 3, H, D // H).permute(2, 0, 3, 1, 4)
    att = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * (D // H) ** -0.5, dim=-1)
    o = (att @ qkv[2]).transpose(1, 2).reshape(Bn, N, D)
    return o @ P[pre + "proj.weight"].T + P[pre + "proj.bias"]


def mlp64(h, P, m1=None, pre="mlp."):
    a = F.gelu(h @ P[pre + "fc1.weight"].T + P[pre + "fc1.bias"])
    if m1 is not None:
        a = a * m1
    return a @ P[pre + "fc2.weight"].T + P[pre + "fc2.bias"]


def _branch(b, gamma, s, m):
    if gamma is not None:
        b = gamma * b
    if m is not None:
        b = m * b
    if s is not None:
        b = s.double()[:, None, None] * b
    return b


def block64(x, P, H, eps, s1=None, s2=None, mp=None, m1=None, m2=None, keep=None):
    """keep: a dict that receives the stream tensors x1, y and the unscaled branch outputs b1, b2, all with retain_grad"""
    D = x.shape[-1]
    b1 = attn64(F.layer_norm(x, (D,), P["norm1.weight"], P["norm1.bias"], eps), P, H)
    x1 = x + _branch(b1, P.get("ls1.gamma"), s1, mp)
    b2 = mlp64(F.layer_norm(x1, (D,), P["norm2.weight"], P["norm2.bias"], eps), P, m1)
    y = x1 + _branch(b2, P.get("ls2.gamma"), s2, m2)
    if keep is not None:
        for k, t in (("x1", x1), ("y", y), ("b1", b1), ("b2", b2)):
            t.retain_grad()
            keep[k] = t
    return y
