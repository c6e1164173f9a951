"""float64 restatement of QK-norm, shared by the tests/test_qk_norm_*.py files (plain torch, runs anywhere), next to layer_scale_ref.py:

    qk_norm64     : the op on the packed buffer qkv [rows, 3, H, dh]: LayerNorm over dh of every (row, head) segment of Q (gamma_q, beta_q)
                    and of K (gamma_k, beta_k), biased variance, eps inside the root; V passes through
    attn64_qkn    : Attention with q_norm / k_norm between the qkv Linear and the scores (reference building_blocks.py:161)
    block64_qkn   : layer_scale_ref.block64 with that attention: drop path, dropout masks and LayerScale act at the branch exits as there

tests/test_qk_norm_cpu.py pins all three to the reference fixtures without a GPU, so the GPU tests that compare against them compare against
the reference."""
import torch
import torch.nn.functional as F

from layer_scale_ref import _branch, mlp64, p64  # noqa: F401  (p64 re-exported)


def qk_norm64(qkv, gq, bq, gk, bk, eps, H, dh, *, whole_row=False, swap_gamma=False, unbiased=False):
    """qkv: float64 [rows, 3 H dh] -> the same with Q and K normalised.  The keyword flags build the plausibly WRONG variants the GPU
    tests' bounds must reject: statistics over the whole H dh row of a third, gamma_q applied to K, the unbiased variance."""
    rows = qkv.shape[0]
    t = qkv.view(rows, 3, H, dh)
    out = []
    for i, (g, b) in enumerate(((gq, bq), (gk if not swap_gamma else gq, bk))):
        x = t[:, i]
        dims = (1, 2) if whole_row else (2,)
        mu = x.mean(dims, keepdim=True)
        var = ((x - mu) ** 2).mean(dims, keepdim=True)
        if unbiased:
            var = var * dh / (dh - 1)
        out.append((x - mu) / torch.sqrt(var + eps) * g + b)
    out.append(t[:, 2])
    return torch.stack(out, 1).reshape(rows, 3 * H * dh)


def attn64_qkn(h, P, H, eps, pre="attn."):
    Bn, N, D = h.shape
    dh = D // H
    bias = P.get(pre + "qkv.bias")
    qkv = h @ P[pre + "qkv.weight"].T
    if bias is not None:
        qkv = qkv + bias
    if pre + "q_norm.weight" in P:
        qkv = qk_norm64(qkv.reshape(Bn * N, 3 * D), P[pre + "q_norm.weight"], P[pre + "q_norm.bias"], P[pre + "k_norm.weight"],
                        P[pre + "k_norm.bias"], eps, H, dh)
    qkv = qkv.view(Bn, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    att = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * dh ** -0.5, dim=-1)
    o = (att @ qkv[2]).transpose(1, 2).reshape(Bn, N, D)
    return o @ P[pre + "proj.weight"].T + P[pre + "proj.bias"]


def block64_qkn(x, P, H, eps, s1=None, s2=None, mp=None, m1=None, m2=None):
    D = x.shape[-1]
    b1 = attn64_qkn(F.layer_norm(x, (D,), P["norm1.weight"], P["norm1.bias"], eps), P, H, eps)
    x1 = x + _branch(b1, P.get("ls1.gamma"), s1, mp)
    b2 = mlp64(F.layer_norm(x1, (D,), P["norm2.weight"], P["norm2.bias"], eps), P, m1)
    return x1 + _branch(b2, P.get("ls2.gamma"), s2, m2)
