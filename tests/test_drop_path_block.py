"""Stochastic depth inside the fused Blocks (HF.BlockFn / HF.TailBlockFn with explicit per-sample scales) against a float64 restatement:

    x1 = x  + s1[b] * proj(attn(norm1(x)))          y = x1 + s2[b] * fc2(gelu(fc1(norm2(x1))))

The reference is torch in float64 (LayerNorm, Linear, softmax attention, erf-GELU) with the recorded scales; tolerances are those
tests/test_hip_ops.py applies to the same Block (conftest.rel_err < 1e-3 in fp32, 3e-2 in bf16).  Exact statements: a sample dropped in
both branches passes through untouched in both directions; s1 = s2 = 1 in fp32 reproduces the Block without drop path bit for bit;
activation checkpointing reproduces the gradients bit for bit.  Three Blocks in a row check the bias-gradient routing: the proj / fc2 bias
gradients are the column sums of the SCALED branch gradients, not those of the stream gradient that the LayerNorm backward kernels
publish for the Block before them."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.float32: 1e-3, torch.bfloat16: 3e-2}
KEEP = 0.8
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
CONFIGS = {"D64": (64, 2, 10), "D128-N197": (128, 2, 197)}      # dim, heads, tokens (N = 197, dh = 64: the fused short-sequence attention)
B = 4


def _mods():
    from UCF_VIT.simple import building_blocks as BB
    from UCF_VIT._hip import functional as HF
    return BB, HF


def _make_block(D, H, seed, dtype):
    BB, _ = _mods()
    torch.manual_seed(seed)
    blk = BB.Block(D, H, qkv_bias=True)
    with torch.no_grad():
        for n in (blk.norm1, blk.norm2):
            n.weight.add_(0.2 * torch.randn(D))
            n.bias.add_(0.2 * torch.randn(D))
    blk = blk.to(DEV)
    BB.set_compute_dtype(blk, dtype)
    return blk


def _input(D, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, D, generator=g).to(DEV, dtype), torch.randn(B, N, D, generator=g).to(DEV, dtype)


def _scale(vals):
    return torch.tensor(vals, dtype=torch.float32, device=DEV)


K = (torch.ones(1) / KEEP).item()
PATTERNS = {                                                       # (s1, s2)
    "all-kept": ([K, K, K, K], [K, K, K, K]),
    "one-dropped-in-both": ([K, 0.0, K, K], [K, 0.0, K, K]),
    "dropped-in-one-branch": ([K, K, 0.0, K], [0.0, K, K, K]),
}


def _args(blk, x):
    a, m = blk.attn, blk.mlp
    return (x, blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias, blk.norm2.weight, blk.norm2.bias,
            m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, a.num_heads, blk.norm1.eps, getattr(blk, "compute_dtype", torch.float32))


def _run(blk, x, s1, s2, recompute=False):
    _, HF = _mods()
    return HF.BlockFn.apply(*_args(blk, x), None, recompute, s1, s2)


def _run_tail(blk, x, s1, s2, recompute=False):
    _, HF = _mods()
    return HF.TailBlockFn.apply(*_args(blk, x), recompute, s1, s2)


def _zero(*blks):
    for b in blks:
        for p in b.parameters():
            p.grad = None


def _grads(blk):
    return {k: p.grad.clone() for k, p in blk.named_parameters()}


def _p64(blk):
    return {k: p.detach().double().requires_grad_(True) for k, p in blk.named_parameters()}


def block64(x, P, H, eps, s1, s2, keep=None):
    """float64 restatement of the Block; keep: a dict that receives the intermediate stream tensors (x1, y) with retain_grad"""
    Bn, N, D = x.shape
    one = torch.ones(Bn, dtype=torch.float64, device=x.device)
    s1 = (one if s1 is None else s1.double())[:, None, None]
    s2 = (one if s2 is None else s2.double())[:, None, None]
    h = F.layer_norm(x, (D,), P["norm1.weight"], P["norm1.bias"], eps)
    qkv = (h @ P["attn.qkv.weight"].T + P["attn.qkv.bias"]).view(Bn, N, 3, H, D // H).permute(2, 0, 3, 1, 4)
    att = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * (D // H) ** -0.5, dim=-1)
    o = (att @ qkv[2]).transpose(1, 2).reshape(Bn, N, D)
    x1 = x + s1 * (o @ P["attn.proj.weight"].T + P["attn.proj.bias"])
    h2 = F.layer_norm(x1, (D,), P["norm2.weight"], P["norm2.bias"], eps)
    m = F.gelu(h2 @ P["mlp.fc1.weight"].T + P["mlp.fc1.bias"]) @ P["mlp.fc2.weight"].T + P["mlp.fc2.bias"]
    y = x1 + s2 * m
    if keep is not None:
        x1.retain_grad(), y.retain_grad()
        keep["x1"], keep["y"] = x1, y
    return y


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_block_vs_fp64(cfg, pattern, dtype):
    D, H, N = CONFIGS[cfg]
    blk = _make_block(D, H, 3, dtype)
    x, gy = _input(D, N, 4, dtype)
    x.requires_grad_(True)
    s1, s2 = (_scale(v) for v in PATTERNS[pattern])
    y = _run(blk, x, s1, s2)
    y.backward(gy)
    assert y.dtype == dtype
    P = _p64(blk)
    x64 = x.detach().double().requires_grad_(True)
    y64 = block64(x64, P, H, blk.norm1.eps, s1, s2)
    y64.backward(gy.double())
    tol = TOL[dtype]
    assert rel_err(y.float(), y64) < tol
    assert rel_err(x.grad.float(), x64.grad) < tol
    for k, p in blk.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32, k
        assert rel_err(p.grad, P[k].grad) < tol, k
    if pattern == "one-dropped-in-both":                            # sample 1 leaves the Block as it came, in both directions
        assert torch.equal(y[1], x[1]) and torch.equal(x.grad[1], gy[1])
        assert not torch.equal(y[0], x[0])
    # activation checkpointing: the recomputed forward uses the saved draw; bit-identical gradients
    g0, dx0 = _grads(blk), x.grad.clone()
    _zero(blk)
    x.grad = None
    y2 = _run(blk, x, s1, s2, recompute=True)
    y2.backward(gy)
    assert torch.equal(y2, y) and torch.equal(x.grad, dx0)
    for k, g in _grads(blk).items():
        assert torch.equal(g, g0[k]), k


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_unit_scales_reproduce_the_block_without_drop_path_fp32(cfg):
    """fp32, s1 = s2 = 1: x + 1 * (acc + bias) is the two fp32 additions the GEMM epilogue does with its residual"""
    D, H, N = CONFIGS[cfg]
    blk = _make_block(D, H, 5, torch.float32)
    x, _ = _input(D, N, 6, torch.float32)
    one = _scale([1.0] * B)
    _, HF = _mods()
    with torch.no_grad():
        assert torch.equal(_run(blk, x, one, one), HF.BlockFn.apply(*_args(blk, x)))
        assert torch.equal(_run(blk, x, None, None), blk(x))


def _chain64(blocks, final, x64, scales, eps):
    keeps, Ps = [], []
    t = x64
    for blk, (s1, s2) in zip(blocks, scales):
        P, keep = _p64(blk), {}
        t = block64(t, P, blk.attn.num_heads, eps, s1, s2, keep)
        Ps.append(P), keeps.append(keep)
    fw, fb = final.weight.detach().double().requires_grad_(True), final.bias.detach().double().requires_grad_(True)
    return F.layer_norm(t, (t.shape[-1],), fw, fb, final.eps), Ps, keeps


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("where", ["middle", "all"])
def test_three_blocks_bias_gradient_routing(where, dtype):
    """Block i + 1's LayerNorm-1 backward (and the final norm's) publishes the column sums of the UNSCALED stream gradient for Block i's fc2
    bias; a Block with drop path must drop them and use the sums of s2 * dy (fc2) and s1 * dx1 (proj)."""
    BB, _ = _mods()
    D, H, N = 64, 2, 10
    blocks = [_make_block(D, H, 10 + i, dtype) for i in range(3)]
    final = BB.LayerNorm(D).to(DEV)
    BB.set_compute_dtype(final, dtype)
    x, gy = _input(D, N, 7, dtype)
    x.requires_grad_(True)
    drop = (_scale([K, 0.0, K, K]), _scale([0.0, K, K, 0.0]))
    scales = [drop if (where == "all" or i == 1) else (None, None) for i in range(3)]
    t = x
    for blk, (s1, s2) in zip(blocks, scales):
        t = _run(blk, t, s1, s2) if s1 is not None else blk(t)
    y = final(t)
    y.backward(gy)
    x64 = x.detach().double().requires_grad_(True)
    y64, Ps, keeps = _chain64(blocks, final, x64, scales, blocks[0].norm1.eps)
    y64.backward(gy.double())
    tol = TOL[dtype]
    assert rel_err(y.float(), y64) < tol and rel_err(x.grad.float(), x64.grad) < tol
    for i, (blk, P, keep, (s1, s2)) in enumerate(zip(blocks, Ps, keeps, scales)):
        for k, p in blk.named_parameters():
            assert rel_err(p.grad, P[k].grad) < tol, (i, k)
        if s1 is not None:                                          # the sums a stale or unscaled hand-over would have delivered
            stale_fc2, stale_proj = keep["y"].grad.sum((0, 1)), keep["x1"].grad.sum((0, 1))
            assert rel_err(blk.mlp.fc2.bias.grad, stale_fc2) > tol, i
            assert rel_err(blk.attn.proj.bias.grad, stale_proj) > tol, i


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_tail_block_class_rows(pattern, dtype):
    """forward_class_rows(x) = forward(x)[:, 0] with the same recorded scales (rows_per_sample = 1 from the attention on, the proj
    residual read from the strided class rows), against fp64 including dx; and bit-identical under activation checkpointing"""
    D, H, N = CONFIGS["D64"]
    blk = _make_block(D, H, 8, dtype)
    x, gy = _input(D, N, 9, dtype)
    gy = gy[:, 0].contiguous()
    x.requires_grad_(True)
    s1, s2 = (_scale(v) for v in PATTERNS[pattern])
    y = _run_tail(blk, x, s1, s2)
    y.backward(gy)
    assert tuple(y.shape) == (B, D)
    P = _p64(blk)
    x64 = x.detach().double().requires_grad_(True)
    y64 = block64(x64, P, H, blk.norm1.eps, s1, s2)[:, 0]
    y64.backward(gy.double())
    tol = TOL[dtype]
    assert rel_err(y.float(), y64) < tol and rel_err(x.grad.float(), x64.grad) < tol
    for k, p in blk.named_parameters():
        assert rel_err(p.grad, P[k].grad) < tol, k
    with torch.no_grad():
        dense = _run(blk, x, s1, s2)[:, 0]
    assert rel_err(y.float(), dense.double()) < tol
    if pattern == "one-dropped-in-both":
        assert torch.equal(y[1], x[1, 0]) and torch.equal(dense[1], x[1, 0])
    g0, dx0 = _grads(blk), x.grad.clone()
    _zero(blk)
    x.grad = None
    y2 = _run_tail(blk, x, s1, s2, recompute=True)
    y2.backward(gy)
    assert torch.equal(y2, y) and torch.equal(x.grad, dx0)
    for k, g in _grads(blk).items():
        assert torch.equal(g, g0[k]), k


def test_module_draws_s1_then_s2_and_eval_is_the_plain_block():
    """Block.forward / forward_class_rows draw two independent scale tensors (attention branch first) and hand them on; eval runs the
    launches of a Block without drop path"""
    BB, _ = _mods()
    torch.manual_seed(1)
    blk = BB.Block(64, 2, qkv_bias=True, drop_path=0.5).to(DEV)
    ref = BB.Block(64, 2, qkv_bias=True).to(DEV)
    ref.load_state_dict(blk.state_dict())
    x, _ = _input(64, 10, 2, torch.float32)
    blk.train()
    torch.manual_seed(5)
    y = blk(x)
    s1, s2 = blk.drop_path1.last_scale, blk.drop_path2.last_scale
    torch.manual_seed(5)
    want1 = torch.empty(B, device=DEV).bernoulli_(0.5) / 0.5
    want2 = torch.empty(B, device=DEV).bernoulli_(0.5) / 0.5
    assert torch.equal(s1, want1) and torch.equal(s2, want2)
    assert torch.equal(y, _run(ref, x, s1, s2))
    torch.manual_seed(5)
    assert torch.equal(blk.forward_class_rows(x), _run_tail(ref, x, s1, s2))
    # the unfused fall-back expression goes through DropPath.forward (HF.DropPathFn): same draw order, same mathematics
    torch.manual_seed(5)
    t = x + blk.drop_path1(blk.attn(blk.norm1(x)))
    t = t + blk.drop_path2(blk.mlp(blk.norm2(t)))
    assert rel_err(t, y.double()) < 1e-5
    blk.eval()
    assert torch.equal(blk(x), ref(x))


def test_drop_path_fn_backward_is_the_same_scaling():
    _, HF = _mods()
    x, gy = _input(64, 10, 3, torch.bfloat16)
    x.requires_grad_(True)
    s = _scale([K, 0.0, K, 0.0])
    y = HF.DropPathFn.apply(x, s)
    y.backward(gy)
    tol = 2.0 ** -8
    assert rel_err(y.float(), s[:, None, None].double() * x.detach().double()) < tol
    assert rel_err(x.grad.float(), s[:, None, None].double() * gy.double()) < tol
    assert torch.equal(y[1], torch.zeros_like(y[1])) and torch.equal(x.grad[3], torch.zeros_like(gy[3]))
