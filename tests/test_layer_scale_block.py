"""LayerScale inside the fused Blocks (HF.BlockFn / HF.TailBlockFn with explicit gammas, recorded drop-path scales and dropout seeds)
against the float64 restatement of tests/layer_scale_ref.py, which tests/test_layer_scale_cpu.py pins to the reference's Block:

    x1 = x  + s1[b] * mp * (gamma1 * proj(attn(norm1(x))))          y = x1 + s2[b] * m2 * (gamma2 * fc2(m1 * gelu(fc1(norm2(x1)))))

Configurations and tolerances are those of tests/test_drop_path_block.py: (dim, heads, tokens) = (64, 2, 10) and (128, 2, 197), B = 4,
conftest.rel_err < 1e-3 in fp32 and 3e-2 in bf16, for the output, dx and every parameter gradient, the two gamma gradients among them.
Exact statements: gamma = 1 in fp32 reproduces the Block without LayerScale bit for bit (see that test for what "the Block without" is
for the two exit biases); activation checkpointing reproduces every gradient bit for bit; a sample dropped in both branches passes
through untouched in both directions and adds nothing to the gamma gradients; two runs give the same bits; eval equals the training
forward without drop path and dropout.  Three Blocks in a row check the bias-gradient routing: the proj / fc2 bias gradients are the
column sums of the gamma-scaled branch gradients, not those of the stream gradient that the LayerNorm backward kernels publish."""
from functools import partial

import pytest
import torch
import torch.nn.functional as F

import dropout_ref as R
import layer_scale_ref as LR
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.float32: 1e-3, torch.bfloat16: 3e-2}
KEEP = 0.8
P_DROP = 0.2
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
CONFIGS = {"D64": (64, 2, 10), "D128-N197": (128, 2, 197)}
B = 4
K = (torch.ones(1) / KEEP).item()
PATTERNS = {                                                       # (s1, s2), as in tests/test_drop_path_block.py
    "all-kept": ([K, K, K, K], [K, K, K, K]),
    "one-dropped-in-both": ([K, 0.0, K, K], [K, 0.0, K, K]),
    "dropped-in-one-branch": ([K, K, 0.0, K], [0.0, K, K, K]),
}
SEEDS = (0x1111111122222222, 0x3333333344444444, 0x5555555566666666)      # proj_drop, Mlp.drop1, Mlp.drop2
COMBOS = {                                                         # (drop-path pattern or None, dropout)
    "gamma": (None, False),
    "gamma+drop_path/all-kept": ("all-kept", False),
    "gamma+drop_path/one-dropped-in-both": ("one-dropped-in-both", False),
    "gamma+drop_path/dropped-in-one-branch": ("dropped-in-one-branch", False),
    "gamma+dropout": (None, True),
    "gamma+drop_path+dropout": ("one-dropped-in-both", True),
}


def _mods():
    from UCF_VIT.simple import building_blocks as BB
    from UCF_VIT._hip import functional as HF
    return BB, HF


def _make_block(D, H, seed, dtype, init_values=0.5, spread=0.3, **kw):
    """a Block whose gammas are init_values + spread * randn: of the order of init_values, different per column"""
    BB, _ = _mods()
    torch.manual_seed(seed)
    blk = BB.Block(D, H, qkv_bias=True, init_values=init_values, **kw)
    with torch.no_grad():
        for n in (blk.norm1, blk.norm2):
            n.weight.add_(0.2 * torch.randn(D))
            n.bias.add_(0.2 * torch.randn(D))
        for ls in (blk.ls1, blk.ls2):
            if init_values:
                ls.gamma.add_(spread * torch.randn(D))
    blk = blk.to(DEV)
    BB.set_compute_dtype(blk, dtype)
    return blk


def _input(D, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, D, generator=g).to(DEV, dtype), torch.randn(B, N, D, generator=g).to(DEV, dtype)


def _scale(vals):
    return None if vals is None else torch.tensor(vals, dtype=torch.float32, device=DEV)


def _args(blk, x):
    a, m = blk.attn, blk.mlp
    return (x, blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias, blk.norm2.weight, blk.norm2.bias,
            m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, a.num_heads, blk.norm1.eps, getattr(blk, "compute_dtype", torch.float32))


def _gammas(blk):
    return (blk.ls1.gamma, blk.ls2.gamma) if hasattr(blk.ls1, "gamma") else (None, None)


def _run(blk, x, s1=None, s2=None, drop=None, recompute=False):
    _, HF = _mods()
    return HF.BlockFn.apply(*_args(blk, x), None, recompute, s1, s2, drop, *_gammas(blk))


def _run_tail(blk, x, s1=None, s2=None, drop=None, recompute=False):
    _, HF = _mods()
    return HF.TailBlockFn.apply(*_args(blk, x), recompute, s1, s2, drop, *_gammas(blk))


def _zero(x, *blks):
    x.grad = None
    for b in blks:
        for p in b.parameters():
            p.grad = None


def _grads(blk):
    return {k: p.grad.clone() for k, p in blk.named_parameters()}


def _p64(blk):
    return LR.p64(blk.named_parameters())


def _masks(N, D, on):
    """the three dense masks [B, N, width] in float64 with 1 / keep folded in, or Nones"""
    if not on:
        return None, None, None
    mk = lambda seed, width: (torch.from_numpy(R.keep_mask(seed, B * N, width, P_DROP)).to(DEV).double().view(B, N, width)
                              * R.inv_keep(P_DROP))
    return mk(SEEDS[0], D), mk(SEEDS[1], 4 * D), mk(SEEDS[2], D)


def _combo(name, N, D):
    pattern, dropout = COMBOS[name]
    s1, s2 = (_scale(v) for v in PATTERNS[pattern]) if pattern else (None, None)
    drop = (P_DROP,) + SEEDS if dropout else None
    return pattern, s1, s2, drop, _masks(N, D, dropout)


def _compare(blk, x, y, P, x64, y64, tol):
    assert rel_err(y.float(), y64) < tol
    assert rel_err(x.grad.float(), x64.grad) < tol
    for k, p in blk.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32, k
        assert rel_err(p.grad, P[k].grad) < tol, k
    for k in ("ls1.gamma", "ls2.gamma"):                              # named explicitly: the parameters this feature adds
        assert float(P[k].grad.abs().max()) > 0 and rel_err(dict(blk.named_parameters())[k].grad, P[k].grad) < tol, k


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_block_vs_fp64(cfg, combo, dtype):
    D, H, N = CONFIGS[cfg]
    blk = _make_block(D, H, 3, dtype)
    x, gy = _input(D, N, 4, dtype)
    x.requires_grad_(True)
    pattern, s1, s2, drop, masks = _combo(combo, N, D)
    y = _run(blk, x, s1, s2, drop)
    y.backward(gy)
    assert y.dtype == dtype
    P = _p64(blk)
    x64 = x.detach().double().requires_grad_(True)
    y64 = LR.block64(x64, P, H, blk.norm1.eps, s1, s2, *masks)
    y64.backward(gy.double())
    _compare(blk, x, y, P, x64, y64, TOL[dtype])
    g0, dx0 = _grads(blk), x.grad.clone()
    # two runs: the same bits
    _zero(x, blk)
    y1 = _run(blk, x, s1, s2, drop)
    y1.backward(gy)
    assert torch.equal(y1, y) and torch.equal(x.grad, dx0)
    for k, g in _grads(blk).items():
        assert torch.equal(g, g0[k]), k
    # activation checkpointing: the recomputed forward rebuilds the unscaled branch outputs; bit-identical gradients
    _zero(x, blk)
    y2 = _run(blk, x, s1, s2, drop, recompute=True)
    y2.backward(gy)
    assert torch.equal(y2, y) and torch.equal(x.grad, dx0)
    for k, g in _grads(blk).items():
        assert torch.equal(g, g0[k]), k
    if pattern == "one-dropped-in-both":
        # sample 1 leaves the Block as it came, in both directions, and adds nothing to the gamma gradients: another sample 1, the same bits
        assert torch.equal(y[1], x[1]) and torch.equal(x.grad[1], gy[1])
        assert not torch.equal(y[0], x[0])
        x2 = x.detach().clone()
        x2[1] = 3.0 * x2[1].flip(0) + 1.0
        x2.requires_grad_(True)
        _zero(x, blk)
        _run(blk, x2, s1, s2, drop).backward(gy)
        for k in ("ls1.gamma", "ls2.gamma"):
            assert torch.equal(_grads(blk)[k], g0[k]), k


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("combo", ["gamma", "gamma+drop_path/dropped-in-one-branch", "gamma+drop_path+dropout"])
def test_tail_block_class_rows(combo, dtype):
    """forward_class_rows(x) = forward(x)[:, 0]: rows_per_sample = 1, the proj residual read from the strided class rows (ldr = N D), class
    row b drawing the mask of dense row b N; against fp64 including dx and both gamma gradients, and bit-identical under checkpointing"""
    D, H, N = CONFIGS["D64"]
    blk = _make_block(D, H, 8, dtype)
    x, gy = _input(D, N, 9, dtype)
    gy = gy[:, 0].contiguous()
    x.requires_grad_(True)
    pattern, s1, s2, drop, masks = _combo(combo, N, D)
    y = _run_tail(blk, x, s1, s2, drop)
    y.backward(gy)
    assert tuple(y.shape) == (B, D)
    P = _p64(blk)
    x64 = x.detach().double().requires_grad_(True)
    y64 = LR.block64(x64, P, H, blk.norm1.eps, s1, s2, *masks)[:, 0]
    y64.backward(gy.double())
    _compare(blk, x, y, P, x64, y64, TOL[dtype])
    with torch.no_grad():
        dense = _run(blk, x, s1, s2, drop)[:, 0]
    assert rel_err(y.float(), dense.double()) < TOL[dtype]
    if pattern == "one-dropped-in-both":
        assert torch.equal(y[1], x[1, 0]) and torch.equal(dense[1], x[1, 0])
    g0, dx0 = _grads(blk), x.grad.clone()
    _zero(x, blk)
    y2 = _run_tail(blk, x, s1, s2, drop, recompute=True)
    y2.backward(gy)
    assert torch.equal(y2, y) and torch.equal(x.grad, dx0)
    for k, g in _grads(blk).items():
        assert torch.equal(g, g0[k]), k


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_block_module_vs_reference_fixture(dtype):
    """the Block module (init_values, gammas of order 1) against the reference's Block recorded in op_block_layerscale.npz"""
    BB, _ = _mods()
    g = load_golden("op_block_layerscale.npz")
    blk = BB.Block(64, 2, qkv_bias=True, init_values=0.5, norm_layer=partial(BB.LayerNorm, eps=1e-6))
    blk.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("w.")})
    blk = blk.to(DEV).train()
    BB.set_compute_dtype(blk, dtype)
    assert blk._fusable()
    x = g["x"].to(DEV).requires_grad_(True)
    y = blk(x)
    y.backward(g["gy"].to(DEV, y.dtype))
    tol = TOL[dtype]
    assert y.dtype == dtype
    assert rel_err(y.float(), g["y"]) < tol
    assert rel_err(x.grad.float(), g["gx"]) < tol
    for k, p in blk.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32, k
        assert rel_err(p.grad, g["g." + k]) < tol, k
    assert rel_err(blk.ls1.gamma.grad, g["g.ls1.gamma"]) < tol and rel_err(blk.ls2.gamma.grad, g["g.ls2.gamma"]) < tol
    # the unfused expression goes through the LayerScale module (HF.LayerScaleFn): the same mathematics
    _zero(x, blk)
    t = x + blk.ls1(blk.attn(blk.norm1(x)))
    t = t + blk.ls2(blk.mlp(blk.norm2(t)))
    t.backward(g["gy"].to(DEV, t.dtype))
    assert rel_err(t.float(), g["y"]) < tol and rel_err(x.grad.float(), g["gx"]) < tol
    assert rel_err(blk.ls1.gamma.grad, g["g.ls1.gamma"]) < tol and rel_err(blk.ls2.gamma.grad, g["g.ls2.gamma"]) < tol
    # the class-row tail of the same module
    with torch.no_grad():
        assert rel_err(blk.forward_class_rows(x).float(), g["y"][:, 0]) < tol


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_unit_gamma_reproduces_the_block_without_layer_scale_fp32(cfg):
    """fp32, gamma = 1: 1 * (acc + bias) is exact, x + that is the addition the GEMM epilogue does with its residual, and 1 * dy is dy.
    Output, dx and every gradient but two equal those of the plain Block (launches of a Block built without init_values) bit for bit.
    The two exit-bias gradients (proj, fc2) of the plain Block are summed by the LayerNorm backward kernels in another order; with a
    gamma they are the folded column sums of the row pass, as under drop path.  They are compared bit for bit with the Block without
    LayerScale under unit drop-path scales, which sums the same values in the same fixed order, and with the plain Block within 1e-4:
    both are fp32 sums of B N <= 788 terms along trees of depth h <= 40, so each is within h U sum|term| of the true sum, and
    sum|term| / max|sum| stays below 40 for these random gradients: 2 * 40 * 2^-24 * 40 = 1.9e-4 at the very worst, a tenth of the
    project's fp32 tolerance.  The gamma gradients are finite."""
    D, H, N = CONFIGS[cfg]
    _, HF = _mods()
    blk = _make_block(D, H, 5, torch.float32, init_values=1.0, spread=0.0)
    assert torch.equal(blk.ls1.gamma, torch.ones(D, device=DEV))
    x, gy = _input(D, N, 6, torch.float32)
    x.requires_grad_(True)
    y = _run(blk, x)
    y.backward(gy)
    g1, dx1 = _grads(blk), x.grad.clone()
    assert bool(torch.isfinite(g1["ls1.gamma"]).all()) and bool(torch.isfinite(g1["ls2.gamma"]).all())
    assert float(g1["ls1.gamma"].abs().max()) > 0 and float(g1["ls2.gamma"].abs().max()) > 0
    _zero(x, blk)
    y0 = HF.BlockFn.apply(*_args(blk, x))
    y0.backward(gy)
    g0, dx0 = _grads_present(blk), x.grad.clone()
    assert torch.equal(y, y0) and torch.equal(dx1, dx0)
    exit_biases = ("attn.proj.bias", "mlp.fc2.bias")
    for k, g in g0.items():
        if k in exit_biases:
            assert rel_err(g1[k], g) < 1e-4, k
        else:
            assert torch.equal(g1[k], g), k
    _zero(x, blk)
    one = _scale([1.0] * B)
    ys = HF.BlockFn.apply(*_args(blk, x), None, False, one, one)
    ys.backward(gy)
    gs = _grads_present(blk)
    assert torch.equal(ys, y) and torch.equal(x.grad, dx1)
    for k, g in gs.items():
        assert torch.equal(g1[k], g), k


def _grads_present(blk):
    return {k: p.grad.clone() for k, p in blk.named_parameters() if p.grad is not None}


def _chain64(blocks, final, x64, eps):
    keeps, Ps = [], []
    t = x64
    for blk in blocks:
        P, keep = _p64(blk), {}
        t = LR.block64(t, P, blk.attn.num_heads, eps, keep=keep)
        Ps.append(P), keeps.append(keep)
    fw, fb = final.weight.detach().double().requires_grad_(True), final.bias.detach().double().requires_grad_(True)
    return F.layer_norm(t, (t.shape[-1],), fw, fb, final.eps), Ps, keeps


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("where", ["middle", "all"])
def test_three_blocks_bias_gradient_routing(where, dtype):
    """Block i + 1's LayerNorm-1 backward (and the final norm's) publishes the column sums of the stream gradient for Block i's fc2 bias; a
    Block with LayerScale must drop them and use the sums of gamma2 * dy (fc2) and gamma1 * dx1 (proj)"""
    BB, _ = _mods()
    D, H, N = 64, 2, 10
    blocks = [_make_block(D, H, 10 + i, dtype, init_values=(0.5 if (where == "all" or i == 1) else None)) for i in range(3)]
    final = BB.LayerNorm(D).to(DEV)
    BB.set_compute_dtype(final, dtype)
    x, gy = _input(D, N, 7, dtype)
    x.requires_grad_(True)
    t = x
    for blk in blocks:
        t = blk(t)
    y = final(t)
    y.backward(gy)
    x64 = x.detach().double().requires_grad_(True)
    y64, Ps, keeps = _chain64(blocks, final, x64, blocks[0].norm1.eps)
    y64.backward(gy.double())
    tol = TOL[dtype]
    assert rel_err(y.float(), y64) < tol and rel_err(x.grad.float(), x64.grad) < tol
    for i, (blk, P, keep) in enumerate(zip(blocks, Ps, keeps)):
        for k, p in blk.named_parameters():
            assert rel_err(p.grad, P[k].grad) < tol, (i, k)
        if hasattr(blk.ls1, "gamma"):
            # what they are: the sums of the gradients of the unscaled branch outputs; what a stale hand-over would have delivered
            assert rel_err(blk.mlp.fc2.bias.grad, keep["b2"].grad.sum((0, 1))) < tol, i
            assert rel_err(blk.attn.proj.bias.grad, keep["b1"].grad.sum((0, 1))) < tol, i
            stale_fc2, stale_proj = keep["y"].grad.sum((0, 1)), keep["x1"].grad.sum((0, 1))
            assert rel_err(blk.mlp.fc2.bias.grad, stale_fc2) > tol, i
            assert rel_err(blk.attn.proj.bias.grad, stale_proj) > tol, i


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_default_init_values_judged_on_gradients(dtype):
    """init_values = 1e-5: the output equals x to bf16 precision, so it says nothing; dx and the gamma gradients (which do not depend on
    gamma's size) against float64"""
    D, H, N = CONFIGS["D64"]
    blk = _make_block(D, H, 12, dtype, init_values=1e-5, spread=0.0).train()
    x, gy = _input(D, N, 13, dtype)
    x.requires_grad_(True)
    y = blk(x)
    y.backward(gy)
    P = _p64(blk)
    x64 = x.detach().double().requires_grad_(True)
    LR.block64(x64, P, H, blk.norm1.eps).backward(gy.double())
    tol = TOL[dtype]
    assert rel_err(x.grad.float(), x64.grad) < tol
    for k in ("ls1.gamma", "ls2.gamma"):
        g = dict(blk.named_parameters())[k].grad
        assert g is not None and float(P[k].grad.abs().max()) > 1e-2 and rel_err(g, P[k].grad) < tol, k


def test_eval_is_the_training_forward_without_drop_path_and_dropout():
    """eval under no_grad overwrites the branch, training (and eval with autograd on) writes the sum to a new buffer and keeps the
    branch: the same bits"""
    blk = _make_block(64, 2, 14, torch.float32, drop_path=0.5, proj_drop=P_DROP)
    x, gy = _input(64, 10, 15, torch.float32)
    blk.eval()
    with torch.no_grad():
        y_eval = blk(x)
        t_eval = blk.forward_class_rows(x)
    xg = x.clone().requires_grad_(True)
    y_eval_grad = blk(xg)                                           # eval with autograd on: the branch outputs are kept
    y_train = _run(blk, xg)
    assert y_train.requires_grad
    assert torch.equal(y_eval, y_train) and torch.equal(y_eval, y_eval_grad) and torch.equal(t_eval, _run_tail(blk, xg))


def test_no_grad_overwrites_the_branch_and_grad_mode_keeps_it(monkeypatch):
    """the module passes torch.is_grad_enabled() on: under no_grad (parameters still require a gradient) both branch exits write over the
    branch, with autograd on they write to a new buffer and keep the branch output; the same bits either way"""
    _, HF = _mods()
    blk = _make_block(64, 2, 18, torch.float32).train()
    x, _ = _input(64, 10, 19, torch.float32)
    seen = []
    real = HF._Exit.forward

    def spy(self, res, y, keep):
        out, saved = real(self, res, y, keep)
        if self.gamma is not None:                                  # the exits of this file's Blocks all have one
            seen.append((keep, out.data_ptr() == y.data_ptr()))
        return out, saved
    monkeypatch.setattr(HF._Exit, "forward", spy)
    assert all(p.requires_grad for p in blk.parameters())
    with torch.no_grad():
        y0 = blk(x)
        t0 = blk.forward_class_rows(x)
    assert seen == [(False, True)] * 4
    del seen[:]
    y1 = blk(x)
    t1 = blk.forward_class_rows(x)
    assert seen == [(True, False)] * 4 and y1.requires_grad
    assert torch.equal(y0, y1) and torch.equal(t0, t1)


def test_module_draws_and_hands_gammas_on():
    """Block.forward in training with all three: the module's draws and its gammas reach the node (the same bits as the explicit call)"""
    blk = _make_block(64, 2, 16, torch.float32, drop_path=0.5, proj_drop=P_DROP).train()
    x, _ = _input(64, 10, 17, torch.float32)
    torch.manual_seed(5)
    y = blk(x)
    s1, s2 = blk.drop_path1.last_scale, blk.drop_path2.last_scale
    drop = (P_DROP, blk.attn.proj_drop.last_seed, blk.mlp.drop1.last_seed, blk.mlp.drop2.last_seed)
    assert torch.equal(y, _run(blk, x, s1, s2, drop))
    torch.manual_seed(5)
    assert torch.equal(blk.forward_class_rows(x), _run_tail(blk, x, s1, s2, drop))
