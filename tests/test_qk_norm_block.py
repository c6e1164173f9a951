"""qk_norm inside the fused autograd nodes (HF.AttentionFn, HF.BlockFn, HF.TailBlockFn) and the Attention / Block modules, against the
reference fixtures op_attn_qknorm.npz / op_block_qknorm.npz and against the float64 restatement of tests/qk_norm_ref.py (which
tests/test_qk_norm_cpu.py pins to those fixtures).  Tolerances are those of tests/test_layer_scale_block.py: conftest.rel_err < 1e-3 in
fp32 and 3e-2 in bf16 for the output, dx and every parameter gradient.  One gradient is judged differently: k_norm.bias, whose gradient
is mathematically 0 (a key bias shifts every score of a query alike); the difference is measured against the largest entry of the
q_norm.bias gradient, the size of the terms that cancel in it.

Shapes: (dim, heads, tokens) = (64, 2, 10), (128, 2, 197) (head width 64, the fused short-sequence route in bf16) and (64, 2, 300) (above
256 tokens: the streaming route), so the qkv bias gradient (Q and K thirds from qk_norm_bwd's column sums, V third from the proj
data-gradient epilogue) is checked on both attention routes.  Exact statements: activation checkpointing and a second run reproduce every
bit; a Block without qk_norm issues the launches of the plain node; a group of same-shaped parameters that requires no gradient gets none
while every other gradient stays right (B = 2: a gradient filed under the wrong argument would have the right shape)."""
import ctypes
from functools import partial

import pytest
import torch

import dropout_ref as R
import qk_norm_ref as QR
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.float32: 1e-3, torch.bfloat16: 3e-2}
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
CONFIGS = {"D64-N10": (64, 2, 10), "D128-N197": (128, 2, 197), "D64-N300": (64, 2, 300)}
B = 4
P_DROP = 0.2
SEEDS = (0x1111111122222222, 0x3333333344444444, 0x5555555566666666)
QK = ("attn.q_norm.weight", "attn.q_norm.bias", "attn.k_norm.weight", "attn.k_norm.bias")


def _mods():
    from UCF_VIT.simple import building_blocks as BB
    from UCF_VIT._hip import functional as HF
    return BB, HF


def _make_block(D, H, seed, dtype, qk_norm=True, **kw):
    """norm weights and biases of order 1 / 0.2, different per element and between q and k"""
    BB, _ = _mods()
    torch.manual_seed(seed)
    blk = BB.Block(D, H, qk_norm=qk_norm, norm_layer=partial(BB.LayerNorm, eps=1e-6), **{"qkv_bias": True, **kw})
    with torch.no_grad():
        norms = [blk.norm1, blk.norm2] + ([blk.attn.q_norm, blk.attn.k_norm] if qk_norm else [])
        for n in norms:
            n.weight.add_(0.3 * torch.randn(n.weight.shape))
            n.bias.add_(0.2 * torch.randn(n.bias.shape))
        for ls in (blk.ls1, blk.ls2):
            if hasattr(ls, "gamma"):
                ls.gamma.add_(0.3 * torch.randn(D))
    blk = blk.to(DEV)
    BB.set_compute_dtype(blk, dtype)
    return blk


def _input(D, N, seed, dtype, b=B):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, N, D, generator=g).to(DEV, dtype), torch.randn(b, N, D, generator=g).to(DEV, dtype)


def _args(blk, x):
    a, m = blk.attn, blk.mlp
    return (x, blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias, blk.norm2.weight, blk.norm2.bias,
            m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, a.num_heads, blk.norm1.eps, getattr(blk, "compute_dtype", torch.float32))


def _tail(blk):
    a = blk.attn
    g = (blk.ls1.gamma, blk.ls2.gamma) if hasattr(blk.ls1, "gamma") else (None, None)
    qk = (a.q_norm.weight, a.q_norm.bias, a.k_norm.weight, a.k_norm.bias, a.q_norm.eps) if hasattr(a.q_norm, "weight") else ()
    return g + (True,) + qk


def _run(blk, x, s1=None, s2=None, drop=None, recompute=False):
    _, HF = _mods()
    return HF.BlockFn.apply(*_args(blk, x), None, recompute, s1, s2, drop, *_tail(blk))


def _run_tail(blk, x, s1=None, s2=None, drop=None, recompute=False):
    _, HF = _mods()
    return HF.TailBlockFn.apply(*_args(blk, x), recompute, s1, s2, drop, *_tail(blk))


def _zero(x, *mods):
    x.grad = None
    for m in mods:
        for p in m.parameters():
            p.grad = None


def _grads(mod):
    return {k: p.grad.clone() for k, p in mod.named_parameters()}


def _grad_err(k, got, ref):
    """ref: {name: reference gradient}; rel_err, but k_norm.bias (mathematically 0) against the scale of q_norm.bias's gradient"""
    if k.endswith("k_norm.bias"):
        scale = ref[k[:-len("k_norm.bias")] + "q_norm.bias"].double().abs().max()
        return ((got.double().cpu() - ref[k].double().cpu()).abs().max() / scale.cpu()).item()
    return rel_err(got, ref[k])


def _compare(mod, x, y, ref, x64grad, y64, tol):
    assert rel_err(y.float(), y64) < tol
    assert rel_err(x.grad.float(), x64grad) < tol
    for k, p in mod.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32, k
        assert _grad_err(k, p.grad, ref) < tol, k
    for k in ref:                                                     # named explicitly: the parameters this feature adds
        if "q_norm" in k or k.endswith("k_norm.weight"):
            assert float(ref[k].abs().max()) > 0, k


def _masks(N, D, on, b=B):
    if not on:
        return None, None, None
    mk = lambda seed, width: (torch.from_numpy(R.keep_mask(seed, b * N, width, P_DROP)).to(DEV).double().view(b, N, width)
                              * R.inv_keep(P_DROP))
    return mk(SEEDS[0], D), mk(SEEDS[1], 4 * D), mk(SEEDS[2], D)


def _route(N, H, dh, dtype, backward):
    from UCF_VIT._hip import lib as L
    buf = ctypes.create_string_buffer(64)
    n = L.load().ucfvit_attention_route(B, N, H, dh, L.BF16 if dtype == torch.bfloat16 else L.F32, int(backward), buf, 64)
    assert 0 < n < 64
    return buf.value.decode()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attention_module_vs_reference_fixture(dtype):
    """the bare Attention (eps 1e-5, HF.AttentionFn) against the reference's, recorded in op_attn_qknorm.npz"""
    BB, HF = _mods()
    g = load_golden("op_attn_qknorm.npz")
    att = BB.Attention(64, num_heads=2, qkv_bias=True, qk_norm=True)
    att.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("w.")})
    att = att.to(DEV).train()
    BB.set_compute_dtype(att, dtype)
    assert att._fusable() and att.q_norm.eps == 1e-5
    x = g["x"].to(DEV).requires_grad_(True)
    y = att(x)
    y.backward(g["gy"].to(DEV, y.dtype))
    assert y.dtype == dtype
    ref = {k[2:]: v for k, v in g.items() if k.startswith("g.")}
    _compare(att, x, y, ref, g["gx"], g["y"], TOL[dtype])
    g0, dx0 = _grads(att), x.grad.clone()
    _zero(x, att)
    y1 = att(x)
    y1.backward(g["gy"].to(DEV, y.dtype))
    assert torch.equal(y1, y) and torch.equal(x.grad, dx0)
    for k, v in _grads(att).items():
        assert torch.equal(v, g0[k]), k
    with torch.no_grad():                                             # nothing saved: the same bits
        assert torch.equal(att(x), y)
    # the module hands its own eps (1e-5 for a bare Attention) and its four parameters to the node
    a = att
    y2 = HF.AttentionFn.apply(x, a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias, 2, dtype, None, None, a.q_norm.weight, a.q_norm.bias,
                              a.k_norm.weight, a.k_norm.bias, 1e-5)
    assert torch.equal(y2, y)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_block_module_vs_reference_fixture(dtype):
    """the Block module (qk_norm, init_values 0.5, eps 1e-6) against the reference's Block of op_block_qknorm.npz: HF.BlockFn, then the
    unfused expression through HF.AttentionFn, then the class-row tail"""
    BB, _ = _mods()
    g = load_golden("op_block_qknorm.npz")
    blk = BB.Block(64, 2, qkv_bias=True, qk_norm=True, init_values=0.5, norm_layer=partial(BB.LayerNorm, eps=1e-6))
    blk.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("w.")})
    blk = blk.to(DEV).train()
    BB.set_compute_dtype(blk, dtype)
    assert blk._fusable() and blk.attn.q_norm.eps == 1e-6
    x = g["x"].to(DEV).requires_grad_(True)
    y = blk(x)
    y.backward(g["gy"].to(DEV, y.dtype))
    tol = TOL[dtype]
    ref = {k[2:]: v for k, v in g.items() if k.startswith("g.")}
    _compare(blk, x, y, ref, g["gx"], g["y"], tol)
    _zero(x, blk)
    t = x + blk.ls1(blk.attn(blk.norm1(x)))
    t = t + blk.ls2(blk.mlp(blk.norm2(t)))
    t.backward(g["gy"].to(DEV, t.dtype))
    _compare(blk, x, t, ref, g["gx"], g["y"], tol)
    # the class-row tail (HF.TailBlockFn), forward and backward: the fixture's gradients for an output gradient that is zero outside token 0
    _zero(x, blk)
    yc = blk.forward_class_rows(x)
    yc.backward(g["gy"][:, 0].to(DEV, yc.dtype).contiguous())
    assert tuple(yc.shape) == (2, 64)
    _compare(blk, x, yc, {k[5:]: v for k, v in g.items() if k.startswith("gcls.")}, g["gx_cls"], g["y"][:, 0], tol)


COMBOS = {"qk_norm": dict(), "qk_norm+drop_path+dropout+init_values": dict(init_values=0.5), "qk_norm-no-qkv-bias": dict(qkv_bias=False)}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_block_vs_fp64(cfg, combo, dtype):
    """HF.BlockFn against the float64 Block; with drop path (sample 1 dropped in both branches), proj_drop / Mlp.drop with recorded seeds
    and LayerScale on the same Block; without a qkv bias; two runs and activation checkpointing give the same bits"""
    D, H, N = CONFIGS[cfg]
    if dtype == torch.bfloat16:                                       # precondition: the shapes do cover both attention routes
        streams = [_route(n, h, d // h, dtype, True).startswith("stream") for d, h, n in (CONFIGS["D128-N197"], CONFIGS["D64-N300"])]
        assert streams == [False, True], streams
    blk = _make_block(D, H, 3, dtype, **COMBOS[combo])
    x, gy = _input(D, N, 4, dtype)
    x.requires_grad_(True)
    full = "drop_path" in combo
    s1 = s2 = torch.tensor([2.0, 0.0, 2.0, 2.0], device=DEV) if full else None
    drop = (P_DROP,) + SEEDS if full else None
    y = _run(blk, x, s1, s2, drop)
    y.backward(gy)
    assert y.dtype == dtype
    P = QR.p64(blk.named_parameters())
    assert all(k in P for k in QK) and ("attn.qkv.bias" in P) == ("no-qkv-bias" not in combo)
    x64 = x.detach().double().requires_grad_(True)
    y64 = QR.block64_qkn(x64, P, H, 1e-6, s1, s2, *_masks(N, D, full))
    y64.backward(gy.double())
    _compare(blk, x, y, {k: v.grad for k, v in P.items()}, x64.grad, y64, TOL[dtype])
    g0, dx0 = _grads(blk), x.grad.clone()
    for recompute in (False, True):
        _zero(x, blk)
        y1 = _run(blk, x, s1, s2, drop, recompute=recompute)
        y1.backward(gy)
        assert torch.equal(y1, y) and torch.equal(x.grad, dx0), recompute
        for k, g in _grads(blk).items():
            assert torch.equal(g, g0[k]), (k, recompute)
    if full:
        assert torch.equal(y[1], x[1]) and torch.equal(x.grad[1], gy[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("combo", ["qk_norm", "qk_norm+drop_path+dropout+init_values"])
def test_tail_block_class_rows(combo, dtype):
    """HF.TailBlockFn: the whole qkv buffer is normalised, then the class rows run; against float64 with dx and every gradient, equal to the
    dense Block's class rows, bit-identical under checkpointing"""
    D, H, N = CONFIGS["D64-N10"]
    blk = _make_block(D, H, 8, dtype, **COMBOS[combo])
    x, gy = _input(D, N, 9, dtype)
    gy = gy[:, 0].contiguous()
    x.requires_grad_(True)
    full = "drop_path" in combo
    s1 = s2 = torch.tensor([2.0, 0.0, 2.0, 2.0], device=DEV) if full else None
    drop = (P_DROP,) + SEEDS if full else None
    y = _run_tail(blk, x, s1, s2, drop)
    y.backward(gy)
    assert tuple(y.shape) == (B, D)
    P = QR.p64(blk.named_parameters())
    x64 = x.detach().double().requires_grad_(True)
    y64 = QR.block64_qkn(x64, P, H, 1e-6, s1, s2, *_masks(N, D, full))[:, 0]
    y64.backward(gy.double())
    _compare(blk, x, y, {k: v.grad for k, v in P.items()}, x64.grad, y64, TOL[dtype])
    with torch.no_grad():
        assert rel_err(y.float(), _run(blk, x, s1, s2, drop)[:, 0].double()) < TOL[dtype]
    g0, dx0 = _grads(blk), x.grad.clone()
    _zero(x, blk)
    y2 = _run_tail(blk, x, s1, s2, drop, recompute=True)
    y2.backward(gy)
    assert torch.equal(y2, y) and torch.equal(x.grad, dx0)
    for k, g in _grads(blk).items():
        assert torch.equal(g, g0[k]), k


# The [D]-shaped parameters of a Block, in the groups that are frozen one at a time below (the qk_norm ones are [head_dim], alike among
# themselves): a gradient that the node files under the wrong argument has the right shape, so only the parameter it lands on can tell.
FROZEN = {"norm1": ("norm1.weight", "norm1.bias"), "norm2": ("norm2.weight", "norm2.bias"), "exit-biases": ("attn.proj.bias", "mlp.fc2.bias"),
          "gammas": ("ls1.gamma", "ls2.gamma"), "qk_norms": QK}
_FROZEN_CASES = {}


def _frozen_case(dtype, tail):
    """the all-features Block at B = 2 (sample 1 dropped in both branches) and its float64 gradients, built once per dtype and node"""
    if (dtype, tail) not in _FROZEN_CASES:
        D, H, N = CONFIGS["D64-N10"]
        blk = _make_block(D, H, 30, dtype, init_values=0.5)
        x, gy = _input(D, N, 31, dtype, 2)
        gy = gy[:, 0].contiguous() if tail else gy
        s = torch.tensor([2.0, 0.0], device=DEV)
        P = QR.p64(blk.named_parameters())
        x64 = x.double().requires_grad_(True)
        y64 = QR.block64_qkn(x64, P, H, 1e-6, s, s, *_masks(N, D, True, 2))
        y64 = y64[:, 0] if tail else y64
        y64.backward(gy.double())
        _FROZEN_CASES[dtype, tail] = (blk, x, gy, s, {k: v.grad for k, v in P.items()}, x64.grad, y64.detach())
    return _FROZEN_CASES[dtype, tail]


@pytest.mark.parametrize("recompute", [False, True], ids=["keep", "recompute"])
@pytest.mark.parametrize("tail", [False, True], ids=["BlockFn", "TailBlockFn"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_frozen_parameter_groups_get_no_gradient_and_the_rest_is_right(dtype, tail, recompute):
    """qk_norm, LayerScale, drop path and dropout on one Block; one group of same-shaped parameters at a time does not require a gradient:
    it gets none, and the output, dx and every other gradient meet the file's bound against float64, as with nothing frozen"""
    blk, x, gy, s, ref, dx64, y64 = _frozen_case(dtype, tail)
    tol = TOL[dtype]
    run = _run_tail if tail else _run
    for group, names in FROZEN.items():
        xg = x.clone().requires_grad_(True)
        for k, p in blk.named_parameters():
            p.requires_grad_(k not in names)
            p.grad = None
        try:
            y = run(blk, xg, s, s, (P_DROP,) + SEEDS, recompute=recompute)
            y.backward(gy)
            _mods()[1].flush_wgrads()
        finally:
            for p in blk.parameters():
                p.requires_grad_(True)
        assert rel_err(y.float(), y64) < tol, group
        assert rel_err(xg.grad.float(), dx64) < tol, group
        for k, p in blk.named_parameters():
            if k in names:
                assert p.grad is None, (group, k)
            else:
                assert p.grad is not None and p.grad.dtype == torch.float32, (group, k)
                assert _grad_err(k, p.grad, ref) < tol, (group, k)


def _record_ops(monkeypatch, HF):
    """every call the nodes make into the operator layer, by name (not the calls the operator layer makes into itself)"""
    seen, depth = [], [0]

    def wrap(f, n):
        def call(*a, **k):
            if depth[0] == 0:
                seen.append(n)
            depth[0] += 1
            try:
                return f(*a, **k)
            finally:
                depth[0] -= 1
        return call
    for name in dir(HF.ops):
        fn = getattr(HF.ops, name)
        if callable(fn) and not name.startswith("_") and getattr(fn, "__module__", "") == HF.ops.__name__:
            monkeypatch.setattr(HF.ops, name, wrap(fn, name))
    return seen


def test_block_without_qk_norm_issues_the_launches_it_issued(monkeypatch):
    """qk_norm=False: the module hands the node every optional argument as None, and its operator calls are those of an explicit plain call,
    none of them qk_norm's, and the bits are the same; with qk_norm the same list grows by exactly one qk_norm_fwd behind the qkv GEMM and
    one qk_norm_bwd behind the attention backward (whose bias-gradient shortcut it replaces)"""
    BB, HF = _mods()
    x, gy = _input(64, 10, 21, torch.bfloat16)
    x.requires_grad_(True)
    plain = _make_block(64, 2, 20, torch.bfloat16, qk_norm=False).train()
    plain(x).backward(gy)                                             # the first pass also casts the parameters to their bf16 shadows
    HF.flush_wgrads()
    _zero(x, plain)
    seen = _record_ops(monkeypatch, HF)
    y = plain(x)
    y.backward(gy)
    HF.flush_wgrads()
    mod_calls, dx = list(seen), x.grad.clone()
    del seen[:]
    _zero(x, plain)
    y0 = HF.BlockFn.apply(*_args(plain, x))
    y0.backward(gy)
    HF.flush_wgrads()
    assert mod_calls == seen and not any("qk_norm" in n for n in seen)
    assert torch.equal(y, y0) and torch.equal(x.grad, dx)
    assert mod_calls.count("attention_fwd") == 1 and mod_calls.count("attention_bwd") == 1
    del seen[:]
    blk = _make_block(64, 2, 20, torch.bfloat16).train()
    blk(x).backward(gy)
    HF.flush_wgrads()
    del seen[:]
    blk(x).backward(gy)
    HF.flush_wgrads()
    assert seen.count("qk_norm_fwd") == 1 and seen.count("qk_norm_bwd") == 1
    assert seen[seen.index("qk_norm_fwd") - 1] == "linear_fwd" and seen[seen.index("qk_norm_fwd") + 1] == "attention_fwd"
    assert seen[seen.index("qk_norm_bwd") - 1] == "attention_bwd"
    # under no_grad nothing is saved; with autograd on the un-normalised Q and K are
    saves = []
    real = HF.ops.qk_norm_fwd
    monkeypatch.setattr(HF.ops, "qk_norm_fwd", lambda *a, **k: (saves.append(k.get("save", True)), real(*a, **k))[1])
    with torch.no_grad():
        y_ng = blk(x)
        blk.forward_class_rows(x)
    y_g = blk(x)
    blk.forward_class_rows(x)
    assert saves == [False, False, True, True] and torch.equal(y_ng, y_g)
