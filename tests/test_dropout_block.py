"""Element-wise dropout inside the fused Block, the class-row tail and the stand-alone Attention / Mlp, against a float64 restatement that
applies the numpy masks of tests/dropout_ref.py with the seeds the modules recorded (HipDropout.last_seed):

    x1 = x  + s1[b] * mp * proj(attn(norm1(x))) / keep         y = x1 + s2[b] * m2 * fc2(m1 * gelu(fc1(norm2(x1))) / keep) / keep

Shapes: D = 64, 2 heads, N = 5, B = 3, fp32 and bf16.  Tolerances are those of tests/test_drop_path_block.py for the same Block, which
takes them from tests/test_hip_ops.py: conftest.rel_err (max |a - b| / max |b|) < 1e-3 in fp32, 3e-2 in bf16; a wrong mask changes a fifth
of the elements by their whole value and misses them by two orders of magnitude (checked below with the seeds swapped).  Exact
statements: activation checkpointing reproduces output and gradients bit for bit; rate 0 and eval() give the bits of a Block built
without dropout.  The class-row tail against the dense Block: the pooled bound of tests/test_tail_rows.py (per element
err_tail <= err_dense + R max|ref|, R the dense path's worst relative error over the tensors of the case), around the float64 reference."""
import pytest
import torch
import torch.nn.functional as F

import dropout_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.float32: 1e-3, torch.bfloat16: 3e-2}
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
D, H, N, B = 64, 2, 5, 3
P_DROP = 0.2


def _mods():
    from UCF_VIT.simple import building_blocks as BB
    from UCF_VIT._hip import functional as HF
    return BB, HF


def _perturb_norms(blk):
    with torch.no_grad():
        for n in (blk.norm1, blk.norm2):
            n.weight.add_(0.2 * torch.randn(D))
            n.bias.add_(0.2 * torch.randn(D))


def _make_block(seed, dtype, **kw):
    BB, _ = _mods()
    torch.manual_seed(seed)
    blk = BB.Block(D, H, qkv_bias=True, **kw)
    _perturb_norms(blk)
    blk = blk.to(DEV)
    BB.set_compute_dtype(blk, dtype)
    return blk


def _input(seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, D, generator=g).to(DEV, dtype), torch.randn(B, N, D, generator=g).to(DEV, dtype)


def _mask(seed, width, p, shape=(B, N)):
    """the mask of a dense [B N, width] matrix as float64 [B, N, width] with 1 / keep folded in"""
    m = torch.from_numpy(R.keep_mask(seed, shape[0] * shape[1], width, p)).to(DEV).double()
    return m.view(*shape, width) * R.inv_keep(p)


def _p64(mod):
    return {k: p.detach().double().requires_grad_(True) for k, p in mod.named_parameters()}


def attn64(h, P, pre=""):
    Bn, Nn, Dn = h.shape
    qkv = (h @ P[pre + "qkv.weight"].T + P[pre + "qkv.bias"]).view(Bn, Nn, 3, H, Dn // H).permute(2, 0, 3, 1, 4)
    att = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * (Dn // H) ** -0.5, dim=-1)
    o = (att @ qkv[2]).transpose(1, 2).reshape(Bn, Nn, Dn)
    return o @ P[pre + "proj.weight"].T + P[pre + "proj.bias"]


def mlp64(h, P, m1, pre=""):
    a = F.gelu(h @ P[pre + "fc1.weight"].T + P[pre + "fc1.bias"]) * m1
    return a @ P[pre + "fc2.weight"].T + P[pre + "fc2.bias"]


def block64(x, P, eps, s1, s2, mp, m1, m2):
    one = torch.ones(x.shape[0], dtype=torch.float64, device=x.device)
    s1 = (one if s1 is None else s1.double())[:, None, None]
    s2 = (one if s2 is None else s2.double())[:, None, None]
    x1 = x + s1 * mp * attn64(F.layer_norm(x, (D,), P["norm1.weight"], P["norm1.bias"], eps), P, "attn.")
    return x1 + s2 * m2 * mlp64(F.layer_norm(x1, (D,), P["norm2.weight"], P["norm2.bias"], eps), P, m1, "mlp.")


def _seeds(blk):
    return blk.attn.proj_drop.last_seed, blk.mlp.drop1.last_seed, blk.mlp.drop2.last_seed


def _scales(blk):
    return tuple(getattr(d, "last_scale", None) for d in (blk.drop_path1, blk.drop_path2))


def _grads(mod):
    return {k: p.grad.clone() for k, p in mod.named_parameters()}


def _zero(mod, x):
    x.grad = None
    for p in mod.parameters():
        p.grad = None


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("drop_path", [0.0, 0.5], ids=["dropout", "dropout+drop_path"])
def test_block_vs_fp64_and_checkpointing(drop_path, dtype):
    blk = _make_block(3, dtype, proj_drop=P_DROP, drop_path=drop_path).train()
    x, gy = _input(4, dtype)
    x.requires_grad_(True)
    torch.manual_seed(21)
    y = blk(x)
    y.backward(gy)
    assert y.dtype == dtype
    sp, sd1, sd2 = _seeds(blk)
    assert len({sp, sd1, sd2}) == 3
    s1, s2 = _scales(blk)
    assert (s1 is not None) == (drop_path > 0)
    P = _p64(blk)
    x64 = x.detach().double().requires_grad_(True)
    masks = (_mask(sp, D, P_DROP), _mask(sd1, 4 * D, P_DROP), _mask(sd2, D, P_DROP))
    y64 = block64(x64, P, blk.norm1.eps, s1, s2, *masks)
    y64.backward(gy.double())
    tol = TOL[dtype]
    assert rel_err(y.float(), y64) < tol
    assert rel_err(x.grad.float(), x64.grad) < tol
    for k, p in blk.named_parameters():                             # the four bias gradients among them
        assert p.grad is not None and p.grad.dtype == torch.float32, k
        assert rel_err(p.grad, P[k].grad) < tol, k
    # the tolerance tells masks apart: the float64 reference under the seeds of the wrong sites is far off
    with torch.no_grad():
        swapped = block64(x64, P, blk.norm1.eps, s1, s2, _mask(sd2, D, P_DROP), _mask(sp, 4 * D, P_DROP), _mask(sd1, D, P_DROP))
    assert rel_err(y.float(), swapped) > tol
    # activation checkpointing: the seeds are kept with the input, the recomputed forward regenerates the masks
    g0, dx0 = _grads(blk), x.grad.clone()
    _zero(blk, x)
    blk.activation_checkpointing = True
    torch.manual_seed(21)
    y2 = blk(x)
    y2.backward(gy)
    assert _seeds(blk) == (sp, sd1, sd2)
    assert torch.equal(y2, y) and torch.equal(x.grad, dx0)
    for k, g in _grads(blk).items():
        assert torch.equal(g, g0[k]), k


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attention_and_mlp_modules_vs_fp64(dtype):
    BB, _ = _mods()
    tol = TOL[dtype]
    torch.manual_seed(5)
    att = BB.Attention(D, num_heads=H, qkv_bias=True, proj_drop=P_DROP).to(DEV).train()
    mlp = BB.Mlp(D, 4 * D, drop=P_DROP).to(DEV).train()
    BB.set_compute_dtype(att, dtype), BB.set_compute_dtype(mlp, dtype)
    x, gy = _input(6, dtype)
    for mod in (att, mlp):
        xi = x.detach().clone().requires_grad_(True)
        torch.manual_seed(22)
        y = mod(xi)
        y.backward(gy)
        Pm = _p64(mod)
        x64 = xi.detach().double().requires_grad_(True)
        if mod is att:
            y64 = _mask(att.proj_drop.last_seed, D, P_DROP) * attn64(x64, Pm)
        else:
            assert mlp.drop1.last_seed != mlp.drop2.last_seed
            y64 = _mask(mlp.drop2.last_seed, D, P_DROP) * mlp64(x64, Pm, _mask(mlp.drop1.last_seed, 4 * D, P_DROP))
        y64.backward(gy.double())
        assert y.dtype == dtype and rel_err(y.float(), y64) < tol
        assert rel_err(xi.grad.float(), x64.grad) < tol
        for k, p in mod.named_parameters():
            assert rel_err(p.grad, Pm[k].grad) < tol, k
        assert float((y == 0).float().mean()) > 0.1                 # a fifth of the output is masked
    # Mlp with a rate on one site only: drop = (p, 0) masks the activation and leaves the output alone
    torch.manual_seed(7)
    one = BB.Mlp(D, 4 * D, drop=(P_DROP, 0.0)).to(DEV).train()
    BB.set_compute_dtype(one, dtype)
    y = one(x)
    assert one.drop2.last_seed is None and one.drop1.last_seed is not None
    with torch.no_grad():
        y64 = mlp64(x.double(), _p64(one), _mask(one.drop1.last_seed, 4 * D, P_DROP))
    assert rel_err(y.float(), y64) < tol


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("drop_path", [0.0, 0.5], ids=["dropout", "dropout+drop_path"])
def test_class_rows_equal_the_dense_block(drop_path, dtype):
    """forward_class_rows(x) against forward(x)[:, 0] under the same torch.manual_seed (so the same seeds and scales): the tail passes
    row_step = N and draws the dense Block's masks.  Both against float64, pooled bound of tests/test_tail_rows.py."""
    blk = _make_block(8, dtype, proj_drop=P_DROP, drop_path=drop_path).train()
    x, gy = _input(9, dtype)
    gy = gy[:, 0].contiguous()
    runs = {}
    for name in ("dense", "tail"):
        xi = x.detach().clone().requires_grad_(True)
        torch.manual_seed(23)
        y = blk(xi)[:, 0] if name == "dense" else blk.forward_class_rows(xi)
        assert tuple(y.shape) == (B, D)
        y.backward(gy)
        runs[name] = dict(_grads(blk), y=y.detach(), dx=xi.grad.clone(), seeds=_seeds(blk), scales=_scales(blk))
        _zero(blk, xi)
    assert runs["dense"]["seeds"] == runs["tail"]["seeds"]
    sp, sd1, sd2 = runs["tail"]["seeds"]
    s1, s2 = runs["tail"]["scales"]
    if s1 is not None:
        assert torch.equal(s1, runs["dense"]["scales"][0]) and torch.equal(s2, runs["dense"]["scales"][1])
    P = _p64(blk)
    x64 = x.detach().double().requires_grad_(True)
    y64 = block64(x64, P, blk.norm1.eps, s1, s2, _mask(sp, D, P_DROP), _mask(sd1, 4 * D, P_DROP), _mask(sd2, D, P_DROP))[:, 0]
    y64.backward(gy.double())
    ref = dict({k: v.grad for k, v in P.items()}, y=y64.detach(), dx=x64.grad)
    Rel = max(float((runs["dense"][k].double() - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref)
    print(f"DROPOUT TAIL R (dense path, worst relative error over tensors) = {Rel:.3e}")
    assert Rel <= (0.1 if dtype == torch.bfloat16 else 1e-3), "premise: the dense path itself is close to the reference"
    for k in ref:
        e_d, e_t = (runs["dense"][k].double() - ref[k]).abs(), (runs["tail"][k].double() - ref[k]).abs()
        scale = float(ref[k].abs().max())
        print(f"DROPOUT TAIL {k}: dense max err {float(e_d.max()):.3e} tail max err {float(e_t.max()):.3e} max|ref| {scale:.3e}")
        bad = e_t > e_d + Rel * scale
        assert not bool(bad.any()), f"{k}: {int(bad.sum())} of {bad.numel()} elements of the tail are further from float64 than the bound"
    # the tolerance tells masks apart: with row_step ignored the class rows would draw the masks of rows 0 .. B - 1 of the dense matrix
    def ignored(seed, width):
        m = _mask(seed, width, P_DROP)
        m[:, 0] = m.view(B * N, width)[:B]
        return m
    with torch.no_grad():
        wrong = block64(x64, P, blk.norm1.eps, s1, s2, ignored(sp, D), ignored(sd1, 4 * D), ignored(sd2, D))[:, 0]
    assert rel_err(runs["tail"]["y"].float(), wrong) > TOL[dtype] > rel_err(runs["tail"]["y"].float(), y64)
    # and the checkpointed tail is the plain tail, bit for bit
    blk.activation_checkpointing = True
    xi = x.detach().clone().requires_grad_(True)
    torch.manual_seed(23)
    y = blk.forward_class_rows(xi)
    y.backward(gy)
    assert torch.equal(y, runs["tail"]["y"]) and torch.equal(xi.grad, runs["tail"]["dx"])
    for k, g in _grads(blk).items():
        assert torch.equal(g, runs["tail"][k]), k


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rate_zero_and_eval_are_the_block_without_dropout(dtype):
    BB, HF = _mods()
    ref = _make_block(12, dtype)
    x, gy = _input(13, dtype)

    def run(blk, fn):
        xi = x.detach().clone().requires_grad_(True)
        y = fn(blk, xi)
        y.backward(gy if y.dim() == 3 else gy[:, 0].contiguous())
        HF.flush_wgrads()
        out = dict(_grads(blk), y=y.detach(), dx=xi.grad.clone())
        _zero(blk, xi)
        return out

    for fn in (lambda b, t: b(t), lambda b, t: b.forward_class_rows(t)):
        want = run(ref.train(), fn)
        for kw, mode in ((dict(proj_drop=0.0), "train"), (dict(proj_drop=0.3), "eval")):
            blk = _make_block(12, dtype, **kw)
            blk.load_state_dict(ref.state_dict())
            got = run(blk.train() if mode == "train" else blk.eval(), fn)
            for k in want:
                assert torch.equal(got[k], want[k]), (kw, mode, k)
            assert _seeds(blk) == (None, None, None)               # nothing was drawn
    # stand-alone modules: inactive dropout is the input itself, the Functions run without a dropout argument
    d = BB.HipDropout(0.3).eval()
    assert d(x) is x
    d.train()
    torch.manual_seed(3)
    y = d(x)
    m = _mask(d.last_seed, D, 0.3)
    assert y.dtype == dtype and rel_err(y.float(), m * x.double()) < 2.0 ** -8
    xi = x.detach().clone().requires_grad_(True)
    d(xi).backward(gy)
    assert rel_err(xi.grad.float(), _mask(d.last_seed, D, 0.3) * gy.double()) < 2.0 ** -8
    one = BB.HipDropout(1.0).train()
    assert torch.equal(one(x), torch.zeros_like(x))                  # p == 1: zeros, no mask needed
