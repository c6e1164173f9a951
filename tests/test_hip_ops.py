"""GPU parity tests of the HIP operators (through the C ABI) against the reference-generated golden vectors and the
CPU oracle.  fp32 mode: tolerances of SURVEY.md §8a (1e-3 rel GEMM/attention ops, 1e-4 LayerNorm, bit-exact gathers);
bf16 mode: same inputs, 2e-2 rel (bf16 has 8 mantissa bits; compared against the fp32 reference)."""
from functools import partial

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {torch.float32: 1e-3, torch.bfloat16: 3e-2}


def _mods():
    from UCF_VIT.simple import building_blocks as BB
    return BB


def load_w(mod, g, prefix="w."):
    mod.load_state_dict({k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)})
    return mod.to(DEV)


# ---------------------------------------------------------------------------------------------- raw GEMM
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(394, 192, 64), (128, 128, 128), (130, 72, 200), (33, 40, 24), (788, 1024, 256), (5, 2, 64)])
def test_gemm_layouts_and_epilogues(dtype, M, N, K):
    from UCF_VIT._hip import ops
    from UCF_VIT._hip.lib import ACT_GELU, ACT_GELU_GRAD, LAYOUT_KC, LAYOUT_KS
    gen = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = torch.randn(M, K, generator=gen)
    W = torch.randn(N, K, generator=gen) * 0.2
    bias = torch.randn(N, generator=gen)
    res = torch.randn(M, N, generator=gen)
    Ad, Wd, bd, rd = (t.to(DEV, dtype) for t in (A, W, bias, res))
    A64, W64, b64, r64 = (t.to(dtype).double() for t in (A, W, bias, res))   # reference sees the same rounded inputs
    tol = TOL[dtype]
    # forward: KC x KC, bias + residual
    y = ops.linear_fwd(Ad, Wd, bd, residual=rd)
    assert rel_err(y.float(), A64 @ W64.T + b64 + r64) < tol
    # forward with GELU and saved pre-activation
    h = torch.empty(M, N, dtype=dtype, device=DEV)
    y = ops.linear_fwd(Ad, Wd, bd, act=ACT_GELU, aux_out=h)
    pre = A64 @ W64.T + b64
    assert rel_err(h.float(), pre) < tol
    assert rel_err(y.float(), torch.nn.functional.gelu(pre)) < tol
    # dgrad: KC x KS  (dy[M,N] @ W[N,K]), with gelu' fused
    dy = torch.randn(M, N, generator=gen)
    dyd, dy64 = dy.to(DEV, dtype), dy.to(dtype).double()
    dx = ops.linear_dgrad(dyd, Wd)
    assert rel_err(dx.float(), dy64 @ W64) < tol
    if K % 4 == 0:
        aux = torch.randn(M, K, generator=gen)
        auxd, aux64 = aux.to(DEV, dtype), aux.to(dtype).double().requires_grad_(True)
        torch.nn.functional.gelu(aux64).sum().backward()
        dx = ops.linear_dgrad(dyd, Wd, act_grad_aux=auxd)
        assert rel_err(dx.float(), (dy64 @ W64) * aux64.grad) < tol
    # wgrad: KS x KS (dy^T @ A) -> fp32, then accumulate
    dw = ops.linear_wgrad(dyd, Ad)
    assert dw.dtype == torch.float32
    assert rel_err(dw, dy64.T @ A64) < tol
    ops.linear_wgrad(dyd, Ad, out=dw, accumulate=True)
    assert rel_err(dw, 2 * (dy64.T @ A64)) < tol
    # bias gradient
    db = ops.colsum(dyd)
    assert rel_err(db, dy64.sum(0)) < (1e-5 if dtype == torch.float32 else 1e-5)


def test_gemm_f32_is_exact_fp32():
    """fp32 MFMA path is an fmaf chain: agreement with an fp64 reference to ~1e-6 relative"""
    from UCF_VIT._hip import ops
    gen = torch.Generator().manual_seed(1)
    A, W = torch.randn(256, 512, generator=gen), torch.randn(384, 512, generator=gen)
    y = ops.linear_fwd(A.to(DEV), W.to(DEV))
    assert rel_err(y, A.double() @ W.double().T) < 5e-6


# ---------------------------------------------------------------------------------------------- module-level operators
def run_module(mod, g, dtype):
    BB = _mods()
    BB.set_compute_dtype(mod, dtype)
    x = g["x"].to(DEV).requires_grad_(True)
    y = mod(x)
    y.backward(g["gy"].to(DEV, y.dtype))
    return x, y


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name,make", [
    ("op_mlp.npz", lambda BB: BB.Mlp(in_features=64, hidden_features=256)),
    ("op_attn_none.npz", lambda BB: BB.Attention(64, num_heads=2, qkv_bias=True)),
    ("op_attn_default.npz", lambda BB: BB.Attention(64, num_heads=2, qkv_bias=True)),
    ("op_attn_n197_dh64.npz", lambda BB: BB.Attention(128, num_heads=2, qkv_bias=True)),
    ("op_block.npz", lambda BB: BB.Block(64, 2, qkv_bias=True, norm_layer=partial(BB.LayerNorm, eps=1e-6))),
    ("op_layernorm.npz", lambda BB: BB.LayerNorm(64, eps=1e-6)),
])
def test_operator_vs_reference(name, make, dtype):
    g = load_golden(name)
    mod = load_w(make(_mods()), g)
    x, y = run_module(mod, g, dtype)
    tol = TOL[dtype] if "layernorm" not in name or dtype == torch.bfloat16 else 1e-4
    assert y.dtype == dtype
    assert rel_err(y.float(), g["y"]) < tol
    assert rel_err(x.grad.float(), g["gx"]) < tol
    for k, p in mod.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32, k
        assert rel_err(p.grad, g["g." + k]) < tol, k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name,kw", [
    ("op_patch2d.npz", dict(img_size=[32, 32], patch_size=8, in_chans=3, embed_dim=64, twoD=True)),
    ("op_patch3d.npz", dict(img_size=[16, 16, 8], patch_size=4, in_chans=1, embed_dim=48, twoD=False)),
])
def test_patch_embed_vs_reference(name, kw, dtype):
    BB = _mods()
    g = load_golden(name)
    mod = load_w(BB.PatchEmbed(**kw), g)
    BB.set_compute_dtype(mod, dtype)
    y = mod(g["x"].to(DEV))
    y.backward(g["gy"].to(DEV, y.dtype))
    tol = TOL[dtype]
    assert rel_err(y.float(), g["y"]) < tol
    for k, p in mod.named_parameters():
        assert rel_err(p.grad, g["g." + k]) < tol, k


def test_im2col_is_exact():
    from UCF_VIT._hip import ops
    x = torch.randn(2, 3, 32, 48)
    cols = ops.im2col(x.to(DEV), 8, torch.float32).cpu()
    ref = x.reshape(2, 3, 4, 8, 6, 8).permute(0, 2, 4, 1, 3, 5).reshape(2 * 24, 3 * 64)
    assert torch.equal(cols, ref)
    x3 = torch.randn(1, 2, 8, 8, 12)
    cols = ops.im2col(x3.to(DEV), 4, torch.float32).cpu()
    ref = x3.reshape(1, 2, 2, 4, 2, 4, 3, 4).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(12, 2 * 64)
    assert torch.equal(cols, ref)


# ---------------------------------------------------------------------------------------------- MAE index math (bit-exact)
def test_mae_masking_bit_exact_vs_reference():
    from UCF_VIT._hip import functional as HF
    g = load_golden("mae_masking.npz")
    kept, mask, ids = HF.RandomMaskFn.apply(g["seq"].to(DEV), g["noise"].to(DEV), 49)
    assert ids.dtype == torch.int64 and torch.equal(ids.cpu(), g["ids_restore"])
    assert torch.equal(mask.cpu(), g["mask"])
    assert torch.equal(kept.cpu(), g["kept"])


@pytest.mark.parametrize("B,L,D,ratio", [(3, 196, 1024, 0.75), (2, 64, 40, 0.5), (1, 1000, 8, 0.9), (2, 16, 64, 0.0)])
def test_mae_masking_properties(B, L, D, ratio):
    """size-independent properties: ids_restore is a permutation, mask has exactly L-len_keep ones, gather/scatter adjoint"""
    from UCF_VIT._hip import functional as HF
    gen = torch.Generator().manual_seed(L)
    seq = torch.randn(B, L, D, generator=gen).to(DEV).requires_grad_(True)
    noise = torch.rand(B, L, generator=gen).to(DEV)
    len_keep = int(L * (1 - ratio))
    kept, mask, ids = HF.RandomMaskFn.apply(seq, noise, len_keep)
    assert torch.equal(torch.sort(ids, dim=1).values, torch.arange(L, device=DEV).expand(B, L))
    assert torch.equal(mask.sum(1), torch.full((B,), float(L - len_keep), device=DEV))
    ref_shuffle = torch.argsort(noise.cpu(), dim=1)
    assert torch.equal(ids.cpu(), torch.argsort(ref_shuffle, dim=1))
    assert torch.equal(kept.detach().cpu(), torch.gather(seq.detach().cpu(), 1, ref_shuffle[:, :len_keep, None].expand(-1, -1, D)))
    gk = torch.randn_like(kept)
    kept.backward(gk)
    ref = torch.zeros(B, L, D)
    ref.scatter_(1, ref_shuffle[:, :len_keep, None].expand(-1, -1, D), gk.cpu())
    assert torch.equal(seq.grad.cpu(), ref)


def test_mae_masking_ties_are_stable():
    from UCF_VIT._hip import ops
    noise = torch.tensor([[0.5, 0.1, 0.5, 0.1, 0.9, 0.5]], device=DEV)
    shuffle, restore, mask = ops.mae_mask(noise, 3)
    assert shuffle.cpu().tolist() == [[1, 3, 0, 2, 5, 4]]
    assert restore.cpu().tolist() == [[2, 0, 3, 1, 5, 4]]
    assert mask.cpu().tolist() == [[0.0, 0.0, 1.0, 0.0, 1.0, 1.0]]


# ---------------------------------------------------------------------------------------------- losses / optimizer
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cross_entropy(dtype):
    from UCF_VIT._hip import functional as HF
    gen = torch.Generator().manual_seed(3)
    logits = (torch.randn(37, 1000, generator=gen) * 3).to(dtype)
    labels = torch.randint(0, 1000, (37,), generator=gen)
    ref_in = logits.float().clone().requires_grad_(True)
    ref = torch.nn.CrossEntropyLoss()(ref_in, labels)
    ref.backward()
    x = logits.to(DEV).requires_grad_(True)
    loss = HF.cross_entropy(x, labels.to(DEV))
    loss.backward()
    assert abs(loss.item() - ref.item()) < 1e-4 * abs(ref.item())
    assert rel_err(x.grad.float(), ref_in.grad) < (1e-4 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("masked", [False, True])
def test_patch_mse(masked):
    from UCF_VIT._hip import functional as HF
    from oracle import ucf_vit_ref as R
    gen = torch.Generator().manual_seed(4)
    img = torch.randn(3, 3, 32, 48, generator=gen)
    pred = torch.randn(3, 24, 192, generator=gen)
    mask = (torch.rand(3, 24, generator=gen) > 0.25).float() if masked else None
    pr = pred.clone().requires_grad_(True)
    tgt = R.patchify(img, 8)
    ref = R.masked_mse(pr, tgt, mask) if masked else torch.nn.MSELoss()(pr, tgt)
    ref.backward()
    pd = pred.to(DEV).requires_grad_(True)
    loss = HF.patch_mse(pd, img.to(DEV), 8, mask.to(DEV) if masked else None)
    loss.backward()
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    assert rel_err(pd.grad, pr.grad) < 1e-5


def test_adamw_matches_torch():
    from UCF_VIT._hip import ops
    gen = torch.Generator().manual_seed(5)
    n = 1003
    p0, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    pr = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pr], lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-2)
    pd = p0.clone().to(DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sh = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    for step in range(1, 4):
        pr.grad = g * step
        opt.step()
        ops.adamw(pd, (g * step).to(DEV), m, v, sh, 1e-3, 0.9, 0.95, 1e-8, 1e-2, step)
    assert rel_err(pd, pr.detach()) < 1e-6
    assert torch.equal(sh.cpu(), pd.cpu().to(torch.bfloat16))


def test_cpu_tensor_is_rejected_loudly():
    BB = _mods()
    mod = BB.Mlp(in_features=64, hidden_features=256)
    with pytest.raises(RuntimeError):
        mod(torch.randn(2, 4, 64))


# ---------------------------------------------------------------------------------------------- large-tile bf16 GEMM (v2 kernel)
@pytest.mark.parametrize("M,N,K", [(3428, 4096, 128), (1000, 512, 256), (2500, 264, 192), (3400, 4096, 200), (700, 384, 136)])
def test_gemm_v2_tiles_edges_epilogues(M, N, K):
    """256x256 (first shape) and 128x128 tile configs, ragged M/N edges, every operand layout and epilogue, vs fp64"""
    from UCF_VIT._hip import ops
    from UCF_VIT._hip.lib import ACT_GELU
    dtype = torch.bfloat16
    gen = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=gen)
    W = torch.randn(N, K, generator=gen) * 0.2
    bias, res = torch.randn(N, generator=gen), torch.randn(M, N, generator=gen)
    Ad, Wd, bd, rd = (t.to(DEV, dtype) for t in (A, W, bias, res))
    A64, W64, b64, r64 = (t.to(dtype).double() for t in (A, W, bias, res))
    y = ops.linear_fwd(Ad, Wd, bd, residual=rd)
    assert rel_err(y.float(), A64 @ W64.T + b64 + r64) < 1e-2
    h = torch.empty(M, N, dtype=dtype, device=DEV)
    y = ops.linear_fwd(Ad, Wd, bd, act=ACT_GELU, aux_out=h)
    pre = A64 @ W64.T + b64
    assert rel_err(h.float(), pre) < 1e-2 and rel_err(y.float(), torch.nn.functional.gelu(pre)) < 1e-2
    dy = torch.randn(M, N, generator=gen)
    dyd, dy64 = dy.to(DEV, dtype), dy.to(dtype).double()
    dx = ops.linear_dgrad(dyd, Wd)
    assert rel_err(dx.float(), dy64 @ W64) < 1e-2
    aux = torch.randn(M, K, generator=gen)
    auxd, aux64 = aux.to(DEV, dtype), aux.to(dtype).double().requires_grad_(True)
    torch.nn.functional.gelu(aux64).sum().backward()
    dx = ops.linear_dgrad(dyd, Wd, act_grad_aux=auxd)
    assert rel_err(dx.float(), (dy64 @ W64) * aux64.grad) < 1e-2


@pytest.mark.parametrize("M", [512, 49152])
def test_gemm_bf16_gelu_epilogue_accuracy(M):
    """fused erf-GELU / GELU' epilogues of the bf16 GEMM (erfc by Abramowitz-Stegun 7.1.28, csrc/common.h) against torch's erf in
    fp64.  Identity weights make the GEMM an exact copy, so only the activation math is compared; tolerance: one bf16 ulp
    (2^-8 relative) + 2e-6 absolute.  M=512 runs the 128x128 kernel, M=49152 the 256x256 ping-pong kernel."""
    from UCF_VIT._hip import ops
    from UCF_VIT._hip.lib import ACT_GELU
    D = 256
    gen = torch.Generator().manual_seed(M)
    x = (torch.randn(M, D, generator=gen) * 3.0).bfloat16()
    x[0, :8] = torch.tensor([0.0, -0.0, 1e-4, -1e-4, 30.0, -30.0, 8.0, -8.0]).bfloat16()
    eye = torch.eye(D).bfloat16().to(DEV)
    xd = x.to(DEV)
    x64 = x.double().requires_grad_(True)
    ref = torch.nn.functional.gelu(x64)
    ref.sum().backward()
    h = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
    y = ops.linear_fwd(xd, eye, None, act=ACT_GELU, aux_out=h)
    assert torch.equal(h.cpu(), x)
    err = (y.cpu().double() - ref.detach()).abs()
    assert bool((err <= ref.detach().abs() * 2.0 ** -8 + 2e-6).all()), float(err.max())
    ones = torch.ones(M, D, dtype=torch.bfloat16, device=DEV)
    dx = ops.linear_dgrad(ones, eye, act_grad_aux=xd)
    err = (dx.cpu().double() - x64.grad).abs()
    assert bool((err <= x64.grad.abs() * 2.0 ** -8 + 2e-6).all()), float(err.max())
    # the derivative-saving pair the bf16 MLP uses: forward stores gelu'(pre-activation), backward multiplies by it
    from UCF_VIT._hip.lib import ACT_GELU_SAVE_DERIV
    gd = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
    y2 = ops.linear_fwd(xd, eye, None, act=ACT_GELU_SAVE_DERIV, aux_out=gd)
    err = (y2.cpu().double() - ref.detach()).abs()
    assert bool((err <= ref.detach().abs() * 2.0 ** -8 + 2e-6).all()), float(err.max())
    err = (gd.cpu().double() - x64.grad).abs()
    assert bool((err <= x64.grad.abs() * 2.0 ** -8 + 2e-6).all()), float(err.max())
    two = torch.full((M, D), 2.0, dtype=torch.bfloat16, device=DEV)
    dx2 = ops.linear_dgrad_t(two, eye, act_grad_aux=gd, aux_is_deriv=True)
    assert torch.equal(dx2.float(), gd.float() * 2.0)


@pytest.mark.parametrize("Mtok,N,K", [(25216 // 8, 1024, 1024), (3200, 256, 384), (6400, 3072, 128), (3208, 512, 256), (4136, 1024, 4096), (3302, 1024, 512)])
def test_gemm_v2_wgrad_splitk(Mtok, N, K):
    """weight gradient (KS x KS) with split-K partial sums: fp32 output, overwrite then accumulate"""
    from UCF_VIT._hip import ops
    gen = torch.Generator().manual_seed(N + K)
    dy = torch.randn(Mtok, N, generator=gen).bfloat16()
    x = torch.randn(Mtok, K, generator=gen).bfloat16()
    ref = dy.double().T @ x.double()
    dw = ops.linear_wgrad(dy.to(DEV), x.to(DEV))
    assert rel_err(dw, ref) < 1e-4
    dw2 = ops.linear_wgrad(dy.to(DEV), x.to(DEV))
    assert torch.equal(dw, dw2), "split-K reduction must be deterministic"
    ops.linear_wgrad(dy.to(DEV), x.to(DEV), out=dw, accumulate=True)
    assert rel_err(dw, 2 * ref) < 1e-4


@pytest.mark.parametrize("Mtok,D", [(1000, 256), (3302, 512)])
def test_wgrad_grouped_one_launch(Mtok, D):
    """the four weight gradients of a Block as one grouped persistent launch (ucfvit_gemm_grouped), ragged token count"""
    from UCF_VIT._hip import ops
    gen = torch.Generator().manual_seed(D)
    shapes = [(3 * D, D), (D, D), (4 * D, D), (D, 4 * D)]       # (N_out, K_in) of qkv, proj, fc1, fc2
    items, refs = [], []
    for i, (n, k) in enumerate(shapes):
        dy = torch.randn(Mtok, n, generator=gen).bfloat16()
        x = torch.randn(Mtok, k, generator=gen).bfloat16()
        out = torch.full((n, k), 0.5, dtype=torch.float32, device=DEV) if i == 1 else None     # one problem accumulates
        items.append((dy.to(DEV), x.to(DEV), out, i == 1))
        refs.append(dy.double().T @ x.double() + (0.5 if i == 1 else 0.0))
    outs = ops.wgrad_grouped(items)
    for o, r in zip(outs, refs):
        assert rel_err(o, r) < 1e-4
    outs2 = ops.wgrad_grouped([(a, b, None, False) for a, b, _, _ in items])
    outs3 = ops.wgrad_grouped([(a, b, None, False) for a, b, _, _ in items])
    for a, b in zip(outs2, outs3):
        assert torch.equal(a, b)


@pytest.mark.parametrize("M,Nout,Kc", [(25216, 512, 256), (700, 384, 136)])
def test_dgrad_output_column_sums_byproduct(M, Nout, Kc):
    """dx = (dy·W) * aux with the column sums of dx (= bias gradient of the layer before) as a by-product of the same launch
    (desc.c_colsum_partial + ucfvit_reduce_rows on the 256x256 kernel: first shape, 99 x 2 tiles; separate column-sum pass on the
    second); overwrite, then accumulate.  The sums are taken in fp32 before dx is rounded to bf16."""
    from UCF_VIT._hip import ops
    gen = torch.Generator().manual_seed(M + Nout)
    dy = torch.randn(M, Kc, generator=gen).bfloat16()
    wT = (torch.randn(Nout, Kc, generator=gen) * 0.1).bfloat16()          # transposed weight: dx[M,Nout] = dy[M,Kc]·wT[Nout,Kc]ᵀ
    aux = torch.randn(M, Nout, generator=gen).bfloat16()
    ref = (dy.double() @ wT.double().T) * aux.double()
    cs = torch.full((Nout,), 5.0, device=DEV)
    dx = ops.linear_dgrad_t(dy.to(DEV), wT.to(DEV), act_grad_aux=aux.to(DEV), aux_is_deriv=True, c_colsum=cs)
    assert rel_err(dx.float(), ref) < 1e-2
    assert rel_err(cs, ref.sum(0)) < 2e-3
    ops.linear_dgrad_t(dy.to(DEV), wT.to(DEV), act_grad_aux=aux.to(DEV), aux_is_deriv=True, c_colsum=cs, c_colsum_accumulate=True)
    assert rel_err(cs, 2 * ref.sum(0)) < 2e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gemm_row_padded_operands(dtype):
    """leading dimensions larger than the row length on every matrix of a GEMM: forward with bias + residual, data gradient with the saved-derivative multiply, weight
    gradient; the 256x256, 128x128 and v1 kernels all take lda / ldb / ldc / ldr / ldaux"""
    from UCF_VIT._hip import ops
    from UCF_VIT._hip.lib import ACT_MUL_AUX
    gen = torch.Generator().manual_seed(9)
    for M, K, N in [(50432, 256, 512), (1000, 384, 256), (300, 96, 72)]:
        def padded(r, c, scale=1.0):
            buf = (torch.randn(r, c + 64, generator=gen) * scale).to(dtype).to(DEV)
            return buf[:, :c]
        x, res, aux, dy = padded(M, K), padded(M, N), padded(M, K), padded(M, N)
        w = (torch.randn(N, K, generator=gen) * 0.1).to(dtype).to(DEV)
        b = torch.randn(N, generator=gen).to(dtype).to(DEV)
        tol = 1e-5 if dtype == torch.float32 else 1e-2
        out = padded(M, N)
        ops.linear_fwd(x, w, b, residual=res, out=out)
        ref = x.double() @ w.double().T + b.double() + res.double()
        assert rel_err(out.float(), ref) < tol
        dx = padded(M, K)
        ops.linear_dgrad(dy, w, act_grad_aux=aux, aux_is_deriv=True, out=dx)
        assert rel_err(dx.float(), (dy.double() @ w.double()) * aux.double()) < tol
        dw = ops.linear_wgrad(dy, x)
        assert rel_err(dw, dy.double().T @ x.double()) < (1e-5 if dtype == torch.float32 else 1e-4)


@pytest.mark.parametrize("N,dh", [(197, 64), (196, 32), (120, 64), (100, 32), (50, 64), (17, 32), (208, 32), (230, 64), (230, 32), (256, 64),
                                  (209, 64), (16, 64), (33, 32), (100, 64), (1, 64)])
def test_attention_kernels_all_short_sequence_paths(N, dh):
    """bf16 attention forward + backward against fp32 softmax(QK^T/sqrt(dh))V on the SAME bf16 inputs, over every dispatch of the
    short-sequence kernels: fused resident forward (N <= 208) / resident forward (N <= 256) and the fused backward for 4 / 8 / 13 / 16
    blocks of 16 tokens (two blocks per wave pass: even and odd block counts, a single block, a single token), head dims 64 and 32.
    Tolerance 2e-2 of the largest reference magnitude (bf16 probabilities and outputs).
    The per-element bounds and the exact cases of these kernels live in tests/test_attention_ops.py."""
    from UCF_VIT._hip import ops
    B, H = 3, 2
    gen = torch.Generator().manual_seed(N * 100 + dh)
    qkv = torch.randn(B * N, 3 * H * dh, generator=gen).bfloat16().to(DEV)
    do = torch.randn(B * N, H * dh, generator=gen).bfloat16().to(DEV)
    o, lse = ops.attention_fwd(qkv, B, N, H, dh, dh ** -0.5)
    dqkv = ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, dh ** -0.5)
    ref_in = qkv.float().view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4).contiguous().requires_grad_(True)   # [3, B, H, N, dh]
    q, k, v = ref_in[0], ref_in[1], ref_in[2]
    p = torch.softmax((q @ k.transpose(-1, -2)) * dh ** -0.5, dim=-1)
    ref_o = (p @ v).transpose(1, 2).reshape(B * N, H * dh)
    ref_o.backward(do.float())
    ref_d = ref_in.grad.permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * dh)
    assert rel_err(o.float(), ref_o.detach()) < 2e-2
    assert rel_err(dqkv.float(), ref_d) < 2e-2
    ref_lse = torch.logsumexp((q @ k.transpose(-1, -2)) * dh ** -0.5, dim=-1).detach() * 1.4426950408889634     # kernels keep it in log2
    assert float((lse - ref_lse).abs().max()) < 2e-2


@pytest.mark.parametrize("N,dh,B,H", [(197, 64, 5, 3), (50, 64, 4, 2), (256, 32, 3, 2), (100, 32, 2, 4), (17, 64, 3, 1)])
def test_attention_backward_hands_out_the_qkv_bias_column_sums(N, dh, B, H):
    """ucfvit_attention_bwd_colsum: partial [B, 2 H dh] = dQ summed over each batch element's tokens (from the fp32 gradients before they are
    rounded) and zeros for dK — against the fp32 sums of the bf16 dqkv the same call returns (tolerance: the rounding of N bf16 values per
    column); the two identities the caller relies on for the other thirds hold on the returned gradient itself (column sums of dK = 0 and
    of dV = column sums of dout, up to the rounding of the stored values); the gradient is bit-identical to the call without column sums
    and a second call bit-identical (no atomics).  N > 256 and head dim 128 report 'not supported'."""
    from UCF_VIT._hip import ops
    gen = torch.Generator().manual_seed(N + dh + B)
    D = H * dh
    qkv = torch.randn(B * N, 3 * D, generator=gen).bfloat16().to(DEV)
    do = torch.randn(B * N, D, generator=gen).bfloat16().to(DEV)
    o, lse = ops.attention_fwd(qkv, B, N, H, dh, dh ** -0.5)
    d0 = ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, dh ** -0.5)
    d1, part = ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, dh ** -0.5, want_colsum=True)
    d2, part2 = ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, dh ** -0.5, want_colsum=True)
    assert part is not None and part.shape == (B, 2 * D) and part.dtype == torch.float32
    assert torch.equal(d0, d1) and torch.equal(d1, d2) and torch.equal(part, part2)
    sums = d1.float().view(B, N, 3 * D).sum(1)                       # [B, 3 D] from the rounded gradient
    scale = float(sums.abs().max())
    assert float((part[:, :D] - sums[:, :D]).abs().max()) < 2e-2 * scale + 1e-3
    assert float(part[:, D:].abs().max()) == 0.0
    assert float(sums[:, D:2 * D].abs().max()) < 3e-2 * scale + 1e-3                                   # sum over keys of dK: rounding noise around 0
    assert float((sums[:, 2 * D:] - do.float().view(B, N, D).sum(1)).abs().max()) < 3e-2 * scale + 1e-3  # sum over keys of dV = sum over queries of dO
    assert ops.attention_bwd_colsum_supported(B, N, H, dh, torch.bfloat16)
    assert not ops.attention_bwd_colsum_supported(B, 300, H, dh, torch.bfloat16) and not ops.attention_bwd_colsum_supported(B, N, H, 128, torch.bfloat16)
    assert not ops.attention_bwd_colsum_supported(B, N, H, dh, torch.float32)


@pytest.mark.parametrize("M,N,K", [(665 * 197, 1024, 1024), (4096, 768, 768), (1000, 512, 256), (300, 64, 128)])
def test_plain_data_gradient_column_sums_from_the_epilogue(M, N, K):
    """dx = dy W with c_colsum: the column sums of dx (the V third of the qkv bias gradient when dx = dO) — from the plain epilogue of the
    256 x 256 ping-pong kernel where it runs (the first three shapes), by a separate pass otherwise; against the fp32 sum of the bf16 dx
    returned; the product equals the call without column sums (bit for bit below K = 1024; at K >= 1024 that call runs the staggered
    kernel, whose second wave group adds its K-tiles in rotated order: last-bit differences); accumulate adds"""
    from UCF_VIT._hip import ops
    gen = torch.Generator().manual_seed(M + N + K)
    dy = torch.randn(M, K, generator=gen).bfloat16().to(DEV)
    wT = (torch.randn(N, K, generator=gen) * 0.05).bfloat16().to(DEV)          # dx[M, N] = dy[M, K] . wT[N, K]^T
    dx0 = ops.linear_dgrad_t(dy, wT)
    cs = torch.full((N,), 7.0, dtype=torch.float32, device=DEV)
    dx1 = ops.linear_dgrad_t(dy, wT, c_colsum=cs)
    assert torch.equal(dx0, dx1) if K < 1024 else rel_err(dx1.float(), dx0.float()) < 4e-3
    want = dx1.float().sum(0)
    assert rel_err(cs, want) < 5e-3
    ops.linear_dgrad_t(dy, wT, c_colsum=cs, c_colsum_accumulate=True)
    assert rel_err(cs, 2 * want) < 5e-3


# ---------------------------------------------------------------------------------------------- adaptive-patching front end
@pytest.mark.parametrize("B,C,S,P", [(2, 3, 12, 64), (3, 1, 50, 256), (1, 4, 7, 27), (2, 3, 196, 256)])
def test_seq_patches_is_an_exact_rearrangement(B, C, S, P):
    """einops 'b c s p -> b s (p c)' (arch.py:466): bit-exact in fp32, one rounding in bf16"""
    from UCF_VIT._hip import ops
    x = torch.randn(B, C, S, P, generator=torch.Generator().manual_seed(B + C + S + P))
    want = x.permute(0, 2, 3, 1).reshape(B * S, P * C)
    got = ops.seq_patches(x.to(DEV), torch.float32)
    assert torch.equal(got.cpu(), want)
    got16 = ops.seq_patches(x.to(DEV), torch.bfloat16)
    assert torch.equal(got16.cpu(), want.bfloat16())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S,D,kin,has_cls", [(2, 12, 64, 3, True), (3, 50, 1024, 4, True), (2, 33, 192, 3, False), (5, 196, 768, 3, True),
                                               (40, 196, 1024, 3, True)])
def test_adaptive_pos_embedding_fwd_bwd(dtype, B, S, D, kin, has_cls):
    """cat(cls, x) + cat(0, GELU(Linear(seq_ps))) (arch.py:311-321, :366-393) against fp32/fp64 torch on the same rounded inputs;
    the gradient reductions run over more than one chunk of rows in the larger cases"""
    from UCF_VIT._hip import ops
    gen = torch.Generator().manual_seed(B * 131 + S * 7 + D + kin)
    x = torch.randn(B * S, D, generator=gen)
    sp = torch.cat([torch.randint(0, 224, (B, S, kin - 1), generator=gen).float(), 2.0 ** torch.randint(1, 6, (B, S, 1), generator=gen).float()], 2)
    w = torch.randn(D, kin, generator=gen) * 0.02
    bias = torch.randn(D, generator=gen) * 0.1
    cls = torch.randn(D, generator=gen) if has_cls else None
    dout = torch.randn(B, S + int(has_cls), D, generator=gen)
    r = lambda t: None if t is None else t.to(dtype).double().requires_grad_(True)       # reference sees the same rounded inputs
    xr, wr, br, cr = r(x), r(w), r(bias), r(cls)
    pos = torch.nn.functional.gelu(sp.double() @ wr.t() + br)
    tok = xr.view(B, S, D) + pos
    want = torch.cat([cr.view(1, 1, D).expand(B, 1, D), tok], 1) if has_cls else tok
    want.backward(dout.to(dtype).double())
    dv = lambda t: None if t is None else t.to(DEV, dtype)
    out = ops.adaptive_pos_fwd(dv(x), sp.to(DEV), dv(w), dv(bias), dv(cls), B, S, D)
    tol = TOL[dtype]
    assert rel_err(out.float().cpu(), want.detach().float()) < (1e-6 if dtype == torch.float32 else 1e-2)
    dx, dw, db, dc = ops.adaptive_pos_bwd(dv(dout), sp.to(DEV), dv(w), dv(bias), B, S, D, has_cls)
    assert torch.equal(dx.view(B, S, D), dv(dout)[:, int(has_cls):])
    assert rel_err(dw.cpu(), wr.grad.float()) < 1e-4 and rel_err(db.cpu(), br.grad.float()) < 1e-4
    if has_cls:
        assert rel_err(dc.cpu(), cr.grad.float()) < 1e-5
    # accumulate bits: a second call with all three set doubles the sums
    ops.adaptive_pos_bwd(dv(dout), sp.to(DEV), dv(w), dv(bias), B, S, D, has_cls, want_dx=False, dw=dw, dbias=db, dcls=dc, acc_bits=7)
    assert rel_err(dw.cpu(), 2 * wr.grad.float()) < 1e-4 and rel_err(db.cpu(), 2 * br.grad.float()) < 1e-4
    if has_cls:
        assert rel_err(dc.cpu(), 2 * cr.grad.float()) < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,R,D,dh", [(3, 24, 64, 32), (5, 1000, 1024, 64), (2, 333, 768, 64), (7, 130, 256, 128), (1, 50, 192, 64)])
def test_variable_aggregation_attention_fwd_bwd(dtype, V, R, D, dh):
    """softmax over the V variables of every token row with one shared query (building_blocks.py:336-366) against fp64 torch on the
    same rounded inputs; D / vector width not a divisor of 256 (768) and a single variable (softmax = 1) included
    The per-element bounds and the exact cases of these kernels live in tests/test_attention_ops.py."""
    from UCF_VIT._hip import ops
    gen = torch.Generator().manual_seed(V * 1000 + R + D)
    kv = torch.randn(V * R, 2 * D, generator=gen)
    q = torch.randn(D, generator=gen)
    dout = torch.randn(R, D, generator=gen)
    H, scale = D // dh, dh ** -0.5
    kvr = kv.to(dtype).double().requires_grad_(True)
    qr = q.double().requires_grad_(True)
    k, v = kvr.view(V, R, 2, H, dh).unbind(2)                                        # [V, R, H, dh]
    s = (k * (qr.view(1, 1, H, dh) * scale)).sum(-1)                                   # [V, R, H]
    p = s.softmax(dim=0)
    want = (p.unsqueeze(-1) * v).sum(0).reshape(R, D)
    want.backward(dout.to(dtype).double())
    out, lse = ops.varagg_fwd(kv.to(DEV, dtype), q.to(DEV), V, R, D, dh, scale)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    assert rel_err(out.float().cpu(), want.detach().float()) < tol
    dkv, dq = ops.varagg_bwd(kv.to(DEV, dtype), q.to(DEV), out, lse, dout.to(DEV, dtype), V, R, D, dh, scale)
    assert rel_err(dkv.float().cpu(), kvr.grad.float()) < (1e-4 if dtype == torch.float32 else 2e-2)
    if V == 1:          # softmax over one variable is 1 whatever q is: the true gradient is exactly zero
        assert float(dq.abs().max()) < 1e-4
    else:
        assert rel_err(dq.cpu(), qr.grad.float()) < (1e-4 if dtype == torch.float32 else 2e-2)


# ---------------------------------------------------------------------------------------------- dynamic tile schedule (multi-GPU hardening)
_DYN_SCRIPT = r'''
import os, sys, torch
sys.path.insert(0, os.path.join(sys.argv[1], "ucf-vit_amd"))
from UCF_VIT._hip import ops
from UCF_VIT._hip.lib import ACT_GELU_SAVE_DERIV
g = torch.Generator().manual_seed(0)
dev = "cuda"
rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).bfloat16().to(dev)
M, D = 9000, 512                       # 36 x 8 = 288 tiles of 256 x 256 for the 4D-wide layers: more than one round, ragged last M-tile
x, x4, res = rnd(M, D), rnd(M, 4 * D), rnd(M, D)
w1, w2, b1, b2 = rnd(4 * D, D, sc=0.05), rnd(D, 4 * D, sc=0.05), rnd(4 * D), rnd(D)
dy, dy4 = rnd(M, D), rnd(M, 4 * D)
out = {}
for rep in range(3):                   # several launches share one schedule state: it must come back zeroed every time
    aux = torch.empty(M, 4 * D, dtype=torch.bfloat16, device=dev)
    out["fc1"] = ops.linear_fwd(x, w1, b1, act=ACT_GELU_SAVE_DERIV, aux_out=aux)
    out["aux"] = aux
    out["fc2"] = ops.linear_fwd(x4, w2, b2, residual=res)
    cs = torch.empty(4 * D, dtype=torch.float32, device=dev)
    out["dg"] = ops.linear_dgrad_t(dy, w2.T.contiguous(), act_grad_aux=aux, aux_is_deriv=True, c_colsum=cs)
    out["cs"] = cs
    out["wg"] = torch.stack([t.reshape(-1)[:4096] for t in ops.wgrad_grouped([(dy4, x, None, False), (dy, x4, None, False), (dy4[:, :1024], x, None, False)])])
torch.cuda.synchronize()
st = [v for v in ops._sched_states.values()]
out["state_sum"] = torch.tensor([float(sum(int(t.abs().sum()) for t in st)), float(len(st))])
torch.save({k: v.cpu() for k, v in out.items()}, sys.argv[2])
'''


def test_gemm_dynamic_tile_schedule_is_result_neutral(tmp_path):
    """desc.sched_state (tiles of the persistent 256x256 kernel handed out by atomic counters, for launches that share the GPU with an
    RCCL collective): bitwise the results of the static order OF THE SAME KERNEL (UCFVIT_GEMM_STAGGER=0: without sched_state some
    launches would take the staggered kernel, whose accumulation order differs) for every epilogue kind and the grouped weight gradient, with the grid
    capped at 256 / 240 / 200 workgroups (UCFVIT_GEMM_CUS: what a collective holding 16 / 56 CUs leaves), and the schedule state is
    all zeros again after every launch."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "dyn.py"
    script.write_text(_DYN_SCRIPT)
    res = {}
    for dyn, cus in (("0", "256"), ("1", "256"), ("1", "240"), ("1", "200"), ("0", "200")):
        f = tmp_path / f"o_{dyn}_{cus}.pt"
        r = subprocess.run([sys.executable, str(script), root, str(f)], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, UCFVIT_GEMM_DYNAMIC=dyn, UCFVIT_GEMM_CUS=cus, UCFVIT_GEMM_STAGGER="0"))
        assert r.returncode == 0, r.stderr[-2000:]
        res[(dyn, cus)] = torch.load(f, weights_only=True)
    ref = res[("0", "256")]
    assert ref["state_sum"][1] == 0                       # static: no state was ever allocated
    for key, o in res.items():
        for k in ("fc1", "aux", "fc2", "dg", "cs", "wg"):
            assert torch.equal(o[k], ref[k]), (key, k)
        if key[0] == "1":
            assert o["state_sum"][1] >= 1 and o["state_sum"][0] == 0, key      # state exists and is zero again
    # and the values are right (fp32 product of the same bf16 operands)
    g = torch.Generator().manual_seed(0)
    assert torch.isfinite(ref["fc2"].float()).all() and float(ref["fc2"].float().abs().max()) > 0.1
