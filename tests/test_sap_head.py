"""SAP segmentation head (HF.SapHeadFn: the ConvTranspose neck and the 1x1 header folded into one Linear layer + scatter) and the Dice + BCE
loss (HF.DiceBCEFn behind utils/metrics.DiceBLoss) on the HIP kernels of csrc/sap_head.hip.

  * model tier: SAP in 3-D + DiceBLoss against tests/golden/model_sap_3d.npz, recorded from the reference model and the reference's own loss
    (make_golden_sap3d.py).  The fixture's model has embed_dim 96 / 3 heads: the reference's SAP constructor cannot build a 3-D model whose
    embed_dim is no multiple of 6.  Its neck gradient (6 MiB) is held as every 11th element, the 2-norm and one random projection.
  * scatter, exact: the kernels are a permutation (+ one add), so torch.equal against torch's rearrange.
  * head, exact tier: small-integer operands for which every product and sum is representable, so fp64 convolutions are reproduced bit for bit.
  * head, tolerance tier: random operands against fp64 conv_transpose + 1x1 convolution on the CPU.
  * Dice + BCE: against an fp64 evaluation of the formula; bounds from the arithmetic (see the test), not from what the kernels give.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_err
from det_weights import det_state_dict, det_tensor, proj_vector

DEV = "cuda"
gpu = pytest.mark.gpu

SAP3D_KW = dict(img_size=[16, 16, 16], patch_size=4, in_chans=1, num_classes=4, embed_dim=96, depth=1, num_heads=3, adaptive_patching=True,
                fixed_length=8, sqrt_len=2, twoD=False, use_adaptive_pos_emb=True, sqrt_len_method=True, class_token=False, weight_init='skip')
GOLDEN_STRIDE = 11                      # make_golden_sap3d.py: STRIDE


# ------------------------------------------------------------------------------------------------ 7. CPU
def test_diceb_loss_on_cpu_reproduces_the_reference_loss():
    """the torch arithmetic DiceBLoss keeps for CPU tensors is the reference's: its loss on the recorded output map and targets"""
    from UCF_VIT.utils.metrics import DiceBLoss
    g = load_golden("model_sap_3d.npz")
    loss = DiceBLoss(num_class=4)(g["out"], g["targets"])
    assert abs(loss.item() - g["loss"].item()) <= 1e-6
    t = g["targets"]
    assert float(t.min()) >= 0.0 and float(t.max()) <= 1.0
    onehot = ((t == 0) | (t == 1)).all(dim=1) & (t.sum(dim=1) == 1)
    assert 0.45 < onehot.float().mean().item() < 0.55          # half hard, half soft targets


def test_binding_names_the_sap_head_symbols():
    from UCF_VIT._hip import lib
    for name in ("ucfvit_sap_fold", "ucfvit_sap_unfold_workspace", "ucfvit_sap_unfold", "ucfvit_sap_scatter_fwd", "ucfvit_sap_scatter_bwd_workspace",
                 "ucfvit_sap_scatter_bwd", "ucfvit_dice_bce_stats_floats", "ucfvit_dice_bce_workspace", "ucfvit_dice_bce_stats",
                 "ucfvit_dice_bce_from_stats"):
        assert name in lib.SIGNATURES, name
    assert lib.ABI_VERSION >= 19


def test_sap_head_and_loss_have_no_cpu_path_except_the_checker():
    from UCF_VIT.simple.arch import SAP
    m = SAP(img_size=[16, 16], patch_size=4, in_chans=1, num_classes=2, embed_dim=32, depth=1, num_heads=2, class_token=False, sqrt_len=4)
    with pytest.raises(RuntimeError):
        m.mask_head(torch.zeros(1, 16, 32))


# ------------------------------------------------------------------------------------------------ 1. model vs reference
@gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (torch.bfloat16, 6e-2)])
def test_sap_3d_with_diceb_loss_vs_reference(dtype, tol):
    from UCF_VIT.simple.arch import SAP
    from UCF_VIT.utils.metrics import DiceBLoss
    g = load_golden("model_sap_3d.npz")
    m = SAP(**SAP3D_KW)
    m.load_state_dict(det_state_dict(m, 81, keep=()))
    m = m.to(DEV)
    m.set_compute_dtype(dtype)
    out = m(g["x"].to(DEV), ["ct"], g["seq_ps"].to(DEV))
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(g["out"].shape)
    loss = DiceBLoss(num_class=4)(out, g["targets"].to(DEV))
    loss.backward()
    assert rel_err(out, g["out"]) < tol
    assert abs(loss.item() - g["loss"].item()) < tol * max(1.0, abs(g["loss"].item()))
    for i, (k, p) in enumerate(m.named_parameters()):
        if "g." + k in g:
            ref = g["g." + k]
            if float(ref.abs().max()) == 0.0:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            else:
                assert p.grad is not None, k
                assert rel_err(p.grad, ref) < tol, k
        else:                            # the neck: a strided sample, the norm and a projection of the whole tensor
            assert p.grad is not None, k
            gr = p.grad.detach().double().cpu()
            assert rel_err(gr.reshape(-1)[::GOLDEN_STRIDE], g["gs." + k]) < tol, k
            gn = g["gn." + k].item()
            assert abs(gr.norm().item() - gn) < tol * gn, k
            gp = (gr * proj_vector(p.shape, i).double()).sum().item()
            assert abs(gp - g["gp." + k].item()) <= tol * gn, k          # |<g - g_ref, r>| ~ |g - g_ref|_2 for a unit-variance direction


# ------------------------------------------------------------------------------------------------ 2. scatter, exact
def _to_map(rows, B, p, s, nd, C):
    if nd == 3:
        return rows.view(B, s, s, s, p, p, p, C).permute(0, 7, 1, 4, 2, 5, 3, 6).reshape(B, C, s * p, s * p, s * p)
    return rows.view(B, s, s, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, s * p, s * p)


def _to_rows(mp, B, p, s, nd, C):
    if nd == 3:
        return mp.view(B, C, s, p, s, p, s, p).permute(0, 2, 4, 6, 3, 5, 7, 1).reshape(B * s ** 3, p ** 3 * C)
    return mp.view(B, C, s, p, s, p).permute(0, 2, 4, 3, 5, 1).reshape(B * s * s, p * p * C)


@gpu
@pytest.mark.parametrize("nd,p,s,C,B", [(2, 8, 4, 3, 2), (2, 3, 3, 3, 1), (3, 4, 2, 4, 2), (3, 2, 3, 2, 1), (3, 1, 2, 5, 3)])
def test_logit_scatter_is_the_exact_rearrangement(nd, p, s, C, B):
    from UCF_VIT._hip import ops
    rows = det_tensor((B * s ** nd, p ** nd * C), 900 + p).to(DEV)
    bias = det_tensor((C,), 901).to(DEV)
    out = ops.sap_scatter_fwd(rows, bias, B, p, s, nd)
    want = _to_map(rows, B, p, s, nd, C) + bias.view(1, C, *([1] * nd))
    assert out.dtype == torch.float32 and out.shape == want.shape
    assert torch.equal(out, want)
    dmap = det_tensor(tuple(want.shape), 902 + s).to(DEV)
    drows, dbias = ops.sap_scatter_bwd(dmap, p, s, nd, torch.float32)
    assert torch.equal(drows, _to_rows(dmap, B, p, s, nd, C))
    db64 = dmap.double().sum(dim=[0] + list(range(2, nd + 2)))
    assert rel_err(dbias, db64) < 1e-6
    drows_b, _ = ops.sap_scatter_bwd(dmap, p, s, nd, torch.bfloat16, want_dbias=False)
    assert torch.equal(drows_b, drows.to(torch.bfloat16))                   # one round-to-nearest-even per element


# ------------------------------------------------------------------------------------------------ 3. / 4. the head
def _head64(x, wn, wh, bh, G, s, nd):
    """fp64 conv_transpose + 1x1 convolution on the CPU, loss (out * G).sum(): -> out, (dx, dW_neck, dW_head, db)"""
    x, wn, wh, bh = (t.detach().double().cpu().requires_grad_(True) for t in (x, wn, wh, bh))
    B, _, D = x.shape
    grid = x.reshape(B, *([s] * nd), D).movedim(-1, 1)
    p = wn.shape[-1]
    if nd == 3:
        out = F.conv3d(F.conv_transpose3d(grid, wn, stride=p), wh, bh)
    else:
        out = F.conv2d(F.conv_transpose2d(grid, wn, stride=p), wh, bh)
    (out * G.double().cpu()).sum().backward()
    return out.detach(), (x.grad, wn.grad, wh.grad, bh.grad)


def _head_hip(x, wn, wh, bh, G, p, s, nd, dtype):
    from UCF_VIT._hip import functional as HF
    x, wn, wh, bh = (t.detach().clone().requires_grad_(True) for t in (x, wn, wh, bh))
    out = HF.SapHeadFn.apply(x, wn, wh, bh, p, s, nd, dtype)
    (out * G).sum().backward()
    return out.detach(), (x.grad, wn.grad, wh.grad, bh.grad)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sap_head_exact_tier(dtype):
    """x in {-2..2}; W_neck with ONE non-zero k per (d, offset), entries in {-2..2}; W_head, bias in {-2..2}; G in {-1, 0, 1}.
    W_eff entries are single products (|.| <= 4, exact in bf16); the map sums 64 terms of |.| <= 8 (<= 512); in fp32 mode the gradients sum
    at most 64 * 64 terms of |.| <= 64 (dW_head; < 2^24), so every value of the fp64 reference is reproduced exactly.  bf16 mode rounds the
    map gradient's rows (exact: {-1, 0, 1}) but holds dW_eff sums only up to 256, so there the output alone is compared."""
    D, K, p, s, nd, C, B = 64, 256, 4, 2, 3, 4, 2
    x = _ints((B, s ** nd, D), -2, 2, 1)
    kstar = torch.randint(0, K, (D, 1, p, p, p), generator=torch.Generator().manual_seed(2))
    wn = torch.zeros(D, K, p, p, p).scatter_(1, kstar, _ints((D, 1, p, p, p), -2, 2, 3))
    wh, bh = _ints((C, K, 1, 1, 1), -2, 2, 4), _ints((C,), -2, 2, 5)
    G = _ints((B, C) + (s * p,) * nd, -1, 1, 6)
    out64, grads64 = _head64(x, wn, wh, bh, G, s, nd)
    out, grads = _head_hip(x.to(DEV), wn.to(DEV), wh.to(DEV), bh.to(DEV), G.to(DEV), p, s, nd, dtype)
    assert out.dtype == torch.float32
    assert torch.equal(out.double().cpu(), out64)
    if dtype == torch.float32:
        for name, a, b in zip(("dx", "dW_neck", "dW_head", "db"), grads, grads64):
            assert torch.equal(a.double().cpu(), b), name


HEAD_SHAPES = [  # nd, D, p, s, C, B, sliced
    (2, 64, 8, 4, 3, 2, False),
    (3, 96, 4, 2, 4, 2, False),
    (3, 64, 2, 3, 2, 1, False),
    (3, 96, 4, 2, 4, 2, True),
]


@gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (torch.bfloat16, 6e-2)])
@pytest.mark.parametrize("nd,D,p,s,C,B,sliced", HEAD_SHAPES)
def test_sap_head_vs_fp64_convolutions(nd, D, p, s, C, B, sliced, dtype, tol):
    S = s ** nd
    full = det_tensor((B, S + 1, D), 40 + D).to(DEV)
    x = full[:, 1:] if sliced else full[:, 1:].contiguous()                # sliced: what pool() hands over when there is a class token
    assert x.is_contiguous() != sliced
    wn = det_tensor((D, 256) + (p,) * nd, 41, 0.05).to(DEV)
    wh, bh = det_tensor((C, 256) + (1,) * nd, 42, 0.05).to(DEV), det_tensor((C,), 43, 0.02).to(DEV)
    G = det_tensor((B, C) + (s * p,) * nd, 44).to(DEV)
    out64, grads64 = _head64(x, wn, wh, bh, G, s, nd)
    out, grads = _head_hip(x, wn, wh, bh, G, p, s, nd, dtype)
    assert out.dtype == torch.float32
    assert rel_err(out, out64) < tol
    for name, a, b in zip(("dx", "dW_neck", "dW_head", "db"), grads, grads64):
        assert a is not None and a.shape == b.shape, name
        assert rel_err(a, b) < tol, name


# ------------------------------------------------------------------------------------------------ 5. Dice + BCE
def _targets(shape, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == "zero":
        return torch.zeros(shape)
    if kind == "soft":
        return torch.rand(shape, generator=gen)
    cls = torch.randint(0, shape[1], (shape[0], 1) + tuple(shape[2:]), generator=gen)
    return torch.zeros(shape).scatter_(1, cls, 1.0)


def _dice_bce64(z, t, weight, smooth, grad_scale, stable=False):
    """the formula of utils/metrics.DiceBLoss in fp64 -> (loss, d(grad_scale * loss)/dz); stable: BCE as clamped softplus (for |z| where
    sigmoid has rounded to 0 or 1; equal to the sigmoid form in exact arithmetic)"""
    z = z.detach().double().cpu().requires_grad_(True)
    t = t.double().cpu()
    # stable: sigmoid as exp(-softplus(-z)), whose autograd derivative is p * sigmoid(-z); torch.sigmoid's is p * (1 - p) with the ROUNDED p,
    # which is 0 at z = +40 even in fp64 (the true value is 4e-18 and decides the gradient when only the dice term is on)
    prob = torch.exp(-F.softplus(-z)) if stable else torch.sigmoid(z)
    pred, true = prob[:, 1:].flatten(), t[:, 1:].flatten()
    inter = (pred * true).sum()
    dice = 1 - (2. * inter + smooth) / (pred.sum() + true.sum() + smooth)
    if stable:
        zz = z[:, 1:].flatten()
        bce = (true * F.softplus(-zz).clamp(max=100.) + (1 - true) * F.softplus(zz).clamp(max=100.)).mean()
    else:
        bce = F.binary_cross_entropy(pred, true, reduction='mean')
    loss = weight * bce + (1 - weight) * dice
    (loss * grad_scale).backward()
    return loss.detach(), z.grad


def _check_dice_bce(z, t, combos, grad_scale, stable=False):
    """Bounds, from the arithmetic: every term costs a few fp32 ulps (expf, log1pf, one division: ~3e-7 relative), the sums are pairwise over
    n <= 4e5 same-sign terms (16 sequential terms per thread, a tree over the workgroup, fp64 over the workgroups: ~1e-6), the stats are
    rounded to fp32 once: about 2e-6 relative in the loss and in the gradient's coefficients; 1e-5 leaves a factor of 5."""
    from UCF_VIT._hip import ops
    zd, td = z.to(DEV), t.to(DEV)
    stats = ops.dice_bce_stats(zd, td)
    for weight, smooth in combos:
        loss, dl = ops.dice_bce_from_stats(zd, td, stats, weight, smooth, grad_scale)
        loss64, g64 = _dice_bce64(z.float() if z.dtype == torch.bfloat16 else z, t, weight, smooth, grad_scale, stable)
        print(f"dice_bce {tuple(z.shape)} {z.dtype} w={weight} smooth={smooth}: loss {loss.item():.8f} fp64 {loss64.item():.8f} "
              f"rel {abs(loss.item() - loss64.item()) / abs(loss64.item()):.2e}  grad {((dl.double().cpu() - g64).abs().max() / g64.abs().max()).item():.2e}")
        assert math.isfinite(loss.item()) and bool(torch.isfinite(dl).all())
        assert abs(loss.item() - loss64.item()) <= 1e-5 * abs(loss64.item())
        assert dl.dtype == torch.float32 and dl.shape == z.shape
        assert bool(((dl.double().cpu() - g64).abs() <= 1e-5 * g64.abs().max()).all())
        assert bool((dl[:, 0] == 0).all())
    loss2, dl2 = ops.dice_bce_from_stats(zd, td, ops.dice_bce_stats(zd, td), weight, smooth, grad_scale)
    assert torch.equal(loss, loss2) and torch.equal(dl, dl2)             # fixed summation order: bitwise reproducible
    return loss, dl


COMBOS = [(w, sm) for w in (0.5, 0.0, 1.0) for sm in (1.0, 1e-5)]
DICE_SHAPES = [(1, 2, 5, 7), (3, 3, 33, 31), (2, 4, 8, 8, 8), (2, 4, 32, 32, 32)]


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["hard", "soft", "zero"])
@pytest.mark.parametrize("shape", DICE_SHAPES)
def test_dice_bce_vs_fp64(shape, kind, dtype):
    z = ((torch.rand(shape, generator=torch.Generator().manual_seed(7)) * 16 - 8)).to(dtype)          # uniform in [-8, 8]
    # weight = 1 with all-zero targets and smooth > 0 leaves the dice term out; every other combination exercises both terms
    _check_dice_bce(z, _targets(shape, kind, 8), COMBOS, grad_scale=3.0)


@gpu
@pytest.mark.parametrize("kind", ["hard", "soft"])
def test_dice_bce_where_sigmoid_saturates(kind):
    """z = +-40: fp32 sigmoid is exactly 0 or 1 there; the loss and the gradient stay finite and equal the clamped-softplus form in fp64"""
    shape = (2, 3, 16, 16)
    sign = torch.randint(0, 2, shape, generator=torch.Generator().manual_seed(9)).float() * 2 - 1
    _check_dice_bce(40.0 * sign, _targets(shape, kind, 10), COMBOS, grad_scale=0.5, stable=True)


# ------------------------------------------------------------------------------------------------ 6. public loss
@gpu
def test_diceb_loss_module_runs_the_kernels_through_autograd():
    from UCF_VIT._hip import ops
    from UCF_VIT.utils.metrics import DiceBLoss
    shape = (2, 4, 8, 8, 8)
    z = (torch.rand(shape, generator=torch.Generator().manual_seed(11)) * 16 - 8)
    t = _targets(shape, "soft", 12)
    out = z.to(DEV).requires_grad_(True)
    loss = DiceBLoss(num_class=4)(out, t.to(DEV))
    loss.backward()
    want_loss, want_dl = _check_dice_bce(z, t, [(0.5, 1.0)], grad_scale=1.0)
    assert torch.equal(loss.detach(), want_loss) and torch.equal(out.grad, want_dl)
    zc = z.clone().requires_grad_(True)
    loss_c = DiceBLoss(num_class=4)(zc, t)                                  # CPU tensors: the torch arithmetic of the same class
    loss_c.backward()
    assert abs(loss.item() - loss_c.item()) <= 1e-5 * abs(loss_c.item())
    assert bool(((out.grad.cpu() - zc.grad).abs() <= 1e-5 * zc.grad.abs().max()).all())
    # smooth and weight are honoured, an upstream factor reaches the kernel, integer targets are cast
    out2 = z.to(DEV).requires_grad_(True)
    hard = _targets(shape, "hard", 13)
    (DiceBLoss(weight=0.25, num_class=4)(out2, hard.long().to(DEV), smooth=1e-5) * 2.0).backward()
    l64, g64 = _dice_bce64(z, hard, 0.25, 1e-5, 2.0)
    assert bool(((out2.grad.double().cpu() - g64).abs() <= 1e-5 * g64.abs().max()).all())
