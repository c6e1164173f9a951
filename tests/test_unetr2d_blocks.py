"""The blocks of the 2-D UNETR decoder (simple/unetr_blocks.py built with spatial_dims = 2): each block's forward_cl — channels-last bf16
[B, X, Y, C] on csrc/conv2d.hip, the 1x1x1 kernels and the channels-last normalisation kernels — against the SAME module's torch forward
(N C H W, torch's fp32 convolutions with the fused normalisation kernels between them) on the same bf16-rounded inputs and parameters:
output, input gradient and every parameter gradient.  Tolerances and metric are those of tests/test_unetr_decoder.py for a bf16 path
against an fp32 one: conftest.rel_err (max |a - b| / max |b|) below 3e-2 on outputs and 6e-2 on gradients.

The torch forward rounds where the HIP path rounds: hooks round the input and the output of every convolution module to bf16, forward and
backward (the yardstick run of tests/test_unetr_decoder_model.py).  That file's tolerances were set for ONE normalisation chain, where both
sides see the same pre-activation signs.  A block has a LeakyReLU behind a convolution: without the hooks the fp32 convolution output and
its bf16 rounding differ by 2^-9 relative, ~0.3 % of the pre-activations lie that close to zero and come out with the other sign, and each
such element changes its gradient by 0.99 of the upstream value — a maximum-norm error of the order of the gradient itself (measured: 0.36
on the input gradient of the 16 -> 16 block at 17 x 20, in three isolated pixels and their 5 x 5 neighbourhoods, with every layer function
alone within 3e-3).  That is a property of comparing two precisions through a kink, not of a kernel; with the roundings at the same places
the two sides decide every sign alike.  Reference: src/UCF_VIT/simple/arch.py:794-940 (monai's blocks with
spatial_dims = 2; monai itself is absent: PARITY UNPINNED against it).  The per-element bounds of the kernels under these blocks are in
tests/test_conv2d_ops.py."""
import pytest
import torch

from conftest import rel_err

DEV = "cuda"
gpu = pytest.mark.gpu
TOL_OUT, TOL_GRAD = 3e-2, 6e-2


def _round_params(m):
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.bfloat16().float())
    return m


class _RoundBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.bfloat16().float()

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().float()


class _bf16_boundaries:
    """round the input and the output of every convolution of m to bf16 (forward and backward) while the torch path runs"""

    def __init__(self, m):
        self.m = m

    def __enter__(self):
        self.hooks = []
        for mod in self.m.modules():
            if isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                self.hooks.append(mod.register_forward_pre_hook(lambda md, inp: (_RoundBf16.apply(inp[0]),)))
                self.hooks.append(mod.register_forward_hook(lambda md, inp, out: _RoundBf16.apply(out)))

    def __exit__(self, *a):
        for h in self.hooks:
            h.remove()


def _cl(t):
    """N C H W fp32 -> channels-last bf16 [B, X, Y, C], a leaf"""
    return t.permute(0, 2, 3, 1).contiguous().bfloat16().requires_grad_(True)


def _grads(m):
    g = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    for p in m.parameters():
        p.grad = None
    return g


def _compare(m, run_cl, run_torch, out_shape, seed):
    gen = torch.Generator().manual_seed(seed)
    gy = torch.randn(out_shape, generator=gen).bfloat16().float().to(DEV)
    with _bf16_boundaries(m):
        y_t, leaves_t = run_torch()
        y_t.backward(gy)
    g_t = _grads(m)
    y_h, leaves_h = run_cl()
    assert y_h.shape == tuple(y_t.permute(0, 2, 3, 1).shape)
    y_h.backward(gy.permute(0, 2, 3, 1).contiguous().to(y_h.dtype))
    g_h = _grads(m)
    assert rel_err(y_h.float().permute(0, 3, 1, 2), y_t.detach()) < TOL_OUT
    for a, b in zip(leaves_h, leaves_t):
        assert a.grad is not None and rel_err(a.grad.float().permute(0, 3, 1, 2), b.grad) < TOL_GRAD
    assert set(g_h) == set(g_t)
    for n in g_t:
        assert g_h[n].shape == g_t[n].shape and g_h[n].dtype == torch.float32
        assert rel_err(g_h[n], g_t[n]) < TOL_GRAD, (n, rel_err(g_h[n], g_t[n]))
    return y_h


@gpu
@pytest.mark.parametrize("cin,cout,img", [(16, 16, (17, 20)), (32, 16, (16, 16)), (64, 32, (9, 36)), (32, 64, (8, 16))])
def test_res_block_2d(cin, cout, img):
    """identity residual (Cin == Cout) and the normalised 1x1 projection; images at, past and below the 3x3 kernel's tiles (pixel counts in
    multiples of 4: the N C H W normalisation kernels of the torch path read 16-byte rows)"""
    from UCF_VIT.simple.unetr_blocks import UnetResBlock
    torch.manual_seed(cin + cout)
    m = _round_params(UnetResBlock(2, cin, cout, 3, 1).to(DEV))
    x = torch.randn(2, cin, *img, generator=torch.Generator().manual_seed(1)).bfloat16().float().to(DEV)

    def run_torch():
        xt = x.clone().requires_grad_(True)
        return m(xt), [xt]

    def run_cl():
        xc = _cl(x)
        return m.forward_cl(xc), [xc]
    y = _compare(m, run_cl, run_torch, (2, cout, *img), 2)
    # deterministic: the same bits on a second run
    assert torch.equal(y, m.forward_cl(_cl(x)))


@gpu
@pytest.mark.parametrize("in_chans", [1, 3])
def test_basic_block_on_the_padded_input_image(in_chans):
    """encoder1: the fp32 N C H W image through ops.pad_channels8 (zero-padded to the 8-channel operand); parameter gradients keep the
    parameter's own shape.  The 1x1 projection of a ONE-channel input into a normalisation has a gradient that is what eps leaves of an exact
    cancellation (tests/test_unetr_decoder_model.py): it is compared only for in_chans = 3"""
    from UCF_VIT._hip import ops
    from UCF_VIT.simple.unetr_blocks import UnetrBasicBlock
    torch.manual_seed(in_chans)
    m = _round_params(UnetrBasicBlock(2, in_chans, 16, kernel_size=3, stride=1, norm_name="instance", res_block=True).to(DEV))
    x = torch.rand(2, in_chans, 34, 18, generator=torch.Generator().manual_seed(3)).bfloat16().float().to(DEV)
    gy = torch.randn(2, 16, 34, 18, generator=torch.Generator().manual_seed(4)).bfloat16().float().to(DEV)
    with _bf16_boundaries(m):
        y_t = m(x)
        y_t.backward(gy)
    g_t = _grads(m)
    xp = ops.pad_channels8(x.contiguous())
    assert tuple(xp.shape) == (2, 34, 18, 8) and torch.equal(xp[..., :in_chans].float(), x.permute(0, 2, 3, 1)) and not xp[..., in_chans:].any()
    y_h = m.forward_cl(xp)
    y_h.backward(gy.permute(0, 2, 3, 1).contiguous().bfloat16())
    g_h = _grads(m)
    assert rel_err(y_h.float().permute(0, 3, 1, 2), y_t.detach()) < TOL_OUT
    for n in g_t:
        assert g_h[n].shape == g_t[n].shape
        if in_chans == 1 and n == "layer.conv3.conv.weight":
            continue
        assert rel_err(g_h[n], g_t[n]) < TOL_GRAD, (n, rel_err(g_h[n], g_t[n]))


@gpu
@pytest.mark.parametrize("cin,cout,layers,img", [(96, 32, 1, (2, 3)), (32, 16, 2, (3, 2)), (128, 64, 0, (4, 4)), (768, 128, 0, (2, 2))])
def test_prup_block_2d(cin, cout, layers, img):
    """transposed convolutions on the 1x1x1 kernel (Cin < 128) and on the GEMM (Cin >= 128), each followed by the shuffle, with residual blocks"""
    from UCF_VIT.simple.unetr_blocks import UnetrPrUpBlock
    torch.manual_seed(cin)
    m = _round_params(UnetrPrUpBlock(2, cin, cout, num_layer=layers, kernel_size=3, stride=1, upsample_kernel_size=2, norm_name="instance", conv_block=True,
                                     res_block=True).to(DEV))
    x = torch.randn(2, cin, *img, generator=torch.Generator().manual_seed(5)).bfloat16().float().to(DEV)
    f = 2 ** (layers + 1)

    def run_torch():
        xt = x.clone().requires_grad_(True)
        return m(xt), [xt]

    def run_cl():
        xc = _cl(x)
        return m.forward_cl(xc), [xc]
    _compare(m, run_cl, run_torch, (2, cout, img[0] * f, img[1] * f), 6)


@gpu
@pytest.mark.parametrize("cin,cout,img", [(32, 16, (8, 9)), (128, 64, (2, 2)), (96, 128, (1, 2))])
def test_up_block_2d_concatenates_the_skip_in_place(cin, cout, img):
    from UCF_VIT.simple.unetr_blocks import UnetrUpBlock
    torch.manual_seed(cout)
    m = _round_params(UnetrUpBlock(2, cin, cout, kernel_size=3, upsample_kernel_size=2, norm_name="instance", res_block=True).to(DEV))
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(2, cin, *img, generator=gen).bfloat16().float().to(DEV)
    skip = torch.randn(2, cout, 2 * img[0], 2 * img[1], generator=gen).bfloat16().float().to(DEV)

    def run_torch():
        xt, st = x.clone().requires_grad_(True), skip.clone().requires_grad_(True)
        return m(xt, st), [xt, st]

    def run_cl():
        xc, sc = _cl(x), _cl(skip)
        return m.forward_cl(xc, sc), [xc, sc]
    _compare(m, run_cl, run_torch, (2, cout, 2 * img[0], 2 * img[1]), 8)
    with pytest.raises(ValueError, match="not on the HIP path"):
        m.forward_cl(_cl(x), _cl(skip), size=(5, 5))            # no resampling in the plane


@gpu
@pytest.mark.parametrize("classes", [2, 4])
def test_out_block_2d_gives_fp32_logits(classes):
    from UCF_VIT.simple.unetr_blocks import UnetOutBlock
    torch.manual_seed(classes)
    m = _round_params(UnetOutBlock(2, 16, classes).to(DEV))
    x = torch.randn(2, 16, 17, 18, generator=torch.Generator().manual_seed(9)).bfloat16().float().to(DEV)

    def run_torch():
        xt = x.clone().requires_grad_(True)
        return m(xt), [xt]
    seen = {}

    def run_cl():
        xc = _cl(x)
        seen["y"] = m.forward_cl(xc)
        return seen["y"], [xc]
    _compare(m, run_cl, run_torch, (2, classes, 17, 18), 10)
    assert seen["y"].dtype == torch.float32 and tuple(seen["y"].shape) == (2, 17, 18, classes)


@gpu
def test_layer_functions_equal_the_fused_block_and_torch():
    """conv3x3 / tconv2x2 / conv1x1x1 / instnorm_act_cl on [B, X, Y, C]: against torch.nn.functional on the same rounded operands, and the
    chain of them against the fused UnetResBlockFn (same kernels, same order: forward bit for bit)"""
    import torch.nn.functional as F
    from UCF_VIT._hip import conv as HC
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 9, 17, 16, generator=gen).bfloat16().to(DEV)
    w1 = (torch.randn(32, 16, 3, 3, generator=gen) * 0.1).bfloat16().float().to(DEV).requires_grad_(True)
    w2 = (torch.randn(32, 32, 3, 3, generator=gen) * 0.1).bfloat16().float().to(DEV)
    w3 = (torch.randn(32, 16, 1, 1, generator=gen) * 0.2).bfloat16().float().to(DEV)
    xl = x.clone().requires_grad_(True)
    y = HC.conv3x3(xl, w1)
    ref_x = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    ref_w = w1.detach().clone().requires_grad_(True)
    ref = F.conv2d(ref_x, ref_w, padding=1)
    gy = torch.randn(ref.shape, generator=gen).bfloat16().float().to(DEV)
    ref.backward(gy)
    y.backward(gy.permute(0, 2, 3, 1).contiguous().bfloat16())
    assert rel_err(y.float().permute(0, 3, 1, 2), ref.detach()) < 1e-2             # one bf16 rounding of the output
    assert rel_err(xl.grad.float().permute(0, 3, 1, 2), ref_x.grad) < 1e-2 and rel_err(w1.grad, ref_w.grad) < 1e-3
    wt = (torch.randn(16, 8, 2, 2, generator=gen) * 0.2).bfloat16().float().to(DEV).requires_grad_(True)
    xt = x.clone().requires_grad_(True)
    up = HC.tconv2x2(xt, wt)
    ref_x2 = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    ref_wt = wt.detach().clone().requires_grad_(True)
    ref_up = F.conv_transpose2d(ref_x2, ref_wt, stride=2)
    gu = torch.randn(ref_up.shape, generator=gen).bfloat16().float().to(DEV)
    ref_up.backward(gu)
    up.backward(gu.permute(0, 2, 3, 1).contiguous().bfloat16())
    assert tuple(up.shape) == (2, 18, 34, 8) and rel_err(up.float().permute(0, 3, 1, 2), ref_up.detach()) < 1e-2
    assert rel_err(xt.grad.float().permute(0, 3, 1, 2), ref_x2.grad) < 1e-2 and rel_err(wt.grad, ref_wt.grad) < 1e-3
    # the fused block against the chain of layer functions
    fused = HC.unet_res_block(x, w1.detach(), w2, w3)
    c1 = HC.instnorm_act_cl(HC.conv3x3(x, w1.detach()))
    c2 = HC.conv3x3(c1, w2)
    c3 = HC.instnorm_act_cl(HC.conv1x1x1(x, w3), None, 1e-5, 1.0)
    chain = HC.instnorm_act_cl(c2, c3)
    assert rel_err(fused.float(), chain.float()) < 1e-2          # the chain rounds the normalised 1x1 branch to bf16, the fused block does not
