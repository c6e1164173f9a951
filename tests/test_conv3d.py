"""Convolution kernels of the UNETR decoder (csrc/conv3d.hip, UCF_VIT/_hip/conv.py) against torch.nn.functional on the same bf16-rounded
operands (fp32 math on the device: the checker, not the product).  monai — where the reference gets these layers — is absent: PARITY UNPINNED
against it; what is pinned here is the layer semantics monai documents: Conv3d(k=3, s=1, p=1, bias=False),
ConvTranspose3d(k=2, s=2, bias=False), InstanceNorm3d(affine=False) + LeakyReLU(0.01)."""
import pytest
import torch
import torch.nn.functional as F


def _cl(t):           # [B, C, X, Y, Z] -> channels-last [B, X, Y, Z, C]
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _ncdhw(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


def _rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-20)).item()


def test_pack_and_unpack_are_inverse_layouts():
    """CPU: the packed forward layout puts w[co, ci, tap] at [chunk][step][co][(tap % TPS) CPC + ci % CPC]; unpack inverts the wgrad layout"""
    from UCF_VIT._hip import conv
    for cin, cout in ((8, 16), (16, 16), (32, 16), (64, 32), (128, 64)):
        w = torch.randn(cout, cin, 3, 3, 3)
        p = conv.pack_conv_weight(w).float()
        cpc = min(cin, 32)
        tps = 32 // cpc
        for (co, ci, tap) in ((0, 0, 0), (cout - 1, cin - 1, 26), (3, cin // 2, 13), (5, 1, 7)):
            ref = w.reshape(cout, cin, 27)[co, ci, tap].bfloat16().float()
            got = p[ci // cpc, tap // tps, co, (tap % tps) * cpc + ci % cpc]
            assert got == ref
        if tps > 1:                                              # the padding taps hold zeros
            assert p[0, -1, :, (27 % tps) * cpc:].abs().max() == 0
        mb16, nbk16 = (32 if cout % 32 == 0 else 16), max(cpc, 16)
        packed = torch.arange((cout // mb16) * (cin // cpc) * 27 * mb16 * nbk16, dtype=torch.float32)
        u = conv.unpack_conv_wgrad(packed, cin, cout)
        co, ci, tap = cout - 2, cin - 3, 11
        idx = ((((co // mb16) * (cin // cpc) + ci // cpc) * 27 + tap) * mb16 + co % mb16) * nbk16 + ci % cpc
        assert u.reshape(cout, cin, 27)[co, ci, tap] == packed[idx]


CONV_CASES = [
    # B, X, Y, Z, Cin, Cout: ragged extents (tile overhang on every axis), every channel-count path of the decoder
    (2, 5, 9, 21, 8, 16),
    (1, 4, 8, 16, 16, 16),
    (2, 3, 10, 33, 32, 16),
    (1, 6, 7, 18, 16, 32),
    (1, 4, 9, 16, 32, 32),
    (1, 5, 4, 20, 64, 32),
    (1, 4, 6, 16, 64, 64),
    (1, 3, 5, 16, 128, 64),
    (1, 2, 4, 16, 256, 128),
]


@pytest.mark.gpu
@pytest.mark.parametrize("B,X,Y,Z,cin,cout", CONV_CASES)
def test_conv3x3x3_forward_and_gradients(B, X, Y, Z, cin, cout):
    from UCF_VIT._hip import conv
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    x = torch.randn(B, cin, X, Y, Z, generator=g).bfloat16().cuda()
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (27 * cin)) ** 0.5).cuda()
    dy = torch.randn(B, cout, X, Y, Z, generator=g).bfloat16().cuda()
    xr, wr = x.float().requires_grad_(True), w.bfloat16().float().requires_grad_(True)
    yr = F.conv3d(xr, wr, padding=1)
    yr.backward(dy.float())
    want_dx = cin % 16 == 0                               # the 8-channel operand is the zero-padded input volume: it never needs a gradient
    xc = _cl(x).requires_grad_(want_dx)
    wp = w.clone().requires_grad_(True)
    y = conv.conv3x3x3(xc, wp)
    assert y.shape == (B, X, Y, Z, cout) and y.dtype == torch.bfloat16
    y.backward(_cl(dy))
    assert _rel(_ncdhw(y), yr) < 1e-2                     # bf16 output rounding (2^-8) of an fp32-accumulated sum
    if want_dx:
        assert _rel(_ncdhw(xc.grad), xr.grad) < 1e-2
    assert _rel(wp.grad, wr.grad) < 2e-3                  # fp32 out
    # deterministic
    xc2 = _cl(x).requires_grad_(want_dx)
    wp2 = w.clone().requires_grad_(True)
    y2 = conv.conv3x3x3(xc2, wp2)
    y2.backward(_cl(dy))
    assert torch.equal(y, y2) and torch.equal(wp.grad, wp2.grad) and (not want_dx or torch.equal(xc.grad, xc2.grad))


@pytest.mark.gpu
def test_conv_strip_kernel_is_bit_identical_to_the_tile_kernel():
    """the software-pipelined column kernel (single-chunk inputs; picked by size, here forced) against the one-tile-per-workgroup kernel, for
    every (Cin, Cout, kernel size) instantiation, ragged extents, fp32 and bf16 output.  Same MFMA order per output — bit-identical — for
    the pointwise layers, the 8-channel input layer and the multi-chunk kernel; the 3x3x3 column kernel with 16 input channels adds
    its taps in another order (a B fragment read once per halo row feeds the three dy taps): equal up to the rounding of the output.
    The accumulate_into form is bf16(base + the kernel's fp32 sum) exactly, in both modes."""
    import subprocess
    import sys
    script = r'''
import sys, torch
sys.path.insert(0, "ucf-vit_amd")
from UCF_VIT._hip import conv, ops
out, share = [], []
for cin, cout, ks in ((8, 16, 3), (16, 16, 3), (32, 16, 3), (16, 32, 3), (32, 32, 3), (32, 64, 3), (16, 64, 3), (8, 16, 1), (32, 128, 1), (16, 16, 1), (32, 32, 1)):
    g = torch.Generator().manual_seed(cin * 100 + cout + ks)
    x = torch.randn(2, 5, 11, 53, cin, generator=g).bfloat16().cuda()
    w = conv.pack_conv_weight(torch.randn(cout, cin, ks, ks, ks, generator=g) * 0.1).cuda()
    b = torch.randn(cout, generator=g).cuda()
    out.append(ops.conv3d_fwd(x, w, cout, ksize=ks).float().cpu())
    out.append(ops.conv3d_fwd(x, w, cout, ksize=ks, bias=b, cout_store=cout - 12, out_dtype=torch.float32).cpu())
    base = torch.randn(2, 5, 11, 53, cout, generator=g).bfloat16().cuda()
    out.append(ops.conv3d_fwd(x, w, cout, ksize=ks, accumulate_into=base.clone()).float().cpu())      # y += conv(x)
    share += [cin == 16 and ks == 3] * 3
    y32 = ops.conv3d_fwd(x, w, cout, ksize=ks, out_dtype=torch.float32).cpu()       # the same kernel's fp32 sums: one rounding of base + sum
    assert torch.equal(out[-1], (y32 + base.float().cpu()).bfloat16().float())
for cin, cout, Z in ((64, 32, 32), (128, 64, 16), (64, 64, 64), (256, 32, 16), (64, 128, 48)):       # multi-chunk column kernel (Z = 16 / 32 / 64; 48: not eligible)
    g = torch.Generator().manual_seed(cin + cout + Z)
    x = torch.randn(2, 5, 11, Z, cin, generator=g).bfloat16().cuda()
    w = conv.pack_conv_weight(torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.05).cuda()
    base = torch.randn(2, 5, 11, Z, cout, generator=g).bfloat16().cuda()
    out.append(ops.conv3d_fwd(x, w, cout).float().cpu())
    out.append(ops.conv3d_fwd(x, w, cout, accumulate_into=base.clone()).float().cpu())
    share += [False] * 2
# instance-norm statistics of the output from the epilogue (column kernels) / from a pass over the output (tile kernel): same numbers
for cin, cout, ks, Z, XY in ((16, 16, 3, 53, (5, 11)), (32, 32, 3, 40, (5, 11)), (8, 16, 1, 53, (5, 11)), (64, 32, 3, 32, (5, 11)), (32, 64, 1, 21, (5, 11)),
                             (16, 16, 3, 40, (64, 96))):           # the last: 768 partial rows per batch element -> two-stage fold
    g = torch.Generator().manual_seed(cin + cout + ks + Z)
    x = torch.randn(2, XY[0], XY[1], Z, cin, generator=g).bfloat16().cuda()
    w = conv.pack_conv_weight(torch.randn(cout, cin, ks, ks, ks, generator=g) * 0.1).cuda()
    yv, mean, rstd = ops.conv3d_fwd(x, w, cout, ksize=ks, stats_eps=1e-5)
    ref = yv.float().reshape(2, -1, cout)
    assert ((mean - ref.mean(1)).abs().max() / ref.std(1).max()).item() < 1e-4
    assert ((rstd * (ref.var(1, unbiased=False) + 1e-5).sqrt() - 1).abs().max()).item() < 1e-4
    out += [yv.float().cpu(), mean.cpu(), rstd.cpu()]
    share += [cin == 16 and ks == 3, False, False]
torch.save({"out": out, "share": share}, sys.argv[1])
'''
    import os
    import tempfile
    res = {}
    with tempfile.TemporaryDirectory() as d:
        for mode in ("0", "2"):
            f = os.path.join(d, mode + ".pt")
            r = subprocess.run([sys.executable, "-c", script, f], env=dict(os.environ, UCFVIT_CONV_STRIP=mode), capture_output=True, text=True,
                               cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
            assert r.returncode == 0, r.stderr[-2000:]
            res[mode] = torch.load(f, weights_only=True)
    assert len(res["0"]["out"]) == 61 and res["0"]["share"] == res["2"]["share"] and sum(res["0"]["share"]) == 11
    for i, (a, b, sh) in enumerate(zip(res["0"]["out"], res["2"]["out"], res["0"]["share"])):
        assert torch.isfinite(a).all()
        if i < 43 or (i - 43) % 3 == 0:
            if sh:                                                        # the SHARE kernel's re-ordered tap sum (see above)
                assert ((a - b).abs().max() / b.abs().max()).item() < 1e-2
            else:
                assert torch.equal(a, b), i                               # every other instantiation: bit-identical
        else:
            assert ((a - b).abs().max() / b.abs().max()).item() < 1e-4       # statistics: epilogue fold vs a pass over the output


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,ks,shape", [(16, 16, 1, (2, 32, 128, 40)), (32, 32, 1, (2, 32, 128, 24)), (16, 16, 3, (2, 32, 128, 48)), (64, 32, 3, (2, 32, 128, 32))])
def test_epilogue_statistics_keep_their_variance_when_the_mean_is_large(cin, cout, ks, shape):
    """instance-norm statistics from the convolution epilogue (count / mean / M2 per wave, accumulated relative to a shift, combined with the
    parallel-variance formula) on outputs whose |mean| is hundreds of standard deviations — the case E[q^2] - mean^2 in fp32 cannot hold
    (round-2 advisor finding): against the double-precision statistics of the stored output and against the stand-alone statistics kernel.
    Pointwise layers: outputs 50 +- a few bf16 steps; 3x3x3: the interior at 50, the zero-padded faces lower (large spread, same check)."""
    from UCF_VIT._hip import conv, ops
    g = torch.Generator().manual_seed(cin + cout + ks)
    B, X, Y, Z = shape
    x = (1.0 + 0.01 * torch.randn(B, X, Y, Z, cin, generator=g)).bfloat16().cuda()
    w = torch.full((cout, cin, ks, ks, ks), 50.0 / (cin * ks ** 3)) * (1.0 + 0.002 * torch.randn(cout, 1, 1, 1, 1, generator=g))
    wp = conv.pack_conv_weight(w).cuda()
    from UCF_VIT._hip import lib
    assert lib.load().ucfvit_conv3d_fwd_stats_rows(B, X, Y, Z, cin, cout, ks, 0) > 0          # these shapes DO take the epilogue path
    y, mean, rstd = ops.conv3d_fwd(x, wp, cout, ksize=ks, stats_eps=1e-5)
    ref = y.double().reshape(B, -1, cout)
    m_ref, v_ref = ref.mean(1), ref.var(1, unbiased=False)
    r_ref = (v_ref + 1e-5).rsqrt()
    if ks == 1:
        assert float((m_ref.abs() / v_ref.sqrt()).min()) > 100            # the pathological regime
    assert float((mean.double() - m_ref).abs().max()) < 1e-4 * float(m_ref.abs().max())
    assert float((rstd.double() / r_ref - 1).abs().max()) < 1e-3
    m2, r2 = ops.instnorm_cl_stats(y, 1e-5)
    assert float((rstd / r2 - 1).abs().max()) < 1e-3 and float((mean - m2).abs().max()) < 1e-4 * float(m_ref.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pad_rows8_dense_rows_and_channel_slices(dtype):
    """narrow channels-last rows -> bf16 rows of 8 (ucfvit_pad_rows8): dense [.., 4], a 4-channel slice of a 16-channel buffer, the permuted
    [B, n, X, Y, Z] view the Dice / CE gradient arrives as; bit-exact against a torch cast, zero padding; rows without a common stride raise"""
    from UCF_VIT._hip import ops
    g = torch.Generator().manual_seed(11)
    a = torch.randn(2, 5, 6, 7, 4, generator=g).to(dtype).cuda()
    o = ops.pad_rows8(a)
    assert o.shape == (2, 5, 6, 7, 8) and o.dtype == torch.bfloat16 and o.is_contiguous()
    assert torch.equal(o[..., :4], a.bfloat16()) and o[..., 4:].abs().max() == 0
    wide = torch.randn(2, 5, 6, 7, 16, generator=g).to(dtype).cuda()
    o2 = ops.pad_rows8(wide[..., 8:11])
    assert torch.equal(o2[..., :3], wide[..., 8:11].bfloat16()) and o2[..., 3:].abs().max() == 0
    ncdhw_view = a.permute(0, 4, 1, 2, 3)                    # what the loss hands back; the head's backward sees movedim(1, -1) of it
    assert torch.equal(ops.pad_rows8(ncdhw_view.movedim(1, -1)), o)
    with pytest.raises(ValueError):
        ops.pad_rows8(a[:, ::2])
    with pytest.raises(TypeError):
        ops.pad_rows8(torch.zeros(4, 9, device="cuda"))


@pytest.mark.gpu
def test_conv3x3x3_single_channel_input_through_the_padded_operand():
    from UCF_VIT._hip import conv, ops
    g = torch.Generator().manual_seed(3)
    vol = torch.randn(2, 6, 9, 20, generator=g).cuda()
    w = (torch.randn(16, 1, 3, 3, 3, generator=g) * 0.2).cuda().requires_grad_(True)
    x8 = ops.pad_channels8(vol[:, None].contiguous())
    assert x8.shape == (2, 6, 9, 20, 8) and torch.equal(x8[..., 0].float(), vol.bfloat16().float()) and x8[..., 1:].abs().max() == 0
    v3 = torch.randn(2, 3, 4, 5, 6, generator=g).cuda()
    x3 = ops.pad_channels8(v3)
    assert torch.equal(x3[..., :3].float(), v3.permute(0, 2, 3, 4, 1).bfloat16().float()) and x3[..., 3:].abs().max() == 0
    y = conv.conv3x3x3(x8, w)
    dy = torch.randn(y.shape, generator=g).bfloat16().cuda()
    y.backward(dy)
    wr = w.detach().bfloat16().float().requires_grad_(True)
    yr = F.conv3d(vol.bfloat16().float()[:, None], wr, padding=1)
    yr.backward(_ncdhw(dy).float())
    assert _rel(_ncdhw(y), yr) < 1e-2
    assert w.grad.shape == (16, 1, 3, 3, 3) and _rel(w.grad, wr.grad) < 2e-3


@pytest.mark.gpu
@pytest.mark.parametrize("B,X,Y,Z,cin,cout", [(2, 3, 4, 5, 768, 128), (1, 4, 4, 4, 128, 64), (1, 5, 6, 7, 32, 16), (1, 2, 3, 4, 768, 32),
                                              (2, 3, 5, 19, 64, 64), (1, 4, 4, 33, 64, 32), (1, 3, 3, 16, 32, 32)])
def test_tconv2x2x2_forward_and_gradients(B, X, Y, Z, cin, cout):
    from UCF_VIT._hip import conv
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(B, cin, X, Y, Z, generator=g).bfloat16().cuda()
    w = (torch.randn(cin, cout, 2, 2, 2, generator=g) * cin ** -0.5).cuda()
    dy = torch.randn(B, cout, 2 * X, 2 * Y, 2 * Z, generator=g).bfloat16().cuda()
    xr, wr = x.float().requires_grad_(True), w.bfloat16().float().requires_grad_(True)
    yr = F.conv_transpose3d(xr, wr, stride=2)
    yr.backward(dy.float())
    xc, wp = _cl(x).requires_grad_(True), w.clone().requires_grad_(True)
    y = conv.tconv2x2x2(xc, wp)
    assert y.shape == (B, 2 * X, 2 * Y, 2 * Z, cout)
    y.backward(_cl(dy))
    assert _rel(_ncdhw(y), yr) < 1e-2
    assert _rel(_ncdhw(xc.grad), xr.grad) < 1e-2
    assert _rel(wp.grad, wr.grad) < 2e-3


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,cs", [(32, 16, 16), (128, 64, 64), (64, 32, 32)])
def test_tconv_with_skip_writes_the_concatenation_in_place(cin, cout, cs):
    """tconv2x2x2(x, w, skip) == cat(tconv2x2x2(x, w), skip) bit for bit, and so are all three gradients when the consumer is a normalisation
    (whose backward reads the skip half of the concatenation's gradient as a strided slice)"""
    from UCF_VIT._hip import conv
    g = torch.Generator().manual_seed(cin + cs)
    x = torch.randn(2, 3, 4, 5, cin, generator=g).bfloat16().cuda()
    w = (torch.randn(cin, cout, 2, 2, 2, generator=g) * cin ** -0.5).cuda()
    skip_pre = torch.randn(2, 6, 8, 10, cs, generator=g).bfloat16().cuda()
    dcat = torch.randn(2, 6, 8, 10, cout + cs, generator=g).bfloat16().cuda()
    res = []
    for fused in (False, True):
        xc, wp, sp = x.clone().requires_grad_(True), w.clone().requires_grad_(True), skip_pre.clone().requires_grad_(True)
        skip = conv.instnorm_act_cl(sp, None, 1e-5, 0.01)                     # the skip is a residual block's output: a normalisation
        cat = conv.tconv2x2x2(xc, wp, skip) if fused else torch.cat((conv.tconv2x2x2(xc, wp), skip), dim=-1)
        assert cat.shape == (2, 6, 8, 10, cout + cs) and cat.is_contiguous()
        cat.backward(dcat)
        res.append((cat.detach(), xc.grad, wp.grad, sp.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout", [(32, 16), (16, 16), (64, 32), (8, 16)])
def test_fused_res_block_equals_the_chain_of_layer_functions(cin, cout):
    """UnetResBlockFn (one autograd node; data gradients summed in the kernel epilogue) against conv3x3x3 / instnorm_act_cl / conv1x1x1 chained
    through autograd: same kernels in the same order, so the forward is bit-identical; the input gradient differs only by where the sum of
    its two branches is rounded to bf16 (fp32 + bf16 -> bf16 in the epilogue instead of bf16 + bf16 -> bf16)"""
    from UCF_VIT._hip import conv
    g = torch.Generator().manual_seed(cin * 7 + cout)
    want_dx = cin % 16 == 0
    wcin = 1 if cin == 8 else cin
    x = torch.randn(2, 5, 9, 20, cin, generator=g).bfloat16().cuda()
    if cin == 8:
        x[..., 1:] = 0
    w1 = (torch.randn(cout, wcin, 3, 3, 3, generator=g) * (2.0 / (27 * wcin)) ** 0.5).cuda()
    w2 = (torch.randn(cout, cout, 3, 3, 3, generator=g) * (2.0 / (27 * cout)) ** 0.5).cuda()
    w3 = (torch.randn(cout, wcin, 1, 1, 1, generator=g) * wcin ** -0.5).cuda() if wcin != cout else None
    dy = torch.randn(2, 5, 9, 20, cout, generator=g).bfloat16().cuda()
    outs = []
    for fused in (True, False):
        xc = x.clone().requires_grad_(want_dx)
        ws = [w.clone().requires_grad_(True) if w is not None else None for w in (w1, w2, w3)]
        if fused:
            y = conv.unet_res_block(xc, *ws)
        else:
            o = conv.instnorm_act_cl(conv.conv3x3x3(xc, ws[0]), None, 1e-5, 0.01)
            o = conv.conv3x3x3(o, ws[1])
            r = conv.instnorm_act_cl(conv.conv1x1x1(xc, ws[2]), None, 1e-5, 1.0) if w3 is not None else xc
            y = conv.instnorm_act_cl(o, r, 1e-5, 0.01)
        y.backward(dy)
        outs.append((y.detach(), xc.grad, [w.grad if w is not None else None for w in ws]))
    if w3 is None:
        assert torch.equal(outs[0][0], outs[1][0])
        for a, b in zip(outs[0][2], outs[1][2]):
            assert (a is None and b is None) or torch.equal(a, b)
    else:
        # the fused tail lrelu(norm(c2) + norm(c3)) never rounds the normalised 1x1x1 branch (nor its gradient) to bf16, and the normalisation
        # backward amplifies such roundings: judge both forms against the fp32 restatement of the block on the same operands —
        # the fused form must be about as close as the chain (slack for the noise of a single draw)
        from oracle import unetr_decoder_ref as R
        xr = _ncdhw(x).float()[:, :wcin].requires_grad_(True)
        wr = [w.detach().bfloat16().float().requires_grad_(True) for w in (w1, w2, w3)]
        yr = R.res_block(xr, wr[0], wr[1], wr[2])
        yr.backward(_ncdhw(dy).float())
        assert _rel(_ncdhw(outs[0][0]), yr) < 1e-2 and _rel(_ncdhw(outs[1][0]), yr) < 1e-2
        for a, b, ref in zip(outs[0][2], outs[1][2], wr):
            e_fused, e_chain = _rel(a, ref.grad), _rel(b, ref.grad)
            assert e_fused < 1.5 * e_chain + 5e-3, (e_fused, e_chain)       # the 1-channel 1x1x1 branch has a pure-cancellation gradient: noisy in both
        if want_dx:
            assert _rel(_ncdhw(outs[0][1]), xr.grad) < 1.1 * _rel(_ncdhw(outs[1][1]), xr.grad) + 2e-3
    if want_dx and w3 is None:
        assert _rel(outs[0][1], outs[1][1]) < 2e-2


@pytest.mark.gpu
def test_depth_to_space_round_trip_is_exact():
    from UCF_VIT._hip import ops
    cols = torch.randn(2 * 3 * 4 * 5, 8 * 16).bfloat16().cuda()
    y = ops.depth_to_space2(cols, 2, 3, 4, 5, 16)
    ref = cols.view(2, 3, 4, 5, 2, 2, 2, 16).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(2, 6, 8, 10, 16)
    assert torch.equal(y, ref)
    assert torch.equal(ops.space_to_depth2(y), cols)


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,bias,fp32", [(16, 4, True, True), (16, 3, True, True), (32, 16, False, False), (8, 16, False, False),
                                                (256, 128, False, False), (64, 32, False, False), (128, 64, True, False)])
def test_conv1x1x1_forward_and_gradients(cin, cout, bias, fp32):
    """the tall-skinny layers through the 1x1x1 instance of the convolution kernels (any channel count below 128), the wide one through the GEMM"""
    from UCF_VIT._hip import conv
    g = torch.Generator().manual_seed(cin)
    x = torch.randn(2, cin, 4, 5, 38, generator=g).bfloat16().cuda()
    w = (torch.randn(cout, cin, 1, 1, 1, generator=g) * cin ** -0.5).cuda()
    b = torch.randn(cout, generator=g).cuda() if bias else None
    dy = torch.randn(2, cout, 4, 5, 38, generator=g).bfloat16().cuda()
    xr, wr = x.float().requires_grad_(True), w.bfloat16().float().requires_grad_(True)
    br = b.detach().clone().requires_grad_(True) if bias else None
    yr = F.conv3d(xr, wr, br)
    yr.backward(dy.float())
    want_dx = cin % 16 == 0
    xc, wp = _cl(x).requires_grad_(want_dx), w.clone().requires_grad_(True)
    bp = b.detach().clone().requires_grad_(True) if bias else None
    y = conv.conv1x1x1(xc, wp, bp, out_fp32=fp32)
    assert y.shape == (2, 4, 5, 38, cout) and y.dtype == (torch.float32 if fp32 else torch.bfloat16) and y.is_contiguous()
    y.backward(_cl(dy).to(y.dtype))
    assert _rel(_ncdhw(y), yr) < (1e-4 if fp32 else 1e-2)
    if want_dx:
        assert _rel(_ncdhw(xc.grad), xr.grad) < 1e-2
    assert _rel(wp.grad, wr.grad) < 2e-3
    if bias:
        assert _rel(bp.grad, br.grad) < 2e-3


@pytest.mark.gpu
@pytest.mark.parametrize("C,with_res,slope", [(16, False, 0.01), (16, True, 0.01), (32, True, 0.01), (128, False, 1.0), (8, True, 0.01)])
def test_instnorm_channels_last_equals_the_row_layout_kernels_and_torch(C, with_res, slope):
    from UCF_VIT._hip import conv
    g = torch.Generator().manual_seed(C)
    B, dims = 2, (6, 10, 37)
    x = (torch.randn(B, C, *dims, generator=g) * 2 + 0.5).bfloat16().cuda()
    res = torch.randn(B, C, *dims, generator=g).bfloat16().cuda() if with_res else None
    dy = torch.randn(B, C, *dims, generator=g).bfloat16().cuda()
    xr = x.float().requires_grad_(True)
    rr = res.float().requires_grad_(True) if with_res else None
    n = F.instance_norm(xr, eps=1e-5)
    yr = F.leaky_relu(n + rr if with_res else n, slope)
    yr.backward(dy.float())
    xc = _cl(x).requires_grad_(True)
    rc = _cl(res).requires_grad_(True) if with_res else None
    y = conv.instnorm_act_cl(xc, rc, 1e-5, slope)
    y.backward(_cl(dy))
    assert _rel(_ncdhw(y), yr) < 1e-2
    assert _rel(_ncdhw(xc.grad), xr.grad) < 2e-2
    if with_res:
        assert _rel(_ncdhw(rc.grad), rr.grad) < 1e-2
        # a residual that needs no gradient: the mask still comes from the saved output (had_res), nothing is written for it
        xc2 = _cl(x).requires_grad_(True)
        y2 = conv.instnorm_act_cl(xc2, _cl(res), 1e-5, slope)
        y2.backward(_cl(dy))
        assert torch.equal(y2, y) and torch.equal(xc2.grad, xc.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [16, 64])
def test_dual_instnorm_tail_vs_torch(C):
    """out = lrelu(norm(x) + norm(x2)) (ucfvit_instnorm_cl_stats x 2 + _apply2) and its one-pair-of-passes backward (_bwd2) against torch fp32"""
    from UCF_VIT._hip import ops
    g = torch.Generator().manual_seed(C)
    B, dims = 2, (6, 10, 37)
    x = (torch.randn(B, C, *dims, generator=g) * 2 + 0.5).bfloat16().cuda()
    x2 = (torch.randn(B, C, *dims, generator=g) * 0.3 - 1.0).bfloat16().cuda()
    dy = torch.randn(B, C, *dims, generator=g).bfloat16().cuda()
    xr, x2r = x.float().requires_grad_(True), x2.float().requires_grad_(True)
    yr = F.leaky_relu(F.instance_norm(xr, eps=1e-5) + F.instance_norm(x2r, eps=1e-5), 0.01)
    yr.backward(dy.float())
    xc, x2c = _cl(x), _cl(x2)
    m, r = ops.instnorm_cl_stats(xc)
    m2, r2 = ops.instnorm_cl_stats(x2c)
    assert _rel(m, xr.detach().mean((2, 3, 4))) < 1e-4 and _rel(r2, (x2r.detach().var((2, 3, 4), unbiased=False) + 1e-5).rsqrt()) < 1e-4
    y = ops.instnorm_cl_apply2(xc, m, r, x2c, m2, r2, 0.01)
    assert _rel(_ncdhw(y), yr) < 1e-2
    dx, dx2 = ops.instnorm_cl_bwd2(_cl(dy), y, xc, m, r, x2c, m2, r2, 0.01)
    # the activation mask comes from the bf16 output: compare where the fp32 reference is not within rounding of zero
    assert _rel(_ncdhw(dx), xr.grad) < 2e-2 and _rel(_ncdhw(dx2), x2r.grad) < 2e-2
    # projections of the instance-norm backward: both gradients are orthogonal to the constant and to their own normalised input
    n2 = (x2r.detach() - x2r.detach().mean((2, 3, 4), keepdim=True)) * (x2r.detach().var((2, 3, 4), unbiased=False, keepdim=True) + 1e-5).rsqrt()
    d2 = _ncdhw(dx2).float()
    assert float(d2.mean((2, 3, 4)).abs().max()) < 2e-3 * float(d2.abs().max())
    assert float((d2 * n2).mean((2, 3, 4)).abs().max()) < 2e-3 * float(d2.abs().max())


@pytest.mark.gpu
def test_dice_ce_on_a_channels_last_view_equals_the_contiguous_call():
    from UCF_VIT._hip import ops
    g = torch.Generator().manual_seed(5)
    B, n, dims, ld = 2, 4, (5, 6, 7), 8
    buf = torch.randn(B, *dims, ld, generator=g).cuda()
    labels = torch.randint(0, n, (B, *dims), generator=g).cuda()
    view = buf[..., :n].permute(0, 4, 1, 2, 3)                   # [B, n, X, Y, Z] over channels-last memory with padded rows
    assert not view.is_contiguous()
    loss_v, dl_v = ops.dice_ce(view, labels)
    loss_c, dl_c = ops.dice_ce(view.contiguous(), labels)
    assert torch.equal(loss_v, loss_c)
    assert dl_v.shape == view.shape and dl_v.stride() == view.stride()
    assert torch.equal(dl_v.contiguous(), dl_c)
    with pytest.raises(RuntimeError):
        ops.dice_ce(buf[..., :n].permute(0, 4, 3, 2, 1), labels)
