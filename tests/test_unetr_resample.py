"""Align-corners trilinear resampling (csrc/resample.hip) and the pointwise transposed convolution of UnetrUpBlock(upsample_kernel_size=1):
the two layers a UNETR needs when its token grid times 16 is not the tile size (reference: src/UCF_VIT/simple/arch.py:887-906, 942-943,
989-991 — basic_ct/unetr: 64^3 tile, adaptive patching with a 9^3 token grid, dec1 72^3 -> 64^3).

CPU: the reference geometry now selects the HIP decoder, and the sequence-sharded (X-slab) decoder, which has no resampling step, refuses
a resampling geometry.  GPU: the kernels against torch.nn.functional.interpolate / conv_transpose3d on the same bf16 operands."""
import os
import socket
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

DEV = "cuda"


def _ref_geometry_kw(**over):
    """model.net.init_args of the reference's basic_ct/unetr config as UNETR keywords (depth reduced: the encoder is not what is tested)"""
    kw = dict(img_size=[64, 64, 64], patch_size=4, in_chans=1, embed_dim=768, depth=4, num_heads=12, mlp_ratio=4, twoD=False,
              default_vars=["ct_res1"], single_channel=True, use_varemb=False, adaptive_patching=True, fixed_length=729, use_adaptive_pos_emb=True,
              num_classes=4, class_token=False, linear_decoder=False, feature_size=16, skip_connection=True, sqrt_len=9, sqrt_len_method=True)
    kw.update(over)
    return kw


def test_reference_unetr_geometry_selects_the_hip_decoder():
    """patch 4 / adaptive patching with a 9^3 token grid on a 64^3 tile, no allow_torch_decoder: the whole decoder is on the HIP kernels
    (decoder2 is the pointwise transposed convolution, dec1 is resampled 72^3 -> 64^3)"""
    from UCF_VIT.simple.arch import UNETR
    torch.manual_seed(0)
    m = UNETR(**_ref_geometry_kw())
    assert not m.allow_torch_decoder
    assert m.feat_size == (9, 9, 9)
    assert tuple(m.decoder2.transp_conv.conv.weight.shape) == (32, 16, 1, 1, 1)
    assert m.resamples_dec1()
    assert m.hip_decoder() is True
    m.force_torch_decoder = True                    # only this selects torch
    assert m.hip_decoder() is False


def test_hip_decoder_rule_for_other_geometries():
    """a non-adaptive resampling geometry is covered too; patch 16 stays covered; a grid that matches the tile on the first axis only (the
    reference's decoder2 then up-samples by 2 and the concatenation with enc1 cannot line up) and 2-D models are not"""
    from UCF_VIT.simple.arch import UNETR
    kw = dict(in_chans=1, embed_dim=96, depth=4, num_heads=3, class_token=False, num_classes=4, linear_decoder=False, feature_size=16,
              skip_connection=True)
    m = UNETR(img_size=[48, 48, 48], patch_size=4, twoD=False, **kw)
    assert m.feat_size == (12, 12, 12) and m.resamples_dec1() and m.hip_decoder()
    m = UNETR(img_size=[32, 32, 32], patch_size=16, twoD=False, **kw)
    assert not m.resamples_dec1() and m.hip_decoder()
    assert tuple(m.decoder2.transp_conv.conv.weight.shape) == (32, 16, 2, 2, 2)
    assert not UNETR(img_size=[32, 40, 32], patch_size=16, twoD=False, **kw).hip_decoder()
    assert not UNETR(img_size=[32, 32], patch_size=4, twoD=True, **kw).hip_decoder()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard_guard_worker(rank, world, port, q):
    for p in (os.path.join(ROOT, "ucf-vit_amd"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from UCF_VIT.fsdp.arch import UNETR
        from UCF_VIT.fsdp.seq_parallel import make_seq_parallel_groups
        # sequence parallelism shards a plain token grid (the constructor asserts adaptive_patching off), so the resampling geometry under
        # it is the non-adaptive patch-4 one: 12^3 tokens (the first axis divides by 2) -> decoder3 at 96^3 -> resampled to 48^3
        kw = dict(img_size=[48, 48, 48], patch_size=4, in_chans=1, embed_dim=96, depth=4, num_heads=4, class_token=False, twoD=False,
                  num_classes=4, linear_decoder=False, feature_size=16, skip_connection=True, seq_par_size=world,
                  seq_par_group=make_seq_parallel_groups([list(range(world))], 4))
        res = {}
        m = UNETR(**kw)
        res["hip"], res["shard"] = m.hip_decoder(), m.shard_decoder()
        try:
            UNETR(shard_decoder=True, **kw).shard_decoder()
            res["forced"] = "no error"
        except ValueError as e:
            res["forced"] = "raised" if "resampling" in str(e) else str(e)
        kw.update(img_size=[64, 64, 64], patch_size=16)                   # control: a 4^3 grid without resampling still shards
        res["control"] = UNETR(**kw).shard_decoder()
        q.put((rank, res))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_sequence_sharded_decoder_refuses_a_resampling_geometry():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_guard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, r in res:
        assert r == {"hip": True, "shard": False, "forced": "raised", "control": True}, (rank, r)


# ---------------------------------------------------------------------------------------------------------------------------------- GPU
def _cl(t):           # [B, C, X, Y, Z] -> channels-last [B, X, Y, Z, C]
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _ncdhw(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


def _rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-20)).item()


def _ordered(t):
    """bf16 -> integers in the order of the values (adjacent bf16 numbers differ by 1; +0 and -0 are both 0)"""
    u = t.contiguous().view(torch.int16).int() & 0xFFFF
    mag = u & 0x7FFF
    return torch.where(u >= 0x8000, -mag, mag)


def _ulps(a, b):
    return (_ordered(a) - _ordered(b)).abs().max().item()


FWD_CASES = [  # (B, C, input extent, output extent)
    (1, 32, (72, 72, 72), (64, 64, 64)),         # dec1 of the reference geometry, resampled first (the reference's order)
    (2, 16, (72, 72, 72), (64, 64, 64)),         # ... and behind the pointwise layer (this build's order)
    (1, 16, (36, 36, 36), (64, 64, 64)),         # up
    (2, 32, (9, 10, 11), (9, 10, 11)),           # identity
    (2, 64, (18, 20, 7), (32, 16, 9)),           # anisotropic, mixed up / down
    (1, 128, (1, 5, 3), (4, 1, 3)),              # input extent 1 (both taps index 0), output extent 1 (scale 0)
    (2, 16, (6, 1, 1), (1, 7, 1)),
    (2, 128, (12, 12, 12), (48, 40, 5)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,src,dst", FWD_CASES)
def test_resample_forward_within_one_ulp_of_interpolate(B, C, src, dst):
    """the same bf16 operand through F.interpolate in fp32, rounded to bf16: at most 1 bf16 ulp apart (only the order of the fp32 operations
    may differ; a wrong index or weight would be far more).  The ulp bound needs operands without cancellation (non-negative: every fp32
    partial sum is within a few fp32 ulps of the exact one); for signed operands the bound holds wherever the result is not a
    cancellation to below 1e-3 of the operands, and an absolute bound of 1e-5 of the operands applies there."""
    from UCF_VIT._hip import conv
    g = torch.Generator().manual_seed(B * 1000 + C + sum(dst))
    xs = torch.randn(B, C, *src, generator=g)
    for x in (xs.abs().bfloat16().to(DEV), xs.bfloat16().to(DEV)):
        want = F.interpolate(x.float(), size=dst, mode="trilinear", align_corners=True)
        y = _ncdhw(conv.resample_trilinear(_cl(x), dst))
        assert tuple(y.shape) == tuple(want.shape) and y.dtype == torch.bfloat16
        if bool((x >= 0).all()):
            assert _ulps(y, want.bfloat16()) <= 1
        else:
            big = want.abs() >= 1e-3 * x.float().abs().max()                  # no cancellation below fp32 noise: the ulp bound holds
            assert _ulps(y[big], want[big].bfloat16()) <= 1
            err = (y.float() - want).abs()[~big]
            assert err.numel() == 0 or err.max().item() <= 1e-5 * x.float().abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("C,Cs,extra", [(16, 16, 0), (32, 16, 0), (16, 32, 16), (64, 0, 24)])
def test_resample_forward_into_a_channel_slice_with_skip(C, Cs, extra):
    """ld_dst > C: the resampled map lands in channels [0, C) of a wider buffer (bit-equal to the dense call), the skip map behind it
    bit-exact, and channels past C + Cs are not touched"""
    from UCF_VIT._hip import ops
    g = torch.Generator().manual_seed(C * 7 + Cs)
    B, src, dst = 2, (72, 9, 20), (64, 13, 16)
    x = _cl(torch.randn(B, C, *src, generator=g).bfloat16()).to(DEV)
    skip = torch.randn(B, *dst, Cs, generator=g).bfloat16().to(DEV) if Cs else None
    buf = torch.full((B, *dst, C + Cs + extra), 7.0, dtype=torch.bfloat16, device=DEV)
    out = ops.resample_trilinear(x, dst, out=buf[..., :C], skip=skip)
    assert out.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[..., :C], ops.resample_trilinear(x, dst))
    if Cs:
        assert torch.equal(buf[..., C:C + Cs], skip)
    assert bool((buf[..., C + Cs:] == 7.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,src,dst,ld", [(2, 16, (72, 72, 72), (64, 64, 64), 32), (1, 32, (36, 36, 36), (64, 64, 64), 32),
                                            (2, 64, (18, 20, 7), (32, 16, 9), 96), (1, 16, (1, 5, 3), (4, 1, 3), 16),
                                            (2, 128, (12, 12, 12), (48, 40, 5), 128), (1, 16, (6, 1, 1), (1, 7, 1), 24)])
def test_resample_backward_against_autograd_and_reproducible(B, C, src, dst, ld):
    """gather-form backward against torch's autograd of the fp32 interpolate on the same dy (dy a channel slice of a wider buffer when
    ld > C); two launches are bitwise equal"""
    from UCF_VIT._hip import ops
    g = torch.Generator().manual_seed(B * 100 + C + ld)
    x = torch.randn(B, C, *src, generator=g).bfloat16().float().to(DEV).requires_grad_(True)
    dbuf = torch.randn(B, *dst, ld, generator=g).bfloat16().to(DEV)
    dy = dbuf[..., :C]
    F.interpolate(x, size=dst, mode="trilinear", align_corners=True).backward(_ncdhw(dy).float())
    want = _cl(x.grad)
    dx = ops.resample_trilinear_bwd(dy, src)
    assert tuple(dx.shape) == (B, *src, C) and dx.dtype == torch.bfloat16
    err = (dx.float() - want).abs()
    assert bool((err <= want.abs() * 2 ** -8 + 1e-5 * want.abs().max()).all()), err.max().item()
    assert torch.equal(dx, ops.resample_trilinear_bwd(dy, src))
    assert torch.equal(dx, ops.resample_trilinear_bwd(dy.contiguous(), src))


@pytest.mark.gpu
def test_resample_autograd_with_skip():
    """resample_trilinear(x, size, skip) as one autograd node: the skip's gradient is the second half of the concatenation's gradient, x's is
    the gather of the first half"""
    from UCF_VIT._hip import conv, ops
    g = torch.Generator().manual_seed(5)
    x = _cl(torch.randn(2, 16, 18, 18, 18, generator=g).bfloat16()).to(DEV).requires_grad_(True)
    skip = torch.randn(2, 16, 16, 16, 16, generator=g).bfloat16().to(DEV).requires_grad_(True)
    dcat = torch.randn(2, 16, 16, 16, 32, generator=g).bfloat16().to(DEV)
    cat = conv.resample_trilinear(x, (16, 16, 16), skip)
    assert tuple(cat.shape) == (2, 16, 16, 16, 32) and cat.is_contiguous()
    cat.backward(dcat)
    assert torch.equal(cat[..., 16:], skip.detach())
    assert torch.equal(skip.grad, dcat[..., 16:])
    assert torch.equal(x.grad, ops.resample_trilinear_bwd(dcat[..., :16], (18, 18, 18)))


@pytest.mark.gpu
@pytest.mark.parametrize("B,X,Y,Z,cin,cout,cs", [(2, 9, 10, 11, 32, 16, 16), (1, 6, 7, 5, 64, 32, 32), (2, 5, 4, 9, 32, 16, 0),
                                                 (1, 4, 4, 4, 128, 64, 64)])
def test_tconv1x1x1_with_skip_forward_and_gradients(B, X, Y, Z, cin, cout, cs):
    """ConvTranspose3d(k=1, s=1, bias=False) + the concatenation with skip: output and the three gradients against F.conv_transpose3d +
    torch.cat in fp32 on the same bf16 operands (tolerances of tests/test_conv3d.py's tconv2x2x2 test)"""
    from UCF_VIT._hip import conv
    g = torch.Generator().manual_seed(cin + cout + cs)
    x = torch.randn(B, cin, X, Y, Z, generator=g).bfloat16().to(DEV)
    w = (torch.randn(cin, cout, 1, 1, 1, generator=g) * cin ** -0.5).to(DEV)
    skip = torch.randn(B, cs, X, Y, Z, generator=g).bfloat16().to(DEV)
    dcat = torch.randn(B, cout + cs, X, Y, Z, generator=g).bfloat16().to(DEV)
    xr, wr, sr = x.float().requires_grad_(True), w.bfloat16().float().requires_grad_(True), skip.float().requires_grad_(True)
    yr = F.conv_transpose3d(xr, wr)
    if cs:
        yr = torch.cat((yr, sr), 1)
    yr.backward(dcat.float())
    xc, wp = _cl(x).requires_grad_(True), w.clone().requires_grad_(True)
    sc = _cl(skip).requires_grad_(True) if cs else None
    y = conv.tconv1x1x1(xc, wp, sc)
    assert tuple(y.shape) == (B, X, Y, Z, cout + cs) and y.is_contiguous()
    y.backward(_cl(dcat))
    assert _rel(_ncdhw(y), yr) < 1e-2
    assert _rel(_ncdhw(xc.grad), xr.grad) < 1e-2
    assert _rel(wp.grad, wr.grad) < 2e-3 and wp.grad.shape == w.shape
    if cs:
        assert torch.equal(_ncdhw(y)[:, cout:], skip)
        assert torch.equal(_ncdhw(sc.grad), dcat[:, cout:])


@pytest.mark.gpu
def test_tconv1x1x1_resample_against_the_reference_order():
    """decoder2's two layers in the commuted order (pointwise at 72^3, then the resampling of its 16 channels into the concatenation) against
    the reference's order in fp32 (resample the 32 channels, then the pointwise layer, then torch.cat): forward and all three gradients"""
    from UCF_VIT._hip import conv
    g = torch.Generator().manual_seed(11)
    B, src, dst = 2, (36, 36, 36), (32, 32, 32)
    x = torch.randn(B, 32, *src, generator=g).bfloat16().to(DEV)
    w = (torch.randn(32, 16, 1, 1, 1, generator=g) * 32 ** -0.5).to(DEV)
    skip = torch.randn(B, 16, *dst, generator=g).bfloat16().to(DEV)
    dcat = torch.randn(B, 32, *dst, generator=g).bfloat16().to(DEV)
    xr, wr, sr = x.float().requires_grad_(True), w.bfloat16().float().requires_grad_(True), skip.float().requires_grad_(True)
    yr = torch.cat((F.conv_transpose3d(F.interpolate(xr, size=dst, mode="trilinear", align_corners=True), wr), sr), 1)
    yr.backward(dcat.float())
    xc, wp, sc = _cl(x).requires_grad_(True), w.clone().requires_grad_(True), _cl(skip).requires_grad_(True)
    y = conv.tconv1x1x1_resample(xc, wp, dst, sc)
    y.backward(_cl(dcat))
    assert _rel(_ncdhw(y), yr) < 1e-2
    assert _rel(_ncdhw(xc.grad), xr.grad) < 1e-2
    assert _rel(wp.grad, wr.grad) < 5e-3
    assert torch.equal(_ncdhw(sc.grad), dcat[:, 16:])
