"""The UNETR decoder's HIP kernels at the geometry they are measured at: BASELINE config 5 (bench.py --workload unetr_512x512x128: B = 2,
patch 16, D = 768, feature_size 16, 4 classes).  At this size the host code of csrc/conv3d.hip picks other kernels than the small-volume tests
reach: the column kernels (>= 512 workgroups), a weight-gradient grid whose workgroups walk many tiles (tiles_per_wg > 1), a 2^31-element
concatenation at full resolution, statistics folded from ~65k partial rows per batch element.

Exact tier: operands in {-1, 0, 1} are exact in bf16 and every product and partial sum is an integer below 2^24, exact in fp32 whatever the
summation order.  A correct forward / data gradient therefore equals, bit for bit, the round-to-nearest-even bf16 of the exact integer sum,
and a correct weight gradient equals the integer sum itself.  The references gather the 27 neighbourhoods of the compared voxels and
multiply in fp64; they never call the project's kernels.

Real-valued tier: normal operands, one bounded check per operation against fp64, each bound written per element and scaled by the operands,
and each one shown to reject a reference that is wrong by one voxel (shifted) or by mirrored taps."""
import pytest
import torch

B = 2
VOL = (512, 512, 128)
FEAT = (32, 32, 8)

# (extent of the layer's output, layer, op, Cin, Cout) at the bench config; op: conv3 (3x3x3, stride 1), conv1 (1x1x1), tconv (2x2x2 stride 2,
# whose input is half the extent), head (1x1x1 with bias, fp32 logits).  Cin is the model's (the one-channel volume is padded to 8 on the device).
GEOMETRY = [
    ((512, 512, 128), "encoder1.layer.conv1", "conv3", 1, 16),
    ((512, 512, 128), "encoder1.layer.conv2", "conv3", 16, 16),
    ((512, 512, 128), "encoder1.layer.conv3", "conv1", 1, 16),
    ((64, 64, 16), "encoder2.transp_conv_init", "tconv", 768, 32),
    ((128, 128, 32), "encoder2.blocks.0.0", "tconv", 32, 32),
    ((128, 128, 32), "encoder2.blocks.0.1.conv1", "conv3", 32, 32),
    ((128, 128, 32), "encoder2.blocks.0.1.conv2", "conv3", 32, 32),
    ((256, 256, 64), "encoder2.blocks.1.0", "tconv", 32, 32),
    ((256, 256, 64), "encoder2.blocks.1.1.conv1", "conv3", 32, 32),
    ((256, 256, 64), "encoder2.blocks.1.1.conv2", "conv3", 32, 32),
    ((64, 64, 16), "encoder3.transp_conv_init", "tconv", 768, 64),
    ((128, 128, 32), "encoder3.blocks.0.0", "tconv", 64, 64),
    ((128, 128, 32), "encoder3.blocks.0.1.conv1", "conv3", 64, 64),
    ((128, 128, 32), "encoder3.blocks.0.1.conv2", "conv3", 64, 64),
    ((64, 64, 16), "encoder4.transp_conv_init", "tconv", 768, 128),
    ((64, 64, 16), "decoder5.transp_conv", "tconv", 768, 128),
    ((64, 64, 16), "decoder5.conv_block.conv1", "conv3", 256, 128),
    ((64, 64, 16), "decoder5.conv_block.conv2", "conv3", 128, 128),
    ((64, 64, 16), "decoder5.conv_block.conv3", "conv1", 256, 128),
    ((128, 128, 32), "decoder4.transp_conv", "tconv", 128, 64),
    ((128, 128, 32), "decoder4.conv_block.conv1", "conv3", 128, 64),
    ((128, 128, 32), "decoder4.conv_block.conv2", "conv3", 64, 64),
    ((128, 128, 32), "decoder4.conv_block.conv3", "conv1", 128, 64),
    ((256, 256, 64), "decoder3.transp_conv", "tconv", 64, 32),
    ((256, 256, 64), "decoder3.conv_block.conv1", "conv3", 64, 32),
    ((256, 256, 64), "decoder3.conv_block.conv2", "conv3", 32, 32),
    ((256, 256, 64), "decoder3.conv_block.conv3", "conv1", 64, 32),
    ((512, 512, 128), "decoder2.transp_conv", "tconv", 32, 16),
    ((512, 512, 128), "decoder2.conv_block.conv1", "conv3", 32, 16),
    ((512, 512, 128), "decoder2.conv_block.conv2", "conv3", 16, 16),
    ((512, 512, 128), "decoder2.conv_block.conv3", "conv1", 32, 16),
    ((512, 512, 128), "out", "head", 16, 4),
]


def _derive_geometry(model):
    """walk the decoder modules of a UNETR and list (output extent, layer, op, Cin, Cout) in GEOMETRY's order"""
    rows = []

    def up(e):
        return tuple(2 * v for v in e)

    def res(name, blk, ext):
        for k in ("conv1", "conv2"):
            w = getattr(blk, k).conv.weight
            rows.append((ext, f"{name}.{k}", "conv3", w.shape[1], w.shape[0]))
        if blk.downsample:
            w = blk.conv3.conv.weight
            rows.append((ext, f"{name}.conv3", "conv1", w.shape[1], w.shape[0]))

    def tconv(name, mod, ext):
        w = mod.conv.weight                                           # ConvTranspose3d: [Cin, Cout, 2, 2, 2]
        assert tuple(w.shape[2:]) == (2, 2, 2)
        rows.append((up(ext), name, "tconv", w.shape[0], w.shape[1]))
        return up(ext)

    res("encoder1.layer", model.encoder1.layer, VOL)
    for name in ("encoder2", "encoder3", "encoder4"):
        m = getattr(model, name)
        ext = tconv(f"{name}.transp_conv_init", m.transp_conv_init, tuple(model.feat_size))
        for i, b in enumerate(m.blocks):
            ext = tconv(f"{name}.blocks.{i}.0", b[0], ext)
            res(f"{name}.blocks.{i}.1", b[1], ext)
    ext = tuple(model.feat_size)
    for name in ("decoder5", "decoder4", "decoder3", "decoder2"):
        m = getattr(model, name)
        ext = tconv(f"{name}.transp_conv", m.transp_conv, ext)
        res(f"{name}.conv_block", m.conv_block, ext)
    w = model.out.conv.conv.weight
    assert model.out.conv.conv.bias is not None
    rows.append((ext, "out", "head", w.shape[1], w.shape[0]))
    return rows


def test_geometry_table_matches_the_bench_model():
    """CPU: GEOMETRY is what UCF_VIT.simple.arch.UNETR builds with the bench workload's arguments (depth 4: the skip taps need depth >= 4)"""
    from UCF_VIT.simple.arch import UNETR
    from UCF_VIT.utils.fused_attn import FusedAttn
    m = UNETR(img_size=list(VOL), patch_size=16, in_chans=1, embed_dim=768, depth=4, num_heads=12, class_token=False, twoD=False,
              num_classes=4, linear_decoder=False, feature_size=16, skip_connection=True, FusedAttn_option=FusedAttn.HIP)
    assert tuple(m.feat_size) == FEAT
    got = [(tuple(e), n, op, int(ci), int(co)) for e, n, op, ci, co in _derive_geometry(m)]
    assert sorted(got, key=lambda r: r[1]) == sorted(GEOMETRY, key=lambda r: r[1])


# ------------------------------------------------------------------------------------------------------------------------- helpers (GPU)
def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _tern(shape, g):
    """integers in {-1, 0, 1} as bf16, generated on the device"""
    return torch.randint(-1, 2, shape, device="cuda", generator=g, dtype=torch.int8).to(torch.bfloat16)


def _samples(Bn, X, Y, Z, n, g):
    """linear voxel indices into [Bn, X, Y, Z]: n random voxels, the 8 corners, the face and edge voxels of the first and last X-plane,
    n / 4 voxels on the seams of the kernels' tiles (z at multiples of 16 +- 1, y at multiples of 4 / 8 +- 1, x at both parities), and the
    whole first and last X-plane of every batch element (the last one of the last batch element lies above 2 GiB of a 32-channel map)"""
    dev = "cuda"
    V = Bn * X * Y * Z
    parts = [torch.randint(0, V, (n,), device=dev, generator=g)]

    def lin(b, x, y, z):
        return ((b * X + x) * Y + y) * Z + z

    ys, zs = torch.arange(Y, device=dev), torch.arange(Z, device=dev)
    for b in range(Bn):
        for x in (0, X - 1):
            for y in (0, Y - 1):
                parts.append(lin(b, x, y, zs))
            for z in (0, Z - 1):
                parts.append(lin(b, x, ys, z))
            yy, zz = torch.meshgrid(ys, zs, indexing="ij")
            parts.append(lin(b, x, yy.reshape(-1), zz.reshape(-1)))
    m = max(n // 4, 1)
    r = lambda hi: torch.randint(0, hi, (m,), device=dev, generator=g)        # noqa: E731
    zseam = (r(max(Z // 16, 1)) * 16 + r(2) - 1).clamp(0, Z - 1)
    yseam = (r(max(Y // 4, 1)) * 4 + r(2) - 1).clamp(0, Y - 1)
    parts.append(lin(r(Bn), r(X), yseam, zseam))
    return torch.unique(torch.cat(parts))


_OFFS = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]     # tap t = w[..., a + 1, b + 1, c + 1]


def _gather27(t, idx, sign=1):
    """t [Bn, X, Y, Z, C] -> fp64 [len(idx), 27, C]: t at voxel idx + sign * offset of every tap, zero outside the volume"""
    Bn, X, Y, Z, C = t.shape
    flat = t.view(-1, C)
    z = idx % Z
    y = (idx // Z) % Y
    x = (idx // (Z * Y)) % X
    b = idx // (Z * Y * X)
    out = torch.empty((idx.numel(), 27, C), dtype=torch.float64, device=t.device)
    for k, (a, bb, c) in enumerate(_OFFS):
        xi, yi, zi = x + sign * a, y + sign * bb, z + sign * c
        ok = (xi >= 0) & (xi < X) & (yi >= 0) & (yi < Y) & (zi >= 0) & (zi < Z)
        li = ((b * X + xi.clamp(0, X - 1)) * Y + yi.clamp(0, Y - 1)) * Z + zi.clamp(0, Z - 1)
        out[:, k] = flat[li].double() * ok[:, None]
    return out


def _conv_ref(x, w, idx, chunk=1 << 15):
    """fp64 Conv3d(k=3, p=1) of x (channels-last) with w [Cout, Cin, 3, 3, 3] at the voxels idx -> [len(idx), Cout]"""
    wt = w.double().reshape(w.shape[0], w.shape[1], 27).permute(0, 2, 1)           # [Cout, tap, Cin]
    return torch.cat([torch.einsum("ntc,otc->no", _gather27(x, idx[i:i + chunk]), wt) for i in range(0, idx.numel(), chunk)])


def _dgrad_ref(dy, w, idx, chunk=1 << 15):
    """fp64 data gradient of that convolution at the voxels idx: dx[v, ci] = sum_{tap, co} dy[v - offset(tap), co] w[co, ci, tap]"""
    wt = w.double().reshape(w.shape[0], w.shape[1], 27)                            # [Cout, Cin, tap]
    return torch.cat([torch.einsum("nto,oit->ni", _gather27(dy, idx[i:i + chunk], -1), wt) for i in range(0, idx.numel(), chunk)])


def _wgrad_ref(x, dy, vox, chunk=1 << 15):
    """fp64 weight gradient [Cout, Cin, 3, 3, 3] summed over the voxels vox (those where dy is nonzero)"""
    Cin, Cout = x.shape[-1], dy.shape[-1]
    acc = torch.zeros((Cout, 27, Cin), dtype=torch.float64, device=x.device)
    d2 = dy.view(-1, Cout)
    for i in range(0, vox.numel(), chunk):
        v = vox[i:i + chunk]
        acc += torch.einsum("no,ntc->otc", d2[v].double(), _gather27(x, v))
    return acc.permute(0, 2, 1).reshape(Cout, Cin, 3, 3, 3)


def _lib():
    from UCF_VIT._hip import lib
    return lib.load()


def _tiles_per_wg(Bn, X, Y, Z, cin, cout):
    """the weight-gradient launch's tiles per workgroup, from its workspace: n_wg partial rows of ucfvit_conv3d_wgrad_size floats each"""
    L = _lib()
    n_wg = L.ucfvit_conv3d_wgrad_workspace(Bn, X, Y, Z, cin, cout, 3) // (4 * L.ucfvit_conv3d_wgrad_size(cin, cout, 3))
    tiles = Bn * -(-X // 2) * -(-Y // 4) * -(-Z // 32)                 # 2 x 4 x 32-voxel tiles
    return -(-tiles // n_wg)


# ------------------------------------------------------------------------------------------------------------- exact tier: forward / dgrad
# (extent, Cin, Cout, with data gradient): every 3x3x3 layer shape of GEOMETRY (the input volume padded to 8 channels)
CONV3_LAYERS = [
    ((512, 512, 128), 8, 16, False),      # encoder1 conv1: 8-channel column kernel
    ((512, 512, 128), 16, 16, True),      # encoder1 / decoder2 conv2: the 16-channel SHARE column kernel
    ((512, 512, 128), 32, 16, True),      # decoder2 conv1 on the 2^31-element concatenation; its data gradient accumulates into dinp
    ((256, 256, 64), 32, 32, True),
    ((256, 256, 64), 64, 32, True),       # decoder3 conv1: multi-chunk kernel, Z = 64
    ((128, 128, 32), 32, 32, True),
    ((128, 128, 32), 64, 64, True),
    ((128, 128, 32), 128, 64, True),      # decoder4 conv1: multi-chunk kernel, Z = 32
    ((64, 64, 16), 256, 128, True),       # decoder5 conv1
    ((64, 64, 16), 128, 128, True),       # decoder5 conv2: multi-chunk kernel, Z = 16
]
NSAMP = 1 << 20


@pytest.mark.gpu
@pytest.mark.parametrize("ext,cin,cout,dgrad", CONV3_LAYERS, ids=[f"{e[0]}-{ci}-{co}" for e, ci, co, _ in CONV3_LAYERS])
def test_conv3_forward_and_data_gradient_are_exact(ext, cin, cout, dgrad):
    from UCF_VIT._hip import conv, ops
    X, Y, Z = ext
    L = _lib()
    g = _gen(cin * 1000 + cout + X)
    whole = B * X * Y * Z <= (1 << 21)                                 # whole volume where the reference is affordable
    # the column kernels serve these launches (their statistics epilogue exists only there)
    assert L.ucfvit_conv3d_fwd_stats_rows(B, X, Y, Z, cin, cout, 3, 0) > 0
    x = _tern((B, X, Y, Z, cin), g)
    w = _tern((cout, cin, 3, 3, 3), g).float()
    idx = torch.arange(B * X * Y * Z, device="cuda") if whole else _samples(B, X, Y, Z, NSAMP, g)
    y = ops.conv3d_fwd(x, conv.pack_conv_weight(w), cout)
    ref = _conv_ref(x, w, idx)
    assert float(ref.abs().max()) < 2 ** 24
    assert torch.equal(y.view(-1, cout)[idx], ref.float().bfloat16())
    del y, ref
    if not dgrad:
        return
    assert L.ucfvit_conv3d_fwd_stats_rows(B, X, Y, Z, cout, cin, 3, 0) > 0
    dy = _tern((B, X, Y, Z, cout), g)
    ref = _dgrad_ref(dy, w, idx)
    wd = conv.pack_conv3_weight_dgrad(w)
    if ext == VOL:
        # the residual block's form: dinp (the 1x1x1 branch's data gradient) += the 3x3x3 branch, bf16(base + sum) in the epilogue
        base = x.clone()
        del x
        ref = ref + base.view(-1, cin)[idx].double()                  # (read before the kernel adds into it in place)
        ops.conv3d_fwd(dy, wd, cin, accumulate_into=base)
        got = base
    else:
        del x
        got = ops.conv3d_fwd(dy, wd, cin)
    assert torch.equal(got.view(-1, cin)[idx], ref.float().bfloat16())


# ----------------------------------------------------------------------------------------------------------- exact tier: weight gradient
# (extent, Cin, Cout, dy density): sparse dy (1 / 16 of the voxels) where the dense sums would pass 2^24
WGRAD_LAYERS = [
    ((512, 512, 128), 8, 16, 16),         # encoder1 conv1 (direct)
    ((512, 512, 128), 16, 16, 16),
    ((512, 512, 128), 32, 16, 16),        # decoder2 conv1: the mirrored role (Cout = 16 under a 32-channel input)
    ((256, 256, 64), 64, 32, 16),
    ((256, 256, 64), 32, 32, 16),
    ((128, 128, 32), 128, 64, 1),
    ((128, 128, 32), 64, 64, 1),
    ((64, 64, 16), 256, 128, 1),
    ((64, 64, 16), 128, 128, 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("ext,cin,cout,sparse", WGRAD_LAYERS, ids=[f"{e[0]}-{ci}-{co}" for e, ci, co, _ in WGRAD_LAYERS])
def test_conv3_weight_gradient_is_exact(ext, cin, cout, sparse):
    from UCF_VIT._hip import conv
    X, Y, Z = ext
    g = _gen(cin * 7 + cout + X)
    mirrored = cout == 16 and cin >= 32
    tpw = _tiles_per_wg(B, X, Y, Z, cout, cin) if mirrored else _tiles_per_wg(B, X, Y, Z, cin, cout)
    if ext == VOL:
        assert tpw > 1, tpw                                           # each workgroup walks many tiles (256 at the bench volume)
    x = _tern((B, X, Y, Z, cin), g)
    dy = _tern((B, X, Y, Z, cout), g)
    if sparse > 1:
        keep = torch.randint(0, sparse, (B, X, Y, Z, 1), device="cuda", generator=g) == 0
        dy.mul_(keep)
        vox = keep.view(-1).nonzero().view(-1)
        del keep
    else:
        vox = torch.arange(B * X * Y * Z, device="cuda")
    assert vox.numel() < 2 ** 24                                       # every partial sum is an integer below 2^24
    got = conv.conv3_wgrad(x, dy, cin, cout)
    assert tuple(got.shape) == (cout, cin, 3, 3, 3)
    ref = _wgrad_ref(x, dy, vox)
    assert torch.equal(got, ref.float())


# ------------------------------------------------------------------------------------------------------------ exact tier: pointwise layers
def _up_ref(x, w):
    """ConvTranspose3d(k=2, s=2) of channels-last x [Bn, X, Y, Z, Cin] with w [Cin, Cout, 2, 2, 2] in fp64 -> [Bn, 2X, 2Y, 2Z, Cout]"""
    Bn, X, Y, Z, Cin = x.shape
    Cout = w.shape[1]
    cols = x.reshape(-1, Cin).double() @ w.double().permute(0, 2, 3, 4, 1).reshape(Cin, 8 * Cout)
    return cols.view(Bn, X, Y, Z, 2, 2, 2, Cout).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(Bn, 2 * X, 2 * Y, 2 * Z, Cout)


def _down(d, Cout):
    """[Bn, 2X, 2Y, 2Z, >= Cout] -> [Bn X Y Z, 8 Cout] fp64 with column blocks (dx, dy, dz, co)"""
    Bn, X2, Y2, Z2 = d.shape[:4]
    t = d[..., :Cout].double().reshape(Bn, X2 // 2, 2, Y2 // 2, 2, Z2 // 2, 2, Cout).permute(0, 1, 3, 5, 2, 4, 6, 7)
    return t.reshape(-1, 8 * Cout)


# (input extent, Cin, Cout, skip channels): decoder2 into the 2^31-element concatenation, decoder4 (128 -> 64, GEMM path), the 768-wide GEMMs
TCONV_LAYERS = [((256, 256, 64), 32, 16, 16), ((64, 64, 16), 128, 64, 64), (FEAT, 768, 128, 128), (FEAT, 768, 64, 0), (FEAT, 768, 32, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("ext,cin,cout,cs", TCONV_LAYERS, ids=[f"{e[0]}-{ci}-{co}-{cs}" for e, ci, co, cs in TCONV_LAYERS])
def test_tconv_forward_and_gradients_are_exact(ext, cin, cout, cs):
    from UCF_VIT._hip import conv
    X, Y, Z = ext
    g = _gen(cin + cout + X)
    x = _tern((B, X, Y, Z, cin), g).requires_grad_(True)
    w = _tern((cin, cout, 2, 2, 2), g).float().requires_grad_(True)
    skip = _tern((B, 2 * X, 2 * Y, 2 * Z, cs), g).requires_grad_(True) if cs else None
    out = conv.tconv2x2x2(x, w, skip)
    assert out.shape == (B, 2 * X, 2 * Y, 2 * Z, cout + cs)
    if cs:
        assert out.numel() <= 2 ** 31 and torch.equal(out[..., cout:], skip.detach())
    xs = max(1, (1 << 20) // (Y * Z))                                  # input X-rows per slab of the fp64 references (~1 M voxels)
    for b in range(B):
        for i in range(0, X, xs):
            assert torch.equal(out[b:b + 1, 2 * i:2 * (i + xs), ..., :cout], _up_ref(x.detach()[b:b + 1, i:i + xs], w.detach()).float().bfloat16())
    dout = _tern(tuple(out.shape), g)
    out.backward(dout)
    del out
    w8 = w.detach().double().permute(0, 2, 3, 4, 1).reshape(cin, 8 * cout)          # [Cin, (dx, dy, dz, co)]
    dw = torch.zeros((cin, 8 * cout), dtype=torch.float64, device="cuda")
    for b in range(B):
        for i in range(0, X, xs):
            dcols = _down(dout[b:b + 1, 2 * i:2 * (i + xs)], cout)
            xb = x.detach()[b:b + 1, i:i + xs].reshape(-1, cin).double()
            assert torch.equal(x.grad[b:b + 1, i:i + xs].reshape(-1, cin), (dcols @ w8.t()).float().bfloat16())
            dw += xb.t() @ dcols
            del dcols, xb
    assert torch.equal(w.grad, dw.view(cin, 2, 2, 2, cout).permute(0, 4, 1, 2, 3).float())
    if cs:
        assert torch.equal(skip.grad, dout[..., cout:])


# (Cin of the kernel operand, Cin of the model, Cout, bias + fp32 output): the 1x1x1 layers at full resolution
POINTWISE_LAYERS = [(8, 1, 16, False), (32, 32, 16, False), (16, 16, 4, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("cin_x,cin,cout,head", POINTWISE_LAYERS)
def test_pointwise_layers_at_full_resolution_are_exact(cin_x, cin, cout, head):
    """encoder1's 1x1x1 branch (the padded one-channel volume), decoder2's 1x1x1 branch on the concatenation, the output head (fp32 logits
    with bias).  Sparse dy (1 / 16 of the voxels) keeps the weight-gradient sums below 2^24."""
    from UCF_VIT._hip import conv
    X, Y, Z = VOL
    g = _gen(cin_x + cout)
    x = _tern((B, X, Y, Z, cin_x), g)
    if cin < cin_x:
        x[..., cin:] = 0
    x.requires_grad_(cin_x % 16 == 0)
    w = _tern((cout, cin, 1, 1, 1), g).float().requires_grad_(True)
    b = torch.randint(-3, 4, (cout,), device="cuda", generator=g).float().requires_grad_(True) if head else None
    y = conv.conv1x1x1(x, w, b, out_fp32=head)
    w2 = torch.zeros((cout, cin_x), dtype=torch.float64, device="cuda")
    w2[:, :cin] = w.detach().double().view(cout, cin)
    x2 = x.detach().view(-1, cin_x)
    step = 1 << 22
    for i in range(0, x2.shape[0], step):
        ref = x2[i:i + step].double() @ w2.t() + (b.detach().double() if head else 0.0)
        got = y.view(-1, cout)[i:i + step]
        assert torch.equal(got, ref.float() if head else ref.float().bfloat16())
    keep = torch.randint(0, 16, (B, X, Y, Z, 1), device="cuda", generator=g) == 0
    dy = (_tern((B, X, Y, Z, cout), g) * keep).to(y.dtype)
    del keep
    y.backward(dy)
    d2 = dy.view(-1, cout)
    dw = torch.zeros((cout, cin_x), dtype=torch.float64, device="cuda")
    db = torch.zeros(cout, dtype=torch.float64, device="cuda")
    for i in range(0, x2.shape[0], step):
        di = d2[i:i + step].double()
        dw += di.t() @ x2[i:i + step].double()
        db += di.sum(0)
        if x.grad is not None:
            assert torch.equal(x.grad.view(-1, cin_x)[i:i + step], (di @ w2).float().bfloat16())
    assert torch.equal(w.grad.view(cout, cin), dw[:, :cin].float())
    if head:
        assert torch.equal(b.grad, db.float())


# --------------------------------------------------------------------------------------------------------------------- real-valued tier
def _rows64(t, C, step=1 << 22):
    """per (batch, channel) fp64 sum and centred sum of squares of a channels-last map over all its voxels -> (mean, var) [B, C]"""
    Bn = t.shape[0]
    v = t.view(Bn, -1, C)
    S = v.shape[1]
    s = sum(v[:, i:i + step].double().sum(1) for i in range(0, S, step))
    mean = s / S
    q = sum(((v[:, i:i + step].double() - mean[:, None]) ** 2).sum(1) for i in range(0, S, step))
    return mean, q / S


@pytest.mark.gpu
@pytest.mark.parametrize("cin", [16, 32])
def test_epilogue_statistics_at_full_resolution(cin):
    """the column kernel's statistics epilogue (decoder2 conv2 / conv1, ~65k partial rows per batch element) against the fp64 statistics of
    the stored output over the whole volume"""
    from UCF_VIT._hip import conv, ops
    X, Y, Z = VOL
    cout = 16
    L = _lib()
    rows = L.ucfvit_conv3d_fwd_stats_rows(B, X, Y, Z, cin, cout, 3, 0)
    assert rows > 0
    g = _gen(cin + 5)
    x = torch.randn((B, X, Y, Z, cin), device="cuda", generator=g, dtype=torch.bfloat16).add_(1.0)     # a channel mean of the order of its spread
    w = torch.randn((cout, cin, 3, 3, 3), device="cuda", generator=g) * (2.0 / (27 * cin)) ** 0.5
    y, mean, rstd = ops.conv3d_fwd(x, conv.pack_conv_weight(w), cout, stats_eps=1e-5)
    del x
    m_ref, v_ref = _rows64(y, cout)
    sd = v_ref.sqrt()
    r_ref = (v_ref + 1e-5).rsqrt()

    def ok(m_r, r_r):
        # mean: fp32 partial means over <= 2^16 voxels, folded in double: 2^-14 of the spread; rstd: 1e-4 relative (fp32 M2 of each row)
        return bool(((mean.double() - m_r).abs() <= 2 ** -14 * sd + 2 ** -22 * m_r.abs()).all()) and \
            bool(((rstd.double() - r_r).abs() <= 1e-4 * r_r).all())
    assert ok(m_ref, r_ref)
    # negative control: the statistics of the volume shifted by one X-plane (the first plane dropped) must be rejected
    m_sh, v_sh = _rows64(y[:, 1:].contiguous(), cout)
    assert not ok(m_sh, (v_sh + 1e-5).rsqrt())


@pytest.mark.gpu
def test_normalisation_passes_at_full_resolution():
    """instnorm_cl_apply / _bwd (with a residual) and _apply2 / _bwd2 on [2, 512, 512, 128, 16] against the fp64 formulas at sampled voxels;
    the global sums of the backward passes are taken in fp64 over the whole volume"""
    from UCF_VIT._hip import ops
    X, Y, Z = VOL
    C, slope = 16, 0.01
    g = _gen(77)
    x = torch.randn((B, X, Y, Z, C), device="cuda", generator=g, dtype=torch.bfloat16).mul_(2).add_(0.5)
    x2 = torch.randn((B, X, Y, Z, C), device="cuda", generator=g, dtype=torch.bfloat16).mul_(0.5).sub_(1)
    m, v = _rows64(x, C)
    m2, v2 = _rows64(x2, C)
    r, r2 = (v + 1e-5).rsqrt(), (v2 + 1e-5).rsqrt()
    mf, rf, m2f, r2f = (t.float().contiguous() for t in (m, r, m2, r2))
    idx = _samples(B, X, Y, Z, NSAMP, g)
    bi = idx // (X * Y * Z)

    def at(t):
        return t.view(-1, C)[idx].double()

    def lrelu(t):
        return torch.where(t > 0, t, slope * t)

    def check(got, ref, scale, shifted):
        # bf16 output (2^-9 relative) + fp32 evaluation of (x - mean) rstd: 2^-8 |ref| + 2^-12 of the operands' scale
        bound = 2 ** -8 * ref.abs() + 2 ** -12 * scale
        assert bool(((got - ref).abs() <= bound).all())
        assert not bool(((got - shifted).abs() <= bound).all())       # negative control: the reference one voxel over (z + 1)

    idx_sh = idx - idx % Z + (idx % Z + 1) % Z
    xh = (at(x) - m[bi]) * r[bi]
    x2h = (at(x2) - m2[bi]) * r2[bi]
    # apply with a residual (x2 as the residual), apply2
    y = ops.instnorm_cl_apply(x, mf, rf, x2, slope)
    ref1 = lrelu(xh + at(x2))
    sh1 = lrelu((x.view(-1, C)[idx_sh].double() - m[bi]) * r[bi] + x2.view(-1, C)[idx_sh].double())
    check(at(y), ref1, 1.0 + xh.abs() + at(x2).abs(), sh1)
    yy = ops.instnorm_cl_apply2(x, mf, rf, x2, m2f, r2f, slope)
    ref2 = lrelu(xh + x2h)
    sh2 = lrelu((x.view(-1, C)[idx_sh].double() - m[bi]) * r[bi] + (x2.view(-1, C)[idx_sh].double() - m2[bi]) * r2[bi])
    check(at(yy), ref2, 1.0 + xh.abs() + x2h.abs(), sh2)
    dy = torch.randn((B, X, Y, Z, C), device="cuda", generator=g, dtype=torch.bfloat16)

    def means(out, xx, mm, rr, step=1 << 22):
        """fp64 over the whole volume: m1 = mean(dy'), m2 = mean(dy' xhat) with dy' = dy lrelu'(out) [B, C]"""
        Bn = xx.shape[0]
        vd, vo, vx = dy.view(Bn, -1, C), out.view(Bn, -1, C), xx.view(Bn, -1, C)
        S = vd.shape[1]
        a1 = torch.zeros((Bn, C), dtype=torch.float64, device="cuda")
        a2 = torch.zeros_like(a1)
        for i in range(0, S, step):
            dp = vd[:, i:i + step].double() * torch.where(vo[:, i:i + step] > 0, 1.0, slope).double()
            a1 += dp.sum(1)
            a2 += (dp * (vx[:, i:i + step].double() - mm[:, None]) * rr[:, None]).sum(1)
        return a1 / S, a2 / S

    def bwd_ref(out, xhat, rr, mm1, mm2, ii):
        dp = dy.view(-1, C)[ii].double() * torch.where(out.view(-1, C)[ii] > 0, 1.0, slope).double()
        ref = rr[bi] * (dp - mm1[bi] - xhat * mm2[bi])
        scale = rr[bi] * (dp.abs() + mm1[bi].abs() + xhat.abs() * mm2[bi].abs())
        return ref, scale, dp

    m1, mm2 = means(y, x, m, r)
    dx, dres = ops.instnorm_cl_bwd(dy, y, x, mf, rf, slope, want_dres=True, had_res=True)
    ref, scale, dp = bwd_ref(y, xh, r, m1, mm2, idx)
    shr, _, _ = bwd_ref(y, (x.view(-1, C)[idx_sh].double() - m[bi]) * r[bi], r, m1, mm2, idx_sh)
    check(at(dx), ref, scale, shr)
    check(at(dres), dp, dp.abs(), dy.view(-1, C)[idx_sh].double() * torch.where(y.view(-1, C)[idx_sh] > 0, 1.0, slope).double())
    del dx, dres, y
    a1, a2 = means(yy, x, m, r)
    b1, b2 = means(yy, x2, m2, r2)
    d1, d2 = ops.instnorm_cl_bwd2(dy, yy, x, mf, rf, x2, m2f, r2f, slope)
    ref, scale, _ = bwd_ref(yy, xh, r, a1, a2, idx)
    shr, _, _ = bwd_ref(yy, (x.view(-1, C)[idx_sh].double() - m[bi]) * r[bi], r, a1, a2, idx_sh)
    check(at(d1), ref, scale, shr)
    ref, scale, _ = bwd_ref(yy, x2h, r2, b1, b2, idx)
    shr, _, _ = bwd_ref(yy, (x2.view(-1, C)[idx_sh].double() - m2[bi]) * r2[bi], r2, b1, b2, idx_sh)
    check(at(d2), ref, scale, shr)


@pytest.mark.gpu
def test_dice_ce_at_full_resolution():
    """Dice + CE on fp32 logits [2, 4, 512, 512, 128] (S = 2^25 voxels per row): loss and gradient against fp64"""
    from UCF_VIT._hip import ops
    X, Y, Z = VOL
    n, S = 4, X * Y * Z
    g = _gen(9)
    logits = torch.randn((B, n, X, Y, Z), device="cuda", generator=g) * 2
    labels = torch.randint(0, n, (B, X, Y, Z), device="cuda", generator=g)
    loss, dl = ops.dice_ce(logits, labels)
    lv, lab = logits.view(B, n, S), labels.view(B, S)
    step = 1 << 22
    inter = torch.zeros((B, n), dtype=torch.float64, device="cuda")
    psq, cnt = torch.zeros_like(inter), torch.zeros_like(inter)
    ce = 0.0
    for i in range(0, S, step):
        z = lv[:, :, i:i + step].double()
        p = z.softmax(1)
        oh = torch.nn.functional.one_hot(lab[:, i:i + step], n).permute(0, 2, 1).double()
        inter += (p * oh).sum(2)
        psq += (p * p).sum(2)
        cnt += oh.sum(2)
        ce -= float((z.log_softmax(1) * oh).sum())
    den = psq + cnt + 1e-5
    loss_ref = float((1 - (2 * inter + 1e-5) / den).mean()) + ce / (B * S)
    assert abs(loss.item() - loss_ref) <= 1e-5 * abs(loss_ref)          # fp32 result of double-folded fp32 chunk sums

    idx = _samples(B, X, Y, Z, NSAMP, g)                                # voxel index over [B, X, Y, Z]
    bi, si = idx // S, idx % S

    def grad_ref(lab_at):
        z = lv[bi, :, si].double()                                       # [N, n]
        p = z.softmax(1)
        oh = torch.nn.functional.one_hot(lab_at, n).double()
        # dice term: d/dp of mean_{b,c} (1 - (2 I + s) / (D + s)); CE term: (p - onehot) / (B S); both through the softmax Jacobian
        gp = -(2 * oh / den[bi] - 2 * p * (2 * inter[bi] + 1e-5) / den[bi] ** 2) / (B * n)
        gz = p * (gp - (gp * p).sum(1, keepdim=True))
        return gz + (p - oh) / (B * S)
    ref = grad_ref(lab[bi, si])
    got = dl.view(B, n, S)[bi, :, si].double()
    unit = 1.0 / (B * S)
    bound = 2 ** -16 * ref.abs() + 2 ** -16 * unit                      # fp32 softmax and products: a few ulps of the CE term's scale
    assert bool(((got - ref).abs() <= bound).all())
    wrong = grad_ref(lab[bi, (si + 1) % S])                              # negative control: labels one voxel over
    assert not bool(((got - wrong).abs() <= bound).all())


@pytest.mark.gpu
def test_dense_centre_tap_weight_gradient_at_full_resolution():
    """dense normal x and dy at 512 x 512 x 128 (decoder2 conv2, 16 -> 16): the centre tap of the weight gradient is one unshifted product
    sum over all 2^26 voxels, compared with an fp64 matmul"""
    from UCF_VIT._hip import conv
    X, Y, Z = VOL
    C = 16
    g = _gen(31)
    x = torch.randn((B, X, Y, Z, C), device="cuda", generator=g, dtype=torch.bfloat16)
    dy = torch.randn((B, X, Y, Z, C), device="cuda", generator=g, dtype=torch.bfloat16)
    got = conv.conv3_wgrad(x, dy, C, C)[:, :, 1, 1, 1].double()
    x2, d2 = x.view(-1, C), dy.view(-1, C)
    step = 1 << 23
    ref = torch.zeros((C, C), dtype=torch.float64, device="cuda")
    shifted = torch.zeros_like(ref)
    absum = torch.zeros_like(ref)
    for i in range(0, x2.shape[0], step):
        xi, di = x2[i:i + step].double(), d2[i:i + step].double()
        ref += di.t() @ xi
        absum += di.abs().t() @ xi.abs()
        xs = x2[i + 1:i + step + 1].double()                           # x one voxel over in z (the tap next to the centre)
        shifted += di[:xs.shape[0]].t() @ xs
    # fp32 accumulation in chains of at most 2^16 voxels per workgroup partial, then a sum of the partials: 2^-16 of the absolute sum
    bound = 2 ** -16 * absum
    assert bool(((got - ref).abs() <= bound).all())
    assert not bool(((got - shifted).abs() <= bound).all())
