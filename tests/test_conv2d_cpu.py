"""Host side of the 2-D UNETR decoder (csrc/conv2d.hip, csrc/conv2d_route.h, UCF_VIT/_hip/conv.py), no GPU: the weight packing against its
definition in include/ucfvit_hip.h, the route and size queries against a table restated here, the argument refusals (which run before any
HIP call), the pointwise factorisation, and the rule that sends a 2-D model to the HIP decoder."""
import ctypes

import pytest
import torch

from UCF_VIT._hip import conv as HC
from UCF_VIT._hip import lib

BF16, F32 = lib.BF16, lib.F32


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("cin", [8, 16, 32, 64])
@pytest.mark.parametrize("cout", [16, 48])
def test_pack_matches_the_definition(cin, cout):
    """w_packed[cc][ts][co][kk] = w[co][cc CPC + kk % CPC][tap], tap = ts TPS + kk / CPC = dx 3 + dy, zero for tap >= 9"""
    g = torch.Generator().manual_seed(cin * 100 + cout)
    w = torch.randn((cout, cin, 3, 3), generator=g).to(torch.bfloat16).float()
    p = HC.pack_conv2d_weight(w)
    cpc = min(cin, 32)
    tps = 32 // cpc
    nts = _cdiv(9, tps)
    assert p.dtype == torch.bfloat16 and tuple(p.shape) == (cin // cpc, nts, cout, 32)
    want = torch.zeros(p.shape)
    for cc in range(cin // cpc):
        for ts in range(nts):
            for kk in range(32):
                tap = ts * tps + kk // cpc
                if tap < 9:
                    want[cc, ts, :, kk] = w[:, cc * cpc + kk % cpc, tap // 3, tap % 3]
    assert torch.equal(p.float(), want)
    # the data gradient's weights: taps flipped, channel roles exchanged
    if cout == 16:                                 # (the gradient's input width is Cout: 48 is no width the kernels take)
        assert torch.equal(HC.pack_conv2d_weight_dgrad(w), HC.pack_conv2d_weight(w.transpose(0, 1).flip(2, 3)))


@pytest.mark.parametrize("cin", [8, 16, 32, 64])
@pytest.mark.parametrize("cout", [16, 32, 48])
def test_unpack_inverts_the_wgrad_layout(cin, cout):
    """[Cout / (16 MB)][Cin / CPC][9][16 MB][max(CPC, 16)] -> [Cout, Cin, 3, 3]; for CPC 8 the columns 8..15 are scratch"""
    L = lib.load()
    cpc, mb16 = min(cin, 32), 32 if cout % 32 == 0 else 16
    nbk16 = max(cpc, 16)
    n = L.ucfvit_conv2d_wgrad_size(cin, cout)
    assert n == (cout // mb16) * (cin // cpc) * 9 * mb16 * nbk16
    dw = torch.arange(cout * cin * 9, dtype=torch.float32).reshape(cout, cin, 3, 3)
    packed = torch.full((n,), float("nan"))
    pv = packed.view(cout // mb16, cin // cpc, 9, mb16, nbk16)
    for co in range(cout):
        for ci in range(cin):
            pv[co // mb16, ci // cpc, :, co % mb16, ci % cpc] = dw[co, ci].reshape(9)
    assert torch.equal(HC.unpack_conv2d_wgrad(packed, cin, cout), dw)


def test_pack_refuses_other_shapes():
    with pytest.raises(ValueError, match="Cin must be 8, 16 or a multiple of 32"):
        HC.pack_conv2d_weight(torch.zeros(16, 24, 3, 3))
    with pytest.raises(ValueError, match=r"\[Cout, Cin, 3, 3\]"):
        HC.pack_conv2d_weight(torch.zeros(16, 16, 3, 3, 3))


# ---------------------------------------------------------------------------------------------- routes and sizes
def _route(pass_, B, X, Y, cin, cout, odt=BF16, ldy=None, cs=None):
    L = lib.load()
    buf = ctypes.create_string_buffer(160)
    cs = cout if cs is None else cs
    n = L.ucfvit_conv2d_route(pass_, B, X, Y, cin, cout, 0, odt, cs if ldy is None else ldy, cs, buf, 160)
    assert n == len(buf.value), L.ucfvit_last_error()
    return buf.value.decode()


def _fwd_plan(B, X, Y, cin, cout):
    """conv2d_fwd_route of csrc/conv2d_route.h, restated"""
    nb16 = cout // 16
    nb = 4 if nb16 % 4 == 0 else 2 if nb16 % 2 == 0 else 1
    tx = 8 if nb == 4 else 16
    return min(cin, 32), nb, tx, B * _cdiv(X, tx) * _cdiv(Y, 16), nb16 // nb


def _wgrad_plan(B, X, Y, cin, cout):
    """conv2d_wgrad_route restated"""
    cpc, mb = min(cin, 32), 2 if cout % 32 == 0 else 1
    nbk = cpc // 16 if cpc >= 16 else 1
    tiles = B * _cdiv(X, 8) * _cdiv(Y, 32)
    n_out = (cin // cpc) * (cout // (16 * mb)) * 9 * 16 * mb * 16 * nbk
    cap = max(1, min(1024, (32 << 20) // n_out))
    n_wg = min(tiles, cap)
    tpw = _cdiv(tiles, n_wg)
    return cpc, mb, _cdiv(tiles, tpw), tpw, n_out


ROUTE_CASES = [(1, 1, 1, 8, 16), (2, 3, 5, 16, 16), (2, 16, 16, 32, 16), (2, 17, 17, 16, 32), (2, 33, 18, 32, 48), (1, 8, 16, 64, 64), (2, 9, 17, 96, 128),
               (64, 256, 256, 16, 16), (64, 128, 128, 64, 32)]


@pytest.mark.parametrize("c", ROUTE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_route_and_size_queries_equal_the_restated_plan(c):
    L = lib.load()
    B, X, Y, cin, cout = c
    for odt, name in ((BF16, "bf16"), (F32, "f32")):
        cpc, nb, tx, gx, gy = _fwd_plan(*c)
        assert _route(0, *c, odt=odt) == f"tile2d cpc{cpc} nb{nb} {tx}x16 {name} grid{gx}x{gy}"
    cpc, mb, n_wg, tpw, n_out = _wgrad_plan(*c)
    assert _route(1, *c) == f"wgrad2d cpc{cpc} mb{mb} n_wg{n_wg} tiles_per_wg{tpw} n_out{n_out}"
    assert L.ucfvit_conv2d_wgrad_size(cin, cout) == n_out
    assert L.ucfvit_conv2d_wgrad_workspace(B, X, Y, cin, cout) == n_wg * n_out * 4


def test_route_names_every_instantiation():
    """CPC 8 / 16 / 32 x NB 1 / 2 / 4 x bf16 / fp32 forward, CPC x MB 1 / 2 weight gradient: all distinct"""
    fwd = {_route(0, 2, 20, 20, cin, cout, odt=odt) for cin in (8, 16, 64) for cout in (16, 32, 64) for odt in (BF16, F32)}
    assert len(fwd) == 18
    wg = {_route(1, 2, 20, 20, cin, cout).split(" n_wg")[0] for cin in (8, 16, 64) for cout in (16, 32)}
    assert len(wg) == 6
    # the partial-sum caps: more than 1024 tiles share workgroups
    assert "n_wg1024 tiles_per_wg2" in _route(1, 64, 64, 128, 16, 16)


def test_sizes_are_zero_for_refused_shapes():
    L = lib.load()
    assert L.ucfvit_conv2d_wgrad_size(24, 16) == 0 and L.ucfvit_conv2d_wgrad_size(16, 20) == 0
    assert L.ucfvit_conv2d_wgrad_workspace(2, 8, 8, 24, 16) == 0 and L.ucfvit_conv2d_wgrad_workspace(0, 8, 8, 16, 16) == 0
    buf = ctypes.create_string_buffer(16)
    assert L.ucfvit_conv2d_route(0, 2, 8, 8, 24, 16, 0, BF16, 16, 16, buf, 16) < 0 and b"refuse" in L.ucfvit_last_error()
    assert L.ucfvit_conv2d_route(2, 2, 8, 8, 16, 16, 0, BF16, 16, 16, buf, 16) < 0
    # the text is cut to the buffer, the whole length is returned
    n = L.ucfvit_conv2d_route(0, 2, 8, 8, 16, 16, 0, BF16, 16, 16, buf, 16)
    assert n > 15 and len(buf.value) == 15


# ---------------------------------------------------------------------------------------------- refusals before any HIP call
def test_argument_refusals_carry_a_message():
    L = lib.load()
    a = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(a) + 15) & ~15           # a 16-byte aligned host address: never dereferenced, the checks come first
    fwd = lambda x, w, y, cin, cout, ldy=None, cs=None, odt=BF16: L.ucfvit_conv2d_fwd(
        x, w, None, y, 2, 4, 4, cin, cout, cout if ldy is None else ldy, cout if cs is None else cs, odt, 0, None)
    assert fwd(p, p, p, 24, 16) == -1 and b"ucfvit_conv2d_fwd: Cin must be 8, 16 or a multiple of 32 (got 24)" in L.ucfvit_last_error()
    assert fwd(p, p, p, 16, 20) == -1 and b"ucfvit_conv2d_fwd: Cout must be a multiple of 16 (got 20)" in L.ucfvit_last_error()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert fwd(*args, 16, 16) == -1 and b"ucfvit_conv2d_fwd: null pointer" in L.ucfvit_last_error()
    assert fwd(p + 2, p, p, 16, 16) == -1 and b"16-byte aligned" in L.ucfvit_last_error()
    assert fwd(p, p, p, 16, 16, cs=17) == -1 and b"cout_store" in L.ucfvit_last_error()
    assert fwd(p, p, p, 16, 16, ldy=8, cs=16) == -1 and b"cout_store" in L.ucfvit_last_error()
    assert fwd(p, p, p, 16, 16, odt=7) == -1 and b"bad out_dtype" in L.ucfvit_last_error()
    assert L.ucfvit_conv2d_fwd(p, p, None, p, 0, 4, 4, 16, 16, 16, 16, BF16, 0, None) == -1 and b"empty image" in L.ucfvit_last_error()
    assert L.ucfvit_conv2d_fwd(p, p, None, p, 1 << 11, 1 << 10, 1 << 10, 16, 16, 16, 16, BF16, 0, None) == -1 and b"2^31" in L.ucfvit_last_error()
    wg = lambda x, dy, dw, ws, cin, cout: L.ucfvit_conv2d_wgrad(x, dy, dw, ws, 2, 4, 4, cin, cout, None)
    assert wg(p, p, p, p, 24, 16) == -1 and b"ucfvit_conv2d_wgrad: Cin must be 8, 16 or a multiple of 32 (got 24)" in L.ucfvit_last_error()
    assert wg(p, p, p, p, 16, 20) == -1 and b"ucfvit_conv2d_wgrad: Cout must be a multiple of 16 (got 20)" in L.ucfvit_last_error()
    assert wg(None, p, p, p, 16, 16) == -1 and b"ucfvit_conv2d_wgrad: null pointer" in L.ucfvit_last_error()
    assert wg(p, p, p, None, 16, 16) == -1 and b"null workspace" in L.ucfvit_last_error()
    d2s = lambda src, dst, C, ld, to_space=1, skip=None, Cs=0: L.ucfvit_depth_to_space2_2d(src, dst, 2, 4, 4, C, ld, to_space, skip, Cs, None)
    assert d2s(None, p, 16, 16) == -1 and b"ucfvit_depth_to_space2_2d: bad arguments" in L.ucfvit_last_error()
    assert d2s(p, p, 12, 16) == -1 and b"bad arguments" in L.ucfvit_last_error()
    assert d2s(p, p, 16, 12) == -1 and b"ld_space" in L.ucfvit_last_error()
    assert d2s(p, p, 16, 24, 1, p, 16) == -1 and b"bad skip operand" in L.ucfvit_last_error()          # ld_space < C + Cs
    assert d2s(p, p, 16, 32, 0, p, 16) == -1 and b"bad skip operand" in L.ucfvit_last_error()          # the gather has no skip
    assert d2s(p, p, 24, 24) == -1 and b"power of two" in L.ucfvit_last_error()


# ---------------------------------------------------------------------------------------------- pointwise factorisation
def test_pointwise_dims_waste_nothing_on_tiled_images_and_least_elsewhere():
    up = lambda n, m: _cdiv(n, m) * m
    for S in (1, 15, 594, 1024, 33 * 18, 96 * 96, 256 * 256, 17 * 17):
        for tile in ((2, 8, 16), (2, 4, 32)):
            x, y, z = HC.pointwise_dims(S, tile)
            assert x * y * z == S
            padded = up(x, tile[0]) * up(y, tile[1]) * up(z, tile[2])
            assert abs(HC.pointwise_waste(S, tile) - padded / S) < 1e-12
            brute = min(up(a, tile[0]) * up(b, tile[1]) * up(S // (a * b), tile[2])
                        for a in range(1, S + 1) if S % a == 0 for b in range(1, S // a + 1) if (S // a) % b == 0) if S <= 1024 else None
            assert brute is None or padded == brute
    assert HC.pointwise_dims(256 * 256) == (64, 8, 128) and HC.pointwise_waste(256 * 256) == 1.0
    assert HC.pointwise_waste(32 * 32) == 1.0 and HC.pointwise_waste(32 * 32, (2, 4, 32)) == 1.0
    assert HC.pointwise_waste(17 * 17) > 1.0            # a prime square: whole tiles around one row of 289 voxels


# ---------------------------------------------------------------------------------------------- the model rule
def test_hip_decoder_supported_rule_table_in_the_plane():
    from UCF_VIT.simple.unetr_blocks import hip_decoder_supported as ok
    # with the kernels of the plane counted, spatial_dims 2 follows the channel rules of 3
    for args in ((1, 768, 16), (3, 768, 32), (8, 96, 64), (1, 16, 16), (1, 8, 128)):
        assert ok(2, *args, conv2d=True) and ok(3, *args, conv2d=True) and ok(3, *args)
    for args in ((9, 768, 16), (0, 768, 16), (1, 768, 48), (1, 768, 8), (1, 72, 16), (1, 120, 16), (1, 768, 96)):
        assert not ok(2, *args, conv2d=True) and not ok(3, *args)
    assert not ok(2, 1, 768, 16, kernel_size=5, conv2d=True) and not ok(2, 1, 768, 16, upsample_kernel_size=1, conv2d=True)
    assert not ok(1, 1, 768, 16, conv2d=True) and not ok(4, 1, 768, 16, conv2d=True)
    assert not ok(2, 1, 768, 16)                    # the 3-D kernels alone: the question the benchmark's host logic asks


KW = dict(in_chans=1, embed_dim=96, depth=4, num_heads=3, class_token=False, num_classes=4, feature_size=16, skip_connection=True, linear_decoder=False)


def test_unetr_2d_selects_the_hip_decoder():
    """fails without csrc/conv2d.hip and its wiring: every 2-D model answered False"""
    from UCF_VIT.simple.arch import UNETR
    m = UNETR(img_size=[32, 32], patch_size=16, twoD=True, **KW)
    assert m.hip_decoder() is True and not m.allow_torch_decoder and not m.resamples_dec1()
    assert UNETR(img_size=[64, 32], patch_size=16, twoD=True, **KW).hip_decoder() is True
    # a resampling geometry in the plane (bilinear, align_corners) has no kernel: it keeps answering False
    assert UNETR(img_size=[32, 32], patch_size=4, twoD=True, **KW).hip_decoder() is False
    # the channel rules hold in the plane as in the volume
    assert UNETR(img_size=[32, 32], patch_size=16, twoD=True, **dict(KW, feature_size=8)).hip_decoder() is False
    assert UNETR(img_size=[32, 32], patch_size=16, twoD=True, **dict(KW, in_chans=9)).hip_decoder() is False
    # the other decoders are not on the HIP path
    assert UNETR(img_size=[32, 32], patch_size=16, twoD=True, **dict(KW, skip_connection=False)).hip_decoder() is False
    m.force_torch_decoder = True
    assert m.hip_decoder() is False
