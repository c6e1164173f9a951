"""The kernels of csrc/conv2d.hip against float64 references of the same rounded operands, element by element, in the manner of
tests/test_conv3d_ops.py.  The references never call the project's kernels: a convolution is 9 shifted slices of a zero-padded float64 image,
each times the tap's [Cin, Cout] matrix (_conv64); the data gradient is the scatter form of the same sum (_dgrad64: every dy pixel adds its
w-weighted vector to the 9 input pixels it was computed from — no flipped weights, which is what the kernel path uses); a weight gradient is
the matching 9 products (_wgrad64).  U = 2^-24 (fp32 unit roundoff), UB = 2^-8 (bf16).  All operands are drawn on the CPU.

The launches go to the library entry points directly, with outputs inside sentinel buffers owned by the test (two sentinel rows behind the
last pixel, the channels cout_store .. ldy of every row): nothing outside the cout_store channels of the image's rows may change.  Operands
are carved from the middle of NaN-filled allocations; results must be NaN-free.  The ops / conv wrappers are checked bit for bit against
the direct launches (test_wrappers_give_the_same_bits).

Cases: Cin {8, 16, 32, 64, 96} x Cout {16, 32, 48, 64, 128} = every instantiation CPC 8 / 16 / 32 x NB 1 / 2 / 4 (asserted from the route text:
test_table_reaches_every_instantiation), over the images (1, 1), (3, 5), one exact tile (16 x 16, or 8 x 16 under 64 output channels per
workgroup), one pixel past the tile on each axis, (33, 18) (three row tiles, a ragged second column tile) and (17, 16), B 1 and 2 (a halo that
runs off one batch element lands in the next).  Epilogues: bf16 and fp32, bias, accumulate (bf16, and fp32 with bias), cout_store = 4 with
fp32 output and ldy = 8, cout_store = 5 = 4 + 1 in bf16 rows of 8 (one vector group and one scalar channel), a channel slice (ldy = Cout + 8).

Tier 1, exact.  Integer operands, {+-3, +-4} ("big": most sums exceed 256, so the bf16 rounding is pinned) and {-1, 0, 1}; bias and base
integers in [-4, 4].  The exactness condition |x| conv |w| + |bias| + |base| < 2^24 (weight gradient: over all pixels) is computed and
asserted; fp32 outputs and weight gradients equal float64 bit for bit, bf16 outputs equal float64 rounded ONCE.  Forward, data gradient and
weight gradient; a second call gives the same bits.

Tier 2, bounds on real-valued operands (randn; randn + 8 sigma; randn times 2^-20 .. 2^20; weights randn at sqrt(2 / fan-in)):
    |got - ref| <= t + ou (|ref| + t),  ou = UB (bf16 output) or U (fp32),  t = d U (|x| conv |w|) + U |v| per epilogue addition.
d is the longest fp32 addition chain (one v_mfma_f32_16x16x32_bf16 counts as 32 additions, then one per further MFMA into the accumulator):
    forward / data gradient: d = steps + 32, steps = K / 32 with K = 9 Cin AS PADDED: 9 (CPC 32), 5 (CPC 16), 3 (CPC 8) per 32-channel chunk
    weight gradient: one MFMA (32 pixels along y) per row of an 8-row tile, tiles_per_wg tiles, then ucfvit_reduce_rows over n_wg partials:
        d = 8 tiles_per_wg + 32 + n_wg.
Every bound must reject the wrong references, each by at least one operand family in every (case, epilogue) (Pool): dx / dy swapped in the
tap; the image shifted by one pixel on either axis, wrapping round (no zero padding); the centre tap dropped, and the last tap (2, 2) —
the one beside the zero-padded contraction slots of CPC 8 / 16 — dropped; the last row or the last column left out.  Weight gradient: taps
swapped, x shifted on either axis, a tap's block zero, the last pixel left out.  Tier 1 asserts the same alternatives differ from the right
result and from what the kernel wrote.

ucfvit_depth_to_space2_2d: both directions, dense and into / out of a channel slice (ld_space > C), with skip: torch.equal with the permuted
tensor, sentinels around the output untouched."""
import ctypes
import itertools
from dataclasses import dataclass

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
U, UB, LIM = 2.0 ** -24, 2.0 ** -8, 2.0 ** 24
BF, F32 = torch.bfloat16, torch.float32
SENT = -12352.0
PAD = 64


def _lib():
    from UCF_VIT._hip import lib
    return lib


def _conv():
    from UCF_VIT._hip import conv
    return conv


def _cdiv(a, b):
    return -(-a // b)


# ============================================================================================== cases
@dataclass(frozen=True)
class Epi:
    name: str
    out32: bool = False
    bias: bool = False
    cs: int = 0              # cout_store, 0 = Cout
    ldx: int = 0             # the output's rows are ceil8(cout_store) + ldx wide
    acc: bool = False

    def cs_of(self, c):
        return self.cs or c.cout

    def ld_of(self, c):
        return _cdiv(self.cs_of(c), 8) * 8 + self.ldx


EPIS = {e.name: e for e in (Epi("plain"), Epi("o32", out32=True), Epi("bias", bias=True), Epi("acc", acc=True), Epi("acc_bias_o32", acc=True, bias=True, out32=True),
                            Epi("cs4_ld8_o32", cs=4, out32=True), Epi("cs5_ld8", cs=5, bias=True), Epi("slice", ldx=8))}


@dataclass(frozen=True)
class FC:
    B: int
    X: int
    Y: int
    cin: int
    cout: int

    @property
    def id(self):
        return f"{self.B}x{self.X}x{self.Y}-{self.cin}to{self.cout}"

    @property
    def shape(self):
        return (self.B, self.X, self.Y)

    @property
    def nb(self):
        n = self.cout // 16
        return 4 if n % 4 == 0 else 2 if n % 2 == 0 else 1

    @property
    def steps(self):
        cpc = min(self.cin, 32)
        return {8: 3, 16: 5, 32: 9}[cpc] * (self.cin // cpc)


def _image(i, nb):
    tx = 8 if nb == 4 else 16
    return [(1, 1, 1), (2, 3, 5), (2, tx, 16), (2, tx + 1, 17), (2, 33, 18), (1, 17, 16)][i % 6]


FWD = [FC(*_image(i, FC(1, 1, 1, ci, co).nb), ci, co) for i, (ci, co) in enumerate(itertools.product((8, 16, 32, 64, 96), (16, 32, 48, 64, 128)))]
FWD += [FC(2, 33, 18, 8, 16), FC(2, 9, 17, 16, 64)]
DGRAD = [FC(2, 3, 5, 16, 16), FC(2, 17, 17, 32, 16), FC(2, 9, 17, 64, 32), FC(1, 33, 18, 16, 96), FC(1, 1, 1, 128, 64)]     # dy has cin channels, dx cout
FWD_IDS = [c.id for c in FWD]
assert len(set(FWD_IDS)) == len(FWD)


@dataclass(frozen=True)
class WC:
    B: int
    X: int
    Y: int
    cin: int
    cout: int
    via: str = "lib"         # lib: ucfvit_conv2d_wgrad + unpack; conv3: conv.conv3_wgrad (swaps the operands' roles for Cout 16 under Cin >= 32)

    @property
    def id(self):
        return f"wgrad-{self.via}-{self.B}x{self.X}x{self.Y}-{self.cin}to{self.cout}"

    @property
    def kdims(self):
        return (self.cout, self.cin) if (self.via == "conv3" and self.cout == 16 and self.cin >= 32) else (self.cin, self.cout)


WGRAD = [WC(1, 1, 1, 8, 16), WC(2, 3, 5, 16, 32), WC(2, 8, 32, 32, 48), WC(2, 9, 33, 64, 32), WC(2, 33, 18, 96, 16), WC(2, 17, 17, 16, 16), WC(1, 8, 33, 8, 64),
         WC(2, 184, 736, 8, 16),                                           # 1058 tiles: tiles_per_wg = 2 under the 1024-workgroup cap
         WC(2, 104, 384, 96, 128),                                         # 312 tiles against the partial-sum cap of 303 workgroups: tiles_per_wg = 2
         WC(2, 9, 33, 32, 16, via="conv3"), WC(2, 17, 17, 64, 16, via="conv3"), WC(2, 9, 33, 16, 32, via="conv3")]


def _wplan(c):
    """conv2d_wgrad_route of csrc/conv2d_route.h restated"""
    kin, kout = c.kdims
    cpc, mb = min(kin, 32), 2 if kout % 32 == 0 else 1
    nbk = cpc // 16 if cpc >= 16 else 1
    tiles = c.B * _cdiv(c.X, 8) * _cdiv(c.Y, 32)
    n_out = (kin // cpc) * (kout // (16 * mb)) * 9 * 16 * mb * 16 * nbk
    n_wg = min(tiles, max(1, min(1024, (32 << 20) // n_out)))
    tpw = _cdiv(tiles, n_wg)
    n_wg = _cdiv(tiles, tpw)
    return dict(n_wg=n_wg, tpw=tpw, n_out=n_out, d=8 * tpw + 32 + n_wg)


# ============================================================================================== operands
def _values(g, kind, shape, scale=1.0):
    if kind == "int":
        return torch.randint(-1, 2, shape, generator=g).double()
    if kind == "int4":
        return torch.randint(-4, 5, shape, generator=g).double()
    if kind == "big":
        return torch.tensor([-4.0, -3.0, 3.0, 4.0], dtype=torch.float64)[torch.randint(0, 4, shape, generator=g)]
    v = torch.randn(shape, generator=g, dtype=torch.float32).double() * scale
    if kind == "offset":
        v = v + 8.0 * scale
    if kind == "exp":
        v = v * torch.exp2(torch.randint(-20, 21, shape, generator=g).double())
    return v


def _carve(vals, fill):
    n = vals.numel()
    buf = torch.full((n + 2 * PAD,), fill, dtype=vals.dtype, device=DEV)
    buf[PAD:PAD + n] = vals.reshape(-1).to(DEV)
    return buf[PAD:PAD + n].view(vals.shape)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


class O:
    pass


def _seed(c, kind):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id + kind)) % (2 ** 31)


def _fwd_operands(c, kind, dgrad=False):
    """dgrad: x plays dy [.., cin], the weight is [cin, cout, 3, 3] (the layer cout -> cin whose data gradient this is)"""
    g = torch.Generator().manual_seed(_seed(c, kind + ("d" if dgrad else "")))
    exact = kind in ("int", "big")
    o = O()
    x = _values(g, kind, c.shape + (c.cin,)).to(BF)
    wshape = (c.cin, c.cout, 3, 3) if dgrad else (c.cout, c.cin, 3, 3)
    w = _values(g, kind if exact else "randn", wshape, 1.0 if exact else (2.0 / (9 * c.cin)) ** 0.5).to(BF)
    bias = _values(g, "int4" if exact else "randn", (c.cout,), 0.5).to(BF)
    base = _values(g, "int4" if exact else "randn", c.shape + (c.cout,)).to(BF)
    o.x = _carve(x, float("nan"))
    o.wp = _carve(_conv().pack_conv2d_weight_dgrad(w.float()) if dgrad else _conv().pack_conv2d_weight(w.float()), float("nan"))
    o.bias = _carve(bias.float(), float("nan"))
    o.x64, o.w64, o.bias64, o.base64 = x.double().to(DEV), w.double().to(DEV), bias.double().to(DEV), base.double().to(DEV)
    return o


# ============================================================================================== float64 references
def _padded(x):
    B, X, Y, C = x.shape
    xp = x.new_zeros((B, X + 2, Y + 2, C))
    xp[:, 1:-1, 1:-1] = x
    return xp


def _conv64(x, w, skip_tap=None):
    """9 shifted slices of the zero-padded image, each times the tap's [Cin, Cout] matrix"""
    B, X, Y, _ = x.shape
    xp = _padded(x)
    out = x.new_zeros((B, X, Y, w.shape[0]))
    for dx in range(3):
        for dy in range(3):
            if (dx, dy) != skip_tap:
                out += xp[:, dx:dx + X, dy:dy + Y] @ w[:, :, dx, dy].T
    return out


def _dgrad64(dy, w):
    """scatter form: w [Cin_of_dy, Cout_of_dx, 3, 3]; the pixel p of dy was computed from input pixels p + tap - 1"""
    B, X, Y, _ = dy.shape
    acc = dy.new_zeros((B, X + 2, Y + 2, w.shape[1]))
    for dx in range(3):
        for dyy in range(3):
            acc[:, dx:dx + X, dyy:dyy + Y] += dy @ w[:, :, dx, dyy]
    return acc[:, 1:-1, 1:-1].contiguous()


def _wgrad64(x, dy):
    cin, cout = x.shape[-1], dy.shape[-1]
    B, X, Y, _ = x.shape
    xp = _padded(x)
    d2 = dy.reshape(-1, cout).T
    out = x.new_zeros((cout, cin, 3, 3))
    for dx in range(3):
        for dyy in range(3):
            out[:, :, dx, dyy] = d2 @ xp[:, dx:dx + X, dyy:dyy + Y].reshape(-1, cin)
    return out


def _fwd_refs(c, o, dgrad=False):
    conv = (lambda x, w, **k: _dgrad64(x, w)) if dgrad else _conv64
    absw = o.w64.abs()
    R = {"ok": conv(o.x64, o.w64), "abs": conv(o.x64.abs(), absw)}
    if dgrad:
        return R
    R["drop_centre"] = _conv64(o.x64, o.w64, skip_tap=(1, 1))
    if c.X > 1 or c.Y > 1:
        R["swap"] = _conv64(o.x64, o.w64.transpose(2, 3))
    if c.X > 1 and c.Y > 1:
        R["drop_last_tap"] = _conv64(o.x64, o.w64, skip_tap=(2, 2))
    if c.X > 1:
        R["shift_x"] = _conv64(o.x64.roll(1, 1), o.w64)
    if c.Y > 1:
        R["shift_y"] = _conv64(o.x64.roll(1, 2), o.w64)
    R["drop_row"] = R["ok"].clone()
    R["drop_row"][:, -1] = 0
    R["drop_col"] = R["ok"].clone()
    R["drop_col"][:, :, -1] = 0
    return R


WRONG = ("swap", "shift_x", "shift_y", "drop_centre", "drop_last_tap", "drop_row", "drop_col")


def _epi(c, e, o, S, A=None, d=0):
    """the epilogue in the kernel's order (sum, + bias, + the values accumulated onto, one rounding) -> (value, tol) in float64"""
    v = S
    t = d * U * A if A is not None else None
    if e.bias:
        v = v + o.bias64
        t = t + U * v.abs() if t is not None else None
    if e.acc:
        v = v + o.base64
        t = t + U * v.abs() if t is not None else None
    cs = e.cs_of(c)
    v = v[..., :cs]
    if t is None:
        return v, None
    t = t[..., :cs]
    return v, t + (U if e.out32 else UB) * (v.abs() + t)


# ============================================================================================== launches
def _launch(c, e, o):
    """ucfvit_conv2d_fwd into a sentinel buffer -> (y view [B, X, Y, cs], assert_guard)"""
    lib = _lib()
    L = lib.load()
    cs, ld = e.cs_of(c), e.ld_of(c)
    odt = F32 if e.out32 else BF
    V = c.B * c.X * c.Y
    buf = torch.full((V + 2, ld), SENT, dtype=odt, device=DEV)
    if e.acc:
        buf[:V, :cs] = o.base64[..., :cs].reshape(V, cs).to(odt)
    snap = buf.clone()
    rc = L.ucfvit_conv2d_fwd(o.x.data_ptr(), o.wp.data_ptr(), o.bias.data_ptr() if e.bias else None, buf.data_ptr(), c.B, c.X, c.Y, c.cin, c.cout,
                             ld, cs, lib.F32 if e.out32 else lib.BF16, 1 if e.acc else 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.ucfvit_last_error()
    y = buf[:V, :cs].reshape(c.shape + (cs,))

    def guard(what):
        now, was = _bits(buf).clone(), _bits(snap).clone()
        now[:V, :cs] = 0
        was[:V, :cs] = 0
        assert torch.equal(now, was), f"{what}: written outside the cout_store channels of the image's rows"
    return y, guard


RATIOS = {}


def _ratio(family, what, got, ref, tol):
    err = (got.detach().double() - ref).abs()
    bad = ~(err <= tol)
    r = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    RATIOS[family] = max(RATIOS.get(family, 0.0), r)
    print(f"RATIO {family} {what}: worst err/bound {r:.3f}")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, worst err/bound {r:.3f}, first at {torch.nonzero(bad)[0].tolist()}"


def _within(got, ref, tol):
    return bool(((got.detach().double() - ref).abs() <= tol).all())


class Pool:
    """the operand families of one (case, epilogue): every family within its bound, every wrong reference rejected by at least one"""

    def __init__(self, what):
        self.what, self.rejected = what, {}

    def check(self, family, got, ref, tol, wrongs):
        _ratio(family, self.what, got, ref, tol)
        for name, w in wrongs.items():
            self.rejected[name] = self.rejected.get(name, False) or not _within(got, w, tol)

    def done(self):
        assert self.rejected, f"{self.what}: no wrong reference to reject"
        missed = [k for k, r in self.rejected.items() if not r]
        assert not missed, f"{self.what}: the bound does not reject the wrong references {missed}"


# ============================================================================================== forward
def _tier1_fwd(c, dgrad=False):
    for kind in ("big", "int"):
        o = _fwd_operands(c, kind, dgrad)
        R = _fwd_refs(c, o, dgrad)
        cond = R["abs"] + o.bias64.abs() + o.base64.abs()
        assert float(cond.max()) < LIM, f"{c.id}: the exactness condition fails"
        for en, e in EPIS.items():
            what = f"{c.id}/{en}/{kind}"
            odt = F32 if e.out32 else BF
            right = _epi(c, e, o, R["ok"])[0].to(odt)
            wrongs = {n: _epi(c, e, o, R[n])[0].to(odt) for n in WRONG if n in R} if kind == "big" else {}
            for n, w in wrongs.items():
                assert not torch.equal(w, right), f"{what}: the wrong result '{n}' equals the right one: it guards nothing"
            y, guard = _launch(c, e, o)
            assert bool(torch.isfinite(y.float()).all()), f"{what}: non-finite output (NaN padding read?)"
            bad = _bits(y) != _bits(right)
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ from the float64 result rounded once, first at {torch.nonzero(bad)[0].tolist()}"
            guard(what)
            for n, w in wrongs.items():
                assert not torch.equal(y, w), f"{what}: the kernel wrote the wrong result '{n}'"
            y2, _ = _launch(c, e, o)                         # a second call: the same bits
            assert torch.equal(_bits(y2), _bits(y))


def _tier2_fwd(c, dgrad=False):
    pools = {en: Pool(f"{c.id}/{en}") for en in EPIS}
    d = c.steps + 32
    for fam in ("randn", "offset", "exp"):
        o = _fwd_operands(c, fam, dgrad)
        R = _fwd_refs(c, o, dgrad)
        for en, e in EPIS.items():
            what = f"{c.id}/{en}/{fam}"
            y, guard = _launch(c, e, o)
            assert bool(torch.isfinite(y.float()).all()), f"{what}: non-finite output (NaN padding read?)"
            guard(what)
            v, tol = _epi(c, e, o, R["ok"], R["abs"], d)
            wrongs = {n: _epi(c, e, o, R[n], R["abs"], d)[0] for n in WRONG if n in R}
            name = ("dgrad " if dgrad else "fwd ") + ("fp32" if e.out32 else "bf16")
            if dgrad:
                _ratio(name, what, y, v, tol)
            else:
                pools[en].check(name, y, v, tol, wrongs)
    if not dgrad:
        for p in pools.values():
            p.done()


@gpu
@pytest.mark.parametrize("c", FWD, ids=FWD_IDS)
def test_conv2d_fwd_exact(c):
    _tier1_fwd(c)


@gpu
@pytest.mark.parametrize("c", FWD, ids=FWD_IDS)
def test_conv2d_fwd_bounds(c):
    _tier2_fwd(c)


@gpu
@pytest.mark.parametrize("c", DGRAD, ids=[c.id for c in DGRAD])
def test_conv2d_dgrad_exact_and_bounds(c):
    """the data gradient: the same entry point on dy with pack_conv2d_weight_dgrad, against the scatter-form float64 sum"""
    _tier1_fwd(c, dgrad=True)
    _tier2_fwd(c, dgrad=True)


def _route(pass_, c, e=None):
    lib = _lib()
    L = lib.load()
    buf = ctypes.create_string_buffer(160)
    e = e or EPIS["plain"]
    n = L.ucfvit_conv2d_route(pass_, c.B, c.X, c.Y, c.cin, c.cout, int(e.bias), lib.F32 if e.out32 else lib.BF16, e.ld_of(c), e.cs_of(c), buf, 160)
    assert n > 0, L.ucfvit_last_error()
    return buf.value.decode()


def test_table_reaches_every_instantiation():
    """host only: the route query names a distinct instantiation for each of the 18 (CPC, NB, output type) families and the 6 (CPC, MB)
    weight-gradient ones, and the tables reach them all"""
    seen = {" ".join(_route(0, c, e).split()[:5]) for c in FWD for e in EPIS.values()}
    want = {f"tile2d cpc{cpc} nb{nb} {8 if nb == 4 else 16}x16 {t}" for cpc in (8, 16, 32) for nb in (1, 2, 4) for t in ("bf16", "f32")}
    assert seen == want and len(want) == 18
    seen_w = {" ".join(_route(1, FC(c.B, c.X, c.Y, *c.kdims)).split()[:3]) for c in WGRAD}
    assert seen_w == {f"wgrad2d cpc{cpc} mb{mb}" for cpc in (8, 16, 32) for mb in (1, 2)}
    for c in WGRAD:
        p = _wplan(c)
        assert _route(1, FC(c.B, c.X, c.Y, *c.kdims)).endswith(f"n_wg{p['n_wg']} tiles_per_wg{p['tpw']} n_out{p['n_out']}")
    assert {_wplan(c)["tpw"] for c in WGRAD} == {1, 2}


# ============================================================================================== weight gradient
def _w_operands(c, kind):
    g = torch.Generator().manual_seed(_seed(c, kind))
    exact = kind in ("int", "big")
    o = O()
    x = _values(g, kind, (c.B, c.X, c.Y, c.cin)).to(BF)
    dy = _values(g, kind if exact else "randn", (c.B, c.X, c.Y, c.cout), 1.0 if exact else 0.05).to(BF)
    o.x, o.dy = _carve(x, float("nan")), _carve(dy, float("nan"))
    o.x64, o.dy64 = x.double().to(DEV), dy.double().to(DEV)
    return o


def _w_launch(c, o):
    conv = _conv()
    if c.via == "conv3":
        return conv.conv3_wgrad(o.x, o.dy, c.cin, c.cout)
    lib = _lib()
    L = lib.load()
    p = _wplan(c)
    assert L.ucfvit_conv2d_wgrad_size(c.cin, c.cout) == p["n_out"] and L.ucfvit_conv2d_wgrad_workspace(c.B, c.X, c.Y, c.cin, c.cout) == p["n_wg"] * p["n_out"] * 4
    dw = torch.full((p["n_out"] + 2 * PAD,), SENT, dtype=F32, device=DEV)
    ws = torch.full((p["n_wg"] * p["n_out"] + 2 * PAD,), SENT, dtype=F32, device=DEV)
    rc = L.ucfvit_conv2d_wgrad(o.x.data_ptr(), o.dy.data_ptr(), dw[PAD:].data_ptr(), ws[PAD:].data_ptr(), c.B, c.X, c.Y, c.cin, c.cout,
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.ucfvit_last_error()
    for b, n in ((dw, p["n_out"]), (ws, p["n_wg"] * p["n_out"])):
        assert bool((b[:PAD] == SENT).all()) and bool((b[PAD + n:] == SENT).all()), f"{c.id}: written outside the gradient / the workspace"
    return conv.unpack_conv2d_wgrad(dw[PAD:PAD + p["n_out"]], c.cin, c.cout)


def _w_refs(c, o):
    R = {"ok": _wgrad64(o.x64, o.dy64), "abs": _wgrad64(o.x64.abs(), o.dy64.abs())}
    R["drop_centre"] = R["ok"].clone()
    R["drop_centre"][:, :, 1, 1] = 0
    if c.X > 1 or c.Y > 1:
        R["swap"] = R["ok"].transpose(2, 3).contiguous()
    if c.X > 1 and c.Y > 1:
        R["drop_last_tap"] = R["ok"].clone()
        R["drop_last_tap"][:, :, 2, 2] = 0
    if c.X > 1:
        R["shift_x"] = _wgrad64(o.x64.roll(1, 1), o.dy64)
    if c.Y > 1:
        R["shift_y"] = _wgrad64(o.x64.roll(1, 2), o.dy64)
    dl = o.dy64.clone()
    dl[-1, -1, -1] = 0
    R["drop_last_pixel"] = _wgrad64(o.x64, dl)
    return R


W_WRONG = ("swap", "shift_x", "shift_y", "drop_centre", "drop_last_tap", "drop_last_pixel")


@gpu
@pytest.mark.parametrize("c", WGRAD, ids=[c.id for c in WGRAD])
def test_conv2d_wgrad_exact(c):
    for kind in ("big", "int"):
        o = _w_operands(c, kind)
        R = _w_refs(c, o)
        assert float(R["abs"].max()) < LIM, f"{c.id}: the exactness condition fails over all pixels"
        right = R["ok"].float()
        got = _w_launch(c, o)
        assert tuple(got.shape) == tuple(right.shape) and got.dtype == F32
        bad = got != right
        assert not bool(bad.any()), f"{c.id}/{kind}: {int(bad.sum())} elements differ from float64, first at {torch.nonzero(bad)[0].tolist()}"
        if kind == "big":
            for n in W_WRONG:
                if n in R:
                    assert not torch.equal(R[n].float(), right), f"{c.id}: the wrong gradient '{n}' equals the right one"
                    assert not torch.equal(got, R[n].float()), f"{c.id}: the kernel wrote the wrong gradient '{n}'"
        assert torch.equal(_w_launch(c, o), got)                  # a second call: the fold has a fixed order


@gpu
@pytest.mark.parametrize("c", WGRAD, ids=[c.id for c in WGRAD])
def test_conv2d_wgrad_bounds(c):
    pool = Pool(c.id)
    d = _wplan(c)["d"]
    first = None
    for fam in ("randn", "offset", "exp"):
        o = _w_operands(c, fam)
        R = _w_refs(c, o)
        got = _w_launch(c, o)
        assert bool(torch.isfinite(got).all()), f"{c.id}/{fam}: non-finite gradient (NaN padding read?)"
        tol = d * U * R["abs"]
        tol = tol + U * (R["ok"].abs() + tol)
        pool.check("wgrad" + ("-swapped" if c.kdims != (c.cin, c.cout) else ""), got, R["ok"], tol, {n: R[n] for n in W_WRONG if n in R})
        if first is None:
            first = (o, got)
    pool.done()
    assert torch.equal(_bits(_w_launch(c, first[0])), _bits(first[1]))     # real-valued operands: still the same bits on a second call


# ============================================================================================== wrappers
@gpu
def test_wrappers_give_the_same_bits():
    """ops.conv2d_fwd (dense, out= slice, accumulate_into, bias, fp32) and ops.conv2d_wgrad against the direct launches; refusals of ops"""
    from UCF_VIT._hip import ops
    c = FC(2, 17, 17, 16, 32)
    o = _fwd_operands(c, "randn")
    y, _ = _launch(c, EPIS["plain"], o)
    assert torch.equal(_bits(ops.conv2d_fwd(o.x, o.wp, c.cout)), _bits(y))
    yb, _ = _launch(c, EPIS["o32"], o)
    assert torch.equal(ops.conv2d_fwd(o.x, o.wp, c.cout, out_dtype=F32), yb)
    wide = torch.full(c.shape + (c.cout + 8,), SENT, dtype=BF, device=DEV)
    ops.conv2d_fwd(o.x, o.wp, c.cout, out=wide[..., :c.cout])
    assert torch.equal(_bits(wide[..., :c.cout]), _bits(y)) and bool((wide[..., c.cout:] == SENT).all())
    ya, _ = _launch(c, EPIS["acc"], o)
    base = o.base64.to(BF).contiguous()
    assert ops.conv2d_fwd(o.x, o.wp, c.cout, accumulate_into=base) is base and torch.equal(_bits(base), _bits(ya))
    yc, _ = _launch(c, EPIS["cs5_ld8"], o)
    got = ops.conv2d_fwd(o.x, o.wp, c.cout, bias=o.bias, cout_store=5)
    assert tuple(got.shape) == c.shape + (5,) and torch.equal(_bits(got), _bits(yc))
    wc = WC(2, 17, 17, 16, 32)
    ow = _w_operands(wc, "randn")
    assert torch.equal(_conv().unpack_conv2d_wgrad(ops.conv2d_wgrad(ow.x, ow.dy), 16, 32), _w_launch(wc, ow))
    with pytest.raises(TypeError):
        ops.conv2d_fwd(o.x.unsqueeze(3), o.wp, c.cout)                      # a volume is not an image
    with pytest.raises(TypeError):
        ops.conv3d_fwd(o.x, o.wp, c.cout)
    with pytest.raises(ValueError, match="w_packed"):
        ops.conv2d_fwd(o.x, o.wp, 16)
    with pytest.raises(ValueError, match="unsupported channel counts"):
        ops.conv2d_wgrad(ow.x, ow.dy[..., :20].contiguous())


# ============================================================================================== depth to space
D2S = [(2, 3, 5, 16, 0, 0), (1, 1, 1, 8, 0, 0), (2, 4, 7, 32, 8, 0), (2, 3, 5, 16, 0, 16), (2, 5, 3, 64, 64, 64), (1, 9, 2, 8, 16, 24), (1, 2, 2, 16, 0, 8)]   # B, Xi, Yi, C, pad, Cs


@gpu
@pytest.mark.parametrize("B,Xi,Yi,C,pad,Cs", D2S)
def test_depth_to_space2_2d_bit_for_bit(B, Xi, Yi, C, pad, Cs):
    from UCF_VIT._hip import ops
    g = torch.Generator().manual_seed(B * 1000 + Xi * 100 + Yi * 10 + C)
    cols = _carve(torch.randn((B * Xi * Yi, 4 * C), generator=g).to(BF), float("nan"))
    want = cols.view(B, Xi, Yi, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * Xi, 2 * Yi, C)
    ld = C + Cs + pad
    V = B * 4 * Xi * Yi
    buf = torch.full((V + 2, ld), SENT, dtype=BF, device=DEV)
    space = buf[:V].view(B, 2 * Xi, 2 * Yi, ld)
    skip = _carve(torch.randn((B, 2 * Xi, 2 * Yi, Cs), generator=g).to(BF), float("nan")) if Cs else None
    if (C + Cs) // 8 & ((C + Cs) // 8 - 1):
        with pytest.raises(Exception, match="power of two"):
            ops.depth_to_space2_2d(cols, B, Xi, Yi, C, out=space[..., :C], skip=skip)
        return
    out = ops.depth_to_space2_2d(cols, B, Xi, Yi, C, out=space[..., :C], skip=skip)
    assert torch.equal(_bits(out), _bits(want))
    if Cs:
        assert torch.equal(_bits(space[..., C:C + Cs]), _bits(skip))
    assert bool((buf[V:] == SENT).all()) and bool((space[..., C + Cs:] == SENT).all())
    # the inverse gather out of the slice, and out of a dense copy
    back = ops.space_to_depth2_2d(space[..., :C])
    assert torch.equal(_bits(back), _bits(cols))
    assert torch.equal(_bits(ops.space_to_depth2_2d(want.contiguous())), _bits(cols))
    if not Cs and not pad:
        assert torch.equal(_bits(ops.depth_to_space2_2d(cols, B, Xi, Yi, C)), _bits(want))
    assert torch.equal(_bits(ops.depth_to_space2_2d(cols, B, Xi, Yi, C, out=space[..., :C], skip=skip)), _bits(want))   # a second call
