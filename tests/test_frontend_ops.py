"""The patch front-end kernels per element: ucfvit_im2col and ucfvit_mae_mask (csrc/elementwise.hip), ucfvit_seq_patches and
ucfvit_adaptive_pos_fwd / _bwd with its reduce kernel (csrc/adaptive.hip).  References are plain torch (permute / reshape for the layouts, a
stable CPU argsort for the ranks, float64 for the arithmetic) on the same rounded operands; none restates a kernel's loop.

Exact tier.  im2col, seq_patches and mae_mask move data or count: both dtypes are compared bit for bit (a bf16 output is one RNE step from
the fp32 value), on index ramps (a misplaced element names its source) and on a block of special values (+-0, +-inf, +-FLT_MAX, bf16 ties
with an even and an odd upper half and their neighbours).  adaptive_pos with w = 0, bias = 0 has h = 0, gelu(0) = 0 and gelu'(0) = 1/2 on
both GELU paths, so out == cat(cls, x) and dx == dout[:, pre:] bit for bit; with dout in multiples of 1/2 in [-4, 4] and seq_ps small
integers every term 0.5 * dout * sp_k is a multiple of 1/4 of magnitude <= 30 and every partial sum stays below 2^24 quarters
(test_tables_reach_every_branch), so dw, dbias and dcls equal the float64 sums exactly in any summation order, with and without
accumulation into integer-filled targets, and whatever the workspace held before.

Real-valued tier (adaptive_pos).  With A = |b| + sum_k |sp_k w_k| the KIN-step fma chain is off by e_h = (KIN + 1) U A.
  forward:  tol = 1.13 e_h + e_g + U (|x| + |g|) + u_out |ref|       1.13 >= |gelu'|, u_out = 2^-8 (bf16) or 0 (fp32)
            e_g = 2e-6 |h| for bf16 (the rational erfc of common.h, the constant test_gemm_bf16_gelu_epilogue_accuracy holds it to),
            e_g = 8 U |h| for fp32 (erff)
  backward: each term dout gelu'(h) sp_k carries |dout sp_k| (0.8 e_h + e_g') + 2 U |term|, 0.8 >= |gelu''|, e_g' = 2e-6 (bf16), 8 U (fp32);
            the sum adds depth U sum|terms|, depth = ceil(rpc / lanes) + lanes + ceil(chunks / 4) + 3 from the restated launch plan;
            dbias is the same without sp_k, dcls the plain sum bound, accumulation adds U |result|; dx stays bit-equal to dout[:, pre:].
The fp32 constants 8 U assume the device library's erff and expf are within 4 ulp.  That figure is an assumption, not derived: the
toolchain ships no document that states an error figure for either function, so none larger could be taken from one.  No other constant
comes from documentation; 2e-6 is the bound tests/test_hip_ops.py already holds the rational erfc to.
Every bound is shown to reject: position rows shifted by one token, the class row given token 0's position, two seq_ps columns swapped, the
bias left out, gelu' replaced by Phi, and tanh-GELU in place of erf-GELU for fp32 (for bf16 outputs the two differ by less than one output
ulp almost everywhere, so that rejection is not asked of the bf16 bounds).  The saturation cases (|w| ~ 1, |h| up to ~2000, both signs) use
the same bounds and also ask for finite outputs: they pin the p^16 overflow -> rcp(inf) = 0 branch of norm_cdf_fast2.

Launch plan.  pos_plan of adaptive.hip is restated below (column-block width cpb, row lanes, gx, rows per chunk, chunks; 8 rows per lane
forward, 32 backward); the case table is proven on the host to reach every property its comments name, and on the GPU the library's
workspace size must equal chunks (kin + 2) D 4 for every case.

Refusals.  Raw library calls with every output and the workspace sentinel-filled: a refused call returns an error and writes nothing.  The
shapes that sit exactly on a limit (im2col band, seq_patches staging tile and mae_mask row of exactly 64 KiB) are ordinary cases above and
must launch.  ucfvit_adaptive_pos_bwd takes no cls pointer (a NULL dcls means "not wanted", like dw and dbias), so "has_cls without a cls
pointer" is a forward refusal only.

Measured on the MI355X, worst err / bound per output and dtype over every case, fresh and accumulated (test_zz_ratios_report):
  pos_fwd   bf16 0.996  fp32 0.787      (bf16: the output rounding, whose bound 2^-8 |ref| is attained at the bottom of a binade)
  pos_dw    bf16 0.103  fp32 0.060
  pos_dbias bf16 0.057  fp32 0.037
  pos_dcls  bf16 0.218  fp32 0.250
No family is below 1e-3.  Within them the saturation cases alone sit lower (dw 0.001 / 0.004, dbias below 0.001 / 0.002 for bf16 / fp32):
there gelu' is exactly 0 or 1 on almost every element while the bound charges 0.8 e_h with A ~ 1000 to each; the bf16 dcls of fresh calls
with B <= 6 is at 0.001 because a sum of a few bf16 values is all but exact in fp32.  The exact tiers hold those outputs bit for bit.
"""
import ctypes
import math
from dataclasses import dataclass

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
UB = 2.0 ** -8
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = -12352.0                            # sentinel of the refusal tests (exact in bf16 and fp32)
RATIOS = {}


def _ops():
    from UCF_VIT._hip import ops
    return ops


def _lib():
    from UCF_VIT._hip import lib
    return lib


def _gen(seed, dev):
    return torch.Generator(device=dev).manual_seed(seed)


def _randn(shape, seed, dev, scale=1.0):
    return torch.randn(shape, generator=_gen(seed, dev), device=dev, dtype=F32) * scale


def _randint(lo, hi, shape, seed, dev):
    return torch.randint(lo, hi, shape, generator=_gen(seed, dev), device=dev)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((_bits(a) == _bits(b)).all())


def _dtn(dtype):
    return "bf16" if dtype == BF else "fp32"


def _within(got, ref, tol):
    return bool(((got.double() - ref).abs() <= tol).all())


def _check(got, ref, tol, wrong, what, key=None):
    """got within tol of ref everywhere, and the same tol rejects every reference in `wrong`; key: the family the worst err / tol is filed under"""
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, "
                                 f"worst excess {float((err - tol)[bad].max()):.3e}")
    if key is not None and bool((tol > 0).any()):
        RATIOS[key] = max(RATIOS.get(key, 0.0), float((err[tol > 0] / tol[tol > 0]).max()))
    for i, w in enumerate(wrong if isinstance(wrong, (list, tuple)) else [wrong]):
        assert not _within(got, w, tol), f"{what}: the bound does not reject wrong reference {i}"


def _check_exact(got, ref, wrong, what):
    """got == ref element for element (ref is float64 or an integer / same-dtype tensor), and every reference in `wrong` differs from it"""
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    ne = got.to(ref.dtype) != ref
    assert not bool(ne.any()), f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, first at flat index {int(ne.flatten().nonzero()[0])}"
    for i, w in enumerate(wrong):
        assert bool((w != ref).any()), f"{what}: wrong reference {i} equals the right one"


# ============================================================================================== special values
def _specials():
    """+-0, +-inf, +-FLT_MAX (rounds to inf in bf16), bf16 ties (low half 0x8000) over an even and an odd upper half, and the neighbours of
    those ties (0x7FFF, 0x8001), in both signs.  No NaN, no subnormals."""
    pos = [0x00000000, 0x7F800000, 0x7F7FFFFF, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x42FE8000, 0x42FF8000]
    words = pos + [w | 0x80000000 for w in pos]
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32).view(F32)


def _truncate_bf16(x):
    """wrong rounding: the low 16 bits cut off instead of round-to-nearest-even"""
    return (x.contiguous().view(torch.int32) & -65536).view(F32).to(BF)


# ============================================================================================== 1. im2col
IM2COL_CASES = [  # (B, C, spatial, p, special values)
    (2, 3, (32, 48), 8, True),
    (1, 1, (6, 10), 1, False),
    (2, 4, (8, 24), 2, False),
    (1, 3, (32, 32), 32, True),             # one patch, gx * p * p > 256
    (3, 1, (48, 16), 16, False),
    (1, 1, (16, 1024), 16, True),           # the band is exactly 64 KiB
    (1, 2, (8, 12, 20), 4, True),
    (2, 1, (16, 32, 48), 16, True),
    (1, 3, (4, 6, 10), 2, False),
]
_IM_IDS = [f"{'x'.join(map(str, sp))}-B{B}C{C}p{p}" for B, C, sp, p, _ in IM2COL_CASES]
_IM_PERM = {2: (0, 2, 4, 1, 3, 5), 3: (0, 2, 4, 6, 1, 3, 5, 7)}
_IM_WRONG = {2: {"ph/pw swapped": (0, 2, 4, 1, 5, 3), "channel innermost": (0, 2, 4, 3, 5, 1)},
             3: {"ph/pw swapped": (0, 2, 4, 6, 1, 5, 3, 7), "channel innermost": (0, 2, 4, 6, 3, 5, 7, 1), "pw/pd swapped": (0, 2, 4, 6, 1, 3, 7, 5)}}


def im2col_ref(x, p, perm=None):
    """rows (b, h, w[, z]), columns (c, ph, pw[, pd])"""
    B, C = x.shape[:2]
    sp = x.shape[2:]
    split = [B, C]
    for s in sp:
        split += [s // p, p]
    rows = B * math.prod(s // p for s in sp)
    return x.reshape(split).permute(perm or _IM_PERM[len(sp)]).reshape(rows, C * p ** len(sp))


def _im2col_input(B, C, sp, p, special, seed):
    x = _randn((B, C) + tuple(sp), seed, "cpu")
    if special:                              # inside the last patch of the last image and channel
        v = _specials()
        assert p ** len(sp) >= v.numel()
        patch = x[(B - 1, C - 1) + tuple(slice(s - p, s) for s in sp)]
        flat = patch.reshape(-1).clone()
        flat[:v.numel()] = v
        patch.copy_(flat.reshape(patch.shape))
    return x


def test_im2col_reference_and_wrong_references():
    """the reference against the definition cols[(b, h, w[, z]), (c, ph, pw[, pd])] = x[b, c, h p + ph, w p + pw[, z p + pd]], and every
    wrong reference differs from it wherever the swapped axes are longer than one"""
    x = _randn((2, 3, 4, 6), 1, "cpu")
    r = im2col_ref(x, 2)
    for b in range(2):
        for h in range(2):
            for w in range(3):
                for c in range(3):
                    for ph in range(2):
                        for pw in range(2):
                            assert r[(b * 2 + h) * 3 + w, (c * 2 + ph) * 2 + pw] == x[b, c, 2 * h + ph, 2 * w + pw]
    x = _randn((1, 2, 2, 4, 6), 2, "cpu")
    r = im2col_ref(x, 2)
    for h in range(1):
        for w in range(2):
            for z in range(3):
                for c in range(2):
                    for e in range(8):
                        ph, pw, pd = e >> 2, (e >> 1) & 1, e & 1
                        assert r[(h * 2 + w) * 3 + z, c * 8 + e] == x[0, c, 2 * h + ph, 2 * w + pw, 2 * z + pd]
    seen = set()
    for i, (B, C, sp, p, special) in enumerate(IM2COL_CASES):
        x = _im2col_input(B, C, sp, p, special, 100 + i)
        ref = im2col_ref(x, p)
        for name, perm in _IM_WRONG[len(sp)].items():
            if p > 1 and (C > 1 or name != "channel innermost"):
                assert not _same_bits(im2col_ref(x, p, perm), ref), f"{_IM_IDS[i]}: {name} equals the reference"
                seen.add((len(sp), name))
        assert not _same_bits(_truncate_bf16(ref), ref.to(BF)), f"{_IM_IDS[i]}: truncation equals rounding"
        if special:                          # the special block survives the reference in one piece and rounds as the docstring says
            v = _specials()
            assert bool(torch.isin(_bits(v), _bits(ref)).all())
    assert seen == {(nd, n) for nd in (2, 3) for n in _IM_WRONG[nd]}
    v16 = _bits(_specials().to(BF)).tolist()[:11]
    assert [w & 0xFFFF for w in v16] == [0x0000, 0x7F80, 0x7F80, 0x3F80, 0x3F82, 0x3F80, 0x3F81, 0x3F81, 0x3F82, 0x42FE, 0x4300]
    assert sum(s for *_, s in IM2COL_CASES) in (4, 5) and max(p * sp[-1] * 4 for _, _, sp, p, _ in IM2COL_CASES) == 64 * 1024


@gpu
@pytest.mark.parametrize("case", range(len(IM2COL_CASES)), ids=_IM_IDS)
def test_im2col_bit_exact(case):
    B, C, sp, p, special = IM2COL_CASES[case]
    ops = _ops()
    x = _im2col_input(B, C, sp, p, special, 100 + case)
    ref = im2col_ref(x, p)
    xd = x.to(DEV)
    for dtype in (F32, BF):
        got = ops.im2col(xd, p, dtype).cpu()
        want = ref.to(dtype)
        assert got.dtype == dtype and got.shape == want.shape
        ne = _bits(got) != _bits(want)
        assert not bool(ne.any()), f"{_dtn(dtype)}: {int(ne.sum())} elements differ, first at {ne.nonzero()[0].tolist()}"


# ============================================================================================== 2. seq_patches
SEQ_CASES = [  # (B, C, S, P)
    (2, 3, 12, 64),      # vector load and vector store; C wraps inside a 16-byte piece
    (1, 1, 7, 27),       # scalar load and scalar store; S % 4 = 3
    (2, 3, 5, 4),        # n = 12: vector store in fp32, scalar store in bf16
    (1, 12, 3, 8),       # C > EPV; S < 4
    (2, 1, 9, 16),       # C = 1
    (1, 5, 1, 9),        # S = 1; P % 4 != 0
    (1, 4, 5, 1024),     # the staging tile is exactly 64 KiB
    (2, 3, 196, 256),    # the bench's adaptive workload
]
_SEQ_IDS = [f"B{B}C{C}S{S}P{P}" for B, C, S, P in SEQ_CASES]
SP_TS = 4                # tokens per workgroup (adaptive.hip)


def seq_ref(x, dtype):
    B, C, S, P = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * S, P * C).to(dtype)


def _seq_wrong(x, dtype):
    B, C, S, P = x.shape
    ref = seq_ref(x, dtype)
    dropped = ref.clone().reshape(B, S, P * C)
    dropped[:, S - 1] = 0
    return {"(c p) order": x.permute(0, 2, 1, 3).reshape(B * S, C * P).to(dtype), "tokens shifted": ref.roll(1, 0),
            "last token dropped": dropped.reshape(B * S, P * C)}


def _seq_inputs(B, C, S, P, seed):
    """the index ramp x[b, c, s, p] = ((b C + c) S + s) P + p (exact in fp32), and normal values with the special block in the last token of
    the last image and channel where a patch is long enough to hold it"""
    ramp = torch.arange(B * C * S * P, dtype=F32).reshape(B, C, S, P)
    assert ramp.numel() < 2 ** 24
    x = _randn((B, C, S, P), seed, "cpu")
    v = _specials()
    if P >= v.numel():
        x[B - 1, C - 1, S - 1, :v.numel()] = v
    return {"ramp": ramp, "values": x}


def test_seq_patches_reference_and_wrong_references():
    x = _seq_inputs(2, 3, 5, 4, 0)["ramp"]
    r = seq_ref(x, F32)
    for b in range(2):
        for s in range(5):
            for p in range(4):
                for c in range(3):
                    assert r[b * 5 + s, p * 3 + c] == ((b * 3 + c) * 5 + s) * 4 + p
    seen = set()
    for i, (B, C, S, P) in enumerate(SEQ_CASES):
        for kind, x in _seq_inputs(B, C, S, P, 200 + i).items():
            for dtype in (F32, BF):
                ref = seq_ref(x, dtype)
                for name, w in _seq_wrong(x, dtype).items():
                    if (name == "(c p) order" and (C == 1 or P == 1)) or (name == "tokens shifted" and B * S == 1):
                        continue
                    assert not _same_bits(w, ref), f"{_SEQ_IDS[i]} {kind} {_dtn(dtype)}: {name} equals the reference"
                    seen.add(name)
    assert seen == {"(c p) order", "tokens shifted", "last token dropped"}


@gpu
@pytest.mark.parametrize("case", range(len(SEQ_CASES)), ids=_SEQ_IDS)
def test_seq_patches_bit_exact(case):
    B, C, S, P = SEQ_CASES[case]
    ops = _ops()
    for kind, x in _seq_inputs(B, C, S, P, 200 + case).items():
        xd = x.to(DEV)
        for dtype in (F32, BF):
            got = ops.seq_patches(xd, dtype).cpu()
            want = seq_ref(x, dtype)
            assert got.dtype == dtype and got.shape == want.shape
            ne = _bits(got) != _bits(want)
            if bool(ne.any()):
                r, c = ne.nonzero()[0].tolist()
                raise AssertionError(f"{kind} {_dtn(dtype)}: {int(ne.sum())} elements differ, first at row {r} column {c}: "
                                     f"got {float(got[r, c])}, want {float(want[r, c])}")


# ============================================================================================== 3. adaptive_pos: plan and cases
def pos_plan(rows, D, epv, rows_per_lane):
    """adaptive.hip pos_plan restated: column vectors per block (a power of two, at most 256), row lanes, column blocks, rows per chunk, chunks"""
    nvec = D // epv
    lg = 0
    while (1 << lg) < nvec and lg < 8:
        lg += 1
    cpb = 1 << lg
    lanes = 256 // cpb
    gx = -(-nvec // cpb)
    chunks = max(1, min(4096, -(-rows // (rows_per_lane * lanes))))
    rpc = -(-rows // chunks)
    return dict(cpb=cpb, lanes=lanes, gx=gx, rpc=rpc, chunks=-(-rows // rpc), inactive=gx * cpb - nvec)


RPL_FWD, RPL_BWD = 8, 32


@dataclass(frozen=True)
class PosC:
    dtype: torch.dtype
    D: int
    B: int
    S: int
    cls: bool
    kin: int
    real: bool = True            # False: exact tier only
    sat: bool = False            # |w| ~ 1

    @property
    def id(self):
        return f"{_dtn(self.dtype)}-D{self.D}-B{self.B}-S{self.S}-{'cls' if self.cls else 'nocls'}-k{self.kin}{'-sat' if self.sat else ''}"

    @property
    def epv(self):
        return 8 if self.dtype == BF else 4

    @property
    def pre(self):
        return 1 if self.cls else 0

    @property
    def rows(self):
        return self.B * (self.S + self.pre)

    def plan(self, backward):
        return pos_plan(self.rows, self.D, self.epv, RPL_BWD if backward else RPL_FWD)


POS_CASES = [
    PosC(F32, 4, 3, 50, True, 3), PosC(BF, 8, 3, 50, True, 4),                # one column vector, 256 row lanes, rows < lanes
    PosC(F32, 192, 5, 33, True, 4), PosC(BF, 192, 5, 33, True, 3),            # cpb above the vector count; forward chunks begin mid-item
    PosC(F32, 2048, 2, 12, True, 3), PosC(BF, 4096, 2, 12, False, 4),         # gx = 2, one row lane, no LDS reduction
    PosC(F32, 1280, 2, 12, True, 4), PosC(BF, 2560, 2, 12, True, 3),          # gx = 2 with 192 inactive columns in the second block
    PosC(F32, 1024, 3, 65, True, 3), PosC(BF, 2048, 3, 65, True, 4),          # backward chunks = 7, rpc = 29
    PosC(F32, 1024, 6, 15, True, 4),                                          # backward rpc = 32 = 2 N
    PosC(BF, 768, 5, 196, True, 3),                                           # two row lanes, 32 inactive columns, 16 backward chunks
    PosC(F32, 1024, 167, 196, True, 3), PosC(BF, 2048, 167, 196, True, 4),    # the forward chunk cap binds
    PosC(F32, 1024, 1, 131100, False, 4, real=False),                         # the backward chunk cap binds
]
SAT_CASES = [PosC(F32, 64, 2, 50, True, 3, sat=True), PosC(BF, 64, 2, 50, True, 4, sat=True)]
REAL_CASES = [c for c in POS_CASES if c.real] + SAT_CASES
HOST_ELEMS = 1 << 19             # the host tests run the cases with at most this many output elements


def test_pos_plan_matches_hand_computed():
    """the restated plan against plans worked out by hand from adaptive.hip for the case table"""
    P = lambda *a: tuple(pos_plan(*a)[k] for k in ("cpb", "lanes", "gx", "rpc", "chunks"))     # noqa: E731
    assert P(153, 4, 4, 8) == (1, 256, 1, 153, 1) and P(153, 8, 8, 32) == (1, 256, 1, 153, 1)
    assert P(170, 192, 4, 8) == (64, 4, 1, 29, 6) and P(170, 192, 4, 32) == (64, 4, 1, 85, 2)
    assert P(170, 192, 8, 8) == (32, 8, 1, 57, 3) and P(170, 192, 8, 32) == (32, 8, 1, 170, 1)
    assert P(26, 2048, 4, 8) == (256, 1, 2, 7, 4) and P(26, 2048, 4, 32) == (256, 1, 2, 26, 1)
    assert P(24, 4096, 8, 8) == (256, 1, 2, 8, 3) and P(24, 4096, 8, 32) == (256, 1, 2, 24, 1)
    assert P(26, 1280, 4, 8) == (256, 1, 2, 7, 4) and P(26, 2560, 8, 32) == (256, 1, 2, 26, 1)
    assert P(198, 1024, 4, 8) == (256, 1, 1, 8, 25) and P(198, 1024, 4, 32) == (256, 1, 1, 29, 7) and P(198, 2048, 8, 32) == (256, 1, 1, 29, 7)
    assert P(96, 1024, 4, 32) == (256, 1, 1, 32, 3)
    assert P(985, 768, 8, 8) == (128, 2, 1, 16, 62) and P(985, 768, 8, 32) == (128, 2, 1, 62, 16)
    assert P(32899, 1024, 4, 8) == (256, 1, 1, 9, 3656) and P(32899, 2048, 8, 32) == (256, 1, 1, 32, 1029)
    assert P(131100, 1024, 4, 32) == (256, 1, 1, 33, 3973) and P(131100, 1024, 4, 8) == (256, 1, 1, 33, 3973)
    assert P(131072, 1024, 4, 32) == (256, 1, 1, 32, 4096)


def test_tables_reach_every_branch():
    """from the restated plan: the case table holds every property its comments name"""
    by = {}
    for c in POS_CASES:
        by.setdefault((c.D, c.B, c.S), []).append(c)
    both = lambda cs: {c.dtype for c in cs} == {F32, BF}       # noqa: E731
    # one column vector, 256 row lanes, rows < lanes, the largest LDS reduction buffer of any plan
    one = by[(4, 3, 50)] + by[(8, 3, 50)]
    assert both(one) and all(c.plan(b)["cpb"] == 1 and c.plan(b)["lanes"] == 256 and c.rows < 256 for c in one for b in (0, 1))
    lds = lambda c: (c.plan(1)["lanes"] - 1) * c.plan(1)["cpb"] * (c.kin + 2) * c.epv * 4      # noqa: E731
    assert max(lds(c) for c in POS_CASES + SAT_CASES) == max(lds(c) for c in one) == 255 * 6 * 8 * 4 <= 64 * 1024
    # cpb above the vector count, forward chunks begin mid-item
    c192 = by[(192, 5, 33)]
    assert both(c192) and sorted(c.plan(0)["inactive"] for c in c192) == [8, 16]
    assert all(c.plan(0)["chunks"] > 1 and c.plan(0)["rpc"] % (c.S + c.pre) != 0 for c in c192)
    # gx = 2, one row lane (no LDS reduction), with and without inactive columns
    full = by[(2048, 2, 12)] + by[(4096, 2, 12)]
    assert both(full) and all(c.plan(b)["gx"] == 2 and c.plan(b)["lanes"] == 1 and c.plan(b)["inactive"] == 0 and lds(c) == 0 for c in full for b in (0, 1))
    assert {c.cls for c in full} == {True, False}
    part = by[(1280, 2, 12)] + by[(2560, 2, 12)]
    assert both(part) and all(c.plan(b)["gx"] == 2 and c.plan(b)["inactive"] == 192 for c in part for b in (0, 1))
    # backward chunks above 4 and no multiple of 4; a chunk length of 2 N
    seven = by[(1024, 3, 65)] + by[(2048, 3, 65)]
    assert both(seven) and all(c.plan(1)["chunks"] == 7 and c.plan(1)["rpc"] == 29 for c in seven)
    (c,) = by[(1024, 6, 15)]
    assert c.plan(1)["rpc"] == 32 == 2 * (c.S + c.pre) and c.plan(1)["chunks"] == 3 and c.cls
    (c,) = by[(768, 5, 196)]
    assert c.dtype == BF and c.plan(1)["lanes"] == 2 and c.plan(1)["inactive"] == 32 and c.plan(1)["chunks"] == 16
    # the chunk caps
    cap = by[(1024, 167, 196)] + by[(2048, 167, 196)]
    assert both(cap) and all(c.plan(0)["rpc"] == 9 > RPL_FWD and -(-c.rows // RPL_FWD) > 4096 for c in cap)
    (c,) = by[(1024, 1, 131100)]
    assert c.plan(1)["rpc"] == 33 > RPL_BWD and -(-c.rows // RPL_BWD) > 4096 and not c.real and not c.cls
    assert sum(not c.real for c in POS_CASES) == 1
    for dtype in (F32, BF):
        cs = [c for c in POS_CASES if c.dtype == dtype]
        assert {c.kin for c in cs} == {3, 4} and {c.cls for c in cs} == {True, False}
    assert {c.dtype for c in SAT_CASES} == {F32, BF} and all(c.D == 64 for c in SAT_CASES)
    # exact tier: |0.5 dout sp_k| <= 30 in quarters, prefill below 64: every partial sum is an integer number of quarters below 2^24
    assert all(4 * (30 * c.B * c.S + 64) < 2 ** 24 for c in POS_CASES + SAT_CASES)
    # the other three families: each load / store path of seq_patches, the tail group, the limits
    assert {(P % 4 == 0, (C * P) % 4 == 0, (C * P) % 8 == 0) for _, C, _, P in SEQ_CASES} >= {(True, True, True), (False, False, False), (True, True, False)}
    assert {S % SP_TS for _, _, S, _ in SEQ_CASES} == {0, 1, 3} and max(C * P * SP_TS * 4 for _, C, _, P in SEQ_CASES) == 64 * 1024
    assert any(C > 8 and S < SP_TS for _, C, S, _ in SEQ_CASES) and any(C == 1 for _, C, _, _ in SEQ_CASES)
    assert max(L for _, L, _ in MAE_CASES) * 4 == 64 * 1024 and {L for _, L, _ in MAE_CASES} >= {1, 255, 256, 257}


# ---------------------------------------------------------------------------------------------- references (float64, any device)
SQ2, SQ2PI = math.sqrt(2.0), math.sqrt(2.0 * math.pi)


def _Phi(h):
    return 0.5 * torch.erfc(-h / SQ2)


def gelu64(h):
    return h * _Phi(h)


def gelu_grad64(h):
    return _Phi(h) + h * torch.exp(-0.5 * h * h) / SQ2PI


def gelu_tanh64(h):
    return 0.5 * h * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (h + 0.044715 * h ** 3)))


def gelu_tanh_grad64(h):
    t = torch.tanh(math.sqrt(2.0 / math.pi) * (h + 0.044715 * h ** 3))
    return 0.5 * (1.0 + t) + 0.5 * h * (1.0 - t * t) * math.sqrt(2.0 / math.pi) * (1.0 + 3 * 0.044715 * h * h)


def pos_fwd_ref(x, sp, w, b, cls, B, S, act=gelu64, cls_pos=False):
    """x [B S, D], sp [B S, kin], w [D, kin], b [D], cls [D] or None, all float64 -> [B, S + pre, D]"""
    g = act(sp @ w.T + b)
    tok = (x + g).reshape(B, S, -1)
    if cls is None:
        return tok
    c = cls.expand(B, 1, -1)
    if cls_pos:
        c = c + g.reshape(B, S, -1)[:, :1]
    return torch.cat([c, tok], 1)


def pos_bwd_ref(dout, sp, w, b, pre, grad=gelu_grad64, rowmask=None, cls_rows=None):
    """dout [B, S + pre, D] float64 -> dw [D, kin], dbias [D], dcls [D] (zeros without a class token).  rowmask [B (S + pre)]: the output
    rows that are summed (wrong references drop some); cls_rows: 'bias' counts the class rows in dbias, 'pos' treats them as token 0"""
    B, N, D = dout.shape
    S = N - pre
    gd = grad(sp @ w.T + b)
    d = dout
    if rowmask is not None:
        d = dout * rowmask.reshape(B, N, 1).to(dout.dtype)
    dh = d[:, pre:].reshape(B * S, D) * gd
    dw, db = dh.T @ sp, dh.sum(0)
    dc = d[:, 0].sum(0) if pre else torch.zeros_like(db)
    if pre and cls_rows == "bias":
        db = db + dc
    if pre and cls_rows == "pos":
        e = d[:, 0] * gd.reshape(B, S, D)[:, 0]
        dw, db = dw + e.T @ sp.reshape(B, S, -1)[:, 0], db + e.sum(0)
    return dw, db, dc


def _seq_ps(c, seed, dev, exact):
    """the patcher's format: integer positions (in [0, 512), exact tier [0, 16)) and a power-of-two size"""
    T = c.B * c.S
    pos = _randint(0, 16 if exact else 512, (T, c.kin - 1), seed, dev)
    size = 2 ** _randint(0, 3 if exact else 7, (T, 1), seed + 1, dev)
    return torch.cat([pos, size], 1).float().reshape(c.B, c.S, c.kin)


def _halves(shape, seed, dev, dtype):
    return (_randint(-8, 9, shape, seed, dev).float() * 0.5).to(dtype)


def _gen_dev(c, dev):
    """the cases the host tests cover are generated on the CPU, so that the GPU tests see the very operands the host tests proved the wrong
    references on; the large ones are generated where they are used"""
    return "cpu" if c.rows * c.D <= HOST_ELEMS else dev


def _to(t, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in t.items()}


def _exact_inputs(c, dev):
    seed = c.D * 7 + c.S
    dev, to = _gen_dev(c, dev), dev
    return _to(dict(x=_randn((c.B * c.S, c.D), seed, dev).to(c.dtype), cls=_randn((c.D,), seed + 1, dev).to(c.dtype) if c.cls else None,
                sp=_seq_ps(c, seed + 2, dev, True), dout=_halves((c.B, c.S + c.pre, c.D), seed + 4, dev, c.dtype),
                w=torch.zeros((c.D, c.kin), dtype=c.dtype, device=dev), b=torch.zeros(c.D, dtype=c.dtype, device=dev)), to)


def _exact_refs(c, t):
    """float64 sums of the exact tier and the wrong references of the issue, from the restated backward plan"""
    sp64 = t["sp"].double().reshape(-1, c.kin)
    d64 = t["dout"].double()
    half = lambda h: torch.full_like(h, 0.5)                    # noqa: E731   gelu'(0)
    right = pos_bwd_ref(d64, sp64, t["w"].double(), t["b"].double(), c.pre, grad=half)
    p = c.plan(True)
    r = torch.arange(c.rows, device=d64.device)
    chunk = r // p["rpc"]
    masks = {"last row of a chunk dropped": (r % p["rpc"] != p["rpc"] - 1) & (r != c.rows - 1), "one chunk dropped": chunk != p["chunks"] // 2}
    if p["chunks"] >= 4:
        masks["fourth reduce lane dropped"] = chunk % 4 != 3
    wrong = {k: pos_bwd_ref(d64, sp64, t["w"].double(), t["b"].double(), c.pre, grad=half, rowmask=m) for k, m in masks.items()}
    if c.cls:
        wrong["class rows counted in dbias"] = pos_bwd_ref(d64, sp64, t["w"].double(), t["b"].double(), c.pre, grad=half, cls_rows="bias")
    wrong["dw written [kin][D]"] = (right[0].T.contiguous().reshape(c.D, c.kin), right[1], right[2])
    return right, wrong


def _flat(ref):
    return torch.cat([r.reshape(-1) for r in ref])


def test_pos_exact_tier_wrong_references_differ():
    """on the host, for the cases small enough: every wrong reference of the exact tier differs from the right one (so bit-equality with the
    right one rejects it), and the sums are exact in fp32 (integers of quarters below 2^24)"""
    seen = set()
    for c in POS_CASES + SAT_CASES:
        if c.rows * c.D > HOST_ELEMS:
            continue
        t = _exact_inputs(c, "cpu")
        right, wrong = _exact_refs(c, t)
        q = _flat(right) * 4
        assert bool((q == q.round()).all()) and float(q.abs().max()) < 2 ** 24
        assert bool((_flat(right).float().double() == _flat(right)).all())
        for k, wr in wrong.items():
            assert bool((_flat(wr) != _flat(right)).any()), f"{c.id}: {k} equals the right reference"
            seen.add(k)
    assert seen == {"last row of a chunk dropped", "one chunk dropped", "fourth reduce lane dropped", "class rows counted in dbias", "dw written [kin][D]"}


def _real_inputs(c, dev):
    seed = c.D * 11 + c.S + (5 if c.sat else 0)
    ws = 1.0 if c.sat else 0.02
    dev, to = _gen_dev(c, dev), dev
    return _to(dict(x=_randn((c.B * c.S, c.D), seed, dev).to(c.dtype), cls=_randn((c.D,), seed + 1, dev).to(c.dtype) if c.cls else None,
                sp=_seq_ps(c, seed + 2, dev, False), dout=_randn((c.B, c.S + c.pre, c.D), seed + 4, dev).to(c.dtype),
                w=_randn((c.D, c.kin), seed + 5, dev, ws).to(c.dtype), b=_randn((c.D,), seed + 6, dev, 0.1).to(c.dtype)), to)


def _real_fwd(c, t):
    """(reference, tolerance, wrong references) of the forward pass"""
    B, S, kin = c.B, c.S, c.kin
    x, sp, w, b = t["x"].double(), t["sp"].double().reshape(-1, kin), t["w"].double(), t["b"].double()
    cls = t["cls"].double() if c.cls else None
    h = sp @ w.T + b
    g = gelu64(h)
    e_h = (kin + 1) * U * (b.abs() + sp.abs() @ w.abs().T)
    e_g = (2e-6 if c.dtype == BF else 8 * U) * h.abs()
    u_out = UB if c.dtype == BF else 0.0
    ref = pos_fwd_ref(x, sp, w, b, cls, B, S)
    tol = (1.13 * e_h + e_g + U * (x.abs() + g.abs())).reshape(B, S, -1)
    if c.cls:
        tol = torch.cat([(U * cls.abs()).expand(B, 1, -1), tol], 1)
    tol = tol + u_out * ref.abs()
    swap = [1, 0] + list(range(2, kin))
    wrong = {"positions shifted by one token": pos_fwd_ref(x, sp.roll(1, 0), w, b, cls, B, S), "two seq_ps columns swapped": pos_fwd_ref(x, sp[:, swap], w, b, cls, B, S),
             "bias left out": pos_fwd_ref(x, sp, w, b * 0, cls, B, S)}
    if c.cls:
        wrong["class row given token 0's position"] = pos_fwd_ref(x, sp, w, b, cls, B, S, cls_pos=True)
    if c.dtype == F32:
        wrong["tanh-GELU"] = pos_fwd_ref(x, sp, w, b, cls, B, S, act=gelu_tanh64)
    return ref, tol, wrong


def _real_bwd(c, t):
    """(references, tolerances, wrong references) of dw, dbias, dcls"""
    kin, pre = c.kin, c.pre
    sp, w, b, d = t["sp"].double().reshape(-1, kin), t["w"].double(), t["b"].double(), t["dout"].double()
    p = c.plan(True)
    depth = -(-p["rpc"] // p["lanes"]) + p["lanes"] + -(-p["chunks"] // 4) + 3
    h = sp @ w.T + b
    e_h = (kin + 1) * U * (b.abs() + sp.abs() @ w.abs().T)
    e_gd = 2e-6 if c.dtype == BF else 8 * U
    dtok = d[:, pre:].reshape(-1, c.D)
    adh = (dtok * gelu_grad64(h)).abs()
    per = dtok.abs() * (0.8 * e_h + e_gd) + (2 + depth) * U * adh            # per term of dbias; times |sp_k| for dw
    ref = pos_bwd_ref(d, sp, w, b, pre)
    tol = (per.T @ sp.abs(), per.sum(0), depth * U * d[:, 0].abs().sum(0) if pre else torch.zeros_like(ref[2]))
    swap = [1, 0] + list(range(2, kin))
    wrong = {"positions shifted by one token": pos_bwd_ref(d, sp.roll(1, 0), w, b, pre), "two seq_ps columns swapped": pos_bwd_ref(d, sp[:, swap], w, b, pre),
             "bias left out": pos_bwd_ref(d, sp, w, b * 0, pre), "gelu' replaced by Phi": pos_bwd_ref(d, sp, w, b, pre, grad=_Phi)}
    if c.cls:
        wrong["class row given token 0's position"] = pos_bwd_ref(d, sp, w, b, pre, cls_rows="pos")
    if c.dtype == F32:
        wrong["tanh-GELU"] = pos_bwd_ref(d, sp, w, b, pre, grad=gelu_tanh_grad64)
    wrong_dc = []
    if c.cls:                                    # dcls does not depend on seq_ps: its wrong references lose or gain one row
        wrong_dc = [d[:-1, 0].sum(0), d[:, 0].sum(0) + d[0, 1]]
    return ref, tol, wrong, wrong_dc


def test_pos_real_tier_bounds_reject_wrong_references():
    """on the host, for the cases small enough: with the correctly rounded reference standing in for the kernel's output, every bound accepts
    it and rejects every wrong reference; the references against torch's own GELU and autograd"""
    h = torch.linspace(-9, 9, 1801, dtype=F64, requires_grad=True)
    y = torch.nn.functional.gelu(h)
    assert float((y - gelu64(h)).detach().abs().max()) < 1e-14
    (gd,) = torch.autograd.grad(y.sum(), h)
    assert float((gd - gelu_grad64(h.detach())).abs().max()) < 1e-14
    yt = torch.nn.functional.gelu(h, approximate="tanh")
    assert float((yt - gelu_tanh64(h)).detach().abs().max()) < 1e-14
    (gt,) = torch.autograd.grad(yt.sum(), h)
    assert float((gt - gelu_tanh_grad64(h.detach())).abs().max()) < 1e-13
    assert float(gd.abs().max()) < 1.13 and float(torch.autograd.grad(gelu_grad64(h).sum(), h)[0].abs().max()) < 0.8
    big = torch.tensor([-2000.0, -40.0, 40.0, 2000.0], dtype=F64)
    assert gelu64(big).tolist() == [0.0, 0.0, 40.0, 2000.0] and gelu_grad64(big).tolist() == [0.0, 0.0, 1.0, 1.0]
    for c in REAL_CASES:
        if c.rows * c.D > HOST_ELEMS:
            continue
        t = _real_inputs(c, "cpu")
        assert bool((t["sp"][..., :-1] < 512).all()) and bool((t["sp"] == t["sp"].round()).all()) and bool((torch.log2(t["sp"][..., -1]) % 1 == 0).all())
        ref, tol, wrong = _real_fwd(c, t)
        _check(ref.to(c.dtype), ref, tol, list(wrong.values()), f"{c.id} forward")
        (rw, rb, rc), (tw, tb, tc), wrong, wrong_dc = _real_bwd(c, t)
        _check(rw.float(), rw, tw, [v[0] for v in wrong.values()], f"{c.id} dw")
        _check(rb.float(), rb, tb, [v[1] for v in wrong.values()], f"{c.id} dbias")
        if c.cls:
            _check(rc.float(), rc, tc, wrong_dc, f"{c.id} dcls")
        if c.sat:
            hh = (t["sp"].double().reshape(-1, c.kin) @ t["w"].double().T).abs()
            assert float(hh.max()) > 1000 and float(hh.min()) < 25


# ---------------------------------------------------------------------------------------------- the kernels
@gpu
@pytest.mark.parametrize("c", POS_CASES + SAT_CASES, ids=lambda c: c.id)
def test_adaptive_pos_exact_tier(c):
    ops, L = _ops(), _lib().load()
    p = c.plan(True)
    need = L.ucfvit_adaptive_pos_bwd_workspace(c.B, c.S, c.D, c.kin, c.pre, ops.dt(torch.empty(0, dtype=c.dtype)))
    assert need == p["chunks"] * (c.kin + 2) * c.D * 4
    t = _exact_inputs(c, DEV)
    B, S, D, pre = c.B, c.S, c.D, c.pre
    out = ops.adaptive_pos_fwd(t["x"], t["sp"], t["w"], t["b"], t["cls"], B, S, D)
    assert out.shape == (B, S + pre, D) and out.dtype == c.dtype
    assert _same_bits(out[:, pre:].reshape(B * S, D), t["x"]), "forward: token rows are not x"
    if c.cls:
        assert _same_bits(out[:, 0], t["cls"].expand(B, D)), "forward: class rows are not cls"
    del out
    (rw, rb, rc), wrong = _exact_refs(c, t)
    want_dx = t["dout"][:, pre:].reshape(B * S, D)
    ops.workspace(need, t["dout"].device).fill_(float("nan"))               # whatever the workspace held must not matter
    dx, dw, db, dc = ops.adaptive_pos_bwd(t["dout"], t["sp"], t["w"], t["b"], B, S, D, c.cls)
    assert _same_bits(dx, want_dx), "dx is not dout[:, pre:]"
    _check_exact(dw, rw, [v[0] for k, v in wrong.items() if k != "class rows counted in dbias"], "dw")
    _check_exact(db, rb, [v[1] for k, v in wrong.items() if k != "dw written [kin][D]"], "dbias")
    if c.cls:
        _check_exact(dc, rc, [], "dcls")
    else:
        assert dc is None
    dx, dw, db, dc = ops.adaptive_pos_bwd(t["dout"], t["sp"], t["w"], t["b"], B, S, D, c.cls, want_dx=False)
    assert dx is None
    _check_exact(dw, rw, [], "dw (want_dx=False)"), _check_exact(db, rb, [], "dbias (want_dx=False)")
    if c.cls:
        _check_exact(dc, rc, [], "dcls (want_dx=False)")
    for bits in (1, 2, 4, 7):
        pw, pb = _randint(-31, 32, (D, c.kin), bits, DEV).float(), _randint(-31, 32, (D,), bits + 10, DEV).float()
        pc = _randint(-31, 32, (D,), bits + 20, DEV).float() if c.cls else None
        tw, tb, tc = pw.clone(), pb.clone(), (pc.clone() if c.cls else None)
        dx, dw, db, dc = ops.adaptive_pos_bwd(t["dout"], t["sp"], t["w"], t["b"], B, S, D, c.cls, dw=tw, dbias=tb, dcls=tc, acc_bits=bits)
        assert dw is tw and db is tb and dc is tc and _same_bits(dx, want_dx)
        _check_exact(tw, rw + pw.double() if bits & 1 else rw, [], f"dw acc_bits={bits}")
        _check_exact(tb, rb + pb.double() if bits & 2 else rb, [], f"dbias acc_bits={bits}")
        if c.cls:
            _check_exact(tc, rc + pc.double() if bits & 4 else rc, [], f"dcls acc_bits={bits}")


@gpu
@pytest.mark.parametrize("c", REAL_CASES, ids=lambda c: c.id)
def test_adaptive_pos_real_tier(c):
    ops = _ops()
    t = _real_inputs(c, DEV)
    B, S, D, pre, n = c.B, c.S, c.D, c.pre, _dtn(c.dtype)
    fam = n                                      # one family per output and dtype: fresh, accumulated and saturated calls share a bound
    out = ops.adaptive_pos_fwd(t["x"], t["sp"], t["w"], t["b"], t["cls"], B, S, D)
    assert bool(torch.isfinite(out).all()), "forward: non-finite output"
    ref, tol, wrong = _real_fwd(c, t)
    _check(out, ref, tol, list(wrong.values()), f"{c.id} forward", f"pos_fwd-{fam}")
    del out, ref, tol, wrong
    (rw, rb, rc), (tw, tb, tc), wrong, wrong_dc = _real_bwd(c, t)
    dx, dw, db, dc = ops.adaptive_pos_bwd(t["dout"], t["sp"], t["w"], t["b"], B, S, D, c.cls)
    assert _same_bits(dx, t["dout"][:, pre:].reshape(B * S, D)), "dx is not dout[:, pre:]"
    assert all(bool(torch.isfinite(g).all()) for g in (dw, db) + ((dc,) if c.cls else ())), "backward: non-finite gradient"
    _check(dw, rw, tw, [v[0] for v in wrong.values()], f"{c.id} dw", f"pos_dw-{fam}")
    _check(db, rb, tb, [v[1] for v in wrong.values()], f"{c.id} dbias", f"pos_dbias-{fam}")
    if c.cls:
        _check(dc, rc, tc, wrong_dc, f"{c.id} dcls", f"pos_dcls-{fam}")
    # accumulated into normal targets: + U |result|
    pw, pb, pc = _randn((D, c.kin), 31, DEV), _randn((D,), 32, DEV), (_randn((D,), 33, DEV) if c.cls else None)
    aw, ab, ac = pw.clone(), pb.clone(), (pc.clone() if c.cls else None)
    ops.adaptive_pos_bwd(t["dout"], t["sp"], t["w"], t["b"], B, S, D, c.cls, want_dx=False, dw=aw, dbias=ab, dcls=ac, acc_bits=7)
    shift = lambda vs, i, pre_: [v[i] + pre_.double() for v in vs]                   # noqa: E731
    _check(aw, rw + pw.double(), tw + U * (rw + pw.double()).abs(), shift(wrong.values(), 0, pw), f"{c.id} dw +=", f"pos_dw-{fam}")
    _check(ab, rb + pb.double(), tb + U * (rb + pb.double()).abs(), shift(wrong.values(), 1, pb), f"{c.id} dbias +=", f"pos_dbias-{fam}")
    if c.cls:
        _check(ac, rc + pc.double(), tc + U * (rc + pc.double()).abs(), [v + pc.double() for v in wrong_dc], f"{c.id} dcls +=", f"pos_dcls-{fam}")


# ============================================================================================== 4. mae_mask
MAE_CASES = [(1, 1, 0), (1, 1, 1), (3, 7, 0), (3, 7, 7), (2, 255, 64), (2, 256, 64), (2, 257, 64), (5, 196, 49), (2, 4097, 1024),
             (2, 16384, 4096)]       # (B, L, len_keep); the last is the LDS row limit
MAE_NOISE = ["rand", "four-levels", "all-equal", "signed-zeros", "inf", "nan"]


def mae_noise(kind, B, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, L), generator=g)
    pick = lambda n: torch.randperm(L, generator=g)[:n]          # noqa: E731
    if kind == "four-levels":
        x = torch.floor(x * 4) / 4
    elif kind == "all-equal":
        x = torch.full((B, L), 0.25)
    elif kind == "signed-zeros":             # -0.0 == +0.0: the index decides
        x[0] = torch.where(torch.rand(L, generator=g) < 0.5, -0.0, 0.0)
        x[0, pick(max(1, L // 3))] = 0.5
    elif kind == "inf":
        x[0, pick(max(1, L // 4))] = float("inf")
        x[0, pick(max(1, L // 4))] = float("-inf")
    elif kind == "nan":                      # at several positions, the first and the last among them, beside infinities
        x[0, pick(max(1, L // 5))] = float("inf")
        x[0, pick(max(1, L // 5))] = float("nan")
        x[0, 0] = x[0, L - 1] = x[0, L // 2] = float("nan")
        x[B - 1, L // 3] = float("nan")
    return x


def mae_ref(noise, len_keep):
    shuffle = torch.argsort(noise, dim=1, stable=True)
    restore = torch.argsort(shuffle, dim=1)
    return shuffle, restore, (restore >= len_keep).float()


def _rank_by_counting(noise, nan_last):
    """the kernel's method on the host: rank = number of keys ordered before this one; nan_last=False is the comparison the kernel had"""
    x, y = noise[:, :, None], noise[:, None, :]
    i, j = torch.arange(noise.shape[1])[None, :, None], torch.arange(noise.shape[1])[None, None, :]
    before, same = y < x, y == x
    if nan_last:
        xn, yn = x != x, y != y
        before, same = torch.where(xn, ~yn, before), torch.where(xn, yn, same)
    return (before | (same & (j < i))).sum(2)


def test_mae_reference_and_the_counting_order():
    """the reference against its definition (a stable sort: keys ascending, -0 == +0, NaN last, index order among equals), the total order
    the kernel counts with reproduces it for every noise kind, and the order it had before does not for NaN"""
    for B, L, keep in MAE_CASES:
        if L > 257:
            continue
        for k, kind in enumerate(MAE_NOISE):
            x = mae_noise(kind, B, L, 300 + k)
            shuffle, restore, mask = mae_ref(x, keep)
            assert bool((shuffle.sort(1).values == torch.arange(L)).all()) and bool((torch.gather(shuffle, 1, restore) == torch.arange(L)).all())
            s = torch.gather(x, 1, shuffle)
            a, b_, ia, ib = s[:, :-1], s[:, 1:], shuffle[:, :-1], shuffle[:, 1:]
            an, bn = a != a, b_ != b_
            assert bool((bn | (~an & (a <= b_))).all()), f"{kind}: not ascending with NaN last"
            assert bool(((ia < ib) | ~((a == b_) | (an & bn))).all()), f"{kind}: equal keys out of index order"
            assert int(mask.sum()) == B * (L - keep)
            assert bool((_rank_by_counting(x, True) == restore).all()), f"{kind} L={L}"
            old = _rank_by_counting(x, False)
            if kind == "nan" and L > 1:
                assert bool((old != restore).any()) and bool((old.sort(1).values != torch.arange(L)).any())
            else:
                assert bool((old == restore).all())
    x = mae_noise("signed-zeros", 2, 64, 1)
    assert bool((x[0] == 0).any()) and bool(torch.signbit(x[0][x[0] == 0]).any()) and not bool(torch.signbit(x[0][x[0] == 0]).all())
    assert int(torch.isnan(mae_noise("nan", 2, 255, 1)).sum()) >= 4


@gpu
@pytest.mark.parametrize("kind", MAE_NOISE)
def test_mae_mask_bit_exact(kind):
    """every case with this kind of noise; the outputs are compared and go nowhere else (with NaN keys the kernel once left slots of
    ids_shuffle unwritten, which a gather would have indexed with)"""
    ops = _ops()
    for i, (B, L, keep) in enumerate(MAE_CASES):
        x = mae_noise(kind, B, L, 300 + MAE_NOISE.index(kind) + 17 * i)
        shuffle, restore, mask = (t.cpu() for t in ops.mae_mask(x.to(DEV), keep))
        rs, rr, rm = mae_ref(x, keep)
        what = f"B={B} L={L} keep={keep}"
        assert restore.dtype == torch.int64 and bool((restore == rr).all()), f"{what}: ids_restore differs in {int((restore != rr).sum())} places"
        assert shuffle.dtype == torch.int64 and bool((shuffle == rs).all()), f"{what}: ids_shuffle differs in {int((shuffle != rs).sum())} places"
        assert mask.dtype == F32 and bool((mask == rm).all()), f"{what}: mask differs"


# ============================================================================================== 5. refusals: loud, and nothing written
@gpu
def test_refusals_write_nothing():
    """the library's own entry checks (raw calls, every output and the workspace sentinel-filled): the call returns an error and no output
    element changes; then the same refusals as ops raises them"""
    ops, lib = _ops(), _lib()
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    N = 1 << 17
    zb, zf = torch.zeros(N, dtype=BF, device=DEV), torch.zeros(N, dtype=F32, device=DEV)
    ob = [torch.full((N,), SENT, dtype=BF, device=DEV) for _ in range(1)]
    of = [torch.full((N,), SENT, dtype=F32, device=DEV) for _ in range(4)]
    oi = [torch.full((N,), int(SENT), dtype=torch.int64, device=DEV) for _ in range(2)]
    ws = torch.full((N,), SENT, dtype=F32, device=DEV)
    P = lambda t: t.data_ptr()            # noqa: E731
    BFC, F32C, BADC = ops.dt(zb), ops.dt(zf), 7
    assert BADC not in (BFC, F32C)

    def refused(what, rc):
        torch.cuda.synchronize()
        assert rc != 0, f"{what}: accepted"
        for t_ in ob + of + oi + [ws]:
            assert bool((t_ == SENT).all()), f"{what}: a refused call wrote to an output or to the workspace"

    dims = lambda *d: (ctypes.c_int64 * 3)(*(list(d) + [1] * (3 - len(d)))[:3])      # noqa: E731
    # im2col: extent no multiple of p, nd of 1 and 4, a bad dtype code, a band of 66560 bytes
    refused("im2col H=30 p=8", L.ucfvit_im2col(P(zf), P(of[0]), 1, 1, dims(30, 32), 2, 8, F32C, st))
    refused("im2col Z=10 p=4", L.ucfvit_im2col(P(zf), P(ob[0]), 1, 1, dims(8, 8, 10), 3, 4, BFC, st))
    refused("im2col nd=1", L.ucfvit_im2col(P(zf), P(of[0]), 1, 1, dims(32), 1, 8, F32C, st))
    refused("im2col nd=4", L.ucfvit_im2col(P(zf), P(of[0]), 1, 1, dims(8, 8, 8), 4, 8, F32C, st))
    refused("im2col dtype", L.ucfvit_im2col(P(zf), P(of[0]), 1, 1, dims(32, 32), 2, 8, BADC, st))
    assert 16 * 1040 * 4 == 66560
    refused("im2col W=1040 p=16", L.ucfvit_im2col(P(zf), P(of[0]), 1, 1, dims(16, 1040), 2, 16, F32C, st))
    # seq_patches: a bad dtype, a row of 4097 floats, no tokens
    refused("seq_patches dtype", L.ucfvit_seq_patches(P(zf), P(of[0]), 1, 3, 8, 16, BADC, st))
    refused("seq_patches C*P=4097", L.ucfvit_seq_patches(P(zf), P(of[0]), 1, 1, 4, 4097, F32C, st))
    refused("seq_patches C*P=4097 bf16", L.ucfvit_seq_patches(P(zf), P(ob[0]), 1, 17, 4, 241, BFC, st))
    refused("seq_patches S=0", L.ucfvit_seq_patches(P(zf), P(of[0]), 2, 3, 0, 16, F32C, st))
    # adaptive_pos forward and backward
    for z, code, o, epv in ((zf, F32C, of[0], 4), (zb, BFC, ob[0], 8)):
        fwd = lambda D=64, kin=3, has_cls=1, cls=P(z), x=P(z), c=code: L.ucfvit_adaptive_pos_fwd(     # noqa: E731
            x, P(zf), P(z), P(z), cls, P(o), 2, 8, D, kin, has_cls, c, st)
        bwd = lambda D=64, kin=3, acc=0, dout=P(z), c=code: L.ucfvit_adaptive_pos_bwd(                # noqa: E731
            dout, P(zf), P(z), P(z), P(o), P(of[1]), P(of[2]), P(of[3]), 2, 8, D, kin, 1, acc, P(ws), c, st)
        for name, call in (("fwd", fwd), ("bwd", bwd)):
            refused(f"adaptive_pos_{name} kin=2", call(kin=2))
            refused(f"adaptive_pos_{name} kin=5", call(kin=5))
            refused(f"adaptive_pos_{name} D % epv", call(D=64 + epv // 2))
            refused(f"adaptive_pos_{name} dtype", call(c=BADC))
        refused("adaptive_pos_fwd has_cls without cls", fwd(cls=None))
        refused("adaptive_pos_fwd misaligned x", fwd(x=P(z) + 4))
        refused("adaptive_pos_bwd accumulate=8", bwd(acc=8))
        refused("adaptive_pos_bwd misaligned dout", bwd(dout=P(z) + 4))
    # mae_mask
    mae = lambda Lp, keep: L.ucfvit_mae_mask(P(zf), P(oi[0]), P(oi[1]), P(of[0]), 2, Lp, keep, st)     # noqa: E731
    refused("mae_mask L=16385", mae(16385, 4))
    refused("mae_mask len_keep > L", mae(16, 17))
    refused("mae_mask len_keep < 0", mae(16, -1))
    # the same through ops
    E = lib.HipLibraryError
    with pytest.raises(E):
        ops.im2col(torch.zeros(1, 1, 30, 32, device=DEV), 8, F32)
    with pytest.raises(E):
        ops.im2col(torch.zeros(1, 1, 16, 1040, device=DEV), 16, BF)
    with pytest.raises(TypeError):
        ops.im2col(torch.zeros(1, 1, 32, 32, dtype=BF, device=DEV), 8, BF)
    with pytest.raises(E):
        ops.seq_patches(torch.zeros(1, 1, 4, 4097, device=DEV), F32)
    with pytest.raises(TypeError):
        ops.seq_patches(torch.zeros(1, 4, 16, device=DEV), F32)
    with pytest.raises(E):
        ops.mae_mask(torch.zeros(2, 16385, device=DEV), 4)
    with pytest.raises(E):
        ops.mae_mask(torch.zeros(2, 16, device=DEV), 17)
    B, S, D = 2, 8, 64
    sp = torch.zeros(B, S, 3, device=DEV)
    x, w, b, cls = (torch.zeros(s, dtype=BF, device=DEV) for s in ((B * S, D), (D, 3), (D,), (D,)))
    dout = torch.zeros(B, S + 1, D, dtype=BF, device=DEV)
    with pytest.raises(ValueError):
        ops.adaptive_pos_fwd(x, sp, w, b.float(), cls, B, S, D)
    with pytest.raises(E):
        ops.adaptive_pos_fwd(x[:, :12].contiguous(), sp, w[:12].contiguous(), b[:12].contiguous(), None, B, S, 12)
    # backward: a bias of the wrong dtype or length is refused before any launch (the kernel would read it with the wrong element size)
    for bad in (b.float(), b[:D - 8].contiguous(), torch.zeros(2 * D, dtype=BF, device=DEV)):
        tw, tb, tc = of[1][:D * 3].view(D, 3), of[2][:D], of[3][:D]
        with pytest.raises(ValueError):
            ops.adaptive_pos_bwd(dout, sp, w, bad, B, S, D, True, dw=tw, dbias=tb, dcls=tc)
        refused("ops.adaptive_pos_bwd bias", 1)
    with pytest.raises(ValueError):
        ops.adaptive_pos_bwd(dout, sp, w.float(), b, B, S, D, True)
    with pytest.raises(E):
        ops.adaptive_pos_bwd(dout, sp, w, b, B, S, D, True, acc_bits=8)
    # the accepted neighbours of the refused calls run (so the refusals above are the checks', not a broken call's)
    ops.adaptive_pos_bwd(dout, sp, w, b, B, S, D, True)
    ops.adaptive_pos_fwd(x, sp, w, b, cls, B, S, D)
    torch.cuda.synchronize()


def test_zz_ratios_report():
    """last test of the file: the worst err / bound per output and dtype seen by this process (with a GPU: the library's)"""
    for k in sorted(RATIOS):
        print(f"RATIO SUMMARY {k}: {RATIOS[k]:.3f}")
    assert all(r <= 1.0 for r in RATIOS.values())
