"""Every dispatch branch of the GEMM family (csrc/gemm.hip, csrc/gemm2.hip, csrc/gemm_stagger.hip) against float64 products of the same
rounded operands, element by element, through UCF_VIT._hip.ops.  U = 2^-24 (fp32 unit roundoff), UB = 2^-8 (bf16 unit roundoff: 8 significant bits, so round
to nearest moves a value v by up to half an ulp = 2^-8 of the bottom of its binade, i.e. up to 2^-8 |v|; 2^-9 |v| holds only at the top of a
binade, and the CPU emulation below shows a correctly rounded bf16 result at 1.64 times a bound written with 2^-9).

Tier 1, exact.  Operands are small integers (entries in [-4, 4]), so every product and every partial sum in any order is an integer
below 2^24 and the fp32 accumulator is exact whatever the K order, the split or the tile schedule.  fp32 outputs are torch.equal to the
float64 result, bf16 outputs bit-equal to the float64 result rounded ONCE; integer bias / residual / aux / old C pin the epilogue order of
include/ucfvit_hip.h (alpha*acc, +bias, act, +residual, +C_old, one rounding): the twice-rounded result (rounded before the residual), the
bias of the neighbouring column and the residual of the neighbouring row are formed on the host, shown to differ from the right result
in the first and the last tile band they guard, and shown to differ from what the kernel wrote.  Column sums equal the float64 column sums
of the UNROUNDED values exactly; the "big" case has |C| > 256 in most elements, so the sums of the rounded outputs differ, and the test
says so.  alpha in {0.5, 2, -1} stays exact.  The exactness condition (sum of absolute values behind every accumulator < 2^24) is computed
in float64 from the operands actually used and asserted, never skipped.  Symmetries are bit for bit: a second call, static vs dynamic tile
schedule, grouped vs alone, UCFVIT_GEMM_CUS = 8 / 200 / 256.

Tier 2, per-element bounds on real-valued operands (families: randn with the scales of the older tests; rows of A with a common offset of
8 sigma, so |ref| << |A|.|B|; entries spanning 2^-20 .. 2^20).  For every output element
    |got - ref| <= t + ou (|ref| + t),      ou = UB (bf16 output) or U (fp32 output)
    t = |alpha| d U (|A|.|B|)[m][n], carried through the epilogue: + U |v| per epilogue operation, times |aux| or |gelu'|.
d is the longest fp32 addition chain a product passes through in the kernel that runs the case, read off that kernel:
    bf16 MFMA kernels (gemm_mfma_kernel<bf16>, gemm2_kernel, gemm3_kernel, the staggered kernel): one v_mfma_f32_16x16x32_bf16 adds 32
        products to its accumulator (counted as 32 additions), and a tile's accumulator goes through ceil(K / 32) of them: d = ceil(K/32) + 32.
        The staggered kernel's rotated K order has the same length.  Split-K: the chain of one slice is shorter, plus `splits` additions in
        splitk_reduce_kernel: d = ceil(K/32) + 32 + splits.
    fp32 MFMA (v_mfma_f32_16x16x4_f32): d = ceil(K/4) + 4.      scalar fallback: one fmaf per k: d = K.
GELU epilogues: the activation's own error is the contract of test_gemm_bf16_gelu_epilogue_accuracy (2^-8 relative + 2e-6 absolute, on
gelu and on gelu'), added to the propagated pre-activation error (sup |gelu'| = 1.13, sup |gelu''| = 0.80).  ACT_GELU with aux_out applies
the activation to the STORED (rounded) pre-activation in every kernel, so there the output is compared with gelu of the aux_out the kernel
wrote, and aux_out with the pre-activation under its own bound.  Column sums: against the float64 column sums of the unrounded reference,
tol = sum_m t + (128 + 2 ceil(M/256) + 2) U sum_m |ref| (the 128 rows of a block, ucfvit_reduce_rows over 2 ceil(M/256) partial rows).
Every Tier 2 comparison goes through Pool.check, which requires the same bound to reject wrong references: the last k element dropped,
the last K tile dropped, one more element added to the contraction, bias of the neighbouring column, residual / aux of the neighbouring
row, residual added before the activation, alpha left out, C_old left out or added twice, column sums of the rounded outputs, column sums
missing the last 128-row block.  Families are pooled per case: the offset family hides a dropped k element of a zero-mean B under the
output rounding of bf16 where |ref| is large, the randn family rejects it; the randn family hides the column sums of rounded outputs at
large M (the sum of M roundings grows as sqrt(M), the bound as M): required up to M = 4096, beyond that the exact "big" case rejects them.
At K = 131005 the bound (d U = 2.5e-4 of |A|.|B|) exceeds 1 / K: no family can show one k element there, the exact tier does; the
all-positive family shows the dropped 61-element last K tile.

Edges: every operand and output is a view into a larger buffer whose remaining elements are NaN (inputs) or a sentinel (outputs): columns
beyond K / N inside lda / ldb / ldc / ldr / ldaux and the rows after the last; the results are NaN-free and every sentinel outside
C[:M,:N], aux_out[:M,:N] and the column-sum vector is untouched bit for bit.  M = 0 and N = 0 return without touching anything.  K = 0
with M, N > 0 is REFUSED loudly ("null operand pointer": a tensor without elements has a NULL data pointer, also as a view) and leaves C
untouched: pinned.  An Inf in one row of A reaches that row of C only.

Dispatch (read off gemm_route and its helpers in csrc/gemm_route.h, and ucfvit_gemm_grouped; _branch() restates it and is asserted to
agree with ucfvit_gemm_colsum_rows > 0 and ucfvit_gemm_workspace > 0 on every case, and to equal the library's own answer,
ucfvit_gemm_route, on the descriptor of every launch whose branch is named here; test_gemm_route_query_* ask it without a GPU, from
descriptors made of fake addresses, for every entry of CASES with both tile schedules and under every UCFVIT_GEMM_STAGGER setting):
    v1-scalar     N % 4 != 0, unaligned ld, M*N < 256                          (5,2,64) (33,42,24) (33,40,20) (130,6,200)
    v1-mfma       fp32 any shape; bf16 with M, N or K < 128                     fp32 x 4 layouts (260,264,200); bf16 (100,264,256) (700,64,136) (304,384,64)
    g2-128        bf16, M,N,K >= 128, t256 < 192, no split                      4 layouts x bf16/fp32 out (696,384,136); every act (1000,520,200)
    g2-128-splitk plain epilogue, t128 < 384, ucfvit_gemm_workspace > 0         (KS,KS) (1024,1024,131005) (1024,4096,4096)
    g2-128        the same plans with the workspace withheld                    (1024,1024,4096) split_k_workspace=False
    g2-256        t256 >= 192 and an operand spanning >= 4 GiB                  A [49152][43696] padded view, K 256, N 256
    g3-PLAIN[+CS] g3-RESIDUAL g3-GELU g3-GELU_GRAD g3-GELU_SAVE_DERIV g3-MUL_AUX[+CS]   (KC,KC), bf16 out, no accumulate, t256 >= 192
    g3-GENERIC    t256 >= 192 and: another layout / fp32 out / accumulate / act + residual / alpha with any of these
    stagger-*     the four epilogues at K % 64 == 0, nk >= 16 (residual nk >= 32); forced with UCFVIT_GEMM_STAGGER = 1 / 2 / 4 / 8
    grouped       1, 4, 5, 32 problems, fp32 and bf16 out, mixed accumulate, dynamic schedule; not groupable -> separate ucfvit_gemm calls
Not covered: ACT_MUL_AUX / GELU_GRAD with a bias on the staggered kernel (it declines them by design: the ping-pong kernel runs them);
K = 0 with non-NULL operand pointers (ops cannot express it: a tensor without elements has a NULL data pointer).

Measured on an MI355X: 217 GPU cases + 7 CPU cases (the emulation, the route query over CASES and its five UCFVIT_GEMM_STAGGER children:
11 s together without a GPU), 30 s (tests/test_gemm_stagger.py in the same run: 35 s, 31 s of it in its three forced
children; the four forced children of this file take 4 - 5 s each, the three UCFVIT_GEMM_CUS children 7 s together).
  worst err / bound         C bf16   C fp32   aux_out   colsum
  v1-mfma                   0.995    0.21     0.99 (pre-activation)
  v1-scalar                 0.97     0.14
  g2-128                    0.995    0.02     0.995 (pre-activation), 0.50 (gelu')
  g2-128-splitk             0.99     0.09
  g2-256                    0.995
  g3 specialised / generic  0.996    0.03     0.50 (gelu')             0.011 plain, 0.004 multiply-by-aux
  stagger                   0.995             0.50 (gelu')
  grouped / its fallback    0.99     0.05 / 0.03
bf16 outputs sit at the bound because the bound there IS the output rounding (half an ulp of a value at the bottom of its binade); the
fp32 outputs show the accumulation itself: the derived d overstates the error of the MFMA chains by 5 to 100 times, as a worst-case
chain bound does for roundings of random sign.  No ratio above 1 and no defect found: every branch passed both tiers at first run.
A bound written with ou = 2^-9 cannot be met by a correctly rounded bf16 result (the CPU case shows 1.64); ou is the unit roundoff 2^-8.
"""
import math
import os
import subprocess
import sys
from dataclasses import dataclass, replace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for _p in (os.path.join(ROOT, "ucf-vit_amd"), ROOT):
        if _p not in sys.path:
            sys.path.insert(0, _p)

gpu = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
UB = 2.0 ** -8
GA, GB = 2.0 ** -8, 2e-6          # the measured contract of the GELU epilogues (test_gemm_bf16_gelu_epilogue_accuracy)
BF, F32 = torch.bfloat16, torch.float32
KC, KS = 0, 1
NONE, GELU, GELU_GRAD, GELU_SD, MUL_AUX = 0, 1, 2, 3, 4
LIM = 2.0 ** 24
SENT = -12352.0                   # sentinel of output padding (exact in bf16 and fp32)
PADC, PADR = 8, 2                 # poisoned columns behind every row, poisoned rows behind the last


def _ops():
    from UCF_VIT._hip import ops
    return ops


def _cdiv(a, b):
    return -(-a // b)


@dataclass(frozen=True)
class Case:
    branch: str
    M: int
    N: int
    K: int
    la: int = KC
    lb: int = KC
    f32: bool = False          # fp32 operands (always fp32 output)
    out32: bool = False
    act: int = NONE
    bias: bool = False
    res: bool = False
    acc: bool = False
    alpha: float = 1.0
    cs: str = ""               # "", "ow" (overwrite), "acc" (accumulate): column sums of C
    aux_out: bool = False      # ACT_GELU only (ACT_GELU_SAVE_DERIV always writes it)
    ws: bool = True            # hand the split-K workspace over
    dyn: bool = False          # dynamic tile schedule
    span4g: bool = False       # A is a row-padded view spanning just over 4 GiB
    gen: str = ""              # Tier 1 generator: "int" [-4, 4] or "big" (entries in {+-3, +-4}); default: big where a bf16 rounding is pinned
    emu_splits: int = 0        # CPU emulation only: K slices of the emulated split-K
    fams: tuple = ("randn", "offset", "exp")

    @property
    def id(self):
        e = {NONE: "", GELU: "gelu", GELU_GRAD: "ggrad", GELU_SD: "gsd", MUL_AUX: "mul"}[self.act]
        f = [self.branch, f"{self.M}x{self.N}x{self.K}", "CS"[self.la] + "CS"[self.lb], "f32" if self.f32 else ("o32" if self.out32 else "bf")]
        f += [x for x, on in ((e, e), ("b", self.bias), ("r", self.res), ("acc", self.acc), (f"a{self.alpha}", self.alpha != 1.0),
                              ("cs" + self.cs, self.cs), ("aux", self.aux_out), ("nows", not self.ws), ("dyn", self.dyn)) if on]
        return "-".join(f)

    @property
    def aux_in(self):
        return self.act in (GELU_GRAD, MUL_AUX)

    @property
    def has_aux_out(self):
        return self.act == GELU_SD or (self.act == GELU and self.aux_out)

    @property
    def lda(self):
        if self.span4g:
            return _cdiv(_cdiv(2 ** 31 + 2 ** 20, self.M), 8) * 8
        return (self.K if self.la == KC else self.M) + PADC

    @property
    def ldb(self):
        return (self.K if self.lb == KC else self.N) + PADC


# ============================================================================================== dispatch predicate (host code restated)
def _stagger_env():
    e = os.environ.get("UCFVIT_GEMM_STAGGER")
    return int(e) if e else -1


def _plan2(c):
    """plan2 of csrc/gemm2.hip: None (v1) or (big, splits)"""
    if c.f32 or c.K < 128 or c.M < 128 or c.N < 128:
        return None
    if (c.la == KC or c.lb == KC) and c.K % 8:
        return None
    t256, t128, kt = _cdiv(c.M, 256) * _cdiv(c.N, 256), _cdiv(c.M, 128) * _cdiv(c.N, 128), _cdiv(c.K, 64)
    plain = c.act == NONE and not (c.bias or c.res)
    if t256 >= 192:
        return True, 1
    s = 1
    if plain and t128 < 384:
        nb64 = _cdiv(_cdiv(c.M, 128), 8) * _cdiv(_cdiv(c.N, 128), 8)
        s = 8 // math.gcd(nb64, 8)
        if nb64 * s > 48:
            s = 1
        s = max(1, min(s, kt // 8))
    kps = _cdiv(kt, s) * 64
    return False, _cdiv(c.K, kps)


def _v2_ok(c):
    a_contig = c.K if c.la == KC else c.M
    b_contig = c.K if c.lb == KC else c.N
    return a_contig % 8 == 0 and b_contig % 8 == 0 and c.N % 8 == 0       # the leading dimensions of this file are multiples of 8


def _cs_capable(c):
    """colsum_rows_for(): the by-product exists on the ping-pong kernel's plain and multiply-by-aux epilogues only"""
    p = _plan2(c)
    return bool(p and p[0] and _v2_ok(c) and not c.span4g and c.la == KC and c.lb == KC and not c.out32 and not c.acc and not c.res
                and not c.has_aux_out and c.act in (NONE, MUL_AUX))


def _stagger(c, dyn):
    """ucfvit_gemm_stagger_try: the epilogue name it would run, or None"""
    ov = _stagger_env()
    if ov == 0 or c.acc or dyn or c.K % 64 or c.N % 8 or c.M * (c.N + PADC) * 2 > 2 ** 31 - 1:
        return None
    if c.act == NONE and not c.res:
        epi = "PLAIN"
    elif c.act == NONE:
        epi = "RESIDUAL"
    elif c.act == GELU_SD and not c.res:
        epi = "GELU_SAVE_DERIV"
    elif c.act == MUL_AUX and not c.res and not c.bias:
        epi = "MUL_AUX"
    else:
        return None
    cs = bool(c.cs) and _cs_capable(c)
    if cs and epi != "MUL_AUX":
        return None
    nk = c.K // 64
    E = 1
    if ov > 0:
        E = ov
    elif nk < 16 or (epi == "RESIDUAL" and nk < 32) or cs:
        return None
    if nk < 2 * E:
        E = 4 if nk >= 8 else (2 if nk >= 4 else (1 if nk >= 2 else 0))
    if E == 0 or (cs and E == 1):
        return None
    return epi + ("+CS" if cs else "")


def _branch(c, dyn=None):
    dyn = c.dyn if dyn is None else dyn
    p = _plan2(c)
    if p is None or not _v2_ok(c):
        epv = 4 if c.f32 else 8
        a_contig = c.K if c.la == KC else c.M
        b_contig = c.K if c.lb == KC else c.N
        ok = a_contig % epv == 0 and b_contig % epv == 0 and c.N % 4 == 0 and c.M * c.N >= 256
        return "v1-mfma" if ok else "v1-scalar"
    big, splits = p
    if not big:
        return "g2-128-splitk" if splits > 1 and c.ws else "g2-128"
    if c.span4g:
        return "g2-256"
    if c.la == KC and c.lb == KC and not c.out32 and not c.acc:
        st = _stagger(c, dyn)
        if st:
            return "stagger-" + st
        cs = "+CS" if c.cs and _cs_capable(c) else ""
        if c.act == NONE and not c.res:
            return "g3-PLAIN" + cs
        if c.act == NONE:
            return "g3-RESIDUAL"
        if not c.res:
            return "g3-" + {GELU: "GELU", GELU_GRAD: "GELU_GRAD", GELU_SD: "GELU_SAVE_DERIV", MUL_AUX: "MUL_AUX"}[c.act] + cs
    return "g3-GENERIC"


def _chain(c, branch):
    """d: the longest fp32 addition chain behind one output element (see the docstring)"""
    if branch == "v1-scalar":
        return c.K
    if c.f32:
        return _cdiv(c.K, 4) + 4
    d = _cdiv(c.K, 32) + 32
    if branch == "g2-128-splitk":
        d += max(c.emu_splits, (_plan2(c) or (0, 1))[1])
    return d


# ============================================================================================== the table
def _dims():
    try:
        import bench
        W = bench.WORKLOADS
        vl, vb, mae = W["vit_l16_224"], W["vit_b16_224"], W["mae_vit_l16_224"]
        tok = (vl["img"] // vl["patch"]) ** 2 + 1
        return vl["dim"], vb["dim"], mae["dec_dim"], tok, vl["batch"]
    except Exception:
        return 1024, 768, 512, 197, 665


DL, DB, DMAE, TOK, BATCH = _dims()
M166 = 166 * TOK                   # 32702 token rows of ViT-L at per-GPU batch 166
KW = BATCH * TOK                   # 131005: the contraction length of the weight gradients at batch 665 (K % 64 = 61)
LAYOUTS = [(KC, KC), (KC, KS), (KS, KS), (KS, KC)]

CASES = []


def _add(*a, **k):
    CASES.append(Case(*a, **k))


# v1
for _la, _lb in LAYOUTS:
    _add("v1-mfma", 260, 264, 200, la=_la, lb=_lb, f32=True, bias=True, res=True, alpha=0.5)
    _add("v1-mfma", 128, 136, 1024, la=_la, lb=_lb, f32=True, acc=True)
_add("v1-mfma", 100, 264, 256, bias=True, res=True)                                  # bf16, M < 128
_add("v1-mfma", 700, 64, 136, la=KC, lb=KS, act=MUL_AUX)                             # N < 128
_add("v1-mfma", 304, 384, 64, la=KS, lb=KS, out32=True, acc=True, alpha=2.0)         # K < 128
_add("v1-mfma", 100, 264, 192, act=GELU, bias=True, aux_out=True)
_add("v1-scalar", 5, 2, 64, bias=True)
_add("v1-scalar", 33, 42, 24, f32=True, res=True)                                    # N % 4 != 0
_add("v1-scalar", 130, 6, 200, bias=True, res=True, alpha=-1.0)
_add("v1-scalar", 33, 40, 20, bias=True)                                             # bf16, K % 8 != 0
# gemm2_kernel 128x128
for _la, _lb in LAYOUTS:
    _add("g2-128", 696, 384, 136, la=_la, lb=_lb, bias=True, res=True)
    _add("g2-128", 696, 384, 136, la=_la, lb=_lb, out32=True, bias=True, acc=True, alpha=0.5)
_add("g2-128", 1000, 520, 200, act=GELU, bias=True, aux_out=True)
_add("g2-128", 1000, 520, 200, act=GELU, bias=True, res=True)
_add("g2-128", 1000, 520, 200, act=GELU_SD, bias=True)
_add("g2-128", 1000, 520, 200, la=KC, lb=KS, act=GELU_GRAD)
_add("g2-128", 1000, 520, 200, la=KC, lb=KS, act=MUL_AUX, alpha=2.0)
_add("g2-128", 1000, 520, 200, acc=True, res=True)                                   # accumulate with a bf16 output
_add("g2-128", 129, 128, 128)
_add("g2-128-splitk", DL, DL, KW, la=KS, lb=KS, out32=True, fams=("randn", "pos"))            # dW_proj at batch 665: ragged last K tile
_add("g2-128-splitk", DL, 4 * DL, 4096, la=KS, lb=KS, out32=True, acc=True, alpha=0.5)
_add("g2-128-splitk", DMAE, DMAE, 1024 + 136, la=KS, lb=KS)                                       # bf16 output through splitk_reduce_kernel
_add("g2-128-splitk", DB, DB, 4096, alpha=-1.0, acc=True, out32=True)
_add("g2-128", DL, DL, 4096, la=KS, lb=KS, out32=True, ws=False)                                  # split-K plan, workspace withheld
_add("g2-128", DB, DB, 4096 + 8, out32=True, acc=True, ws=False)
# gemm2_kernel 256x256: only for an operand of 4 GiB or more
_add("g2-256", 49152, 256, 256, span4g=True, bias=True, res=True, fams=("randn",))
# gemm3_kernel (ping-pong): K below the staggered kernel's threshold or K % 64 != 0
_G3 = [(12608, 1024, 256), (3073, 4104, 136), (49150, 264, 200)]
for _M, _N, _K in _G3:
    _add("g3-PLAIN", _M, _N, _K, bias=True)
    _add("g3-PLAIN+CS", _M, _N, _K, cs="ow")
    _add("g3-RESIDUAL", _M, _N, _K, bias=True, res=True)
    _add("g3-GELU_SAVE_DERIV", _M, _N, _K, act=GELU_SD, bias=True)
    _add("g3-MUL_AUX+CS", _M, _N, _K, act=MUL_AUX, cs="acc")
_add("g3-PLAIN", 12608, 1024, 256, alpha=2.0, bias=True)
_add("g3-RESIDUAL", 12608, 1024, 256, alpha=0.5, bias=True, res=True)
_add("g3-GELU", 12608, 1024, 256, act=GELU, bias=True, aux_out=True)
_add("g3-GELU", 3073, 4104, 136, act=GELU, bias=True)                               # ACT_GELU without aux_out
_add("g3-GELU_GRAD", 12608, 1024, 256, act=GELU_GRAD)
_add("g3-GELU_GRAD", 3073, 4104, 136, act=GELU_GRAD, alpha=-1.0)
_add("g3-MUL_AUX", 12608, 1024, 256, act=MUL_AUX, alpha=0.5)
_add("g3-PLAIN+CS", 512, 24576, 1536, cs="ow", gen="big", dyn=True)                 # |C| > 256 in most elements; dyn keeps it off the staggered kernel
_add("g3-MUL_AUX+CS", 768, 16384, 256, act=MUL_AUX, cs="ow")
_add("g3-GENERIC", 12608, 1024, 256, la=KC, lb=KS, bias=True, res=True)
_add("g3-GENERIC", 12600, 1024, 200, la=KS, lb=KC, bias=True)
_add("g3-GENERIC", 12600, 1032, 200, la=KS, lb=KS, out32=True, acc=True)
_add("g3-GENERIC", 12608, 1024, 1024, out32=True, bias=True)                        # fp32 output pushes (KC, KC) off the specialised epilogues
_add("g3-GENERIC", 12608, 1024, 1024, acc=True, bias=True, res=True, alpha=2.0)     # accumulate with a bf16 output
_add("g3-GENERIC", 12608, 1024, 256, act=GELU, bias=True, res=True, aux_out=True)   # act + residual
_add("g3-GENERIC", 3073, 4104, 136, act=GELU_SD, bias=True, res=True)
_add("g3-GENERIC", 12608, 1024, 256, la=KC, lb=KS, act=MUL_AUX)
# staggered kernel at its default thresholds (the ViT-L shapes of the training step at per-GPU batch 166, and a 200-tile shape)
_add("stagger-PLAIN", 12608, 1024, 1024, bias=True)
_add("stagger-PLAIN", 12545, 1000, 1024, bias=True, alpha=0.5)                      # ragged last N tile (232 columns), M one above a multiple
_add("stagger-RESIDUAL", 12608, 1024, 2048, bias=True, res=True)
_add("stagger-GELU_SAVE_DERIV", 12608, 1024, 1024, act=GELU_SD, bias=True)
_add("stagger-MUL_AUX", 12608, 1000, 1024, act=MUL_AUX, alpha=2.0)
_add("stagger-PLAIN", M166, 3 * DL, DL, bias=True, fams=("randn",))                 # ViT-L qkv forward
_add("stagger-RESIDUAL", M166, DL, 4 * DL, bias=True, res=True, fams=("randn",))    # fc2 forward
_add("stagger-GELU_SAVE_DERIV", M166, 4 * DL, DL, act=GELU_SD, bias=True, fams=("randn",))   # fc1 forward
_add("g3-MUL_AUX+CS", M166, 4 * DL, DL, act=MUL_AUX, cs="ow", fams=("randn",))      # fc1 data gradient with the bias-gradient by-product


# cases that the forced staggered runs (UCFVIT_GEMM_STAGGER = 1 / 2 / 4 / 8) re-run: everything that kernel can take
def _stagger_able(c):
    return (not c.f32 and not c.out32 and c.la == KC and c.lb == KC and not c.acc and not c.dyn and not c.span4g and c.K % 64 == 0
            and _plan2(c) is not None and _plan2(c)[0] and c.M <= 13000)


def _forced_stagger_takes(c):
    """of the cases above: the ones every forced setting UCFVIT_GEMM_STAGGER = 1 / 2 / 4 / 8 puts on the staggered kernel"""
    return (c.act == NONE or (c.act == GELU_SD and not c.res) or (c.act == MUL_AUX and not c.res and not c.bias)) and not c.cs


# ============================================================================================== operands
def _values(g, kind, shape, scale, dtype, is_a=False):
    if kind == "int":
        v = torch.randint(-4, 5, shape, generator=g, device=g.device).double()
    elif kind == "big":
        if True:
            v = torch.tensor([-4.0, -3.0, 3.0, 4.0], dtype=torch.float64, device=g.device)[torch.randint(0, 4, shape, generator=g, device=g.device)]
    else:
        v = torch.randn(shape, generator=g, device=g.device, dtype=torch.float32).double() * scale
        if kind == "offset" and is_a:
            v = v + 8.0 * scale
        if kind == "pos":
            v = v.abs()
        if kind == "exp":
            v = v * torch.exp2(torch.randint(-20, 21, shape, generator=g, device=g.device).double())
    return v.to(dtype)


def _padded(vals, fill, pad_c=PADC, pad_r=PADR, ld=None):
    """vals as a view into a larger buffer filled with `fill`"""
    r, cols = vals.shape
    ld = ld or cols + pad_c
    buf = torch.full((r + pad_r, ld), fill, dtype=vals.dtype, device=vals.device)
    buf[:r, :cols] = vals
    return buf, buf[:r, :cols]


class Operands:
    pass


def _make(c, kind, seed, dev=None):
    dev = dev or DEV
    g = torch.Generator(device=dev).manual_seed(seed)
    dt = F32 if c.f32 else BF
    odt = F32 if (c.f32 or c.out32) else BF
    nan = float("nan")
    o = Operands()
    ekind = kind if kind in ("int", "big") else "randn"
    a_shape = (c.M, c.K) if c.la == KC else (c.K, c.M)
    b_shape = (c.N, c.K) if c.lb == KC else (c.K, c.N)
    if c.span4g:
        buf = torch.empty((c.M, c.lda), dtype=dt, device=dev)            # uninitialised: only the view is filled
        buf[:, :c.K] = _values(g, kind, a_shape, 1.0, dt, True)
        buf[:, c.K:c.K + PADC] = nan
        o.A = buf[:, :c.K]
    else:
        _, o.A = _padded(_values(g, kind, a_shape, 1.0, dt, True), nan)
    _, o.B = _padded(_values(g, kind, b_shape, 1.0 if kind in ("int", "big") else 0.05, dt), nan)
    o.A64 = o.A.double() if c.la == KC else o.A.double().T
    o.B64 = o.B.double().T if c.lb == KC else o.B.double()
    o.bias = o.res = o.aux = o.aux_buf = o.cold = None
    if c.bias:
        bb = torch.full((c.N + 2 * PADC,), nan, dtype=dt, device=dev)
        bb[PADC:PADC + c.N] = _values(g, "int" if ekind == "big" else ekind, (c.N,), 1.0, dt)
        o.bias = bb[PADC:PADC + c.N]
    if c.res:
        _, o.res = _padded(_values(g, "int" if ekind == "big" else ekind, (c.M, c.N), 1.0, dt), nan)
    if c.aux_in:
        _, o.aux = _padded(_values(g, ekind, (c.M, c.N), 1.0, dt), nan)
    if c.has_aux_out:
        o.aux_buf, o.aux = _padded(torch.full((c.M, c.N), SENT, dtype=dt, device=dev), SENT)
    cold = _values(g, ekind, (c.M, c.N), 1.0, odt) if c.acc else torch.full((c.M, c.N), SENT, dtype=odt, device=dev)
    o.C_buf, o.C = _padded(cold, SENT)
    if c.acc:
        o.cold = cold.double()
    o.cs_buf = o.cs = o.cs_old = None
    if c.cs:
        o.cs_buf = torch.full((c.N + 2 * PADC,), SENT, dtype=F32, device=dev)
        o.cs = o.cs_buf[PADC:PADC + c.N]
        if c.cs == "acc":
            o.cs.copy_(_values(g, ekind, (c.N,), 1.0, F32))
            o.cs_old = o.cs.double().clone()
    return o


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _snapshot(o):
    return {k: getattr(o, k).clone() for k in ("C_buf", "aux_buf", "cs_buf") if getattr(o, k) is not None}


def _assert_padding_untouched(c, o, snap, what):
    for k, b in snap.items():
        now = _bits(getattr(o, k)).clone()
        was = _bits(b).clone()
        if k == "cs_buf":
            now[PADC:PADC + c.N] = 0
            was[PADC:PADC + c.N] = 0
        else:
            now[:c.M, :c.N] = 0
            was[:c.M, :c.N] = 0
        assert torch.equal(now, was), f"{what}: {k} was written outside its [:M, :N] region"


def _launch(c, o):
    ops = _ops()
    return ops.gemm(o.A, o.B, c.M, c.N, c.K, c.la, c.lb, out=o.C, bias=o.bias, residual=o.res, act=c.act,
                    aux_in=o.aux if c.aux_in else None, aux_out=o.aux if c.has_aux_out else None, accumulate=c.acc, alpha=c.alpha,
                    c_colsum=o.cs, c_colsum_accumulate=c.cs == "acc", split_k_workspace=c.ws)


def _desc(c, o=None):
    """the descriptor ops.gemm builds for the case, workspace / c_colsum_partial / sched_state left NULL: from the operands o, or without a
    GPU (o None) from fake addresses with the alignment and the leading dimensions _make gives them (never dereferenced: the queries below
    are host code)"""
    from UCF_VIT._hip import lib as L
    d = L.GemmDesc()
    aux_used = c.aux_in or c.has_aux_out
    if o is not None:
        p = lambda t: None if t is None else t.data_ptr()
        d.A, d.B, d.C, d.bias, d.residual = o.A.data_ptr(), o.B.data_ptr(), o.C.data_ptr(), p(o.bias), p(o.res)
        aux = p(o.aux) if aux_used else None
        d.lda, d.ldb, d.ldc = o.A.stride(0), o.B.stride(0), o.C.stride(0)
        d.ldr = o.res.stride(0) if o.res is not None else 0
        d.ldaux = o.aux.stride(0) if o.aux is not None else 0
    else:
        es = 4 if c.f32 else 2
        d.A, d.B, d.C = 1 << 30, 2 << 30, 3 << 30
        d.bias = (4 << 30) + PADC * es if c.bias else None           # _make: a view PADC elements into its buffer
        d.residual = 5 << 30 if c.res else None
        aux = 6 << 30 if aux_used else None
        d.lda, d.ldb, d.ldc = c.lda, c.ldb, c.N + PADC
        d.ldr = c.N + PADC if c.res else 0
        d.ldaux = c.N + PADC if aux_used else 0
    d.aux_in, d.aux_out = aux if c.aux_in else None, aux if c.has_aux_out else None
    d.M, d.N, d.K = c.M, c.N, c.K
    d.a_layout, d.b_layout = c.la, c.lb
    d.dtype = L.F32 if c.f32 else L.BF16
    d.out_dtype = L.F32 if (c.f32 or c.out32) else L.BF16
    d.act, d.accumulate, d.alpha = c.act, 1 if c.acc else 0, c.alpha
    d.workspace, d.workspace_bytes, d.c_colsum_partial, d.sched_state = None, 0, None, None
    return d


def _lib_route(c, d, dyn):
    """ucfvit_gemm_route on d with the three fields the name depends on set as ops.gemm sets them for the case: the split-K workspace
    handed over where the case allows it and the epilogue is plain, c_colsum_partial where the column sums are asked for and the library
    has rows for them, sched_state under the dynamic schedule (fake addresses: the query is host code)"""
    import ctypes
    from UCF_VIT._hip import lib as L
    lib = L.load()
    rows, ws = lib.ucfvit_gemm_colsum_rows(ctypes.byref(d)), lib.ucfvit_gemm_workspace(ctypes.byref(d))
    if c.ws and ws > 0 and c.act == NONE and not c.bias and not c.res:
        d.workspace, d.workspace_bytes = 7 << 30, ws
    if c.cs and rows > 0:
        d.c_colsum_partial = (8 << 30) + PADC * 4
    if dyn:
        d.sched_state = 9 << 30
    buf = ctypes.create_string_buffer(64)
    n = lib.ucfvit_gemm_route(ctypes.byref(d), buf, 64)
    d.workspace, d.workspace_bytes, d.c_colsum_partial, d.sched_state = None, 0, None, None
    assert 0 < n < 64, f"{c.id}: ucfvit_gemm_route returned {n}"
    name = buf.value.decode()
    assert len(name) == n
    return name


def _witness(c, o):
    """the ABI's route queries on the very descriptor ops.gemm builds, against the restated dispatch"""
    import ctypes
    from UCF_VIT._hip import lib as L
    d = _desc(c, o)
    lib = L.load()
    rows = lib.ucfvit_gemm_colsum_rows(ctypes.byref(d))
    ws = lib.ucfvit_gemm_workspace(ctypes.byref(d))
    assert (rows > 0) == _cs_capable(c), f"{c.id}: ucfvit_gemm_colsum_rows = {rows}, the restated dispatch says {_cs_capable(c)}"
    if rows > 0:
        assert rows == 2 * _cdiv(c.M, 256)
    p2 = _plan2(c)
    want_ws = bool(p2 and p2[1] > 1)
    assert (ws > 0) == want_ws, f"{c.id}: ucfvit_gemm_workspace = {ws}, the restated plan2 says splits = {p2}"
    if ws > 0:
        assert ws == p2[1] * c.M * c.N * 4
    ops = _ops()
    got = _branch(c, dyn=bool(ops._dynamic_sched))
    if _stagger_env() < 0:
        assert got == c.branch, f"{c.id}: this case no longer covers branch {c.branch}: the dispatch now takes {got}"
    said = _lib_route(c, d, bool(ops._dynamic_sched))
    assert said == got, f"{c.id}: ucfvit_gemm_route says {said}, the restated dispatch {got}"
    return got


# ============================================================================================== float64 reference and bound
def _gelu64(h):
    cdf = 0.5 * (1.0 + torch.erf(h * 0.7071067811865476))
    pdf = 0.3989422804014327 * torch.exp(-0.5 * h * h)
    return h * cdf, cdf + h * pdf


def _acc_variant(o, acc, variant):
    K = o.A64.shape[1]
    if variant == "drop_k1":
        return acc - o.A64[:, K - 1:] @ o.B64[K - 1:]
    if variant == "drop_ktile":
        k0 = ((K - 1) // 64) * 64
        return acc - o.A64[:, k0:] @ o.B64[k0:]
    if variant == "pad_k":                       # one more element in the contraction (a finite stand-in for a padding element)
        return acc + o.A64[:, :1] @ o.B64[:1]
    return acc


def _ref(c, o, acc, absab, d, variant="ok", h_given=None):
    """(value, tol, t, aux_ref, aux_tol) in float64: the epilogue of include/ucfvit_hip.h in its order, with the error carried along"""
    acc = _acc_variant(o, acc, variant)
    v = acc if variant == "no_alpha" else c.alpha * acc
    t = abs(c.alpha) * d * U * absab + U * v.abs()
    if c.bias:
        b = o.bias.double()
        v = v + (b.roll(1) if variant == "bias_shift" else b)
        t = t + U * v.abs()
    if variant == "res_before_act":
        v = v + o.res.double()
    aux_ref = aux_tol = None
    aux = None
    if c.aux_in:
        aux = o.aux.double()
        if variant == "aux_shift":
            aux = aux.roll(1, 0)
    if c.act == GELU:
        if c.aux_out:
            aux_ref, aux_tol = v, t + UB * (v.abs() + t)
            v, _ = _gelu64(h_given if h_given is not None else v)
            t = GA * v.abs() + GB + (0.0 if h_given is not None else 1.13 * aux_tol)
        else:
            v, _ = _gelu64(v)
            t = 1.13 * t + GA * v.abs() + GB
    elif c.act == GELU_SD:
        v, dg = _gelu64(v)
        ta = 0.80 * t + GA * dg.abs() + GB
        aux_ref, aux_tol = dg, ta + UB * (dg.abs() + ta)
        t = 1.13 * t + GA * v.abs() + GB
    elif c.act == GELU_GRAD:
        _, dg = _gelu64(aux)
        t = t * dg.abs() + v.abs() * (GA * dg.abs() + GB)
        v = v * dg
        t = t + U * v.abs()
    elif c.act == MUL_AUX:
        v = v * aux
        t = t * aux.abs() + U * v.abs()
    if c.res and variant != "res_before_act":
        r = o.res.double()
        v = v + (r.roll(1, 0) if variant == "res_shift" else r)
        t = t + U * v.abs()
    if c.acc:
        v = v + o.cold * {"no_cold": 0.0, "cold_twice": 2.0}.get(variant, 1.0)
        t = t + U * v.abs()
    ou = U if (c.f32 or c.out32) else UB
    return v, t + ou * (v.abs() + t), t, aux_ref, aux_tol


def _variants(c):
    # K > 16384: d U = (K / 32 + 40) U exceeds 1 / K, so no family can show one k element; the 61-element last K tile shows in "pos"
    w = ["drop_k1", "pad_k"] if c.K <= 16384 else []
    if c.K > 64:
        w.append("drop_ktile")
    if c.bias:
        w.append("bias_shift")
    if c.res:
        w.append("res_shift")
        if c.act != NONE:
            w.append("res_before_act")
    if c.aux_in:
        w.append("aux_shift")
    if c.alpha != 1.0:
        w.append("no_alpha")
    if c.acc:
        w += ["no_cold", "cold_twice"]
    return w


def _cs_ref(c, o, v, t, variant="ok"):
    M = v.shape[0]
    odt = F32 if (c.f32 or c.out32) else BF
    if variant == "cs_rounded":
        s = v.to(odt).double().sum(0)
    elif variant == "cs_drop_block":
        s = v[:((M - 1) // 128) * 128].sum(0)
    else:
        s = v.sum(0)
    if o.cs_old is not None:
        s = s + o.cs_old
    tol = t.sum(0) + (128 + 2 * _cdiv(M, 256) + 2) * U * (v.abs().sum(0) + (o.cs_old.abs() if o.cs_old is not None else 0.0))
    return s, tol


RATIOS = {}


def _ratio(family, what, got, ref, tol):
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    r = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    RATIOS[family] = max(RATIOS.get(family, 0.0), r)
    print(f"RATIO {family} {what}: worst err/bound {r:.3f}")
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, worst err/bound {r:.3f}, "
                                 f"first at {torch.nonzero(bad)[0].tolist()}")
    return r


def _within(got, ref, tol):
    return bool(((got.double() - ref).abs() <= tol).all())


class Pool:
    """_check over the operand families of one case: every family within its bound, every wrong reference rejected by at least one"""

    def __init__(self, what):
        self.what, self.rejected = what, {}

    def check(self, family, out, got, ref, tol, wrongs):
        _ratio(family, f"{self.what} {out}", got, ref, tol)
        for name, w in wrongs.items():
            key = f"{out}:{name}"
            self.rejected[key] = self.rejected.get(key, False) or not _within(got, w, tol)

    def done(self):
        assert self.rejected, f"{self.what}: no wrong reference to reject"
        missed = [k for k, r in self.rejected.items() if not r]
        assert not missed, f"{self.what}: the bound does not reject the wrong references {missed}"


# ============================================================================================== Tier 2
def _tier2_case(c, launch=None, dev=None):
    launch = launch or _launch
    pool = Pool(c.id)
    for fi, fam in enumerate(c.fams):
        o = _make(c, fam, 1000 + 17 * fi + c.M + c.N + c.K, dev)
        branch = _witness(c, o) if launch is _launch else c.branch
        d = _chain(c, branch)
        snap = _snapshot(o)
        got = launch(c, o)
        if launch is _launch:
            _assert_padding_untouched(c, o, snap, c.id)
        assert bool(torch.isfinite(got.float()).all()), f"{c.id} [{fam}]: non-finite output from finite operands (NaN padding leaked?)"
        acc, absab = o.A64 @ o.B64, o.A64.abs() @ o.B64.abs()
        hg = o.aux.double() if (c.act == GELU and c.aux_out) else None
        v, tol, t, aux_ref, aux_tol = _ref(c, o, acc, absab, d, h_given=hg)
        fam_key = f"{branch.split('+')[0]}"
        wrongs = {}
        pre_kinds = ("drop_k1", "drop_ktile", "pad_k", "bias_shift", "no_alpha")
        for name in _variants(c):
            if hg is not None and name in pre_kinds:
                continue                                  # C is compared with gelu of the stored aux_out: these show in aux_out
            wrongs[name] = _ref(c, o, acc, absab, d, variant=name, h_given=hg)[0]
        if hg is not None:                                # gelu of the neighbouring row's pre-activation
            wrongs["h_shift"] = _ref(c, o, acc, absab, d, h_given=hg.roll(1, 0))[0]
        pool.check(fam_key, "C", got, v, tol, wrongs)
        del wrongs
        if c.has_aux_out:
            assert bool(torch.isfinite(o.aux.float()).all())
            wa = {n: _ref(c, o, acc, absab, d, variant=n)[3] for n in _variants(c) if n in pre_kinds}
            pool.check(fam_key, "aux_out", o.aux, aux_ref, aux_tol, wa)
            del wa
        if c.cs:
            # without ACT_GELU the unrounded reference is v itself (no h_given)
            s, stol = _cs_ref(c, o, v, t)
            wc = {"cs_drop_block": _cs_ref(c, o, v, t, "cs_drop_block")[0]}
            if c.M <= 4096:        # the deviation of a sum of M roundings grows as sqrt(M), the bound as M: beyond this Tier 1 ("big") rejects it
                wc["cs_rounded"] = _cs_ref(c, o, v, t, "cs_rounded")[0]
            pool.check(fam_key + " colsum", "colsum", o.cs, s, stol, wc)
        del o, acc, absab, v, tol, t, got
    pool.done()


# ============================================================================================== Tier 1
def _bands(M, N, tile=256):
    m1, n1 = ((M - 1) // tile) * tile, ((N - 1) // tile) * tile
    return {"first rows": (slice(0, min(tile, M)), slice(None)), "last rows": (slice(m1, M), slice(None)),
            "first cols": (slice(None), slice(0, min(tile, N))), "last cols": (slice(None), slice(n1, N))}


def _assert_differs_in_bands(right, wrong, bands, what):
    for name in bands:
        sl = _bands(*right.shape)[name]
        assert bool((right[sl] != wrong[sl]).any()), f"{what}: the wrong result equals the right one in the {name} band: it guards nothing there"


def _exact_condition(c, o, absab):
    s = abs(c.alpha) * absab
    if c.bias:
        s = s + o.bias.double().abs()
    if c.aux_in:
        s = s * o.aux.double().abs()
    if c.res:
        s = s + o.res.double().abs()
    if c.acc:
        s = s + o.cold.abs()
    return s


def _tier1_case(c, launch=None, dev=None):
    launch = launch or _launch
    assert c.act in (NONE, MUL_AUX)
    gen = c.gen or ("big" if not (c.f32 or c.out32) and (c.res or c.bias) else "int")
    o = _make(c, gen, 7 + c.M + 3 * c.N + 5 * c.K, dev)
    if launch is _launch:
        _witness(c, o)
    acc, absab = o.A64 @ o.B64, o.A64.abs() @ o.B64.abs()
    cond = _exact_condition(c, o, absab)
    assert float(cond.max()) < LIM, f"{c.id}: the exactness condition fails: {float(cond.max())} >= 2^24"
    odt = F32 if (c.f32 or c.out32) else BF
    snap = _snapshot(o)
    got = launch(c, o).clone()
    v = _ref(c, o, acc, absab, 1)[0]
    assert torch.equal(_bits(got), _bits(v.to(odt).contiguous())), (
        f"{c.id}: {int((got.double() != v.to(odt).double()).sum())} elements differ from the float64 result rounded once")
    if launch is not _launch:
        return
    _assert_padding_untouched(c, o, snap, c.id)
    if odt == BF:
        if c.res:          # rounded before the residual is added
            pre = (c.alpha * acc + (o.bias.double() if c.bias else 0.0)) * (o.aux.double() if c.aux_in else 1.0)
            twice = (pre.to(BF).double() + o.res.double() + (o.cold if c.acc else 0.0)).to(BF)
            _assert_differs_in_bands(v.to(BF), twice, ("last rows", "last cols"), c.id + " twice-rounded")
            assert not torch.equal(got, twice)
            rs = _ref(c, o, acc, absab, 1, variant="res_shift")[0].to(BF)
            _assert_differs_in_bands(v.to(BF), rs, ("first rows", "last rows"), c.id + " residual of the neighbouring row")
            assert not torch.equal(got, rs)
        if c.bias:
            bs = _ref(c, o, acc, absab, 1, variant="bias_shift")[0].to(BF)
            _assert_differs_in_bands(v.to(BF), bs, ("first cols", "last cols"), c.id + " bias of the neighbouring column")
            assert not torch.equal(got, bs)
    if c.cs:
        assert float(v.abs().sum(0).max() + (o.cs_old.abs().max() if o.cs_old is not None else 0.0)) < LIM, f"{c.id}: column sums leave 2^24"
        s = _cs_ref(c, o, v, torch.zeros_like(v))[0]
        assert torch.equal(o.cs, s.float()), f"{c.id}: column sums differ from the float64 sums of the unrounded values"
        if gen == "big":
            assert float((v.abs() > 256).double().mean()) > 0.5
            assert not torch.equal(_cs_ref(c, o, v, torch.zeros_like(v), "cs_rounded")[0].float(), o.cs), \
                f"{c.id}: the sums of the rounded outputs equal the exact ones: this case guards nothing"
    # a second call: bit for bit (for accumulate / cs accumulate from the same old values)
    if not c.acc and c.cs != "acc":
        first_cs = o.cs.clone() if c.cs else None
        o.C.fill_(SENT)
        again = launch(c, o)
        assert torch.equal(_bits(again), _bits(got)) and (first_cs is None or torch.equal(first_cs, o.cs))


def _cs_exact(c):
    """column sums stay below 2^24 by arithmetic: M * max |C| from the generators' ranges"""
    return c.M * (abs(c.alpha) * 16.0 * c.K * (4.0 if c.aux_in else 1.0) + (4.0 if c.bias else 0.0)) < LIM


def _t1_ok(c):
    return c.act in (NONE, MUL_AUX) and (not c.cs or _cs_exact(c))


T1_CASES = [c for c in CASES if _t1_ok(c)]
T2_CASES = CASES


@gpu
@pytest.mark.parametrize("c", T1_CASES, ids=lambda c: c.id)
def test_gemm_exact(c):
    ops = _ops()
    ops.set_dynamic_tile_schedule(c.dyn)
    try:
        _tier1_case(c)
    finally:
        ops.set_dynamic_tile_schedule(False)
        torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("c", T2_CASES, ids=lambda c: c.id)
def test_gemm_bounds(c):
    ops = _ops()
    ops.set_dynamic_tile_schedule(c.dyn)
    try:
        _tier2_case(c)
    finally:
        ops.set_dynamic_tile_schedule(False)
        torch.cuda.empty_cache()


# ============================================================================================== symmetries and selection
def _run_outputs(c, kind, seed):
    o = _make(c, kind, seed)
    _launch(c, o)
    return [t.clone() for t in (o.C_buf, o.aux_buf, o.cs_buf) if t is not None]


G3_SCHED_CASES = [c for c in CASES if c.branch.startswith("g3-") and not c.dyn and c.M < 20000]


@gpu
@pytest.mark.parametrize("c", G3_SCHED_CASES, ids=lambda c: c.id)
def test_gemm3_static_and_dynamic_schedule_bit_identical(c):
    """the ping-pong kernel hands out the same tiles in another order: C, aux_out and the column sums are the same bits"""
    ops = _ops()
    assert _branch(c, dyn=True) == c.branch
    assert _lib_route(c, _desc(c), True) == c.branch and _lib_route(c, _desc(c), False) == _branch(c, dyn=False)
    stat = _run_outputs(c, "randn", 5)
    try:
        assert ops.set_dynamic_tile_schedule(True) is True
        dyn = _run_outputs(c, "randn", 5)
        dyn2 = _run_outputs(c, "randn", 5)
    finally:
        ops.set_dynamic_tile_schedule(False)
    for a, b, b2 in zip(stat, dyn, dyn2):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(b), _bits(b2))
    for st in ops._sched_states.values():
        assert int(st.abs().sum()) == 0           # the schedule state is zero again after every launch


SEL_CASES = [Case("v1-mfma", 260, 264, 200, la=a, lb=b, f32=True) for a, b in LAYOUTS] + \
            [Case("g2-128", 696, 384, 136, la=a, lb=b) for a, b in LAYOUTS] + \
            [Case("g3-GENERIC", 12600, 1032, 200, la=a, lb=b) for a, b in LAYOUTS[1:]] + \
            [Case("g3-PLAIN", 12600, 1032, 200), Case("stagger-PLAIN", 12608, 1000, 1024), Case("v1-mfma", 100, 264, 256),
             Case("g2-128-splitk", DMAE, DMAE, 1024 + 136, la=KS, lb=KS), Case("v1-scalar", 130, 6, 200)]


@gpu
@pytest.mark.parametrize("c", SEL_CASES, ids=lambda c: c.id)
def test_gemm_selection_copies_bits(c):
    """A with one 1 per row selects rows of B; B = identity blocks copies A: bit for bit, NaN padding never reaches the output"""
    dt = F32 if c.f32 else BF
    g = torch.Generator(device=DEV).manual_seed(c.M + c.K)
    # selection: C[m] = B[:, perm[m]] for the K x N operand
    o = _make(c, "randn", 3)
    sel = torch.randint(0, c.K, (c.M,), generator=g, device=DEV)
    sel[-1], sel[0] = c.K - 1, 0                                     # the last k element and the first
    A = torch.zeros(c.M, c.K, dtype=dt, device=DEV)
    A[torch.arange(c.M, device=DEV), sel] = 1.0
    (o.A if c.la == KC else o.A.T).copy_(A)
    _witness(c, o)
    got = _launch(c, o)
    B_kn = o.B.T if c.lb == KC else o.B
    assert torch.equal(_bits(got.contiguous()), _bits(B_kn[sel].to(got.dtype).contiguous()))
    # identity blocks: C[:, n] = A[:, n % K]
    o = _make(c, "randn", 4)
    eye = torch.zeros(c.K, c.N, dtype=dt, device=DEV)
    eye[torch.arange(c.N, device=DEV) % c.K, torch.arange(c.N, device=DEV)] = 1.0
    (o.B.T if c.lb == KC else o.B).copy_(eye)
    got = _launch(c, o)
    A_mk = o.A if c.la == KC else o.A.T
    assert torch.equal(_bits(got.contiguous()), _bits(A_mk[:, torch.arange(c.N, device=DEV) % c.K].to(got.dtype).contiguous()))


# ============================================================================================== grouped weight gradients
def _group_items(sizes, Mtok, seed, out_dtype, kind="int", accs=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    items, refs, tols = [], [], []
    for i, (n, k) in enumerate(sizes):
        _, dy = _padded(_values(g, kind, (Mtok, n), 1.0, BF, True), float("nan"))
        _, x = _padded(_values(g, kind, (Mtok, k), 1.0 if kind == "int" else 0.05, BF), float("nan"))
        acc = bool(accs and accs[i])
        old = _values(g, kind, (n, k), 1.0, out_dtype) if acc else torch.full((n, k), SENT, dtype=out_dtype, device=DEV)
        buf, out = _padded(old, SENT)
        items.append((dy, x, out, acc, buf, old.double() if acc else None))
    return items


def _group_check(items, Mtok, exact, family):
    for dy, x, out, acc, buf, old in items:
        ref = dy.double().T @ x.double()
        ab = dy.double().abs().T @ x.double().abs()
        if acc:
            ref = ref + old
        n, k = out.shape
        chk = _bits(buf).clone()
        chk[:n, :k] = 0
        ok = _bits(torch.full_like(buf, SENT)).clone()
        ok[:n, :k] = 0
        assert torch.equal(chk, ok), "grouped: output padding written"
        if exact:
            assert float((ab + (old.abs() if acc else 0.0)).max()) < LIM
            assert torch.equal(_bits(out.contiguous()), _bits(ref.to(out.dtype).contiguous()))
        else:
            t = (_cdiv(Mtok, 32) + 32 + 8) * U * ab + U * ref.abs()        # + 8: a split-K launch of the not-groupable fallback
            ou = U if out.dtype == F32 else UB
            tol = t + ou * (ref.abs() + t)
            _ratio(family, f"dW {n}x{k}", out, ref, tol)
            if Mtok <= 4096:       # beyond that d U exceeds 1 / K (see the docstring): the exact tier rejects it
                assert not _within(out, ref - dy.double()[-1:].T @ x.double()[-1:], tol), "grouped: the bound does not reject a dropped last token"


_GSIZES = [(384, 256), (1024, 520), (136, 128), (640, 1032), (256, 256), (392, 264), (512, 2048), (768, 136)]


@gpu
@pytest.mark.parametrize("n,out_dtype,dyn,Mtok", [(1, F32, False, 1024), (4, F32, False, 200), (5, BF, False, 1024), (32, F32, False, 197 * 3),
                                                   (5, F32, True, 200), (32, BF, True, 1024), (4, F32, False, KW)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_gemm_grouped(n, out_dtype, dyn, Mtok):
    """ucfvit_gemm_grouped over problems of unequal sizes with mixed accumulate flags: exact on integers, within bound on randn, bit-identical
    to each problem launched alone through the same kernel (a group of one), with the static and the dynamic schedule"""
    ops = _ops()
    sizes = [_GSIZES[(i * 3) % len(_GSIZES)] for i in range(n)] if Mtok != KW else [(DL, DL), (384, 256), (256, 1032), (136, 128)]
    accs = [i % 3 == 1 for i in range(n)]
    ops.set_dynamic_tile_schedule(dyn)
    try:
        for kind in ("int", "randn"):
            items = _group_items(sizes, Mtok, 11 + n, out_dtype, kind, accs)
            ops.wgrad_grouped([(dy, x, out, acc) for dy, x, out, acc, _, _ in items])
            _group_check(items, Mtok, kind == "int", "grouped" + ("" if out_dtype == F32 else " bf16"))
            # each problem alone in a group of one: the same kernel, the same bits
            alone = _group_items(sizes, Mtok, 11 + n, out_dtype, kind, accs)
            for (dy, x, out, acc, _, _), ref_item in zip(alone, items):
                ops.wgrad_grouped([(dy, x, out, acc)])
                assert torch.equal(_bits(out.contiguous()), _bits(ref_item[2].contiguous()))
            del items, alone
    finally:
        ops.set_dynamic_tile_schedule(False)
        torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("odd", ["narrow", "other_k"])
def test_gemm_grouped_not_groupable_falls_back(odd):
    """one problem with N < 128, or with another contraction length: the set runs as separate ucfvit_gemm launches — the same bits as
    ops.gemm on each problem with the split-K workspace withheld (the same dispatcher), and the same values within bound as the grouped kernel gives the groupable ones"""
    ops = _ops()
    Mtok = 1024
    sizes = [(384, 256), (256, 64 if odd == "narrow" else 256), (640, 1032)]
    for kind in ("int", "randn"):
        items = _group_items(sizes, Mtok, 5, F32, kind, [False, True, False])
        if odd == "other_k":
            dy, x, out, acc, buf, old = items[1]
            items[1] = (dy[:-8], x[:-8], out, acc, buf, old)
        ops.wgrad_grouped([(dy, x, out, acc) for dy, x, out, acc, _, _ in items])
        sep = _group_items(sizes, Mtok, 5, F32, kind, [False, True, False])
        if odd == "other_k":
            dy, x, out, acc, buf, old = sep[1]
            sep[1] = (dy[:-8], x[:-8], out, acc, buf, old)
        for (dy, x, out, acc, _, _), it in zip(sep, items):
            # the fallback hands no split-K workspace over: the same launch as ops.gemm without one, on the branch the library names
            c = Case("", dy.shape[1], x.shape[1], dy.shape[0], la=KS, lb=KS, out32=True, acc=acc, ws=False)
            o = Operands()
            o.A, o.B, o.C, o.bias, o.res, o.aux = dy, x, out, None, None, None
            assert _lib_route(c, _desc(c, o), False) == _branch(c, dyn=False)
            assert _branch(c, dyn=False) == ("v1-mfma" if odd == "narrow" and x.shape[1] == 64 else "g2-128")
            ops.gemm(dy, x, dy.shape[1], x.shape[1], dy.shape[0], KS, KS, out=out, accumulate=acc, split_k_workspace=False)
            assert torch.equal(out, it[2])
        for it in items:
            _group_check([it], it[0].shape[0], kind == "int", "grouped fallback")


# ============================================================================================== edges
@gpu
def test_gemm_empty_problems():
    ops = _ops()
    from UCF_VIT._hip.lib import HipLibraryError
    for dt in (BF, F32):
        out = torch.full((8, 16), SENT, dtype=dt, device=DEV)
        keep = out.clone()
        a0, b = torch.empty(0, 64, dtype=dt, device=DEV), torch.ones(16, 64, dtype=dt, device=DEV)
        ops.gemm(a0, b, 0, 16, 64, KC, KC, out=out[:0])                                  # M = 0
        ops.gemm(torch.ones(8, 64, dtype=dt, device=DEV), torch.empty(0, 64, dtype=dt, device=DEV), 8, 0, 64, KC, KC, out=out[:, :0])   # N = 0
        assert torch.equal(out, keep)
        # K = 0 with empty tensors (NULL data pointers): refused loudly, C untouched
        with pytest.raises(HipLibraryError, match="null operand pointer"):
            ops.gemm(torch.empty(8, 0, dtype=dt, device=DEV), torch.empty(16, 0, dtype=dt, device=DEV), 8, 16, 0, KC, KC, out=out)
        assert torch.equal(out, keep)


INF_CASES = [Case("v1-mfma", 260, 264, 200, f32=True), Case("g2-128", 696, 384, 136), Case("g3-PLAIN", 12608, 1024, 256),
             Case("stagger-PLAIN", 12608, 1024, 1024), Case("g2-128-splitk", DMAE, DMAE, 1024 + 136, la=KS, lb=KS),
             Case("g3-GENERIC", 12600, 1032, 200, la=KS, lb=KS, out32=True)]


@gpu
@pytest.mark.parametrize("c", INF_CASES, ids=lambda c: c.id)
def test_gemm_non_finite_operands_stay_in_their_row(c):
    o = _make(c, "randn", 9)
    _witness(c, o)
    row = c.M - 3
    (o.A if c.la == KC else o.A.T)[row, c.K - 1] = float("inf")
    got = _launch(c, o)
    fin = torch.isfinite(got.float())
    assert not bool(fin[row].any()), "the Inf of A's row did not reach every element of that row of C (B has no zeros)"
    fin[row] = True
    assert bool(fin.all()), "a non-finite value of one row of A reached another row of C"


# ============================================================================================== subprocess runs
def _child(args, env, timeout):
    r = subprocess.run([sys.executable] + args, env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
    return r


STAGGER_CASES = [c for c in CASES if _stagger_able(c)]


@gpu
@pytest.mark.parametrize("c", STAGGER_CASES, ids=lambda c: c.id)
def test_gemm_stagger_family(c):
    """the cases the staggered kernel can take, both tiers; under UCFVIT_GEMM_STAGGER = E (test_gemm_stagger_forced) every one of them runs that
    kernel with E epilogue steps, at the default only those the table names stagger-*"""
    c = replace(c, fams=("randn", "offset"))
    if _stagger_env() > 0:
        able = _forced_stagger_takes(c)
        c = replace(c, branch=_branch(c))
        assert not able or c.branch.startswith("stagger-"), f"{c.id}: the forced staggered run takes {c.branch}"
    if _t1_ok(c):
        _tier1_case(c)
    _tier2_case(c)
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("steps", ["1", "2", "4", "8"])
def test_gemm_stagger_forced(steps):
    _child(["-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "test_gemm_stagger_family"],
           {"UCFVIT_GEMM_STAGGER": steps}, 600)


_CUS_CASES = [Case("g3-PLAIN+CS", 12608, 1024, 256, cs="ow"), Case("g3-RESIDUAL", 3073, 4104, 136, bias=True, res=True),
              Case("g3-GELU_SAVE_DERIV", 12608, 1024, 256, act=GELU_SD, bias=True), Case("g3-MUL_AUX+CS", 12608, 1024, 256, act=MUL_AUX, cs="ow"),
              Case("g3-GENERIC", 12600, 1032, 200, la=KS, lb=KS, out32=True)]


def _cus_payload(path):
    """child process: ping-pong and grouped results (static, then dynamic schedule) saved for the parent to compare"""
    ops = _ops()
    out = {}
    for dyn in (False, True):
        ops.set_dynamic_tile_schedule(dyn)
        for i, c in enumerate(_CUS_CASES):
            for j, t in enumerate(_run_outputs(c, "randn", 21)):
                out[f"{i}.{j}.{int(dyn)}"] = _bits(t).cpu()
        items = _group_items([_GSIZES[(i * 3) % len(_GSIZES)] for i in range(5)], 200, 3, F32, "randn", [False, True, False, False, True])
        ops.wgrad_grouped([(dy, x, o, acc) for dy, x, o, acc, _, _ in items])
        for j, it in enumerate(items):
            out[f"g.{j}.{int(dyn)}"] = _bits(it[4]).cpu()
    torch.cuda.synchronize()
    torch.save(out, path)


@gpu
def test_gemm_cus_values_bit_identical(tmp_path):
    """UCFVIT_GEMM_CUS = 8 / 200 / 256 (another tile-to-workgroup map): every tile is computed by one workgroup in a fixed order, so the
    ping-pong and grouped results are the same bits, with either schedule; read once per process, hence the children"""
    res = {}
    for cus in ("256", "200", "8"):
        f = tmp_path / f"cus{cus}.pt"
        _child([os.path.abspath(__file__), "cus", str(f)], {"UCFVIT_GEMM_CUS": cus, "UCFVIT_GEMM_STAGGER": "0"}, 300)
        res[cus] = torch.load(f, weights_only=True)
    ref = res["256"]
    assert len(ref) > 20
    for cus, o in res.items():
        for k, v in ref.items():
            assert torch.equal(o[k], v), (cus, k)
            if k.endswith(".1"):
                assert torch.equal(v, ref[k[:-1] + "0"]), ("static vs dynamic", k)


@gpu
def test_gemm_ratios_report():
    """last test of the file: the worst err / bound per kernel family and output seen by this process"""
    for k in sorted(RATIOS):
        print(f"RATIO SUMMARY {k}: {RATIOS[k]:.3f}")
    assert all(r <= 1.0 for r in RATIOS.values())


# ============================================================================================== CPU case
def _emulate(a, b, mode, splits=1):
    """fp32 accumulation of a [M,K] . b [K,N], every addition done in float64 and rounded to fp32 (products of bf16 values are exact)"""
    M, K = a.shape
    N = b.shape[1]
    a, b = a.double(), b.double()

    def chain(ks, acc=None):
        acc = torch.zeros(M, N, dtype=F32) if acc is None else acc
        for k in ks:
            acc = (acc.double() + a[:, k, None] * b[None, k, :]).float()
        return acc

    if mode == "seq":
        return chain(range(K))
    if mode == "blocks32":              # one MFMA: 32 products summed, then added to the accumulator
        acc = torch.zeros(M, N, dtype=F32)
        for k0 in range(0, K, 32):
            acc = (acc.double() + chain(range(k0, min(K, k0 + 32))).double()).float()
        return acc
    if mode == "rot":                   # the staggered kernel's rows 128-255: K tiles in rotated order
        nk = _cdiv(K, 64)
        order = [(i + nk // 2) % nk for i in range(nk)]
        return chain([k for t in order for k in range(64 * t, min(K, 64 * t + 64))])
    if mode == "splitk":
        kps = _cdiv(_cdiv(K, 64), splits) * 64
        parts = [chain(range(k0, min(K, k0 + kps))) for k0 in range(0, K, kps)]
        acc = torch.zeros(M, N, dtype=F32)
        for p in parts:
            acc = (acc.double() + p.double()).float()
        return acc
    raise ValueError(mode)


def _emu_launch(mode, splits):
    def launch(c, o):
        acc = _emulate(o.A64.float(), o.B64.float(), mode, splits).double()
        odt = F32 if (c.f32 or c.out32) else BF
        v = (torch.tensor(c.alpha, dtype=F32) * acc.float())
        f = lambda x: x.float()                    # every epilogue step rounded to fp32
        if c.bias:
            v = f(v.double() + o.bias.double())
        if c.act == MUL_AUX:
            v = f(v.double() * o.aux.double())
        if c.res:
            v = f(v.double() + o.res.double())
        if c.acc:
            v = f(v.double() + o.cold)
        out = v.to(odt)
        o.C.copy_(out)
        if c.cs:
            s = v.double().sum(0) + (o.cs_old if o.cs_old is not None else 0.0)
            o.cs.copy_(s.float())
        return o.C
    return launch


def test_gemm_bounds_vs_float64_emulation():
    """no GPU: fp32 accumulation emulated in float64-checked steps (sequential chain, chain of 32-wide blocks, the staggered kernel's
    rotated K order, split-K partials) over the Tier 2 families stays inside the Tier 2 bound of the SHORTEST chain the table uses
    (d = ceil(K/32) + 32) wherever the emulated order is a kernel's (blocks32, rot, splitk), and inside d = K for the sequential chain;
    every wrong reference falls outside; and the Tier 1 generators meet the 2^24 condition at every shape of the table, from their ranges"""
    small = [Case("g2-128", 24, 16, 200, bias=True, res=True), Case("g2-128", 17, 24, 1024, out32=True, acc=True, alpha=0.5),
             Case("g2-128", 24, 16, 136, act=MUL_AUX, alpha=2.0), Case("g2-128", 160, 16, 256, cs="ow", fams=("randn", "offset"))]
    for c in small:
        for mode, splits in (("seq", 1), ("blocks32", 1), ("rot", 1), ("splitk", 3)):
            cc = replace(c, branch="v1-scalar" if mode == "seq" else ("g2-128-splitk" if mode == "splitk" else "g2-128"))
            cc = replace(cc, emu_splits=splits if mode == "splitk" else 0)
            _tier2_case(cc, launch=_emu_launch(mode, splits), dev="cpu")
        if c.act in (NONE, MUL_AUX):
            _tier1_case(c, launch=_emu_launch("rot", 1), dev="cpu")
    # the 2^24 condition from the generators' ranges (entries in [-4, 4]; "big": |a| = 4, |b| <= 4), no allocation
    for c in CASES + SEL_CASES + _CUS_CASES:
        s = abs(c.alpha) * 16.0 * c.K + (4.0 if c.bias else 0.0)
        if c.aux_in:
            s *= 4.0
        s += (4.0 if c.res else 0.0) + (4.0 if c.acc else 0.0)
        assert s < LIM, f"{c.id}: |alpha| 16 K + ... = {s} >= 2^24"
        if c.cs and c in T1_CASES:
            assert _cs_exact(c)
    assert sum(1 for c in T1_CASES if c.cs) >= 2
    for Mtok in (200, 1024, 197 * 3, KW):
        assert 16.0 * Mtok + 4.0 < LIM
    # every branch of the table has a case, and the restated dispatch puts each case on the branch it names
    if _stagger_env() < 0:
        for c in CASES:
            assert _branch(c) == c.branch, f"{c.id}: the restated dispatch takes {_branch(c)}"
            assert _lib_route(c, _desc(c), c.dyn) == c.branch, f"{c.id}: ucfvit_gemm_route says {_lib_route(c, _desc(c), c.dyn)}"
    names = {c.branch for c in CASES}
    for b in ("v1-mfma", "v1-scalar", "g2-128", "g2-128-splitk", "g2-256", "g3-PLAIN", "g3-PLAIN+CS", "g3-RESIDUAL", "g3-GELU", "g3-GELU_GRAD",
              "g3-GELU_SAVE_DERIV", "g3-MUL_AUX", "g3-MUL_AUX+CS", "g3-GENERIC", "stagger-PLAIN", "stagger-RESIDUAL",
              "stagger-GELU_SAVE_DERIV", "stagger-MUL_AUX"):
        assert b in names, f"no case for branch {b}"


# ============================================================================================== the route query, without a GPU
def _route_table():
    """every entry of CASES (the 4 GiB view and the withheld workspace among them) with either tile schedule and with the split-K workspace
    handed over or withheld: the library's route on a descriptor of fake addresses is the restated one — under the UCFVIT_GEMM_STAGGER of
    this process; returns the names the static schedule gives"""
    names = []
    for c in CASES:
        for dyn in (False, True):
            for cc in (c, replace(c, ws=not c.ws)):
                said, want = _lib_route(cc, _desc(cc), dyn), _branch(cc, dyn=dyn)
                assert said == want, f"{cc.id} dyn={dyn}: ucfvit_gemm_route says {said}, the restated dispatch {want}"
        names.append(_lib_route(c, _desc(c), False))
    return names


def test_gemm_route_query_every_case():
    names = _route_table()
    if _stagger_env() < 0:
        assert names == [c.branch if not c.dyn else _branch(c, dyn=False) for c in CASES]
        c = next(c for c in CASES if c.dyn)
        assert c.branch == "g3-PLAIN+CS" and _lib_route(c, _desc(c), False) == "g3-PLAIN+CS" and _lib_route(replace(c, cs=""), _desc(c), False) == "stagger-PLAIN"
    # the text is cut to the room given, the length returned is the whole name's
    import ctypes
    from UCF_VIT._hip import lib as L
    c = next(c for c in CASES if c.branch == "g2-256")
    buf = ctypes.create_string_buffer(b"x" * 16, 16)
    assert L.load().ucfvit_gemm_route(ctypes.byref(_desc(c)), buf, 4) == len("g2-256") and buf.raw[:5] == b"g2-\0x"


@pytest.mark.parametrize("steps", ["0", "1", "2", "4", "8"])
def test_gemm_route_query_forced_stagger(steps):
    """UCFVIT_GEMM_STAGGER is read once per process: the table again in a child under every setting the hook documents"""
    r = _child([os.path.abspath(__file__), "routes"], {"UCFVIT_GEMM_STAGGER": steps}, 300)
    n_st = int(r.stdout.split("stagger:")[1].split()[0])
    n_forced = sum(1 for c in STAGGER_CASES if _forced_stagger_takes(c))
    assert n_forced > 0
    assert (n_st == 0) if steps == "0" else (n_st >= n_forced), r.stdout


def _routes_payload():
    names = _route_table()
    ov = _stagger_env()
    for c, name in zip(CASES, names):
        if ov == 0:
            assert not name.startswith("stagger-"), f"{c.id}: UCFVIT_GEMM_STAGGER=0, routed to {name}"
        elif ov > 0 and _stagger_able(c) and _forced_stagger_takes(c):
            assert name.startswith("stagger-"), f"{c.id}: forced to {ov} steps, routed to {name}"
    print("stagger:", sum(n.startswith("stagger-") for n in names), "of", len(names))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "cus":
        _cus_payload(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "routes":
        _routes_payload()
    else:
        sys.exit("usage: test_gemm_ops.py cus OUT.pt | routes")
