"""Every entry point of csrc/unetr_decoder.hip (the instance-norm / LeakyReLU / residual chain in both layouts, the Dice + cross-entropy loss)
against float64 references of the same rounded operands, element by element, through UCF_VIT._hip.ops (the fold-only case and the refusal
test call the library as ops does).  The references never call the project's kernels.  U = 2^-24 (fp32 unit roundoff), UB = 2^-8 (bf16).  All
operands are drawn on the CPU from seeds (the same values with and without a GPU); B = 2 throughout, so a stride or chunk error lands in the
other batch element.

Kernels and the cases that reach them (chunks_of, cl_chunks_of, apply_grid, cl_apply_grid and the rows > 512 rule are restated here;
test_tables_reach_every_branch asserts this list from them):
    in_stats_partial / in_stats_final,     test_row_family: fp32 and bf16, rows 2x3 and 2x5 (apply_grid caps 342 / 205), S = 4 | 8 (one short chunk),
      in_apply<T, RES 0 / 1>,              16376 (one ragged chunk), 16384, 16392 (a second chunk of one vector), 32776 (3 chunks); forward with
      in_bwd_partial, bwd_means<2>,        and without res, slope 0.01 and 1; backward with dres (a residual was added) and without
      in_bwd_apply<T, RES 0 / 1>
    incl_stats_partial, incl_stats_fold    test_cl_family[stats]: C = 8, 32, 64, 128, 256 (cv = C / 8 = 1 .. 32: the threadIdx.x % cv ownership and the
                                           t += cv LDS folds) x S cv = CLV - cv, CLV, CLV + cv, 2 CLV + 3 cv (1, 1, 2, 3 chunks), and S cv < 256
    incl_apply<RES 0 / 1>, incl_apply2     test_cl_family[apply]: the same shapes
    incl_bwd_partial<NEED_Y 0 / 1>,        test_cl_family[bwd]: the same shapes; dy dense (ld = C) and a channel slice (ld = 2 C at offset C, ld = C + 8 at
      cl_fold, bwd_means<2>,               offset 8, ld 48 at 16), each with one and with several chunks; the three instantiations: mask from y with dres,
      incl_bwd_apply<1,1> <1,0> <0,0>      mask from y without, mask recomputed from x; the buffer behind a sliced dy is compared bit for bit afterwards
    incl_bwd2_partial, bwd_means<3>,       test_cl_family[bwd2]: the same shapes and slices
      incl_bwd2_apply
    (bwd_means<K> is one kernel for both layouts, the row layout being C = 1; cl_fold is cl_stage + cl_channel_sums, which incl_stats_partial
    calls directly; the double wave butterfly of every final kernel is wave_sum(double) of common.h, the triples' is mom_wave_fold)
    C = 512, 2048 (cv = 64, 256 = NT)      test_cl_wide_channels: all four parts at S = 6 and 3.  The library computes them, so correct values are required
                                           (any library error, a refusal included, fails); the fold is single-stage there (C > NT)
    incl_stats_fold1 + incl_stats_fold     test_cl_stats_fold_stages: C = 256 through ops.instnorm_cl_stats at S = 65536 (512 partial rows: one stage) and
                                           65537 (513 rows: two stages, G = 3 groups of 171); test_cl_stats_fold_group_cap: 65836 partial rows at C = 8
                                           handed to ucfvit_instnorm_cl_stats_fold as the convolution epilogue does (G = 256, the cap; 258 rows a group,
                                           the last group short; rows with count 0 among them)
    dice_partial<T>, dice_final,           test_dice: S = 1, 255, 16384, 16385, 49159 (1, 1, 1, 2, 4 chunks) x n = 2, 3, 4, 5, 8, every n and every S with
      dice_bwd<T>                          fp32 and bf16 logits and, over the table, contiguous [B, n, S], channels-last views with ld = n and with
                                           ld = 8 > n (NaN in the padding columns of the logits); ucfvit_dice_ce with and without the gradient, default
                                           and other smoothing terms, grad_scale 1, 1.75, 1/4; ucfvit_dice_ce_stats -> ucfvit_dice_ce_from_stats with the
                                           sums of a second slab added, S_total = the next power of two above S
Nothing is near 512 x 512 x 128, and the grid caps of the apply kernels are out of reach of small shapes: tests/test_decoder_full_volume.py
keeps that role.

Tier 1, exact.  Every condition below is computed in float64 from the operands used and asserted (_assert_exact_sum: the terms are multiples
of a power of two and the sum of their magnitudes stays below 2^24 of it, so every partial sum in any order is an fp32 number; _assert_fits:
every intermediate of the expression is an fp32 number); the conditions run without a GPU too (the *_on_the_host tests), where an fp32
emulation must reproduce the float64 result exactly.
    _apply, _apply2, _bwd_apply, _bwd2, the row backward: integer means, power-of-two rstd (different for the channels c, c + 1 and c + 8),
        slope 1/2, small-integer x / res / dy (x = mean + {0, +-1, +-2} in the backward passes, so that n is a power of two), m1 / m2 dyadic:
        bf16 outputs bit-equal to the float64 result rounded ONCE.  The passes that form their own means (_bwd2, the row backward) are exact at
        the power-of-two S of each table (the means are then dyadic) and held to the Tier 2 bound at the others; dres is exact everywhere.
    _bwd_sums: the sums are exact, so m1 / m2 must equal (float)(s / (double) S) bit for bit at every S.
    statistics: integer rows within 3 of an integer centre, the first element of every chunk (the shift) at the centre, chunk populations
        powers of two (the case is left to Tier 2 otherwise): count, mean and the fold are exact, mean must equal the fp32 of the float64 mean;
        M2_c = s2 - s1 (s1 / n) rounds where it is no fp32 number, which is bounded from the operands (<= 1.25 U of the variance, asserted), so
        rstd must be the fp32 of the float64 value or its neighbour.  Two-stage fold: every chunk a rearrangement of one balanced set.
    Dice: logits 0 (the predicted class) and -200 (exp below 2^-150: exactly 0 in fp32), 3 + b + class mispredicted voxels per (batch element,
        class): I, P, C are exact integers; the gradient is exactly 0 on correctly predicted voxels and +- grad_scale / (B S_total) on the
        others where B S_total is a power of two (every sharded case: this pins S_total), within the Tier 2 bound elsewhere.  The CE sum and
        the loss go through __logf: Tier 2.

Tier 2, per-element bounds on real-valued operands: randn; randn + 8; per-channel scales 2^-6 .. 2^6; for the kernels that form statistics
also the two edge cases of tests/test_unetr_decoder.py, one outlier of 300 sigma in front and |mean| / sigma >= 1000.  The outlier family's bound is
LOOSE by derivation: the chunk that takes the outlier as its shift sums (x - shift)^2 ~ 9e4 per element, and (3 D + 8) U of that is about a tenth of
the row's variance at these sizes: the median tolerance is about 11 % of rstd and about 11 |y| for the fused forward, so that family shows little more
than finite, NaN-free statistics here (tests/test_unetr_decoder.py holds it to 1e-3 at 2^20 voxels); the other four families hold tight.
    |got - ref| <= t + ou (|ref| + t),   ou = UB (bf16 output) or U (fp32),   t = d U (sum of the absolute values of the expression's terms),
d = the fp32 roundings on the output's path, read off the kernel:
    reductions: chain D = 64 + 6 + 4 = 74 for a row chunk (64 elements a thread, the wave butterfly, 4 wave sums), D = 16 + 256 / cv channels-last
        (16 vectors a thread, the NT / cv threads of a channel group folded in sequence); chunk sums are folded in double.
    statistics (ref_stats): per chunk dmean_c = (D + 2) U mean|x - shift| + U |mean_c|, dM2_c = (3 D + 8) U sum (x - shift)^2 (the product
        s1 (s1 / n) by Cauchy-Schwarz), combined with the parallel-variance formula; + U |mean| for the result; two stages add U of the group means
        and of M2.  rho = (1 - dvar / (var + eps))^-1/2 - 1 + 2 U bounds rstd relatively (infinite where a chunk's bound reaches the variance: Pool.check asserts that no case has such a tolerance).
    y = lrelu((x - m) r + res): d = 3 (4 with res, 6 for _apply2) on (|x| + |m|) r + |res|.  The fused row forward uses the kernel's own statistics:
        t = (t0 + r dmean) (1 + rho) + rho |n|; the kernel's mean / rstd are never read into the reference.
    m1, m2(, m3): ((D + 1) | (D + 4)) U mean|terms| + U |m|.   dx = r (dn - m1 - n m2): d = 7 on r (|dn| + |m1| + |n| |m2|), + r (dm1 + |n| dm2)
        where the pass formed the means itself.   dres: U |dn|.
    softmax: __expf and __logf are the native approximations (HIP Programming Guide, "HIP math API", single-precision intrinsics; lowered to
        v_exp_f32 and v_log_f32, which the CDNA ISA guide gives 1 ULP): 4 U each as in tests/test_attention_ops.py, plus the argument scaling:
        a probability carries (4 xm + 17) U relatively (xm: how far the lowest logit lies below the largest), log p carries 4 U (|log p| + 1).
        I, P, CE: those per voxel + (D + 2) U of the sum; the loss: the sums' bounds through 1 - (2 I + s) / (P + C + s) and the CE mean, + U: a margin
        relative to the float64 loss that comes from the fp32 chunk sums alone (64-element chains folded in double).
        The gradient: ref_dice carries the relative errors of a_c, bq_c (from the sums' bounds), g, the 8-term dot product and both terms.
Each d was validated before any GPU run: the *_on_the_host tests run the same drivers on an fp32 emulation (numpy / torch fp32, reductions once
in the kernels' per-thread order with the thread sums in sequence, once pairwise) and require err / bound <= 1 everywhere, the wide, fold-stage
and group-cap cases included.  The fold itself has no fp32 sum (double combination, fp32 storage of the group triples): its two orders are the kernel's
triple-by-triple mom_add and the closed form of the combined moments; its double arithmetic enters the bound as 10 rows 2^-53 of the magnitudes.

Wrong references.  Every comparison goes through Pool.check; per case and kernel, over the operand families (Tier 1 included), every applicable
wrong reference must differ from the right one by more than the bound (shown without a GPU as well) and be rejected; no case opts out:
the statistics of channel c + 1 and of c + 8 (the next 16-byte group; the neighbouring row in the row family), the volume shifted by one voxel,
the residual (or the second branch) dropped, the mask from n although a residual was added, the mask with the tie at y = 0 taken the other way
(y >= 0 for y > 0: what a y rounded the other way at 0 amounts to; Tier 1 has such voxels), dy read densely where it is a slice, the last
chunk left out of the means, m2 / m3 exchanged, the last partial row left out of the fold, labels one voxel over, class and voxel strides
exchanged, S_total = S, class n - 1 left out of the softmax.

Guards.  Operands are carved from the middle of NaN-filled, 16-byte-aligned allocations, results must be NaN-free; the padding columns of a padded
channels-last Dice gradient are zero bit for bit; a sliced dy's buffer and the caller's Dice sums are unchanged after the call; every call is made
twice and must repeat bit for bit.  test_refusals_write_nothing pins, with sentinel outputs that must stay untouched: S not a multiple of the vector
width (both types, forward and backward), C = 24, 12, 4 on all six channels-last entry points, ld_dy < C and ld_dy = 20, dres without a residual,
n = 1 and n = 9 on the three Dice entry points, S_total < S; then the same refusals as ops raises them.
The tie of the activation mask (y = 0, or n = 0 where the mask is recomputed from x) occurs in Tier 1 only, which rejects `>=` for `>` in every
instantiation; the real-valued families have no such voxel.
Not covered: the means kept in the workspace by ops.instnorm_cl_bwd (the two halves are tested apart), strides beyond 2^31.

Measured on an MI355X: 135 GPU tests + 67 CPU tests, 50 s for the file (the GPU tests 15 s); the two fold-stage cases take 2.0 s each (the float64
reference of 2 x 65537 x 256 values), every other GPU test stays below half a second.
Mutation check (nothing of it committed), one line each: the mask from n in incl_bwd_apply<RES> failed test_cl_family[*-bwd] on all 22 cases and
test_cl_wide_channels[*-bwd] on both; t starting at cg + cv in cl_fold (the loop is now cl_channel_sums) failed the same 24; S for S_total in dice_bwd failed all 25 test_dice cases.
  worst err / bound                               bf16 out   fp32 out
  in_apply y (own statistics)                     0.994      0.180
  in_bwd dx / dres                                0.995 / 0.928      0.134 / 0.492
  in_stats mean / rstd                            0.704 / 0.039      Tier 1: mean exact, rstd 1 ulp at most
  incl_stats mean / rstd                          0.491 / 0.247      one stage 0.183 / 0.013, two stages 0.222 / 0.016, group cap 0.246 / 0.066
  incl_apply<res> / <nores> / incl_apply2         0.996 / 0.996 / 0.996
  incl_bwd_partial<y> / <x>: m1, m2                                  0.137, 0.139 / 0.118, 0.154
  incl_bwd_apply<y,dres> / <y> / <x> dx           0.996 / 0.996 / 0.996      dres 0.928
  incl_bwd2 dx / dx2                              0.995 / 0.996
  dice_partial sums / CE, loss                                       0.109 / 0.028, 0.024 (0.028 sharded)
  dice_bwd gradient (dice_ce / from_stats)        0.996 / 0.995      0.570 / 0.341
bf16 outputs sit at the bound because the bound there IS the output rounding; the fp32 columns show the arithmetic itself.  Every Tier 1
comparison was exact.  No defect found: no ratio above 1, no NaN, no sentinel or padding column touched; C = 512 and 2048 are computed correctly
(test_cl_wide_channels requires it), so the entry check stays as it is.
"""
import math
from dataclasses import dataclass

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
UB = 2.0 ** -8
LIM = 2.0 ** 24
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
PAD = 64                                   # NaN elements in front of and behind every carved operand (128 / 256 bytes: 16-byte aligned)
SENT = -12352.0                            # sentinel of the refusal tests (exact in bf16 and fp32)
EPS = float(np.float32(1e-5))              # the kernels take eps, slope, the smoothing terms and grad_scale as C floats
SLOPE = float(np.float32(0.01))
RATIOS = {}

# ---- csrc/unetr_decoder.hip restated: workgroup size, chunk sizes, grids, the fold's stage rule -------------------------------------------
NT, CHUNK, CLV, MAXC = 256, 16384, 4096, 8
DSTAT = 3 * MAXC + 1                        # per batch element: I[8], P[8], C[8], the CE sum
D_ROW = CHUNK // NT + 6 + NT // 64         # longest fp32 addition chain of a row chunk: 64 per thread, wave butterfly, the 4 wave sums


def chunks_of(S):
    return -(-S // CHUNK)


def cl_chunks_of(S, C):
    return -(-(S * (C // 8)) // CLV)


def apply_grid(S, rows):
    return max(1, min((S // 4 + NT - 1) // NT, (2048 + rows - 1) // rows))


def cl_apply_grid(S, C, B):
    return max(1, min((S * (C // 8) + NT - 1) // NT, (4096 + B - 1) // B))


def fold_plan(rows, C):
    """ucfvit_instnorm_cl_stats_fold with a workspace -> (stages, G, rows per group)"""
    if rows > 512 and C & (C - 1) == 0 and C <= NT:
        G = min(256, -(-rows // 256))
        return 2, G, -(-rows // G)
    return 1, rows, 1


def d_cl(C):
    """longest fp32 addition chain of a channels-last chunk: CLV / NT vectors per thread, then the NT / cv threads of a channel group in LDS"""
    return CLV // NT + max(1, NT // (C // 8))


def _ops():
    from UCF_VIT._hip import ops
    return ops


def _lib():
    from UCF_VIT._hip import lib
    return lib


# ============================================================================================== cases
@dataclass(frozen=True)
class RowC:
    dt: str                  # "f32" | "bf16"
    Cc: int                  # channels: rows = 2 Cc
    S: int

    @property
    def id(self):
        return f"row-{self.dt}-2x{self.Cc}x{self.S}"

    @property
    def dtype(self):
        return F32 if self.dt == "f32" else BF


ROW_S = ("small", 16376, 16384, 16392, 2 * 16384 + 8)
ROWS = [RowC(dt, (3, 5)[(i + k) % 2], ({"f32": 4, "bf16": 8}[dt] if S == "small" else S)) for k, dt in enumerate(("f32", "bf16"))
        for i, S in enumerate(ROW_S)]


@dataclass(frozen=True)
class ClC:
    C: int
    S: int
    ld: int = 0              # row stride of dy (0: dense = C)
    off: int = 0             # first channel of the slice
    tag: str = ""

    @property
    def id(self):
        return f"cl-C{self.C}-S{self.S}-ld{self.ldy}" + (f"-{self.tag}" if self.tag else "")

    @property
    def ldy(self):
        return self.ld or self.C

    @property
    def cv(self):
        return self.C // 8


CLS = []
for _C in (8, 32, 64, 128, 256):
    _cv, _v = _C // 8, CLV // (_C // 8)
    CLS += [ClC(_C, _v - 1), ClC(_C, _v, 2 * _C, _C), ClC(_C, _v + 1), ClC(_C, 2 * _v + 3, _C + 8, 8)]
CLS += [ClC(32, 32, 48, 16, "onegroup"), ClC(8, 16, 0, 0, "onegroup")]            # S cv < 256: a single row group of threads
WIDE = [ClC(512, 6, 0, 0, "wide"), ClC(2048, 3, 2048 + 8, 8, "wide")]
FOLD = [ClC(256, 512 * CLV // 32, 0, 0, "512rows"), ClC(256, 512 * CLV // 32 + 1, 0, 0, "513rows")]
GCAP_ROWS = 65536 + 300                    # partial rows of the C = 8 fold-only case: G = 256 (the cap), 258 rows per group, the last group short


@dataclass(frozen=True)
class DiceC:
    n: int
    S: int
    lay: str                 # "nc": contiguous [B, n, S]; "cl": channels-last view, ld = n; "pad": channels-last view, ld = 8 > n
    dt: str

    @property
    def id(self):
        return f"dice-n{self.n}-S{self.S}-{self.lay}-{self.dt}"

    @property
    def dtype(self):
        return F32 if self.dt == "f32" else BF

    @property
    def ld(self):
        return 8 if self.lay == "pad" else self.n


DICE_S = (1, 255, 16384, 16385, 3 * 16384 + 7)
DICE_N = (2, 3, 4, 5, 8)
DICE = [DiceC(n, S, ("nc", "cl", "pad")[(i + j) % 3], ("f32", "bf16")[(i + j) % 2]) for i, S in enumerate(DICE_S) for j, n in enumerate(DICE_N)]


def _ids(cs):
    return [c.id for c in cs]


# ============================================================================================== small tools
def _seed(*parts):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate("|".join(str(p) for p in parts))) % (2 ** 31)


def _gen(*parts):
    return torch.Generator().manual_seed(_seed(*parts))


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _fits32(t):
    """every value of the float64 tensor is an fp32 number"""
    return bool((t.float().double() == t).all())


def _xyz(S):
    """S = X Y Z for the [B, X, Y, Z, C] maps ops takes"""
    for a in (2, 3, 5, 7):
        if S % a == 0:
            for b in (2, 3, 5, 7, 11, 13):
                if (S // a) % b == 0:
                    return a, b, S // a // b
            return a, 1, S // a
    return 1, 1, S


def _fsum(a, order, T=1):
    """fp32 sum over the last axis.  "seq": element i goes to thread i % T as in the kernels, a thread adds its elements in sequence and the T
    thread sums are added in sequence; "pair": pairwise over all elements.  (Zeros appended to fill the shape: exact.)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    n = a.shape[-1]
    if order == "seq":
        if n % T:
            a = np.concatenate([a, np.zeros(a.shape[:-1] + (T - n % T,), np.float32)], -1)
        a = np.cumsum(a.reshape(a.shape[:-1] + (-1, T)), axis=-2, dtype=np.float32)[..., -1, :]
        return np.cumsum(a, axis=-1, dtype=np.float32)[..., -1]
    p = 1 << max(0, (n - 1).bit_length())
    if p != n:
        a = np.concatenate([a, np.zeros(a.shape[:-1] + (p - n,), np.float32)], -1)
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def _csum(terms, L, order, T):
    """what the kernels do with a reduction: fp32 sums per chunk of L elements, the chunk sums added in double -> float64 [R]"""
    t = terms.numpy() if isinstance(terms, torch.Tensor) else terms
    tot = np.zeros(t.shape[0], np.float64)
    for lo in range(0, t.shape[1], L):
        tot += _fsum(t[:, lo:lo + L], order, T).astype(np.float64)
    return tot


def _rows(t):
    """[B, S, C] -> rows [B C, S]"""
    B, S, C = t.shape
    return t.permute(0, 2, 1).reshape(B * C, S)


def _unrows(r, B, C):
    """rows [B C, S] -> [B, S, C]"""
    return r.view(B, C, -1).permute(0, 2, 1).contiguous()


def _chan_roll(v, B, k):
    """per-row values [B C] taken from channel c + k of the same batch element"""
    return v.view(B, -1).roll(-k, 1).reshape(-1)


def _tol(ref, t, ou):
    return t + ou * (ref.abs() + t)


def _within(got, ref, tol):
    return bool(((got.double() - ref).abs() <= tol).all())


class Pool:
    """every comparison of one case goes through check(): the result must be within the bound of the right reference, and over the operand
    families of the case every applicable wrong reference must (a) differ from the right one by more than the bound and (b) be rejected"""

    def __init__(self, what, be):
        self.what, self.be, self.rej, self.differs = what, be, {}, {}

    def check(self, kernel, family, got, ref, tol, wrongs=None):
        got = got.double()
        assert got.shape == ref.shape, f"{self.what} {kernel}: shape {tuple(got.shape)} against {tuple(ref.shape)}"
        assert not bool(torch.isnan(got).any()), f"{self.what} {kernel} {family}: NaN in the result"
        tol = tol if isinstance(tol, torch.Tensor) else torch.full_like(ref, tol)
        err = (got - ref).abs()
        bad = ~(err <= tol)
        assert bool(torch.isfinite(tol).all()), f"{self.what} {kernel} {family}: the bound is vacuous (infinite) for {int((~torch.isfinite(tol)).sum())} elements"
        fin = torch.isfinite(tol)
        q = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))[fin]
        r = float(q.max()) if q.numel() else 0.0
        key = f"{kernel} [{self.be.name}]"
        RATIOS[key] = max(RATIOS.get(key, 0.0), r)
        print(f"RATIO {key} {self.what} {family}: worst err/bound {r:.3f}")
        assert not bool(bad.any()), (f"{self.what} {kernel} {family}: {int(bad.sum())} of {bad.numel()} elements out of bound, worst err/bound {r:.3g}, "
                                     f"first at {torch.nonzero(bad)[0].tolist()}")
        for name, w in (wrongs or {}).items():
            k = f"{kernel.split()[0]}:{name}"                     # per kernel (the first word of the label): any of its outputs and families may tell
            self.differs[k] = self.differs.get(k, False) or not _within(ref, w, tol)
            self.rej[k] = self.rej.get(k, False) or not _within(got, w, tol)

    def done(self, need=()):
        have = {k.split(":")[1] for k in self.rej}
        assert set(need) <= have, f"{self.what}: wrong references never formed: {sorted(set(need) - have)}"
        same = [k for k, d in self.differs.items() if not d]
        assert not same, f"{self.what}: wrong references within the bound of the right one in every family: {same}"
        missed = [k for k, r in self.rej.items() if not r]
        assert not missed, f"{self.what}: the bound does not reject the wrong references {missed}"


# ============================================================================================== operand families
def _family(kind, B, C, S, dtype, g):
    """[B, C, S] float64 values already rounded to dtype (drawn on the CPU: the same with and without a GPU)"""
    if kind == "int":                      # Tier 1: small integers
        v = torch.randint(-4, 5, (B, C, S), generator=g).double()
    else:
        v = torch.randn((B, C, S), generator=g, dtype=F32).double()
        if kind == "offset":
            v = v + 8.0
        elif kind == "chscale":
            v = v * torch.exp2(((torch.arange(C) * 5) % 13 - 6).double()).view(1, C, 1)
        elif kind == "outlier":
            v[:, :, 0] = 300.0
        elif kind == "bigmean":
            if dtype == BF:                # bf16 steps are 8 wide at 1024: a sparse two-level row
                v = 1024.0 + 8.0 * (torch.rand((B, C, S), generator=g) < 0.05).double()
            else:
                v = v + 1100.0
    return v.to(F32).to(dtype).double()


REAL = ("randn", "offset", "chscale")
STAT_REAL = REAL + ("outlier", "bigmean")


# ============================================================================================== float64 references with their bounds (rows form)
def ref_stats(x, L, d, stages=(1, 0, 1), drop_last=False):
    """x float64 [R, S] -> mean, rstd (float64), dmean (absolute bound), rho (relative bound of rstd; inf where the bound on the variance
    reaches the variance).  The kernels: per chunk of L elements shift = first element, v = x - shift, s1 = sum v, s2 = sum v^2 (fp32 chains of
    length d), mean_c = shift + s1 / n, M2_c = s2 - s1 (s1 / n); the chunks are combined in double; two stages round the group triples to fp32."""
    R, S = x.shape
    xs = x[:, :(-(-S // L) - 1) * L] if drop_last else x
    N = xs.shape[1]
    mean = xs.mean(1)
    M2 = ((xs - mean[:, None]) ** 2).sum(1)
    var = M2 / N
    rstd = (var + EPS) ** -0.5
    dmc, mcs, ns, dM2 = [], [], [], torch.zeros(R, dtype=F64)
    for lo in range(0, N, L):
        c = xs[:, lo:lo + L]
        n = c.shape[1]
        v = c - c[:, :1]
        A1, A2, mc = v.abs().sum(1), (v * v).sum(1), c.mean(1)
        dmc.append((d + 2) * U * A1 / n + U * mc.abs())            # v (1), the chain (d), the division, the addition of the shift
        dM2 += (3 * d + 8) * U * A2                               # s2: (d + 3) A2; s1 (s1 / n): 2 (d + 1) |s1 / n| A1 + 2 s1^2 / n, both <= A2 (Cauchy-Schwarz); the difference
        mcs.append(mc), ns.append(n)
    dmean = sum(n * e for n, e in zip(ns, dmc)) / N
    mmax = torch.stack(mcs).abs().amax(0)
    if stages[0] == 2:
        dmean = dmean + U * mmax                                  # group means and group M2 stored as fp32
        dM2 = dM2 + U * M2
    for n, mc, e in zip(ns, mcs, dmc):
        em = e + dmean + (U * mmax if stages[0] == 2 else 0.0)
        dM2 += n * (2 * (mc - mean).abs() * em + em * em)
    dmean = dmean + U * mean.abs()                                # (float) of the double mean
    q = dM2 / N / (var + EPS)
    rho = torch.where(q < 1, (1 - q.clamp(max=1 - 1e-12)) ** -0.5 - 1, torch.full_like(q, math.inf)) + 2 * U
    return mean, rstd, dmean, rho


def ref_apply(x, m, r, res, slope, x2=None, m2=None, r2=None):
    """y = lrelu((x - m) r [+ res | + (x2 - m2) r2], slope) -> (y, t): one rounding per subtraction, product, addition and the slope product"""
    v = (x - m[:, None]) * r[:, None]
    A = (x.abs() + m.abs()[:, None]) * r[:, None]
    d = 3
    if res is not None:
        v, A, d = v + res, A + res.abs(), 4
    if x2 is not None:
        v, A, d = v + (x2 - m2[:, None]) * r2[:, None], A + (x2.abs() + m2.abs()[:, None]) * r2[:, None], 6
    return torch.where(v >= 0, v, v * slope), d * U * A


def mask_of(src, slope, ge=False):
    return torch.where((src >= 0) if ge else (src > 0), torch.ones_like(src), torch.full_like(src, slope))


def ref_sums(dn, ns, nabs, S, L, d, drop_last=False):
    """means over the S voxels of dn and of dn n_k for every n_k of ns -> [(mean, bound)]: the kernel's terms carry 1 (dn) and 4 (dn (x - m) r)
    roundings, the chain d, the double fold is exact, the quotient is rounded to fp32"""
    hi = (-(-dn.shape[1] // L) - 1) * L if drop_last else dn.shape[1]
    out = [(dn[:, :hi].sum(1) / S, None)]
    out[0] = (out[0][0], (d + 1) * U * dn.abs().sum(1) / S + U * out[0][0].abs())
    for n, na in zip(ns, nabs):
        mk = (dn * n)[:, :hi].sum(1) / S
        out.append((mk, (d + 4) * U * (dn.abs() * na).sum(1) / S + U * mk.abs()))
    return out


def ref_dx(dn, n, nabs, r, a1, a2, da1=0.0, da2=0.0):
    """dx = r (dn - a1 - n a2): roundings dn, n (2), n a2, two subtractions, the product with r"""
    a1, a2, r = a1[:, None], a2[:, None], r[:, None]
    da1 = da1[:, None] if isinstance(da1, torch.Tensor) else da1
    da2 = da2[:, None] if isinstance(da2, torch.Tensor) else da2
    return r * (dn - a1 - n * a2), 7 * U * r * (dn.abs() + a1.abs() + nabs * a2.abs()) + r * (da1 + n.abs() * da2)


# ============================================================================================== the two backends: fp32 emulation and the library
class Emu:
    """numpy / torch fp32 emulation of the kernels' expressions, reductions in the given order: validates every bound without a GPU"""

    def __init__(self, order):
        self.order, self.name, self.dev = order, "emu-" + order, None

    # ---- rows form helpers
    def _stats(self, x, L, stages, T):
        x32 = x.float().numpy()
        R, S = x32.shape
        trip = []
        for lo in range(0, S, L):
            c = x32[:, lo:lo + L]
            n = np.float32(c.shape[1])
            sh = c[:, 0]
            v = c - sh[:, None]
            s1, s2 = _fsum(v, self.order, T), _fsum(v * v, self.order, T)
            q = s1 / n
            trip.append((float(n), (sh + q).astype(np.float64), np.maximum(s2 - s1 * q, np.float32(0)).astype(np.float64)))

        def fold(ts):
            n, m, M2 = 0.0, np.zeros(R), np.zeros(R)
            for nb, mb, m2b in ts:
                if nb <= 0:
                    continue
                nn, dd = n + nb, mb - m
                m = m + dd * (nb / nn)
                M2 = M2 + m2b + dd * dd * (n * nb / nn)
                n = nn
            return n, m, M2
        if stages[0] == 2:
            _, G, rpg = stages
            trip = [tuple(np.float32(v).astype(np.float64) if i else v for i, v in enumerate(fold(trip[g * rpg:(g + 1) * rpg]))) for g in range(G)]
        n, m, M2 = fold(trip)
        var = np.maximum(M2 / n, 0.0)
        return torch.from_numpy(m.astype(np.float32)), torch.from_numpy((1.0 / np.sqrt(var + np.float64(np.float32(EPS)))).astype(np.float32))

    def _apply(self, x, m, r, res, slope, x2=None, m2=None, r2=None, out=None):
        v = (x.float() - m[:, None]) * r[:, None]
        if res is not None:
            v = v + res.float()
        if x2 is not None:
            v = v + (x2.float() - m2[:, None]) * r2[:, None]
        return torch.where(v >= 0, v, v * np.float32(slope)).to(out or x.dtype)

    def _dn(self, dy, src, slope):
        return dy.float() * torch.where(src.float() > 0, torch.ones((), dtype=F32), torch.tensor(np.float32(slope)))

    def _sums(self, dn, ns, S, L, T):
        out = [_csum(dn, L, self.order, T)] + [_csum(dn * n, L, self.order, T) for n in ns]
        return [torch.from_numpy((s / float(S)).astype(np.float32)) for s in out]

    def _dx(self, dn, n, r, a1, a2, dtype):
        return (r[:, None] * (dn - a1[:, None] - n * a2[:, None])).to(dtype)

    # ---- row family: x [B, Cc, S]
    def row_fwd(self, x, res, slope):
        B, Cc, S = x.shape
        xr = x.reshape(B * Cc, S)
        m, r = self._stats(xr, CHUNK, (1, 0, 1), NT)
        y = self._apply(xr, m, r, None if res is None else res.reshape(B * Cc, S), slope)
        return y.view(B, Cc, S), m, r

    def row_bwd(self, dy, y, x, m, r, slope, want_dres):
        B, Cc, S = x.shape
        f = lambda t: t.reshape(B * Cc, S)                         # noqa: E731
        dn = self._dn(f(dy), f(y), slope)
        n = (f(x).float() - m[:, None]) * r[:, None]
        a1, a2 = self._sums(dn, [n], S, CHUNK, NT)
        return self._dx(dn, n, r, a1, a2, x.dtype).view(B, Cc, S), (dn.to(x.dtype).view(B, Cc, S) if want_dres else None)

    # ---- channels-last family: x [B, S, C] bf16, statistics [B C] in rows order (= [B, C] flattened)
    def cl_stats(self, x):
        B, S, C = x.shape
        return self._stats(_rows(x), CLV // (C // 8), fold_plan(cl_chunks_of(S, C), C), max(1, NT // (C // 8)))

    def cl_apply(self, x, m, r, res, slope):
        B, S, C = x.shape
        return _unrows(self._apply(_rows(x), m, r, None if res is None else _rows(res), slope), B, C)

    def cl_apply2(self, x, m, r, x2, m2, r2, slope):
        B, S, C = x.shape
        return _unrows(self._apply(_rows(x), m, r, None, slope, _rows(x2), m2, r2), B, C)

    def _cl_dn(self, dyw, off, y, x, m, r, slope, had_res):
        B, S, C = x.shape
        n = (_rows(x).float() - m[:, None]) * r[:, None]
        return self._dn(_rows(dyw[..., off:off + C]), _rows(y) if had_res else n, slope), n

    def cl_bwd_sums(self, dyw, off, y, x, m, r, slope, had_res):
        B, S, C = x.shape
        dn, n = self._cl_dn(dyw, off, y, x, m, r, slope, had_res)
        return tuple(self._sums(dn, [n], S, CLV // (C // 8), max(1, NT // (C // 8))))

    def cl_bwd_apply(self, dyw, off, y, x, m, r, a1, a2, slope, want_dres, had_res):
        B, S, C = x.shape
        dn, n = self._cl_dn(dyw, off, y, x, m, r, slope, had_res)
        return _unrows(self._dx(dn, n, r, a1, a2, BF), B, C), (_unrows(dn.to(BF), B, C) if want_dres else None)

    def cl_bwd2(self, dyw, off, y, x, m, r, x2, m2, r2, slope):
        B, S, C = x.shape
        dn, n = self._cl_dn(dyw, off, y, x, m, r, slope, True)
        n2 = (_rows(x2).float() - m2[:, None]) * r2[:, None]
        a1, a2, a3 = self._sums(dn, [n, n2], S, CLV // (C // 8), max(1, NT // (C // 8)))
        return _unrows(self._dx(dn, n, r, a1, a2, BF), B, C), _unrows(self._dx(dn, n2, r2, a1, a3, BF), B, C)


def _carve(t, dev, fill=float("nan")):
    """t as a view into the middle of a larger device allocation filled with NaN (16-byte aligned: PAD elements in front)"""
    n = t.numel()
    buf = torch.full((n + 2 * PAD,), fill, dtype=t.dtype, device=dev)
    buf[PAD:PAD + n] = t.reshape(-1).to(dev)
    return buf[PAD:PAD + n].view(t.shape)


def _same(a, b, what):
    for p, q in zip(a, b):
        if p is not None:
            assert torch.equal(_bits(p), _bits(q)), f"{what}: a second call on the same inputs differs"


class Hip:
    """UCF_VIT._hip.ops on operands carved from NaN-filled allocations; every call is made twice and must repeat bit for bit"""
    name = "hip"

    def __init__(self):
        self.dev = DEV

    def _twice(self, what, f):
        a = f()
        a = a if isinstance(a, tuple) else (a,)
        b = f()
        _same(a, b if isinstance(b, tuple) else (b,), what)
        out = tuple(None if t is None else t.cpu() for t in a)
        return out if len(out) > 1 else out[0]

    def row_fwd(self, x, res, slope):
        xd, rd = _carve(x, DEV), None if res is None else _carve(res, DEV)
        return self._twice("instnorm_fwd", lambda: _ops().instnorm_fwd(xd, rd, EPS, slope))

    def row_bwd(self, dy, y, x, m, r, slope, want_dres):
        a = [_carve(t, DEV) for t in (dy, y, x, m, r)]
        return self._twice("instnorm_bwd", lambda: _ops().instnorm_bwd(*a, slope, want_dres))

    @staticmethod
    def _map(t):
        B, S, C = t.shape
        return _carve(t, DEV).view(B, *_xyz(S), C)

    @staticmethod
    def _st(v, B):
        return _carve(v.view(B, -1), DEV)

    @staticmethod
    def _back(t):
        return None if t is None else t.reshape(t.shape[0], -1, t.shape[-1])

    def cl_stats(self, x):
        xd = self._map(x)
        m, r = self._twice("instnorm_cl_stats", lambda: _ops().instnorm_cl_stats(xd, EPS))
        return m.reshape(-1), r.reshape(-1)

    def cl_apply(self, x, m, r, res, slope):
        B = x.shape[0]
        a = (self._map(x), self._st(m, B), self._st(r, B), None if res is None else self._map(res))
        return self._back(self._twice("instnorm_cl_apply", lambda: _ops().instnorm_cl_apply(*a, slope)))

    def cl_apply2(self, x, m, r, x2, m2, r2, slope):
        B = x.shape[0]
        a = (self._map(x), self._st(m, B), self._st(r, B), self._map(x2), self._st(m2, B), self._st(r2, B))
        return self._back(self._twice("instnorm_cl_apply2", lambda: _ops().instnorm_cl_apply2(*a, slope)))

    def _dy(self, dyw, off, C):
        """the wide gradient on the device and the channel slice of it that the kernels read in place"""
        wide = self._map(dyw)
        dy = wide[..., off:off + C]
        assert _ops().cl_row_stride(dy) == dyw.shape[-1], "the sliced gradient must be read in place"
        return wide, dy

    def _untouched(self, wide, dyw, what):
        assert torch.equal(_bits(wide.cpu().reshape(dyw.shape)), _bits(dyw)), f"{what}: the gradient buffer behind the slice was written"

    def cl_bwd_sums(self, dyw, off, y, x, m, r, slope, had_res):
        B, S, C = x.shape
        wide, dy = self._dy(dyw, off, C)
        a = (self._map(y), self._map(x), self._st(m, B), self._st(r, B))
        m1, m2 = self._twice("instnorm_cl_bwd_sums", lambda: _ops().instnorm_cl_bwd_sums(dy, *a, slope, had_res)[:2])
        self._untouched(wide, dyw, "instnorm_cl_bwd_sums")
        return m1.reshape(-1), m2.reshape(-1)

    def cl_bwd_apply(self, dyw, off, y, x, m, r, a1, a2, slope, want_dres, had_res):
        B, S, C = x.shape
        wide, dy = self._dy(dyw, off, C)
        a = (self._map(y), self._map(x), self._st(m, B), self._st(r, B), self._st(a1, B), self._st(a2, B))
        dx, dres = self._twice("instnorm_cl_bwd_apply", lambda: _ops().instnorm_cl_bwd_apply(dy, *a, slope, want_dres, had_res))
        self._untouched(wide, dyw, "instnorm_cl_bwd_apply")
        return self._back(dx), self._back(dres)

    def cl_bwd2(self, dyw, off, y, x, m, r, x2, m2, r2, slope):
        B, S, C = x.shape
        wide, dy = self._dy(dyw, off, C)
        a = (self._map(y), self._map(x), self._st(m, B), self._st(r, B), self._map(x2), self._st(m2, B), self._st(r2, B))
        dx, dx2 = self._twice("instnorm_cl_bwd2", lambda: _ops().instnorm_cl_bwd2(dy, *a, slope))
        self._untouched(wide, dyw, "instnorm_cl_bwd2")
        return self._back(dx), self._back(dx2)


HOST = (Emu("seq"), Emu("pair"))


# ============================================================================================== exactness conditions (Tier 1)
def _assert_exact_sum(terms, quantum, what):
    """every partial sum of `terms` in any order is an fp32 number: the terms are multiples of the power of two `quantum` and the sum of their
    magnitudes stays below 2^24 quanta"""
    q = terms / quantum
    assert bool((q == q.round()).all()), f"{what}: terms are not multiples of {quantum}"
    worst = float(q.abs().sum(-1).max())
    assert worst < LIM, f"{what}: the exactness condition fails: sum of magnitudes {worst} quanta >= 2^24"


def _assert_fits(what, **vals):
    for k, v in vals.items():
        assert _fits32(v), f"{what}: the exactness condition fails: {k} is not an fp32 number everywhere"


def _once(v, dtype):
    """a float64 result that is an fp32 number, rounded ONCE to dtype"""
    return v.to(F32).to(dtype).double()


def _t1_stats(B, C):
    """Tier 1 statistics as inputs: integer means, power-of-two rstd, different for the channels c, c + 1 and c + 8 and for the two batch elements"""
    c = torch.arange(B * C) % C
    b = torch.arange(B * C) // C
    return ((c * 3) % 7 - 3 + b).double(), torch.exp2(((c + (c // 8)) % 3 - 1).double())


# ============================================================================================== backward references shared by both layouts
def _bwd_core(dy, msrc, x, m, r, slope, S, L, d, ge=False, drop_last=False, x2=None, m2=None, r2=None, swap=False):
    """rows form, float64.  msrc: what the activation mask is taken from (None: n itself) -> dict of results and bounds"""
    n, nabs = (x - m[:, None]) * r[:, None], (x.abs() + m.abs()[:, None]) * r[:, None]
    dn = dy * mask_of(n if msrc is None else msrc, slope, ge)
    ns, nas = [n], [nabs]
    if x2 is not None:
        ns.append((x2 - m2[:, None]) * r2[:, None]), nas.append((x2.abs() + m2.abs()[:, None]) * r2[:, None])
    sums = ref_sums(dn, ns, nas, S, L, d, drop_last)
    o = dict(dn=dn, n=n, nabs=nabs, m1=sums[0][0], t1=sums[0][1], m2=sums[1][0], t2=sums[1][1], dres=dn, tdres=U * dn.abs())
    o["dx"], o["tdx"] = ref_dx(dn, n, nabs, r, o["m1"], o["m2"], o["t1"], o["t2"])
    if x2 is not None:
        (a2, e2), (a3, e3) = (sums[2], sums[1]) if swap else (sums[1], sums[2])
        o["dx"], o["tdx"] = ref_dx(dn, n, nabs, r, o["m1"], a2, o["t1"], e2)
        o["dx2"], o["tdx2"] = ref_dx(dn, ns[1], nas[1], r2, o["m1"], a3, o["t1"], e3)
    return o


def _t1_x(m, S, g, for_bwd):
    """Tier 1 values around the integer means m [R]: any small integer for the forward kernels; m + {0, +-1, +-2} for the backward ones, so that
    n = (x - m) rstd is a power of two and its product with a mean of many bits stays an fp32 number"""
    R = m.numel()
    if for_bwd:
        d = torch.tensor([-2.0, -1.0, 0.0, 1.0, 2.0], dtype=F64)[torch.randint(0, 5, (R, S), generator=g)]
    else:
        d = torch.randint(-4, 5, (R, S), generator=g).double()
    return m[:, None] + d


def _ints(R, S, lo, hi, g):
    return torch.randint(lo, hi + 1, (R, S), generator=g).double()


def _t1_stat_rows(R, S, L, g):
    """Tier 1 rows for the statistics kernels: integers within 3 of an integer centre (different per row), the first element of every chunk AT
    the centre (the shift), -> (x, eligible): eligible when every chunk population is a power of two"""
    mu = ((torch.arange(R) * 5) % 17 - 8).double()
    x = mu[:, None] + _ints(R, S, -3, 3, g)
    x[:, 0::L] = mu[:, None]
    pops = [min(L, S - lo) for lo in range(0, S, L)]
    return x, all(p & (p - 1) == 0 for p in pops)


def _check_t1_stats(pool, kernel, x, L, got_m, got_r, stages=(1, 0, 1)):
    """exactness conditions computed from the operands, then: mean equal to the fp32 of the float64 mean, rstd that of the float64 rstd or its
    neighbour"""
    R, S = x.shape
    relvar = torch.zeros(R, dtype=F64)
    mean, rstd, _, _ = ref_stats(x, L, 0)
    M2 = ((x - mean[:, None]) ** 2).sum(1)
    for lo in range(0, S, L):
        c = x[:, lo:lo + L]
        v = c - c[:, :1]
        n = c.shape[1]
        _assert_exact_sum(v, 1.0, f"{pool.what} {kernel}: s1 of the chunk at {lo}")
        _assert_exact_sum(v * v, 1.0, f"{pool.what} {kernel}: s2 of the chunk at {lo}")
        s1, s2 = v.sum(1), (v * v).sum(1)
        _assert_fits(f"{pool.what} {kernel} chunk at {lo}", quotient=s1 / n, chunk_mean=c[:, 0] + s1 / n)
        p = s1 * s1 / n                                            # M2_c = s2 - s1 (s1 / n): a rounding where the product / the difference is no fp32 number
        relvar += torch.where(p.float().double() == p, 0.0, U * p) + torch.where((s2 - p).float().double() == s2 - p, 0.0, U * (s2 - p))
    if stages[0] == 2:
        relvar += U * M2
    relvar = relvar / M2.clamp_min(1e-300)
    assert float(relvar.max()) <= 1.25 * U, f"{pool.what} {kernel}: the variance is not within 1.25 U by construction ({float(relvar.max()) / U:.2f} U)"
    m32 = mean.to(F32)
    r32 = rstd.to(F32)
    ulp = torch.from_numpy(np.spacing(r32.numpy())).double()
    wr = {}
    if S > L:
        wr["drop_last"] = ref_stats(x, L, 0, drop_last=True)[0].to(F32).double()
    pool.check(kernel + " mean T1", "int", got_m, m32.double(), 0.0, wr)
    pool.check(kernel + " rstd T1", "int", got_r, r32.double(), ulp)


# ============================================================================================== row family
def run_row(c, be):
    B, Cc, S, dt = 2, c.Cc, c.S, c.dtype
    R, ou = B * Cc, (U if dt == F32 else UB)
    pool = Pool(c.id, be)
    sh = lambda t: t.to(F32).to(dt).view(B, Cc, S)                # noqa: E731  rows form float64 -> the operand
    ch = chunks_of(S)
    # ---- Tier 1: statistics of the fused forward
    g = _gen(c.id, "t1")
    x, eligible = _t1_stat_rows(R, S, CHUNK, g)
    if eligible:
        _, gm, gr = be.row_fwd(sh(x), None, 1.0)
        _check_t1_stats(pool, "in_stats", x, CHUNK, gm, gr)
    # ---- Tier 1: backward with the statistics as inputs (integer means, power-of-two rstd), slope 1/2
    m = ((torch.arange(R) * 3) % 7 - 3).double()
    r = torch.exp2((torch.arange(R) % 3 - 1).double())
    for with_res in (True, False):
        x = _t1_x(m, S, g, True)
        res = _ints(R, S, -4, 4, g) if with_res else None
        dy = _ints(R, S, -3, 3, g)
        y, _ = ref_apply(x, m, r, res, 0.5)
        _assert_fits(f"{c.id} T1 forward", y=y)
        y = _once(y, dt)
        o = _bwd_core(dy, y, x, m, r, 0.5, S, CHUNK, D_ROW)
        wrongs = _bwd_wrongs(dy, y, x, m, r, 0.5, S, CHUNK, D_ROW, B, with_res, ch)
        gdx, gdres = be.row_bwd(sh(dy), sh(y), sh(x), m.float(), r.float(), 0.5, with_res)
        _assert_exact_sum(o["dn"], 0.5, f"{c.id} T1 s1")
        _assert_exact_sum(o["dn"] * o["n"], 0.25, f"{c.id} T1 s2")
        if S & (S - 1) == 0:              # the means are dyadic: every operation of dx is exact
            _assert_fits(f"{c.id} T1 backward", m1=o["m1"], m2=o["m2"], p=o["n"] * o["m2"][:, None], q=o["dn"] - o["m1"][:, None],
                         s=o["dn"] - o["m1"][:, None] - o["n"] * o["m2"][:, None], dx=o["dx"])
            pool.check("in_bwd dx T1", f"int res={with_res}", gdx.reshape(R, S), _once(o["dx"], dt), 0.0, {k: _once(w["dx"], dt) for k, w in wrongs.items()})
        else:
            pool.check("in_bwd dx", f"int res={with_res}", gdx.reshape(R, S), o["dx"], _tol(o["dx"], o["tdx"], ou), {k: w["dx"] for k, w in wrongs.items()})
        if with_res:
            _assert_fits(f"{c.id} T1 dres", dn=o["dn"])
            pool.check("in_bwd dres T1", "int", gdres.reshape(R, S), _once(o["dn"], dt), 0.0, {k: _once(w["dres"], dt) for k, w in wrongs.items()})
        else:
            assert gdres is None
    # ---- Tier 2
    for fam in STAT_REAL:
        g = _gen(c.id, fam)
        x = _family(fam, B, Cc, S, dt, g).view(R, S)
        mean, rstd, dmean, rho = ref_stats(x, CHUNK, D_ROW)
        for with_res, slope in ((True, SLOPE), (False, SLOPE if fam != "randn" else 1.0)):
            res = _family("randn", B, Cc, S, dt, g).view(R, S) if with_res else None
            gy, gm, gr = be.row_fwd(sh(x), None if res is None else sh(res), slope)
            yr, t0 = ref_apply(x, mean, rstd, res, slope)
            n = (x - mean[:, None]) * rstd[:, None]
            rh = rho[:, None]
            t = torch.where(torch.isinf(rh), torch.full_like(n, math.inf),
                            (t0 + rstd[:, None] * dmean[:, None]) * (1 + rh.clamp(max=1e300)) + rh.clamp(max=1e300) * n.abs())
            wr = {"chan+1": ref_apply(x, _chan_roll(mean, B, 1), _chan_roll(rstd, B, 1), res, slope)[0], "shift": torch.roll(yr, 1, 1)}
            wm = {"chan+1": _chan_roll(mean, B, 1)}
            if with_res:
                wr["nores"] = ref_apply(x, mean, rstd, None, slope)[0]
            if ch > 1:
                ml, rl, _, _ = ref_stats(x, CHUNK, D_ROW, drop_last=True)
                wr["drop_last"], wm["drop_last"] = ref_apply(x, ml, rl, res, slope)[0], ml
            pool.check("in_stats mean", fam, gm, mean, dmean, wm)
            pool.check("in_stats rstd", fam, gr, rstd, rho * rstd)
            pool.check("in_apply y", f"{fam} res={with_res}", gy.reshape(R, S), yr, _tol(yr, t, ou), wr)
        if fam not in REAL:
            continue
        m32, r32 = mean.to(F32).double(), rstd.to(F32).double()
        for with_res in (True, False):
            res = _family("randn", B, Cc, S, dt, g).view(R, S) if with_res else None
            dy = _family("randn", B, Cc, S, dt, g).view(R, S)
            y = ref_apply(x, m32, r32, res, SLOPE)[0].to(F32).to(dt).double()
            o = _bwd_core(dy, y, x, m32, r32, SLOPE, S, CHUNK, D_ROW)
            wrongs = _bwd_wrongs(dy, y, x, m32, r32, SLOPE, S, CHUNK, D_ROW, B, with_res, ch)
            gdx, gdres = be.row_bwd(sh(dy), sh(y), sh(x), m32.float(), r32.float(), SLOPE, with_res)
            pool.check("in_bwd dx", f"{fam} res={with_res}", gdx.reshape(R, S), o["dx"], _tol(o["dx"], o["tdx"], ou), {k: w["dx"] for k, w in wrongs.items()})
            if with_res:
                pool.check("in_bwd dres", fam, gdres.reshape(R, S), o["dres"], _tol(o["dres"], o["tdres"], ou), {k: w["dres"] for k, w in wrongs.items()})
    pool.done(need=("chan+1", "shift", "nores", "mask_n", "mask_ge") + (("drop_last",) if ch > 1 else ()))
    return pool


def _bwd_wrongs(dy, y, x, m, r, slope, S, L, d, B, had_res, ch, C8=False, dense_dy=None, x2=None, m2=None, r2=None):
    """the wrong references of a backward pass (rows form): statistics of the neighbouring channel (+1, and +8 = the next 16-byte group), the
    volume shifted by one voxel, the mask from n although a residual was added, the mask with the tie at y = 0 taken the other way, the last
    chunk left out of the means, dy read densely where it is a slice, m2 / m3 exchanged"""
    kw = dict(x2=x2, m2=m2, r2=r2)
    rk = lambda k: dict(x2=x2, m2=None if m2 is None else _chan_roll(m2, B, k), r2=None if r2 is None else _chan_roll(r2, B, k))  # noqa: E731
    w = {"chan+1": _bwd_core(dy, y, x, _chan_roll(m, B, 1), _chan_roll(r, B, 1), slope, S, L, d, **rk(1)),
         "shift": _bwd_core(dy, y, torch.roll(x, 1, 1), m, r, slope, S, L, d, **kw)}
    if C8:
        w["chan+8"] = _bwd_core(dy, y, x, _chan_roll(m, B, 8), _chan_roll(r, B, 8), slope, S, L, d, **rk(8))
    if had_res:
        w["mask_n"] = _bwd_core(dy, None, x, m, r, slope, S, L, d, **kw)
    w["mask_ge"] = _bwd_core(dy, y, x, m, r, slope, S, L, d, ge=True, **kw)       # (y None: the tie at n = 0 of the mask recomputed from x)
    if ch > 1:
        w["drop_last"] = _bwd_core(dy, y, x, m, r, slope, S, L, d, drop_last=True, **kw)
    if dense_dy is not None:
        w["dense_dy"] = _bwd_core(dense_dy, y, x, m, r, slope, S, L, d, **kw)
    if x2 is not None:
        w["swap_m2m3"] = _bwd_core(dy, y, x, m, r, slope, S, L, d, swap=True, **kw)
    return w


@pytest.mark.parametrize("c", ROWS, ids=_ids(ROWS))
def test_row_family_on_the_host(c):
    """no GPU: the generators' exactness conditions, every wrong reference differing from the right one by more than the bound, and the fp32
    emulation (sequential and pairwise sums) inside every bound"""
    for be in HOST:
        run_row(c, be)


@gpu
@pytest.mark.parametrize("c", ROWS, ids=_ids(ROWS))
def test_row_family(c):
    run_row(c, Hip())


# ============================================================================================== channels-last family
def _wide(dy_rows, B, C, ld, off, g):
    """the gradient [B, S, C] (from rows form) as the channels off .. off + C of a wider random buffer [B, S, ld] -> (wide bf16, dense misreading)"""
    dy = _unrows(dy_rows, B, C)
    S = dy.shape[1]
    wide = torch.randint(-3, 4, (B, S, ld), generator=g).double() if ld > C else dy.clone()
    wide[..., off:off + C] = dy
    dense = None
    if ld > C:                            # what a kernel that ignored the row stride would read from the slice's first element on
        dense = _rows(wide.reshape(-1)[off:off + B * S * C].view(B, S, C))
    return wide.to(F32).to(BF), dense


def run_cl_stats(c, be, fams=STAT_REAL, tier1=True):
    B, C, S = 2, c.C, c.S
    R, Lv, d = B * C, CLV // c.cv, d_cl(c.C)
    stages = fold_plan(cl_chunks_of(S, C), C)
    pool = Pool(c.id + " stats", be)
    phys = lambda rows: _unrows(rows, B, C).to(F32).to(BF)         # noqa: E731
    if tier1:
        x, eligible = _t1_stat_rows(R, S, Lv, _gen(c.id, "t1s"))
        if stages[0] == 2:                # group means must stay fp32 numbers: every chunk a rearrangement of one balanced set, the last voxel at the centre
            eligible = False
        if eligible:
            gm, gr = be.cl_stats(phys(x))
            _check_t1_stats(pool, "incl_stats", x, Lv, gm, gr, stages)
    for fam in fams:
        x = _family(fam, B, C, S, BF, _gen(c.id, fam, "s")).view(R, S)
        mean, rstd, dmean, rho = ref_stats(x, Lv, d, stages)
        gm, gr = be.cl_stats(phys(x))
        wm = {"chan+1": _chan_roll(mean, B, 1)}
        if C > 8:
            wm["chan+8"] = _chan_roll(mean, B, 8)
        if S > Lv:
            wm["drop_last"] = ref_stats(x, Lv, d, drop_last=True)[0]
        pool.check("incl_stats mean", fam, gm, mean, dmean, wm)
        pool.check("incl_stats rstd", fam, gr, rstd, rho * rstd)
    pool.done(need=("chan+1",) + (("chan+8",) if C > 8 else ()) + (("drop_last",) if S > Lv else ()))
    return pool


def _cl_inputs(c, fam, g):
    """rows-form float64 operands of the kernels that take the statistics as inputs"""
    B, C, S = 2, c.C, c.S
    R = B * C
    if fam == "int":
        m, r = _t1_stats(B, C)
        m2, r2 = _chan_roll(m, B, 3) + 1, _chan_roll(r, B, 1)
        mk = lambda mm, bwd: _t1_x(mm, S, g, bwd)                  # noqa: E731
        return dict(m=m, r=r, m2=m2, r2=r2, x=mk(m, False), xb=mk(m, True), x2=mk(m2, False), x2b=mk(m2, True), res=_ints(R, S, -4, 4, g),
                    dy=_ints(R, S, -3, 3, g), slope=0.5)
    x = _family(fam, B, C, S, BF, g).view(R, S)
    x2 = _family(fam, B, C, S, BF, g).view(R, S).roll(3, 0) * 0.5
    x2 = x2.to(F32).to(BF).double()
    st = lambda v: [t.to(F32).double() for t in ref_stats(v, S, 0)[:2]]            # noqa: E731  the statistics are operands here: rounded to fp32
    (m, r), (m2, r2) = st(x), st(x2)
    return dict(m=m, r=r, m2=m2, r2=r2, x=x, xb=x, x2=x2, x2b=x2, res=_family("randn", B, C, S, BF, g).view(R, S),
                dy=_family("randn", B, C, S, BF, g).view(R, S), slope=SLOPE)


def run_cl_apply(c, be):
    B, C, S = 2, c.C, c.S
    pool = Pool(c.id + " apply", be)
    phys = lambda rows: _unrows(rows, B, C).to(F32).to(BF)         # noqa: E731
    for fam in ("int",) + REAL:
        o = _cl_inputs(c, fam, _gen(c.id, fam, "a"))
        x, m, r, res, slope = o["x"], o["m"], o["r"], o["res"], o["slope"]
        exact = fam == "int"
        for kern, kw in (("incl_apply<res>", dict(res=res)), ("incl_apply<nores>", dict(res=None)), ("incl_apply2", dict(res=None, x2=o["x2"], m2=o["m2"], r2=o["r2"]))):
            ref, t = ref_apply(x, m, r, slope=slope, **kw)
            rk = {k: (_chan_roll(v, B, 1) if k in ("m2", "r2") else v) for k, v in kw.items()}
            wr = {"chan+1": ref_apply(x, _chan_roll(m, B, 1), _chan_roll(r, B, 1), slope=slope, **rk)[0], "shift": ref_apply(torch.roll(x, 1, 1), m, r, slope=slope, **kw)[0]}
            if C > 8:
                r8 = {k: (_chan_roll(v, B, 8) if k in ("m2", "r2") else v) for k, v in kw.items()}
                wr["chan+8"] = ref_apply(x, _chan_roll(m, B, 8), _chan_roll(r, B, 8), slope=slope, **r8)[0]
            if kw.get("res") is not None:
                wr["nores"] = ref_apply(x, m, r, None, slope)[0]
            if "x2" in kw:
                wr["nores"] = ref_apply(x, m, r, None, slope)[0]    # the second branch dropped
                got = be.cl_apply2(phys(x), m.float(), r.float(), phys(kw["x2"]), kw["m2"].float(), kw["r2"].float(), slope)
            else:
                got = be.cl_apply(phys(x), m.float(), r.float(), None if kw["res"] is None else phys(kw["res"]), slope)
            got = _rows(got)
            if exact:
                v = (x - m[:, None]) * r[:, None]
                _assert_fits(f"{c.id} {kern} T1", d=x - m[:, None], n=v, v=ref / torch.where(ref < 0, slope, 1.0), y=ref,
                             n2=(kw["x2"] - kw["m2"][:, None]) * kw["r2"][:, None] if "x2" in kw else v)
                exp = _once(ref, BF)
                pool.check(kern + " T1", fam, got, exp, 0.0, {k: _once(w, BF) for k, w in wr.items()})
                assert torch.equal(_bits(got), _bits(exp.to(BF))), f"{c.id} {kern}: not bit-equal to the float64 result rounded once"
            else:
                pool.check(kern, fam, got, ref, _tol(ref, t, UB), wr)
    pool.done(need=("chan+1", "shift", "nores") + (("chan+8",) if C > 8 else ()))
    return pool


BWD_APPLY = (("incl_bwd_apply<y,dres>", True, True), ("incl_bwd_apply<y>", True, False), ("incl_bwd_apply<x>", False, False))


def run_cl_bwd(c, be):
    """ucfvit_instnorm_cl_bwd_sums (mask from y / from x) and the three instantiations behind ucfvit_instnorm_cl_bwd_apply"""
    B, C, S = 2, c.C, c.S
    Lv, d, ch = CLV // c.cv, d_cl(c.C), cl_chunks_of(c.S, c.C)
    pool = Pool(c.id + " bwd", be)
    phys = lambda rows: _unrows(rows, B, C).to(F32).to(BF)         # noqa: E731
    for fam in ("int",) + REAL:
        g = _gen(c.id, fam, "b")
        o = _cl_inputs(c, fam, g)
        x, m, r, dy, slope = o["xb"], o["m"], o["r"], o["dy"], o["slope"]
        exact = fam == "int"
        dyw, dense = _wide(dy, B, C, c.ldy, c.off, g)
        for kern, had_res, want_dres in BWD_APPLY:
            y = ref_apply(x, m, r, o["res"] if had_res else None, slope)[0]
            if exact:
                _assert_fits(f"{c.id} T1 y", y=y)
            y = y.to(F32).to(BF).double()
            ok = _bwd_core(dy, y if had_res else None, x, m, r, slope, S, Lv, d)
            wr = _bwd_wrongs(dy, y if had_res else None, x, m, r, slope, S, Lv, d, B, had_res, ch, C > 8, dense)
            if not want_dres:             # the sums: once per mask source
                sk = f"incl_bwd_partial<{'y' if had_res else 'x'}>"
                g1, g2 = be.cl_bwd_sums(dyw, c.off, phys(y), phys(x), m.float(), r.float(), slope, had_res)
                if exact:                 # exact sums, one correctly rounded quotient: what (float)(s / (double) S) gives
                    _assert_exact_sum(ok["dn"], 0.5, f"{c.id} T1 s1")
                    _assert_exact_sum(ok["dn"] * ok["n"], 0.25, f"{c.id} T1 s2")
                    f32 = lambda v: v.to(F32).double()             # noqa: E731
                    pool.check(sk + " m1 T1", fam, g1, f32(ok["m1"]), 0.0, {k: f32(w["m1"]) for k, w in wr.items()})
                    pool.check(sk + " m2 T1", fam, g2, f32(ok["m2"]), 0.0, {k: f32(w["m2"]) for k, w in wr.items()})
                    if S & (S - 1) == 0:
                        _assert_fits(f"{c.id} T1 means", m1=ok["m1"], m2=ok["m2"])
                else:
                    pool.check(sk + " m1", fam, g1, ok["m1"], _tol(ok["m1"], ok["t1"], 0.0), {k: w["m1"] for k, w in wr.items()})
                    pool.check(sk + " m2", fam, g2, ok["m2"], _tol(ok["m2"], ok["t2"], 0.0), {k: w["m2"] for k, w in wr.items()})
            # the apply pass takes m1 / m2 as inputs: dyadic ones in Tier 1, the rounded float64 means otherwise
            if exact:
                cc = torch.arange(B * C) % C
                a1, a2 = ((cc % 5) - 2).double() / 4, ((cc % 3) - 1).double() / 2
            else:
                a1, a2 = ok["m1"].to(F32).double(), ok["m2"].to(F32).double()

            def dxref(o_, k=0, r=r, a1=a1, a2=a2):
                return ref_dx(o_["dn"], o_["n"], o_["nabs"], r, _chan_roll(a1, B, k), _chan_roll(a2, B, k))
            ref, t = dxref(ok)
            wdx = {k: dxref(w, k=(1 if k == "chan+1" else 8 if k == "chan+8" else 0))[0] for k, w in wr.items() if k != "drop_last"}
            gdx, gdres = be.cl_bwd_apply(dyw, c.off, phys(y), phys(x), m.float(), r.float(), a1.float(), a2.float(), slope, want_dres, had_res)
            if exact:
                na2 = ok["n"] * a2[:, None]
                _assert_fits(f"{c.id} {kern} T1", dn=ok["dn"], n=ok["n"], na2=na2, q=ok["dn"] - a1[:, None], s=ok["dn"] - a1[:, None] - na2, dx=ref)
                exp = _once(ref, BF)
                pool.check(kern + " dx T1", fam, _rows(gdx), exp, 0.0, {k: _once(w, BF) for k, w in wdx.items()})
                assert torch.equal(_bits(_rows(gdx)), _bits(exp.to(BF))), f"{c.id} {kern}: dx not bit-equal to the float64 result rounded once"
            else:
                pool.check(kern + " dx", fam, _rows(gdx), ref, _tol(ref, t, UB), wdx)
            if want_dres:
                wd = {k: w["dres"] for k, w in wr.items() if k != "drop_last"}
                if exact:
                    exp = _once(ok["dres"], BF)
                    pool.check(kern + " dres T1", fam, _rows(gdres), exp, 0.0, {k: _once(w, BF) for k, w in wd.items()})
                    assert torch.equal(_bits(_rows(gdres)), _bits(exp.to(BF)))
                else:
                    pool.check(kern + " dres", fam, _rows(gdres), ok["dres"], _tol(ok["dres"], ok["tdres"], UB), wd)
            else:
                assert gdres is None
    need = ("chan+1", "shift", "mask_n", "mask_ge") + (("chan+8",) if C > 8 else ()) + (("drop_last",) if ch > 1 else ()) + (("dense_dy",) if c.ldy > C else ())
    pool.done(need=need)
    return pool


def run_cl_bwd2(c, be):
    B, C, S = 2, c.C, c.S
    Lv, d, ch = CLV // c.cv, d_cl(c.C), cl_chunks_of(c.S, c.C)
    pool = Pool(c.id + " bwd2", be)
    phys = lambda rows: _unrows(rows, B, C).to(F32).to(BF)         # noqa: E731
    for fam in ("int",) + REAL:
        g = _gen(c.id, fam, "b2")
        o = _cl_inputs(c, fam, g)
        x, m, r, x2, m2, r2, dy, slope = o["xb"], o["m"], o["r"], o["x2b"], o["m2"], o["r2"], o["dy"], o["slope"]
        exact = fam == "int"
        dyw, dense = _wide(dy, B, C, c.ldy, c.off, g)
        y = ref_apply(x, m, r, None, slope, x2, m2, r2)[0]
        if exact:
            _assert_fits(f"{c.id} T1 y", y=y)
        y = y.to(F32).to(BF).double()
        kw = dict(x2=x2, m2=m2, r2=r2)
        ok = _bwd_core(dy, y, x, m, r, slope, S, Lv, d, **kw)
        wr = _bwd_wrongs(dy, y, x, m, r, slope, S, Lv, d, B, True, ch, C > 8, dense, **kw)
        gdx, gdx2 = be.cl_bwd2(dyw, c.off, phys(y), phys(x), m.float(), r.float(), phys(x2), m2.float(), r2.float(), slope)
        if exact and S & (S - 1) == 0:    # dyadic means: every operation exact
            _assert_exact_sum(ok["dn"], 0.5, f"{c.id} T1 s1")
            for k in ("n", "n2"):
                nk = ok["n"] if k == "n" else (x2 - m2[:, None]) * r2[:, None]
                _assert_exact_sum(ok["dn"] * nk, 0.25, f"{c.id} T1 sum dn {k}")
            _assert_fits(f"{c.id} incl_bwd2 T1", dx=ok["dx"], dx2=ok["dx2"], m1=ok["m1"])
            a3 = ((ok["dn"] * (x2 - m2[:, None]) * r2[:, None]).sum(1) / S)
            _assert_fits(f"{c.id} incl_bwd2 T1", m2=ok["m2"], m3=a3, p2=ok["n"] * ok["m2"][:, None], p3=(x2 - m2[:, None]) * r2[:, None] * a3[:, None],
                         s2=ok["dn"] - ok["m1"][:, None] - ok["n"] * ok["m2"][:, None], s3=ok["dn"] - ok["m1"][:, None] - (x2 - m2[:, None]) * r2[:, None] * a3[:, None])
            for k, got in (("dx", gdx), ("dx2", gdx2)):
                exp = _once(ok[k], BF)
                pool.check(f"incl_bwd2 {k} T1", fam, _rows(got), exp, 0.0, {n_: _once(w[k], BF) for n_, w in wr.items()})
                assert torch.equal(_bits(_rows(got)), _bits(exp.to(BF))), f"{c.id} incl_bwd2 {k}: not bit-equal to the float64 result rounded once"
        else:
            for k, got in (("dx", gdx), ("dx2", gdx2)):
                pool.check(f"incl_bwd2 {k}", fam, _rows(got), ok[k], _tol(ok[k], ok["t" + k], UB), {n_: w[k] for n_, w in wr.items()})
    need = ("chan+1", "shift", "mask_n", "mask_ge", "swap_m2m3") + (("chan+8",) if C > 8 else ()) + (("drop_last",) if ch > 1 else ()) + (("dense_dy",) if c.ldy > C else ())
    pool.done(need=need)
    return pool


CL_PARTS = {"stats": run_cl_stats, "apply": run_cl_apply, "bwd": run_cl_bwd, "bwd2": run_cl_bwd2}


@pytest.mark.parametrize("c", CLS, ids=_ids(CLS))
def test_cl_family_on_the_host(c):
    """no GPU: exactness conditions, wrong references, and the fp32 emulation in both summation orders inside every bound"""
    for be in HOST:
        for f in CL_PARTS.values():
            f(c, be)


@gpu
@pytest.mark.parametrize("part", list(CL_PARTS))
@pytest.mark.parametrize("c", CLS, ids=_ids(CLS))
def test_cl_family(c, part):
    CL_PARTS[part](c, Hip())


# ---- widths incl_check accepts but no model uses: C > NT forces the single-stage fold.  The library computes them (measured), so correct values
# are required: any error of the library, a refusal included, fails the test
@pytest.mark.parametrize("c", WIDE, ids=_ids(WIDE))
def test_cl_wide_channels_on_the_host(c):
    for be in HOST:
        for f in CL_PARTS.values():
            f(c, be)


@gpu
@pytest.mark.parametrize("part", list(CL_PARTS))
@pytest.mark.parametrize("c", WIDE, ids=_ids(WIDE))
def test_cl_wide_channels(c, part):
    CL_PARTS[part](c, Hip())


# ---- the two-stage statistics fold through ops.instnorm_cl_stats: both sides of rows = 512
def _t1_balanced(R, S, Lv):
    """every full chunk of Lv voxels a rearrangement of one balanced set around the row's integer centre (sum of deviations 0), the ragged rest AT
    the centre: every chunk mean is the centre, so group means stay fp32 numbers through a two-stage fold"""
    pat = torch.zeros(Lv, dtype=F64)
    q = Lv // 4
    pat[:q], pat[q:2 * q], pat[2 * q:2 * q + q // 2], pat[2 * q + q // 2:3 * q] = 1.0, -1.0, 2.0, -2.0
    mu = ((torch.arange(R) * 5) % 17 - 8).double()
    v = torch.arange(S)
    idx = ((v % Lv)[None, :] * (2 * (torch.arange(R) % 5) + 1)[:, None] + (v // Lv)[None, :] * 7 + torch.arange(R)[:, None]) % Lv
    x = mu[:, None] + pat[idx]
    x[:, (S // Lv) * Lv:] = mu[:, None]
    return x


def run_cl_fold(c, be):
    B, C, S = 2, c.C, c.S
    R, Lv = B * C, CLV // c.cv
    stages = fold_plan(cl_chunks_of(S, C), C)
    pool = Pool(c.id + " fold", be)
    x = _t1_balanced(R, S, Lv)
    gm, gr = be.cl_stats(_unrows(x, B, C).to(BF))
    _check_t1_stats(pool, f"incl_stats_fold{stages[0]}", x, Lv, gm, gr, stages)
    del x
    for fam in ("offset",):
        x = _family(fam, B, C, S, BF, _gen(c.id, fam, "s")).view(R, S)
        mean, rstd, dmean, rho = ref_stats(x, Lv, d_cl(C), stages)
        gm, gr = be.cl_stats(_unrows(x, B, C).to(BF))
        wm = {"chan+1": _chan_roll(mean, B, 1), "chan+8": _chan_roll(mean, B, 8), "drop_last": ref_stats(x[:, :(S // Lv - (S % Lv == 0)) * Lv], Lv, 0)[0]}
        pool.check(f"incl_stats_fold{stages[0]} mean", fam, gm, mean, dmean, wm)
        pool.check(f"incl_stats_fold{stages[0]} rstd", fam, gr, rstd, rho * rstd)
    pool.done(need=("chan+1", "chan+8"))
    return pool


@pytest.mark.parametrize("be", HOST, ids=[b.name for b in HOST])
@pytest.mark.parametrize("c", FOLD, ids=_ids(FOLD))
def test_cl_stats_fold_stages_on_the_host(c, be):
    assert fold_plan(cl_chunks_of(c.S, c.C), c.C)[0] == (2 if c.tag == "513rows" else 1)
    run_cl_fold(c, be)


@gpu
@pytest.mark.parametrize("c", FOLD, ids=_ids(FOLD))
def test_cl_stats_fold_stages(c):
    run_cl_fold(c, Hip())


# ---- the G = 256 cap of the first stage: more than 65536 partial rows at C = 8, handed to ucfvit_instnorm_cl_stats_fold as the convolution epilogue does
def _gcap_rows():
    B, C, rows = 2, 8, GCAP_ROWS
    g = _gen("gcap")
    n = torch.tensor([0.0, 4.0, 8.0], dtype=F64)[torch.randint(0, 3, (B, rows, 1, C), generator=g)]
    m = (torch.randn((B, rows, 1, C), generator=g, dtype=F32) + 5.0 * (torch.arange(C) % 3).view(1, 1, 1, C)).double()
    M2 = (torch.rand((B, rows, 1, C), generator=g, dtype=F32).double() * n).to(F32).double()
    return torch.cat([n, m, M2], 2)       # [B][rows][3][C]: count, mean, M2


def _gcap_ref(part, last_dropped=False):
    p = part[:, :-1] if last_dropped else part
    n, m, M2 = p[:, :, 0], p[:, :, 1], p[:, :, 2]
    N = n.sum(1)
    mean = (n * m).sum(1) / N
    M2t = M2.sum(1) + (n * (m - mean[:, None]) ** 2).sum(1)
    var = M2t / N
    mmax = m.abs().amax(1)
    ud = 10 * p.shape[1] * 2.0 ** -53                              # the double arithmetic: at most 10 roundings a mom_add, at most `rows` of them in a chain
    dmean = U * mmax + U * mean.abs() + ud * 2 * mmax              # group means as fp32, (float) of the result, the double updates d nb / n with |d| <= 2 max|m|
    dM2 = 2 * U * M2t + 2 * (n * (m - mean[:, None]).abs()).sum(1) * (U * mmax + dmean) + ud * M2t
    q = dM2 / N / (var + EPS)
    return mean.reshape(-1), ((var + EPS) ** -0.5).reshape(-1), dmean.reshape(-1), ((1 - q) ** -0.5 - 1 + 2 * U).reshape(-1)


def _gcap_emu(part, order):
    """the fold has no fp32 sum: triples are combined in double and only the group triples and the result are stored as fp32.  "seq": the
    kernel's mom_add, one triple after the other; "pair": the closed form of the combined moments (numpy's pairwise double sums)"""
    B, rows, _, C = part.shape
    _, G, rpg = fold_plan(rows, C)
    p = part.numpy()

    def fold(n, m, M2):
        if order == "seq":
            N, mean, tot = np.zeros_like(n[:, 0]), np.zeros_like(n[:, 0]), np.zeros_like(n[:, 0])
            for k in range(n.shape[1]):
                nb, nn = n[:, k], N + n[:, k]
                d = m[:, k] - mean
                w = nb / np.maximum(nn, 1e-300)                    # (count 0: the triple drops out, as in mom_add)
                mean, tot, N = mean + d * w, tot + np.where(nb > 0, M2[:, k] + d * d * (N * w), 0.0), nn
            return N, mean, tot
        N = n.sum(1)
        mean = (n * m).sum(1) / np.maximum(N, 1e-300)
        return N, mean, M2.sum(1) + (n * (m - mean[:, None]) ** 2).sum(1)
    gs = [fold(p[:, g * rpg:(g + 1) * rpg, 0], p[:, g * rpg:(g + 1) * rpg, 1], p[:, g * rpg:(g + 1) * rpg, 2]) for g in range(G)]
    f32 = lambda k: np.stack([t[k] for t in gs], 1).astype(np.float32).astype(np.float64)       # noqa: E731
    N, mean, M2 = fold(f32(0), f32(1), f32(2))
    return torch.from_numpy(mean.astype(np.float32)).reshape(-1), torch.from_numpy((1 / np.sqrt(M2 / N + EPS)).astype(np.float32)).reshape(-1)


def _gcap_hip(part):
    L = _lib().load()
    B, rows, _, C = part.shape
    pd = _carve(part.float(), DEV)
    ws = torch.full((B * 256 * 3 * C,), float("nan"), dtype=F32, device=DEV)
    out = []
    for _ in range(2):
        mean, rstd = (torch.full((B, C), float("nan"), dtype=F32, device=DEV) for _ in range(2))
        _lib().check(L.ucfvit_instnorm_cl_stats_fold(pd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, int(part[:, :, 0].sum(1).max()), C, rows, EPS, ws.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream), "ucfvit_instnorm_cl_stats_fold")
        out.append((mean.cpu().reshape(-1), rstd.cpu().reshape(-1)))
    _same(out[0], out[1], "ucfvit_instnorm_cl_stats_fold")
    return out[0]


def _run_gcap(be):
    part = _gcap_rows()
    stages, G, rpg = fold_plan(part.shape[1], 8)
    assert (stages, G) == (2, 256) and rpg > 256 and G * rpg > part.shape[1] > (G - 1) * rpg, "the case must sit on the G = 256 cap with a short last group"
    gm, gr = _gcap_hip(part) if be.dev else _gcap_emu(part, be.order)
    mean, rstd, dmean, rho = _gcap_ref(part)
    pool = Pool("fold1 G cap", be)
    wm = {"chan+1": _chan_roll(mean, 2, 1), "last_row": _gcap_ref(part, last_dropped=True)[0]}
    wr = {"chan+1": _chan_roll(rstd, 2, 1), "last_row": _gcap_ref(part, last_dropped=True)[1]}
    pool.check("incl_stats_fold1 cap mean", "triples", gm, mean, dmean, wm)
    pool.check("incl_stats_fold1 cap rstd", "triples", gr, rstd, rho * rstd, wr)
    pool.done(need=("chan+1", "last_row"))


@pytest.mark.parametrize("be", HOST, ids=[b.name for b in HOST])
def test_cl_stats_fold_group_cap_on_the_host(be):
    _run_gcap(be)


@gpu
def test_cl_stats_fold_group_cap():
    _run_gcap(Hip())


# ============================================================================================== Dice + cross-entropy
# Device functions (HIP Programming Guide, "HIP math API", single-precision intrinsics: __expf and __logf are the native approximations,
# lowered to x log2(e) -> v_exp_f32 and v_log_f32 -> ln 2; the CDNA ISA guide gives both instructions 1 ULP).  Allowed here, as in
# tests/test_attention_ops.py: 4 U for each instruction, plus the rounding of the argument scaling: relative (2 |a| + 4) U for __expf(a)
# (a itself is a rounded difference), absolute 4 U (|log p| + 1) for __logf(p).
def _eps_p(xm):
    """relative error of a probability whose farthest logit lies xm below the maximum: the numerator and the 8-term denominator carry
    (2 xm + 4) U each, 7 additions, the reciprocal and the product"""
    return (4 * xm + 17) * U


def ref_dice(z, lab, n, snr, sdr, gscale, other=None, S_total=None, drop_class=False):
    """float64 Dice + CE of logits z [B, n, S] (already rounded to the operand type), labels [B, S] -> dict: stats [B, 25], loss, grad and their
    bounds.  other: the sums of the rest of a sharded volume (fp32 numbers), added in fp32 by the caller."""
    B, _, S = z.shape
    S_total = S_total or S
    zz = z[:, :n - 1] if drop_class else z
    mx = zz.amax(1, keepdim=True)
    e = torch.exp(zz - mx)
    e = torch.where(e < 2.0 ** -150, torch.zeros_like(e), e)       # below half the smallest fp32 number: exactly 0 in fp32 (Tier 1 relies on it)
    p = e / e.sum(1, keepdim=True)
    if drop_class:
        p = torch.cat([p, torch.zeros(B, 1, S, dtype=F64)], 1)
    ep = _eps_p((zz - mx).abs().amax(1, keepdim=True))             # [B, 1, S]
    oh = torch.nn.functional.one_hot(lab, n).movedim(-1, 1).double()
    lp = torch.log(p.clamp_min(1e-38))
    I, P, Cn, ce = (p * oh).sum(2), (p * p).sum(2), oh.sum(2), -(oh * lp).sum((1, 2))
    d = D_ROW + 2                                                  # the chain, the product, the (float) of the folded sum
    tI, tP = (p * oh * ep).sum(2) + d * U * I, (p * p * 2 * ep).sum(2) + (d + 1) * U * P
    tce = (oh * (ep + 4 * U * (lp.abs() + 1))).sum((1, 2)) + d * U * (oh * lp.abs()).sum((1, 2))
    stats, tst = torch.zeros(B, DSTAT, dtype=F64), torch.zeros(B, DSTAT, dtype=F64)
    stats[:, :n], stats[:, 8:8 + n], stats[:, 16:16 + n], stats[:, 24] = I, P, Cn, ce
    tst[:, :n], tst[:, 8:8 + n], tst[:, 24] = tI, tP, tce
    local, tlocal = stats.clone(), tst.clone()
    if other is not None:
        stats = stats + other
        tst = tst + U * stats.abs()
        I, P, Cn, ce, tI, tP, tce = stats[:, :n], stats[:, 8:8 + n], stats[:, 16:16 + n], stats[:, 24], tst[:, :n], tst[:, 8:8 + n], tst[:, 24]
    D = P + Cn + sdr
    N2 = 2 * I + snr
    loss = (1 - N2 / D).mean() + ce.sum() / (B * S_total)
    tloss = ((2 * tI) / D + N2 * tP / D ** 2).mean() + tce.sum() / (B * S_total)
    tloss = tloss + U * ((1 + N2 / D).mean() + ce.abs().sum() / (B * S_total))
    # gradient: g_c = a_c onehot_c + bq_c p_c, dz_c = gscale (p_c (g_c - sum_k g_k p_k) + (p_c - onehot_c) wce)
    wb, wce = 1.0 / (B * n), 1.0 / (B * S_total)
    eD = tP / D + 2 * U
    a, bq = (-2 / D * wb)[:, :, None], (2 * N2 / D ** 2 * wb)[:, :, None]
    ea, ebq = (eD + 6 * U)[:, :, None], (2 * tI / N2 + U + 2 * eD + 10 * U)[:, :, None]
    g = a * oh + bq * p
    G = a.abs() * oh + bq * p
    dg = a.abs() * oh * ea + bq * p * (ebq + ep + U) + U * G
    dot, Gdot = (g * p).sum(1, keepdim=True), (G * p).sum(1, keepdim=True)
    ddot = (dg * p + G * p * (ep + U)).sum(1, keepdim=True) + 8 * U * Gdot
    grad = gscale * (p * (g - dot) + (p - oh) * wce)
    t1, t2 = p * (G + Gdot), (p + oh) * wce
    tg = gscale * (p * (dg + ddot) + t1 * (ep + 2 * U) + wce * (p * ep + 3 * U * (p + oh)) + 2 * U * (t1 + t2))
    return dict(stats=stats, tstats=tst, local=local, tlocal=tlocal, loss=loss.reshape(()), tloss=tloss.reshape(()), grad=grad, tgrad=tg, p=p)


def _dice_operands(c, fam, g, S=None):
    """-> logits [B, n, S] float64 rounded to the case's type, labels [B, S].  "int" (Tier 1): the predicted class has logit 0, every other one
    -200, so __expf gives exactly 1 and 0; 3 + b + class voxels per (batch element, class) are mispredicted where the volume is large enough"""
    B, n, S = 2, c.n, S or c.S
    lab = torch.randint(0, n, (B, S), generator=g)
    if fam == "int":
        pred = lab.clone()
        for b in range(B):
            for k in range(n):
                idx = torch.nonzero(lab[b] == k).reshape(-1)[:3 + b + k]
                pred[b, idx] = (k + 1 + (idx % max(n - 1, 1))) % n
                pred[b, idx] = torch.where(pred[b, idx] == k, (k + 1) % n, pred[b, idx])
        z = torch.full((B, n, S), -200.0, dtype=F64)
        z.scatter_(1, pred[:, None, :], 0.0)
        return z, lab
    z = torch.randn((B, n, S), generator=g, dtype=F32).double() * 2.0
    if fam == "offset":
        z = z + 8.0
    elif fam == "chscale":
        z = z * torch.exp2(((torch.arange(n) * 2) % 3 - 1).double()).view(1, n, 1)
    return z.to(F32).to(c.dtype).double(), lab


def _dice_buffer(c, z, padval=float("nan")):
    """the logits in the case's layout -> (flat buffer float64 with NaN in the padding columns, the [B, n, S] view's (shape, strides, offset))"""
    B, n, S = z.shape
    if c.lay == "nc":
        return z.reshape(-1).clone(), (B, n, S), (n * S, S, 1)
    buf = torch.full((B, S, c.ld), padval, dtype=F64)
    buf[..., :n] = z.movedim(1, -1)
    return buf.reshape(-1), (B, n, S), (S * c.ld, 1, c.ld)


def _dice_misread(c, z):
    """class and voxel strides exchanged: the same buffer read as [S][n] where it is [n][S] and the other way round"""
    B, n, S = z.shape
    flat, _, _ = _dice_buffer(c, z, padval=0.0)                    # (zeros in the padding columns, as the decoder leaves them)
    flat = flat.view(B, -1)
    ci, vi = torch.arange(n).view(n, 1), torch.arange(S).view(1, S)
    return flat[:, (vi * n + ci) if c.lay == "nc" else (ci * S + vi)]


class EmuDice:
    def __init__(self, order):
        self.order, self.name, self.dev = order, "emu-" + order, None

    def _p(self, z):
        z = z.float()
        e = torch.exp(z - z.amax(1, keepdim=True))
        den = torch.zeros_like(e[:, 0])
        for k in range(e.shape[1]):
            den = den + e[:, k]
        return e * (1.0 / den)[:, None]

    def stats(self, c, z, lab):
        B, n, S = z.shape
        p = self._p(z)
        oh = torch.nn.functional.one_hot(lab, n).movedim(-1, 1).float()
        lp = torch.log(p.clamp_min(1e-38))
        st = torch.zeros(B, DSTAT, dtype=F32)
        for k, t in ((0, p * oh), (8, p * p), (16, oh)):
            st[:, k:k + n] = torch.from_numpy(_csum((t.reshape(B * n, S)), CHUNK, self.order, NT).astype(np.float32)).view(B, n)
        st[:, 24] = torch.from_numpy(_csum(-(oh * lp).sum(1), CHUNK, self.order, NT).astype(np.float32))
        return st

    def from_stats(self, c, z, lab, stats, S_total, snr, sdr, gscale, want_grad=True):
        B, n, S = z.shape
        f = np.float32
        st = stats.double()
        I, P, Cn, ce = st[:, :n], st[:, 8:8 + n], st[:, 16:16 + n], st[:, 24]
        loss = ((1 - (2 * I + float(f(snr))) / (P + Cn + float(f(sdr)))).mean() + ce.sum() / (B * S_total)).to(F32)
        if not want_grad:
            return loss, None
        p = self._p(z)
        oh = torch.nn.functional.one_hot(lab, n).movedim(-1, 1).float()
        wb, wce = f(1) / (f(B) * f(n)), f(1) / (f(B) * f(S_total))
        I, D = stats[:, :n], stats[:, 8:8 + n] + stats[:, 16:16 + n] + f(sdr)
        a, bq = (f(-2) / D * wb)[:, :, None], (f(2) * (f(2) * I + f(snr)) / (D * D) * wb)[:, :, None]
        g = a * oh + bq * p
        dot = torch.zeros_like(p[:, 0])
        for k in range(n):
            dot = dot + g[:, k] * p[:, k]
        return loss, (f(gscale) * (p * (g - dot[:, None]) + (p - oh) * wce)).to(c.dtype)

    def dice(self, c, z, lab, snr, sdr, gscale, want_grad=True):
        return self.from_stats(c, z, lab, self.stats(c, z, lab), z.shape[2], snr, sdr, gscale, want_grad)


class HipDice:
    name, dev = "hip", DEV

    def _put(self, c, z, lab):
        flat, shape, strides = _dice_buffer(c, z)
        buf = _carve(flat.to(F32).to(c.dtype), DEV)
        logits = buf.as_strided(shape, strides, buf.storage_offset())
        assert _ops().dice_strides(logits) == ((strides[0], strides[1], strides[2]) if not logits.is_contiguous() else (shape[1] * shape[2], shape[2], 1))
        return logits, _carve(lab, DEV, fill=7)

    def _grad(self, c, dl):
        """[B, n, S] on the host; the padding columns of a padded channels-last gradient must be zero bit for bit"""
        if dl is None:
            return None
        B, n, S = dl.shape
        if c.lay == "pad" and c.ld > n:
            raw = torch.as_strided(dl, (B, S, c.ld), (S * c.ld, c.ld, 1))
            assert bool((_bits(raw[..., n:]) == 0).all()), f"{c.id}: the padding columns of the gradient are not zero bit for bit"
        return dl.cpu().contiguous()

    def _twice(self, what, f):
        a, b = f(), f()
        _same([t for t in a if t is not None], [t for t in b if t is not None], what)
        return a

    def stats(self, c, z, lab):
        lg, lb = self._put(c, z, lab)
        return self._twice("dice_ce_stats", lambda: (_ops().dice_ce_stats(lg, lb),))[0].cpu()

    def from_stats(self, c, z, lab, stats, S_total, snr, sdr, gscale, want_grad=True):
        lg, lb = self._put(c, z, lab)
        st = _carve(stats, DEV)
        loss, dl = self._twice("dice_ce_from_stats", lambda: _ops().dice_ce_from_stats(lg, lb, st, S_total, snr, sdr, gscale, want_grad))
        assert torch.equal(st.cpu(), stats), "dice_ce_from_stats: the caller's statistics were rewritten"
        return loss.cpu(), self._grad(c, dl)

    def dice(self, c, z, lab, snr, sdr, gscale, want_grad=True):
        lg, lb = self._put(c, z, lab)
        loss, dl = self._twice("dice_ce", lambda: _ops().dice_ce(lg, lb, snr, sdr, gscale, want_grad))
        return loss.cpu(), self._grad(c, dl)


HOST_DICE = (EmuDice("seq"), EmuDice("pair"))
SMOOTH = ((1e-5, 1e-5, 1.0), (1.0, 0.5, 1.75))                    # (smooth_nr, smooth_dr, grad_scale): the default and another; Tier 1 scales by 1 / 4


def _s_total(S):
    """voxels of the whole sharded volume: the next power of two above S (2 S_total is then a power of two as well)"""
    return 1 << S.bit_length()


def run_dice(c, be):
    B, n, S, ou = 2, c.n, c.S, (U if c.dtype == F32 else UB)
    St = _s_total(S)
    pool = Pool(c.id, be)
    f32 = lambda v: float(np.float32(v))                           # noqa: E731
    for fam in ("int",) + REAL:
        g = _gen(c.id, fam)
        exact = fam == "int"
        z, lab = _dice_operands(c, fam, g)
        z2, lab2 = _dice_operands(c, fam, g, S=St - S)             # the rest of the sharded volume: only its sums matter
        for si, (snr, sdr, gs) in enumerate(SMOOTH):
            gs = 0.25 if exact and si else gs
            kw = dict(snr=f32(snr), sdr=f32(sdr), gscale=f32(gs))
            other = ref_dice(z2, lab2, n, **kw)["local"].to(F32)
            for sharded in ((False, True) if si else (False,)):
                skw = dict(other=other.double(), S_total=St) if sharded else {}
                ok = ref_dice(z, lab, n, **kw, **skw)
                wr = {"drop_class": ref_dice(z, lab, n, drop_class=True, **kw, **skw)}
                if S > 1:
                    wr["lab_shift"] = ref_dice(z, torch.roll(lab, 1, 1), n, **kw, **skw)
                    mis = _dice_misread(c, z)
                    wr["stride_swap"] = ref_dice(mis, lab, n, **kw, **skw)
                if sharded:
                    wr["S_total=S"] = ref_dice(z, lab, n, other=other.double(), S_total=S, **kw)
                    st = be.stats(c, z, lab)
                    lo, tl = ok["local"], ok["tlocal"]
                    if exact:             # I, P, C are integers: exact; the CE sum goes through __logf
                        ez = torch.exp(z - z.amax(1, keepdim=True))
                        assert bool(((ez == 1) | (ez < 2.0 ** -150)).all()) and bool((ok["p"] == ok["p"].round()).all()) and float(lo[:, :24].max()) < LIM, \
                            f"{c.id}: the exactness condition fails"
                        pool.check("dice_partial stats T1", fam, st[:, :24], lo[:, :24], 0.0, {k: w["local"][:, :24] for k, w in wr.items() if k != "S_total=S"})
                    else:
                        pool.check("dice_partial stats", fam, st[:, :24], lo[:, :24], _tol(lo[:, :24], tl[:, :24], U), {k: w["local"][:, :24] for k, w in wr.items() if k != "S_total=S"})
                    pool.check("dice_partial ce", fam, st[:, 24], lo[:, 24], _tol(lo[:, 24], tl[:, 24], U))
                    loss, grad = be.from_stats(c, z, lab, st + other, St, snr, sdr, gs)
                    kern = "dice_from_stats"
                else:
                    loss, grad = be.dice(c, z, lab, snr, sdr, gs)
                    l2, g2 = be.dice(c, z, lab, snr, sdr, gs, want_grad=False)
                    assert g2 is None and torch.equal(l2, loss), f"{c.id}: want_grad=False changes the loss"
                    kern = "dice_ce"
                pool.check(kern + " loss", fam, loss, ok["loss"], _tol(ok["loss"], ok["tloss"], 0.0), {k: w["loss"] for k, w in wr.items()})
                tot = B * (St if sharded else S)
                if exact and tot & (tot - 1) == 0:                # 0 on the correctly predicted voxels, +- grad_scale / (B S_total) on the others
                    step = kw["gscale"] / tot
                    assert bool(((ok["grad"] / step).round() == ok["grad"] / step).all()) and _fits32(ok["grad"]), f"{c.id}: the exactness condition fails"
                    wrong_vox = (ok["grad"] != 0).any(1).sum(1)
                    assert bool((wrong_vox >= min(S, 3)).all()) or n == 2 and S == 1, f"{c.id}: too few mispredicted voxels"
                    pool.check(kern + " grad T1", fam, grad, _once(ok["grad"], c.dtype), 0.0, {k: _once(w["grad"], c.dtype) for k, w in wr.items()})
                else:
                    pool.check(kern + " grad", fam, grad, ok["grad"], _tol(ok["grad"], ok["tgrad"], ou), {k: w["grad"] for k, w in wr.items()})
    pool.done(need=("drop_class", "S_total=S") + (("lab_shift", "stride_swap") if S > 1 else ()))
    return pool


@pytest.mark.parametrize("c", DICE, ids=_ids(DICE))
def test_dice_on_the_host(c):
    for be in HOST_DICE:
        run_dice(c, be)


@gpu
@pytest.mark.parametrize("c", DICE, ids=_ids(DICE))
def test_dice(c):
    run_dice(c, HipDice())


# ============================================================================================== refusals: loud, and nothing written
@gpu
def test_refusals_write_nothing():
    """the library's own entry checks (called as ops calls them, with every output a sentinel-filled buffer): the call returns an error and no
    output element changes; then the same refusals as ops raises them"""
    ops, lib = _ops(), _lib()
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    N = 1 << 16
    zb, zf = torch.zeros(N, dtype=BF, device=DEV), torch.zeros(N, dtype=F32, device=DEV)
    ones = torch.ones(N, dtype=F32, device=DEV)
    lab = torch.zeros(N, dtype=torch.int64, device=DEV)
    ws = torch.zeros(1 << 20, dtype=F32, device=DEV)
    ob = [torch.full((N,), SENT, dtype=BF, device=DEV) for _ in range(2)]       # every output of a refused call: bf16 ...
    of = [torch.full((N,), SENT, dtype=F32, device=DEV) for _ in range(3)]      # ... and fp32
    P = lambda t: t.data_ptr()            # noqa: E731
    BFC, F32C = ops.dt(zb), ops.dt(zf)

    def refused(what, rc):
        torch.cuda.synchronize()
        assert rc != 0, f"{what}: accepted"
        for t in ob + of:
            assert bool((t == SENT).all()), f"{what}: a refused call wrote to an output"
        assert bool((ws == 0).all()), f"{what}: a refused call wrote to the workspace"

    # S not a multiple of the vector width (8 bf16, 4 fp32)
    for S, z, code, o in ((12, zb, BFC, ob), (6, zf, F32C, of)):
        refused(f"instnorm_fwd S={S}", L.ucfvit_instnorm_fwd(P(z), None, P(o[0]), P(of[1]), P(of[2]), 6, S, EPS, SLOPE, P(ws), code, st))
        refused(f"instnorm_bwd S={S}", L.ucfvit_instnorm_bwd(P(z), P(z), P(z), P(zf), P(ones), P(o[0]), P(o[1]), 6, S, SLOPE, P(ws), code, st))
    # C not a power of two, C below 8
    for C in (24, 4, 12):
        a = (2, 8, C)
        refused(f"cl_stats C={C}", L.ucfvit_instnorm_cl_stats(P(zb), P(of[0]), P(of[1]), *a, EPS, P(ws), st))
        refused(f"cl_apply C={C}", L.ucfvit_instnorm_cl_apply(P(zb), P(zb), P(ob[0]), P(zf), P(ones), *a, SLOPE, st))
        refused(f"cl_apply2 C={C}", L.ucfvit_instnorm_cl_apply2(P(zb), P(zf), P(ones), P(zb), P(zf), P(ones), P(ob[0]), *a, SLOPE, st))
        refused(f"cl_bwd_sums C={C}", L.ucfvit_instnorm_cl_bwd_sums(P(zb), P(zb), P(zb), P(zf), P(ones), P(of[0]), P(of[1]), *a, 24, SLOPE, 1, P(ws), st))
        refused(f"cl_bwd_apply C={C}", L.ucfvit_instnorm_cl_bwd_apply(P(zb), P(zb), P(zb), P(zf), P(ones), P(zf), P(zf), P(ob[0]), P(ob[1]), *a, 24, SLOPE, 1, st))
        refused(f"cl_bwd2 C={C}", L.ucfvit_instnorm_cl_bwd2(P(zb), P(zb), P(zb), P(zf), P(ones), P(zb), P(zf), P(ones), P(ob[0]), P(ob[1]), *a, 24, SLOPE, P(ws), st))
    # ld_dy below C, ld_dy not a multiple of 8
    for ld in (8, 20):
        a = (2, 8, 16, ld)
        refused(f"cl_bwd_sums ld_dy={ld}", L.ucfvit_instnorm_cl_bwd_sums(P(zb), P(zb), P(zb), P(zf), P(ones), P(of[0]), P(of[1]), *a, SLOPE, 1, P(ws), st))
        refused(f"cl_bwd_apply ld_dy={ld}", L.ucfvit_instnorm_cl_bwd_apply(P(zb), P(zb), P(zb), P(zf), P(ones), P(zf), P(zf), P(ob[0]), P(ob[1]), *a, SLOPE, 1, st))
        refused(f"cl_bwd2 ld_dy={ld}", L.ucfvit_instnorm_cl_bwd2(P(zb), P(zb), P(zb), P(zf), P(ones), P(zb), P(zf), P(ones), P(ob[0]), P(ob[1]), *a, SLOPE, P(ws), st))
    # dres asked for although the forward pass added no residual
    refused("cl_bwd_apply dres without a residual",
            L.ucfvit_instnorm_cl_bwd_apply(P(zb), P(zb), P(zb), P(zf), P(ones), P(zf), P(zf), P(ob[0]), P(ob[1]), 2, 8, 16, 16, SLOPE, 0, st))
    # 1 class, 9 classes; S_total below S
    for n in (1, 9):
        s = (2, n, 64, n * 64, 64, 1)
        refused(f"dice_ce n={n}", L.ucfvit_dice_ce(P(zf), P(lab), P(of[0]), P(of[1]), *s, 1e-5, 1e-5, 1.0, P(ws), F32C, st))
        refused(f"dice_ce_stats n={n}", L.ucfvit_dice_ce_stats(P(zf), P(lab), P(of[0]), *s, P(ws), F32C, st))
        refused(f"dice_ce_from_stats n={n}", L.ucfvit_dice_ce_from_stats(P(zf), P(lab), P(of[0]), P(of[1]), P(of[2]), *s[:3], 64, *s[3:], 1e-5, 1e-5, 1.0, F32C, st))
    refused("dice_ce_from_stats S_total < S", L.ucfvit_dice_ce_from_stats(P(zf), P(lab), P(of[0]), P(of[1]), P(of[2]), 2, 4, 64, 63, 256, 64, 1, 1e-5, 1e-5, 1.0, F32C, st))
    # the same through ops
    x5 = lambda C, S=8: torch.zeros(2, 2, 2, S // 4, C, dtype=BF, device=DEV)     # noqa: E731
    v = lambda C: torch.ones(2, C, dtype=F32, device=DEV)                         # noqa: E731
    with pytest.raises(ValueError):
        ops.instnorm_fwd(torch.zeros(2, 3, 12, dtype=BF, device=DEV))
    with pytest.raises(ValueError):
        ops.instnorm_fwd(torch.zeros(2, 3, 6, dtype=F32, device=DEV))
    for C in (24, 4):
        with pytest.raises(lib.HipLibraryError):
            ops.instnorm_cl_stats(x5(C))
        with pytest.raises(lib.HipLibraryError):
            ops.instnorm_cl_apply(x5(C), v(C), v(C))
    with pytest.raises(lib.HipLibraryError):
        ops.instnorm_cl_bwd_apply(x5(16), x5(16), x5(16), v(16), v(16), v(16), v(16), SLOPE, True, False)
    for n in (1, 9):
        with pytest.raises(lib.HipLibraryError):
            ops.dice_ce(torch.zeros(2, n, 64, device=DEV), torch.zeros(2, 64, dtype=torch.int64, device=DEV))
    with pytest.raises(lib.HipLibraryError):
        ops.dice_ce_from_stats(torch.zeros(2, 4, 64, device=DEV), torch.zeros(2, 64, dtype=torch.int64, device=DEV), torch.zeros(2, DSTAT, device=DEV), 63)


# ============================================================================================== coverage of the case tables
def test_tables_reach_every_branch():
    """from the restated grid and chunk arithmetic: the cases reach every branch the docstring lists"""
    # row family: a single short chunk, one ragged below a full chunk, exactly one chunk, a ragged second chunk of one vector, three chunks
    for dt, V in (("f32", 4), ("bf16", 8)):
        S = sorted(c.S for c in ROWS if c.dt == dt)
        assert S == [V, CHUNK - 8, CHUNK, CHUNK + 8, 2 * CHUNK + 8] and all(s % V == 0 for s in S)
        assert [chunks_of(s) for s in S] == [1, 1, 1, 2, 3]
        assert {c.Cc for c in ROWS if c.dt == dt} == {3, 5}
    assert {(2048 + r - 1) // r for r in (6, 10)} == {342, 205} and {apply_grid(c.S, 2 * c.Cc) for c in ROWS} >= {1, 16, 17, 33}
    # channels-last: every channel-group stride, one vector row either side of a chunk, two chunks + 3, dense and sliced dy for every width
    for C in (8, 32, 64, 128, 256):
        cs = [c for c in CLS if c.C == C and not c.tag]
        cv = C // 8
        assert sorted(c.S * cv for c in cs) == [CLV - cv, CLV, CLV + cv, 2 * CLV + 3 * cv]
        assert sorted(cl_chunks_of(c.S, C) for c in cs) == [1, 1, 2, 3]
        assert {c.ldy > C for c in cs} == {True, False} and all(c.ldy % 8 == 0 and c.off % 8 == 0 and c.off + C <= c.ldy for c in cs)
        assert {(c.ldy > C, cl_chunks_of(c.S, C) > 1) for c in cs} >= {(True, True), (True, False), (False, True), (False, False)}
        assert NT % cv == 0 and CLV % cv == 0                      # what the threadIdx.x % cv ownership rests on
        assert all(fold_plan(cl_chunks_of(c.S, C), C)[0] == 1 for c in cs)
    assert any(c.S * c.cv < NT for c in CLS if c.tag == "onegroup")
    assert all(cl_apply_grid(c.S, c.C, 2) < 2048 for c in CLS)      # the grid cap is out of reach of small shapes: tests/test_decoder_full_volume.py
    assert {c.C for c in WIDE} == {512, 2048} and all(c.C > NT and fold_plan(10 ** 6, c.C)[0] == 1 for c in WIDE)
    assert [fold_plan(cl_chunks_of(c.S, c.C), c.C) for c in FOLD] == [(1, 512, 1), (2, 3, 171)]
    assert fold_plan(GCAP_ROWS, 8) == (2, 256, 258) and -(-GCAP_ROWS // 256) > 256
    assert [(h, w) for _, h, w in BWD_APPLY] == [(True, True), (True, False), (False, False)]
    # Dice + CE
    assert [chunks_of(s) for s in DICE_S] == [1, 1, 1, 2, 4] and DICE_S[2] == CHUNK
    for n in DICE_N:
        assert {c.lay for c in DICE if c.n == n} == {"nc", "cl", "pad"} and {c.dt for c in DICE if c.n == n} == {"f32", "bf16"}
    for S in DICE_S:
        assert {c.n for c in DICE if c.S == S} == set(DICE_N) and {c.dt for c in DICE if c.S == S} == {"f32", "bf16"}
    assert {(c.lay, c.dt) for c in DICE} == {(a, b) for a in ("nc", "cl", "pad") for b in ("f32", "bf16")}
    assert any(c.lay == "pad" and c.ld > c.n for c in DICE) and all(_s_total(c.S) > c.S for c in DICE)


def test_zz_ratios_report():
    """last test of the file: the worst err / bound per kernel seen by this process (emulation without a GPU, the library with one)"""
    for k in sorted(RATIOS):
        print(f"RATIO SUMMARY {k}: {RATIOS[k]:.3f}")
    assert all(r <= 1.0 for r in RATIOS.values())
