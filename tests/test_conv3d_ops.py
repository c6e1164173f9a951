"""Every kernel of csrc/conv3d.hip that can serve a launch, against float64 references of the same rounded operands, element by element,
through UCF_VIT._hip.ops and UCF_VIT._hip.conv.  The references never call the project's kernels: a convolution is 27 shifted slices of a
zero-padded float64 volume, each times the tap's [Cin, Cout] matrix (_conv64); a weight gradient is the matching 27 products (_wgrad64).
U = 2^-24 (fp32 unit roundoff), UB = 2^-8 (bf16).  All operands are drawn on the CPU (the same values with and without a GPU).

Routing (_plan restates conv_fwd_route of csrc/conv_route.h, _wplan restates conv_wgrad_route; neither calls the library).  Asserted against
the library for every case under every UCFVIT_CONV_STRIP value: ucfvit_conv3d_fwd_stats_rows is > 0 exactly when the kind is 1 or 2 and
equals ceil(X/TX) ceil(Y/TY) 4 for the restated tile, ucfvit_conv3d_wgrad_workspace equals n_wg SLOTS n_out 4 with the restated n_wg
(test_conv_route_queries_every_mode: one child per value, the hook is read once per process; test_conv_wgrad_plan_...); the text of
ucfvit_conv3d_route, which takes the hook value as an argument, equals the restated plan for every (case, epilogue, mode) in one process
(test_conv_route_text_equals_the_restated_plan, test_conv_wgrad_route_text_equals_the_restated_plan).  Branches and the
cases that reach them (test_conv_table_reaches_every_branch asserts this list from the restated plans):
    tile  conv_fwd_kernel            hook 0 and the default at small sizes: every entry of the table.  CPC 8 / 16 / 32 x KS 3 / 1 (the 17 channel
                                     pairs of _COMBOS), NB 4 / 2 / 1 (Cout 64, 32, 16 and 48), multi-chunk Cin 64 / 128 / 256 (the "mc" shapes and two
                                     pointwise ones), bf16 and fp32 output; Z 1, 15, 16 stay on it under every hook value
    strip-fast[-share]               hook 2: DEPTH 2 for CPC 8 / 16, DEPTH 1 for CPC 32; tiles (2,4) Cout 64, (2,8) Cout 32 and CPC 32 with Cout 16 / 48,
      conv_fwd_strip_kernel<FAST>    (4,8) CPC 8 / 16 with Cout 16 / 48; SHARE = every 16-channel 3x3x3 one; KS 1; Z 17, 31, 32, 33, 53 (2 .. 4 z tiles, ragged last
                                     one, DEPTH 2 prefetching beyond the last tile); `slice` (ldy = Cout + 8) keeps FAST with ldy != Cout
    strip-branching[-share]          hook 3: the same table; hook 2: cout_store 3, 5 (= 4 + 1), Cout - 11 (= Cout - 12 + 1) and `slice_odd` (row stride a
      conv_fwd_strip_kernel<!FAST>   multiple of 8, cout_store = Cout - 3)
    mc1 / mc2 / mc4                  hooks 2 and 3: Z 16 / 32 / 64, Cin 64 / 128 / 256, Cout 32 / 64 / 128, X 5 / 3 / 1, Y 11 / 7 / 9 / 1; with bias, fp32, a slice or
      conv3_fwd_mc_kernel<TZT>       Cout 48 the same shapes fall back to the tile kernel, and so does Z = 48 (MC48: asserted)
    default selection, in-process    SEL: 2x32x128x24 16->16 (512 columns: strip-fast-share (4,8)), 2x32x120x24 (480: tile), 2x16x128x16 64->64 (512
                                     workgroups: mc1), 2x16x120x16 (tile), 2x64x72x17 8->16 k1 (576 statistics rows per batch element: the two-stage fold)
    epilogues (EPIS), every one on every family that accepts it: bias, cout_store < Cout, out= channel slice, fp32, accumulate_into (bf16, fp32,
                                     with bias), the statistics by-product (with and without bias)
    weight gradient conv_wgrad_kernel   MB 2 / 1 x CPC 8 / 16 / 32 x KS 3 / 1 (SLOTS 4); tiles_per_wg = 2 at 2x8x12x40 256->128 (48 tiles, 24 workgroups
                                     under the partial-sum cap) and at 2x34x64x33 (1088 tiles, the 1024-workgroup cap) for KS 3 and KS 1, n_wg < tiles read
                                     from the workspace QUERY; role-swapped conv.conv3_wgrad (32->16, 64->16) and conv._pointwise_wgrad (32->8);
                                     Z 31, 32, 33, 40, 65; extent 1 on X and on Y
    around them                      tconv2x2x2 on the 1x1x1 kernel (32->8, 16->16) and the GEMM (768->32, 128->64), with skip; tconv1x1x1 with and without skip;
                                     conv1x1x1 small (fp32 logits of 3 and 4 channels with bias, 8->16, 256->32) and on the GEMM (128->128 with bias, 256->128
                                     fp32); depth_to_space2 / space_to_depth2 into and out of channel slices with skip; pad_channels8 / pad_rows8
                                     (torch.equal: exact rearrangements)
Shapes: B = 2 (a halo that runs off one batch element lands in the next); X in {1, 3, 5}, Y in {1, 7, 9, 11}, Z around the tile edges;
extent 1 on every axis once per family (every tap on that axis is padding); nothing near 512 x 512 x 128.

Tier 1, exact.  Operands and weights are integers, {-1, 0, 1} ("int") and {+-3, +-4} ("big": most 3x3x3 sums exceed 256, so the bf16 rounding
is pinned); bias and base are integers in [-4, 4].  The exactness condition — |x| conv |w| + |bias| + |base| < 2^24 behind every accumulator,
for the weight gradient over all voxels — is computed in float64 from the operands used and asserted.  fp32 outputs and every weight gradient
are equal to the float64 result, bf16 outputs bit-equal to it rounded ONCE, accumulate_into = bf16(base + bias + sum).  Wrong alternatives
formed on the host, shown (also without a GPU: test_conv_tier1_wrong_references_differ_on_the_host) to differ from the right result in all six
faces and in the first / last z-tile band, and shown to differ from what the kernel wrote: the taps mirrored, the volume shifted by one voxel
on each axis, edge replication instead of zero padding, the last input channel dropped, the last 32-channel chunk dropped (Cin > 32), the
bias of the neighbouring channel, the twice-rounded result (3x3x3 with Cin >= 16 and all channels stored: below that fan-in the sums stay
under 256 and both roundings agree).  Weight gradient: taps mirrored, x and dy offset by one voxel on each axis, edge replication, the last z
plane left out.  Symmetries bit for bit: a second call; hook 0 against 2 against 3 for every non-SHARE instantiation and 2 against 3 for the
SHARE ones (test_conv_forced_modes_agree, on real-valued operands); the fused unet_res_block forward against the chain of layer functions.

Tier 2, per-element bounds on real-valued operands (x: randn; randn + 8 sigma; randn times 2^-20 .. 2^20; weights randn at the layers' scale
sqrt(2 / fan-in)):     |got - ref| <= t + ou (|ref| + t),   ou = UB (bf16 output) or U (fp32),   t = d U (|x| conv |w|) + U |v| per epilogue addition.
d is the longest fp32 addition chain of the kernel that serves the case, read off that kernel (the GEMM convention: one
v_mfma_f32_16x16x32_bf16 counts as 32 additions, then one per further MFMA into the same accumulator):
    forward, every kernel: d = steps + 32 with steps = K / 32, K = taps x Cin AS PADDED: per 32-channel chunk 27 (CPC 32), 14 (CPC 16), 7 (CPC 8)
        steps at KS 3 and 1 at KS 1, times Cin / CPC chunks; the SHARE arrangement has 15 steps.  The column kernels and the multi-chunk kernel
        keep one accumulator per output over all chunks: the same d.
    weight gradient: one MFMA (32 voxels along z) per (x, y) row of a tile: 8 rows a tile at KS 3, 2 per wave at KS 1, over tiles_per_wg tiles,
        then ucfvit_reduce_rows over n_wg x SLOTS partial rows: d = (8 | 2) tiles_per_wg + 32 + n_wg SLOTS.
    the GEMM routes of tconv2x2x2 / conv1x1x1: ceil(K / 32) + 32 (tests/test_gemm_ops.py), + 8 for the weight gradient, which may split K.
Every comparison goes through Pool.check: each applicable wrong reference above must be rejected by at least one family, in every (case,
epilogue); no case opts out.  The twice-rounded result is not a Tier 2 reference: it lies within one bf16 ulp of the right one, inside any
bound that admits a correctly rounded output — Tier 1 shows it.  The bias of the neighbouring channel cannot show in the 2^-20 .. 2^20
family under bf16 rounding (|ref| reaches 2^20), the randn family shows it.  Statistics by-product: the contract of tests/test_conv3d.py (mean
within 1e-4 of the output's spread, rstd within 1e-4 relative, against the float64 statistics of the STORED output) on every statistics launch
of the randn and offset families and of Tier 1, on every column-kernel instantiation, with a bias, and through the two-stage fold.

Guards.  x, dy, packed weights, bias and base are carved from the middle of NaN-filled allocations (128 bytes in front: 16-byte aligned);
results must be NaN-free.  Outputs are views into sentinel buffers wherever ops lets the caller own the output: every bf16 launch through
out= (two sentinel rows behind the last voxel, the channels cout_store .. ld of every row) and every accumulate_into (sentinels around the
base); every sentinel is untouched bit for bit — the FAST kernels' range-limited stores stay inside one batch element, the scalar store path
writes exactly cout_store channels.  Refusals pinned: unsupported Cin, Cout not a multiple of 16, statistics on a non-dense output (ops and
the library itself), statistics handed to a launch without an epilogue — and a refused launch writes nothing.
Not covered: sentinels around fp32 outputs without accumulation, the dense cout_store = 3 output and the statistics launches (ops allocates
those itself); statistics at Cout = 48 (ucfvit_instnorm_cl_stats needs a power of two and says so); the 4 GB limit of the FAST predicate and
extents beyond 2^31 (no small shape reaches them; tests/test_decoder_full_volume.py runs the workload's volume); the instance-norm and Dice
kernels (their own files).

Forced modes: UCFVIT_CONV_STRIP = 0, 2, 3 each run the forced table (48 cases, both tiers) in one fresh child (subprocess.run, return code
checked, no further child after a failure); the children save the outputs of four epilogues, the parent compares the Tier 1 ones with the
float64 reference computed in the parent and the real-valued ones with each other.

Finding.  The hook value 3 could not do what the source said: the forward plan (conv_fwd_route today) tested the hook for == 2, so under 3 the column kernels were chosen by
size as under the default, and no shape of a test's size reached conv_fwd_strip_kernel<FAST = false> that way.  csrc/conv3d.hip now forces
the column kernels for 2 and 3 alike (the default and 0 are unchanged).  With that, the branching kernel passed both tiers at first run,
bit-identical to the FAST one.  No defect found in any kernel: no ratio above 1, no sentinel touched, no NaN.

Measured on an MI355X: 170 GPU tests + 11 CPU tests, 45 s for the file; a forced child takes 5.2 - 6.0 s (most of it the start of
python and torch), a route-query child 1.9 - 3.3 s, a quarter of the host half of Tier 1 1.6 - 3.9 s; the child timeouts are ten times the
measured run (60 s, 30 s).  Every other test stays below one second.
Mutation check (nothing of it committed): with one tap of every 3x3x3 weight zeroed inside pack_conv_weight, test_conv_fwd_exact and
test_conv_fwd_bounds failed on every 3x3x3 case tried (18 of 18, tile, column, multi-chunk and selection cases alike); the fused-block
symmetry passed, as it must: both of its sides pack the same weights.
  worst err / bound                 bf16 out   fp32 out
  tile (hooks 0, 1, 2, 3)           0.996      0.347
  strip-fast / strip-branching      0.996      0.337
  strip-*-share                     0.995      0.123
  mc1 / mc2 / mc4                   0.991 / 0.979 / 0.991
  weight gradient KS 3 / KS 1                  0.094 / 0.044      role-swapped 0.047 / 0.010
  tconv2x2x2 kernel / GEMM          0.993 / 0.992 fwd, 0.983 / 0.992 dx       0.011 / 0.041 dw
  tconv1x1x1                        0.993 fwd, 0.992 dx                       0.009 dw
  conv1x1x1 kernel / GEMM           0.991 / 0.992 fwd, 0.994 dx               0.028 / 0.041 fwd fp32, 0.004 / 0.012 dw
  statistics by-product             mean 1.1e-6 of the spread, rstd 8.9e-6 relative (contract: 1e-4)
bf16 outputs sit at the bound because the bound there IS the output rounding; the fp32 outputs show the accumulation itself, a third of the
worst-case chain bound at most.
"""
import os
import subprocess
import sys
import time
from dataclasses import dataclass

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
LIM = 2.0 ** 24
BF, F32 = torch.bfloat16, torch.float32
SENT = -12352.0                   # sentinel of output padding (exact in bf16 and fp32)
PAD = 64                          # NaN / sentinel elements in front of and behind every carved operand (128 bytes of bf16: 16-byte aligned)
EPS = 1e-5
CHILD_TIMEOUT = 60                # seconds: ten times the measured 5.2 - 6.0 s of a forced child (see "Measured" in the docstring)
ROUTE_TIMEOUT = 30                # ten times the 1.9 - 3.3 s of a route-query child


def _ops():
    from UCF_VIT._hip import ops
    return ops


def _conv():
    from UCF_VIT._hip import conv
    return conv


def _cdiv(a, b):
    return -(-a // b)


def _mode():
    """strip_mode() of csrc/conv3d.hip"""
    e = os.environ.get("UCFVIT_CONV_STRIP")
    return int(e[0]) if e and "0" <= e[0] <= "3" else 1


# ============================================================================================== epilogues and cases
@dataclass(frozen=True)
class Epi:
    name: str
    out32: bool = False
    bias: bool = False
    cs: int = 0              # cout_store: 0 = Cout, > 0 that many, < 0 Cout + cs
    ldx: object = None       # None: ops allocates the output; k: out= is a channel slice of a sentinel buffer ceil8(cout_store) + k wide
    acc: bool = False
    stats: bool = False

    def cs_of(self, c):
        return c.cout if self.cs == 0 else (self.cs if self.cs > 0 else c.cout + self.cs)

    def ld_of(self, c):
        cs = self.cs_of(c)
        return cs if self.ldx is None else _cdiv(cs, 8) * 8 + self.ldx


EPIS = {e.name: e for e in (
    Epi("plain", ldx=0),                               # dense bf16 through out=: the rows behind the last voxel are sentinels
    Epi("o32", out32=True),
    Epi("bias", bias=True, ldx=0),
    Epi("bias_o32", bias=True, out32=True),
    Epi("cs3", cs=3),                                  # ldy = 3: no vector store at all
    Epi("cs3_ld8", cs=3, ldx=0),                       # ldy = 8, 3 channels stored: channels 3..7 of every row are sentinels
    Epi("cs5_ld8", cs=5, bias=True, ldx=0),            # 4 + 1: one vector group and one scalar channel
    Epi("csm11_o32", cs=-11, bias=True, out32=True),   # Cout - 12 + 1, fp32, ldy odd
    Epi("slice", ldx=8),                               # Cout channels of a buffer Cout + 8 wide
    Epi("slice_odd", cs=-3, ldx=0),                    # row stride a multiple of 8, cout_store not a multiple of 4
    Epi("acc", acc=True),
    Epi("acc_o32", acc=True, out32=True),
    Epi("acc_bias", acc=True, bias=True),
    Epi("stats", stats=True),
    Epi("stats_bias", stats=True, bias=True),
)}
ALL = tuple(EPIS)
FEW = ("plain", "acc", "stats")
SAVE_EPIS = ("plain", "bias_o32", "acc", "cs5_ld8")   # what a forced child hands to its parent


@dataclass(frozen=True)
class FC:
    fam: str                 # the family the case is in the table for: tile, strip, mc, sel (default-mode selection by size)
    B: int
    X: int
    Y: int
    Z: int
    cin: int
    cout: int
    ks: int = 3
    epis: tuple = ALL
    forced: bool = True      # part of the table the forced children run

    @property
    def id(self):
        return f"{self.fam}-{self.B}x{self.X}x{self.Y}x{self.Z}-{self.cin}to{self.cout}-k{self.ks}"

    @property
    def shape(self):
        return (self.B, self.X, self.Y, self.Z)


def _epis(c):
    """the statistics epilogues need a power-of-two Cout (ucfvit_instnorm_cl_stats and the apply kernels refuse any other, loudly)"""
    return tuple(en for en in c.epis if not (EPIS[en].stats and c.cout & (c.cout - 1)))


@dataclass(frozen=True)
class Plan:
    kind: int                # 0 conv_fwd_kernel, 1 conv_fwd_strip_kernel, 2 conv3_fwd_mc_kernel
    TX: int
    TY: int
    NB: int
    steps: int               # 32-wide MFMA steps behind one accumulator
    fast: bool = False
    depth: int = 1
    share: bool = False
    tzt: int = 0

    @property
    def name(self):
        if self.kind == 0:
            return "tile"
        if self.kind == 2:
            return f"mc{self.tzt}"
        return "strip-" + ("fast" if self.fast else "branching") + ("-share" if self.share else "")


def _plan(c, e, mode):
    """conv_fwd_route of csrc/conv_route.h, restated"""
    cpc, nb16 = min(c.cin, 32), c.cout // 16
    nch = c.cin // cpc
    cs, ldy = e.cs_of(c), e.ld_of(c)
    NB = 4 if nb16 % 4 == 0 else 2 if nb16 % 2 == 0 else 1
    nts = 1 if c.ks == 1 else {8: 7, 16: 14, 32: 27}[cpc]
    if (cpc == 32 and c.ks == 3 and not e.out32 and c.cin > 32 and not e.bias and c.cout % 32 == 0 and cs == c.cout and ldy == c.cout and mode
            and c.Z in (16, 32, 64)):
        wgs = c.B * _cdiv(c.X, 2) * _cdiv(c.Y, 8) * (c.cout // 32)
        if mode >= 2 or wgs >= 512:
            return Plan(2, 2, 8, 2, 27 * nch, tzt=c.Z // 16)
    if c.cin == cpc and c.Z > 16 and mode:
        cols = c.B * _cdiv(c.X, 2) * _cdiv(c.Y, 8)
        f = nb16 // 4 if nb16 % 4 == 0 else nb16 // 2 if nb16 % 2 == 0 else nb16
        if mode >= 2 or cols * f >= 512:
            tx, ty = (2, 4) if nb16 % 4 == 0 else (2, 8) if (nb16 % 2 == 0 or cpc == 32) else (4, 8)
            vox, lim = c.X * c.Y * c.Z, 2 ** 32 - 64
            fast = ldy % 4 == 0 and cs % 4 == 0 and vox * c.cin * 2 < lim and vox * ldy * (4 if e.out32 else 2) < lim and mode != 3
            share = c.ks == 3 and cpc == 16
            return Plan(1, tx, ty, NB, 15 if share else nts, fast=fast, depth=2 if (fast and cpc <= 16) else 1, share=share)
    tx, ty = (2, 4) if NB == 4 else (2, 8)
    return Plan(0, tx, ty, NB, nts * nch)


def _stats_rows(c, bias, mode):
    """ucfvit_conv3d_fwd_stats_rows restated: the dense bf16 launch of the case"""
    p = _plan(c, Epi("q", bias=bias), mode)
    return _cdiv(c.X, p.TX) * _cdiv(c.Y, p.TY) * 4 if p.kind else 0


@dataclass(frozen=True)
class WC:
    B: int
    X: int
    Y: int
    Z: int
    cin: int
    cout: int
    ks: int = 3
    via: str = "ops"         # ops: ops.conv3d_wgrad + unpack; conv3: conv.conv3_wgrad; pw: conv._pointwise_wgrad

    @property
    def id(self):
        return f"wgrad-{self.via}-{self.B}x{self.X}x{self.Y}x{self.Z}-{self.cin}to{self.cout}-k{self.ks}"

    @property
    def swapped(self):
        return (self.via == "conv3" and self.cout == 16 and self.cin >= 32) or (self.via == "pw" and self.cout % 16 != 0)

    @property
    def kdims(self):
        """(Cin, Cout) as the kernel sees them"""
        return (self.cout, self.cin) if self.swapped else (self.cin, self.cout)


def _wplan(c):
    """conv_wgrad_route of csrc/conv_route.h restated -> dict(MB, cpc, tiles, n_wg, tpw, slots, n_out, d)"""
    kin, kout = c.kdims
    cpc = min(kin, 32)
    MB = 2 if kout % 32 == 0 else 1
    nbk = cpc // 16 if cpc >= 16 else 1
    tiles = c.B * _cdiv(c.X, 2) * _cdiv(c.Y, 4) * _cdiv(c.Z, 32)
    gy = (kin // cpc) * (kout // (16 * MB))
    nt, slots = (27, 1) if c.ks == 3 else (1, 4)
    n_out = gy * nt * 16 * MB * 16 * nbk
    cap = max(1, min(1024, (32 << 20) // (n_out * slots)))
    n_wg = min(tiles, cap)
    tpw = _cdiv(tiles, n_wg)
    n_wg = _cdiv(tiles, tpw)
    # one MFMA (32 voxels along z) per (x, y) row of a tile and accumulator: 8 rows a tile (KS 3), 2 per wave (KS 1); then the fold
    d = (8 if c.ks == 3 else 2) * tpw + 32 + n_wg * slots
    return dict(MB=MB, cpc=cpc, tiles=tiles, n_wg=n_wg, tpw=tpw, slots=slots, n_out=n_out, d=d)


# ---------------------------------------------------------------------------------------------- the tables
FWD = []
_SHAPES = [(2, 5, 11, 53), (2, 3, 7, 17), (2, 5, 9, 33), (2, 1, 7, 32), (2, 3, 1, 31), (2, 5, 11, 1), (2, 3, 9, 15), (2, 3, 7, 16)]
_COMBOS = [(8, 16, 3), (16, 16, 3), (32, 16, 3), (16, 32, 3), (32, 32, 3), (8, 64, 3), (16, 64, 3), (32, 64, 3), (16, 48, 3), (8, 32, 3), (32, 48, 3),
           (8, 16, 1), (16, 32, 1), (32, 64, 1), (32, 48, 1), (16, 16, 1), (8, 64, 1)]
for _i, (_ci, _co, _ks) in enumerate(_COMBOS):
    # every single-chunk instantiation on a shape with several z tiles (column kernels under 2 / 3) ...
    FWD.append(FC("strip", *[(2, 5, 11, 53), (2, 3, 7, 17), (2, 5, 9, 33), (2, 1, 7, 32), (2, 3, 1, 31)][_i % 5], _ci, _co, _ks))
    # ... and on one that stays on the tile kernel in every mode (Z <= 16)
    FWD.append(FC("tile", *[(2, 5, 11, 1), (2, 3, 9, 15), (2, 3, 7, 16)][_i % 3], _ci, _co, _ks, epis=("plain", "bias_o32", "cs5_ld8", "acc", "stats")))
# SHARE and DEPTH 2 beyond the last tile: odd tile counts (Z 17: 2 tiles, 33: 3, 53: 4) for the 16-channel 3x3x3 column kernel at every tile
for _co, _z in ((16, 17), (32, 53), (64, 33), (16, 32)):
    FWD.append(FC("strip", 2, 3, 9, _z, 16, _co, 3, epis=("plain", "bias", "acc", "stats", "slice", "slice_odd")))
# multi-chunk: the column kernel at TZT 1 / 2 / 4 under 2 / 3, the tile kernel otherwise; odd X, Y not a multiple of 8
for _ci, _co, _z, _xy in ((64, 32, 16, (5, 11)), (128, 64, 32, (3, 7)), (256, 32, 64, (1, 9)), (64, 64, 64, (3, 1)), (256, 128, 16, (3, 7)),
                          (128, 32, 33, (3, 7)), (64, 48, 32, (3, 7))):
    FWD.append(FC("mc", 2, _xy[0], _xy[1], _z, _ci, _co, 3, epis=("plain", "acc", "stats", "bias", "o32", "cs5_ld8", "slice")))
MC48 = FC("mc", 2, 3, 7, 48, 64, 64, 3, epis=("plain", "acc", "stats"))          # Z = 48: not eligible, falls back to the tile kernel
FWD.append(MC48)
FWD.append(FC("tile", 2, 3, 7, 16, 64, 16, 1, epis=("plain", "bias_o32", "acc")))       # multi-chunk pointwise (the data gradient of a tconv)
FWD.append(FC("tile", 2, 3, 7, 33, 128, 32, 1, epis=("plain", "bias_o32", "acc")))
# default-mode selection by size (the 512-workgroup thresholds), in-process only
SEL = [FC("sel", 2, 32, 128, 24, 16, 16, 3, epis=FEW, forced=False),        # 512 columns: conv_fwd_strip_kernel (4, 8), SHARE
       FC("sel", 2, 32, 120, 24, 16, 16, 3, epis=FEW, forced=False),        # 480: stays on the tile kernel
       FC("sel", 2, 16, 128, 16, 64, 64, 3, epis=FEW, forced=False),        # 512 workgroups: conv3_fwd_mc_kernel<1>
       FC("sel", 2, 16, 120, 16, 64, 64, 3, epis=FEW, forced=False),        # 480: tile kernel
       FC("sel", 2, 64, 72, 17, 8, 16, 1, epis=("plain", "stats", "stats_bias"), forced=False)]   # 576 statistics rows per batch element: two-stage fold
FWD += SEL

WGRAD = [WC(2, 5, 11, 33, 8, 16), WC(2, 3, 7, 65, 16, 32), WC(2, 1, 9, 32, 32, 48), WC(2, 3, 1, 31, 64, 32), WC(2, 5, 7, 33, 16, 16),
         WC(2, 3, 7, 33, 8, 32), WC(2, 8, 12, 40, 256, 128),                                         # the partial-sum cap: tiles_per_wg > 1 at a small volume
         WC(2, 34, 64, 33, 8, 16),                                           # more than 1024 tiles: tiles_per_wg = 2 under the other cap
         WC(2, 5, 11, 33, 8, 16, 1), WC(2, 3, 7, 65, 16, 32, 1), WC(2, 1, 9, 32, 32, 16, 1), WC(2, 3, 1, 31, 64, 64, 1),
         WC(2, 34, 64, 33, 16, 32, 1),                                       # KS 1, tiles_per_wg = 2, SLOTS = 4
         WC(2, 3, 7, 33, 32, 16, via="conv3"), WC(2, 3, 7, 31, 64, 16, via="conv3"), WC(2, 3, 7, 33, 16, 32, via="conv3"),
         WC(2, 3, 7, 33, 32, 8, 1, via="pw"), WC(2, 3, 7, 33, 16, 16, 1, via="pw")]


# ============================================================================================== operands
def _values(g, kind, shape, scale=1.0):
    if kind == "int":
        v = torch.randint(-1, 2, shape, generator=g).double()
    elif kind == "int4":
        v = torch.randint(-4, 5, shape, generator=g).double()
    elif kind == "big":
        v = torch.tensor([-4.0, -3.0, 3.0, 4.0], dtype=torch.float64)[torch.randint(0, 4, shape, generator=g)]
    else:
        v = torch.randn(shape, generator=g, dtype=torch.float32).double() * scale
        if kind == "offset":
            v = v + 8.0 * scale
        if kind == "exp":
            v = v * torch.exp2(torch.randint(-20, 21, shape, generator=g).double())
    return v


def _carve(vals, fill, dev):
    """vals as a view into the middle of a larger allocation filled with `fill` -> (buffer, view)"""
    n = vals.numel()
    buf = torch.full((n + 2 * PAD,), fill, dtype=vals.dtype, device=dev)
    buf[PAD:PAD + n] = vals.reshape(-1).to(dev)
    return buf, buf[PAD:PAD + n].view(vals.shape)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


class O:
    pass


def _seed(c, kind):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id + kind)) % (2 ** 31)


def _fwd_operands(c, kind, dev):
    """the same values on every device: drawn on the CPU.  Weights at the layers' scale sqrt(2 / fan-in); everything rounded to bf16 first."""
    g = torch.Generator().manual_seed(_seed(c, kind))
    exact = kind in ("int", "big")
    nt = c.ks ** 3
    o = O()
    x = _values(g, kind, c.shape + (c.cin,)).to(BF)
    w = _values(g, kind if exact else "randn", (c.cout, c.cin, c.ks, c.ks, c.ks), 1.0 if exact else (2.0 / (nt * c.cin)) ** 0.5).to(BF)
    bias = _values(g, "int4" if exact else "randn", (c.cout,), 0.5).to(BF)
    base = _values(g, "int4" if exact else "randn", c.shape + (c.cout,)).to(BF)
    nan = float("nan")
    _, o.x = _carve(x, nan, dev)
    _, o.wp = _carve(_conv().pack_conv_weight(w.float()), nan, dev)
    _, o.bias = _carve(bias.float(), nan, dev)
    o.x64, o.w64, o.bias64, o.base64 = x.double().to(dev), w.double().to(dev), bias.double().to(dev), base.double().to(dev)
    return o


# ============================================================================================== float64 references
def _padded(x, mode):
    B, X, Y, Z, C = x.shape
    if mode == "zero":
        xp = x.new_zeros((B, X + 2, Y + 2, Z + 2, C))
        xp[:, 1:-1, 1:-1, 1:-1] = x
        return xp
    ix = [torch.arange(-1, n + 1, device=x.device).clamp(0, n - 1) for n in (X, Y, Z)]       # edge replication
    return x[:, ix[0]][:, :, ix[1]][:, :, :, ix[2]]


def _conv64(x, w, mode="zero"):
    """27 shifted slices of the padded volume, each times the tap's [Cin, Cout] matrix (1x1x1: one product)"""
    if w.shape[2] == 1:
        return x @ w[:, :, 0, 0, 0].T
    B, X, Y, Z, _ = x.shape
    xp = _padded(x, mode)
    out = x.new_zeros((B, X, Y, Z, w.shape[0]))
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                out += xp[:, dx:dx + X, dy:dy + Y, dz:dz + Z] @ w[:, :, dx, dy, dz].T
    return out


def _wgrad64(x, dy, ks, mode="zero"):
    """[Cout, Cin, k, k, k]: the matching 27 products dy^T x(shifted)"""
    cin, cout = x.shape[-1], dy.shape[-1]
    d2 = dy.reshape(-1, cout).T
    if ks == 1:
        return (d2 @ x.reshape(-1, cin)).reshape(cout, cin, 1, 1, 1)
    B, X, Y, Z, _ = x.shape
    xp = _padded(x, mode)
    if cin <= 16:             # the same 27 products in one call, the shifted slices side by side: 27 skinny float64 products are slow
        cols = torch.cat([xp[:, dx:dx + X, dyy:dyy + Y, dz:dz + Z].reshape(-1, cin) for dx in range(3) for dyy in range(3) for dz in range(3)], 1)
        return (d2 @ cols).reshape(cout, 27, cin).permute(0, 2, 1).reshape(cout, cin, 3, 3, 3)
    out = x.new_zeros((cout, cin, 3, 3, 3))
    for dx in range(3):
        for dyy in range(3):
            for dz in range(3):
                out[:, :, dx, dyy, dz] = d2 @ xp[:, dx:dx + X, dyy:dyy + Y, dz:dz + Z].reshape(-1, cin)
    return out


GEOM = ("mirror", "shift_x", "shift_y", "shift_z", "replicate", "drop_ch", "drop_chunk")


def _fwd_refs(c, o, wrongs=True):
    """the right sums, |x| conv |w|, and the sums of every applicable wrong alternative"""
    R = {"ok": _conv64(o.x64, o.w64), "abs": _conv64(o.x64.abs(), o.w64.abs())}
    if not wrongs:
        return R
    if c.ks == 3:
        R["mirror"] = _conv64(o.x64, o.w64.flip(2, 3, 4))
        R["replicate"] = _conv64(o.x64, o.w64, "replicate")
    for ax, n in (("x", 1), ("y", 2), ("z", 3)):
        if o.x64.shape[n] > 1:
            R["shift_" + ax] = _conv64(o.x64.roll(1, n), o.w64)
    R["drop_ch"] = R["ok"] - _conv64(o.x64[..., -1:], o.w64[:, -1:])
    if c.cin > 32:
        R["drop_chunk"] = R["ok"] - _conv64(o.x64[..., -32:], o.w64[:, -32:])
    return R


def _epi(c, e, o, S, A=None, d=0, variant="ok"):
    """the epilogue in the kernels' order (sum, + bias, + the values accumulated onto, one rounding) -> (value, tol) in float64"""
    v = S
    t = d * U * A if A is not None else None
    b = o.bias64.roll(1) if variant == "bias_shift" else o.bias64
    if variant == "twice":                               # rounded to bf16 before the last addition
        v = ((v + b if e.bias else v).to(BF).double() + o.base64) if e.acc else (v.to(BF).double() + b)
    else:
        if e.bias:
            v = v + b
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


def _epi_wrongs(c, e, tier1):
    """bias of the neighbouring channel; Tier 1 only, the twice-rounded result where the fan-in (3x3x3, 16 channels or more: 432 products of
    magnitude 9 .. 16) takes most sums beyond 256, the first integers bf16 cannot hold — below that both roundings are exact and agree"""
    w = ["bias_shift"] if e.bias else []
    if tier1 and not e.out32 and (e.bias or e.acc) and c.cin >= 16 and c.ks == 3 and e.cs == 0:
        w.append("twice")
    return w


def _bands(c):
    a = slice(None)
    zt = ((c.Z - 1) // 16) * 16
    return {"x0": (a, slice(0, 1)), "x1": (a, slice(c.X - 1, c.X)), "y0": (a, a, slice(0, 1)), "y1": (a, a, slice(c.Y - 1, c.Y)),
            "z0": (a, a, a, slice(0, 1)), "z1": (a, a, a, slice(c.Z - 1, c.Z)), "first z tile": (a, a, a, slice(0, min(16, c.Z))),
            "last z tile": (a, a, a, slice(zt, c.Z))}


def _assert_differs_in_bands(c, right, wrong, what, names=None):
    for name, sl in _bands(c).items():
        if names is None or name in names:
            assert bool((right[sl] != wrong[sl]).any()), f"{what}: the wrong result equals the right one in the {name} band: it guards nothing there"


# ============================================================================================== launches and guards
class Run:
    pass


def _launch(c, e, o):
    """one ops.conv3d_fwd call of epilogue e -> Run(y, mean, rstd, buf, region): buf the sentinel buffer around the output (None where ops
    allocates it: fp32 outputs without accumulation, cout_store = 3 dense, the statistics launches), region(buf) the part the kernel may write"""
    ops = _ops()
    cs = e.cs_of(c)
    odt = F32 if e.out32 else BF
    dev = o.x.device
    kw = dict(ksize=c.ks, bias=o.bias if e.bias else None, cout_store=cs, out_dtype=odt)
    r = Run()
    r.buf = r.region = r.mean = r.rstd = None
    V = c.B * c.X * c.Y * c.Z
    if e.acc:
        r.buf, y = _carve(o.base64[..., :cs].to(odt).contiguous(), SENT, dev)
        r.region = lambda b: b[PAD:PAD + V * cs]
        r.snap = r.buf.clone()
        r.y = ops.conv3d_fwd(o.x, o.wp, c.cout, accumulate_into=y, **kw)
    elif e.ldx is not None:
        ld = e.ld_of(c)
        r.buf = torch.full((V + 2, ld), SENT, dtype=BF, device=dev)
        r.region = lambda b: b[:V, :cs]
        r.snap = r.buf.clone()
        r.y = ops.conv3d_fwd(o.x, o.wp, c.cout, out=r.buf[:V].view(c.shape + (ld,))[..., :cs], **kw)
    elif e.stats:
        r.y, r.mean, r.rstd = ops.conv3d_fwd(o.x, o.wp, c.cout, stats_eps=EPS, **kw)
    else:
        r.y = ops.conv3d_fwd(o.x, o.wp, c.cout, **kw)
    assert tuple(r.y.shape) == c.shape + (cs,) and r.y.dtype == odt
    return r


def _assert_guard(r, what):
    if r.buf is None:
        return
    now, was = _bits(r.buf).clone(), _bits(r.snap).clone()
    r.region(now).zero_()
    r.region(was).zero_()
    assert torch.equal(now, was), f"{what}: written outside the cout_store channels of the output's voxel rows"


def _assert_stats(c, r, what):
    """the contract of tests/test_conv3d.py: against the float64 statistics of the STORED output"""
    ref = r.y.double().reshape(c.B, -1, c.cout)
    m, var = ref.mean(1), ref.var(1, unbiased=False)
    spread = float(var.sqrt().max())
    em = float((r.mean.double() - m).abs().max()) / max(spread, 1e-30)
    er = float((r.rstd.double() * (var + EPS).sqrt() - 1).abs().max())
    print(f"STATS {what}: mean err / spread {em:.2e}, rstd rel err {er:.2e}")
    assert em < 1e-4 and er < 1e-4, f"{what}: statistics by-product off: mean {em:.2e} of the spread, rstd {er:.2e} relative"


RATIOS = {}


def _ratio(family, what, got, ref, tol):
    err = (got.detach().double() - ref).abs()
    bad = ~(err <= tol)
    r = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    RATIOS[family] = max(RATIOS.get(family, 0.0), r)
    print(f"RATIO {family} {what}: worst err/bound {r:.3f}")
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, worst err/bound {r:.3f}, "
                                 f"first at {torch.nonzero(bad)[0].tolist()}")
    return r


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


def _witness(c, mode):
    """the library's two size queries against the restated plan, for this process's UCFVIT_CONV_STRIP"""
    from UCF_VIT._hip import lib
    L = lib.load()
    for bias in (False, True):
        rows = L.ucfvit_conv3d_fwd_stats_rows(c.B, c.X, c.Y, c.Z, c.cin, c.cout, c.ks, int(bias))
        want = _stats_rows(c, bias, mode)
        assert rows == want, f"{c.id} bias={bias} mode {mode}: ucfvit_conv3d_fwd_stats_rows = {rows}, the restated plan says {want}"


def _witness_w(c):
    from UCF_VIT._hip import lib
    L = lib.load()
    kin, kout = c.kdims
    p = _wplan(c)
    ws = L.ucfvit_conv3d_wgrad_workspace(c.B, c.X, c.Y, c.Z, kin, kout, c.ks)
    assert ws == p["n_wg"] * p["slots"] * p["n_out"] * 4, f"{c.id}: ucfvit_conv3d_wgrad_workspace = {ws}, the restated plan says {p}"
    return ws // (p["slots"] * p["n_out"] * 4), p


# ============================================================================================== forward: Tier 1
def _tier1_fwd(c, mode, dev, launch=True, save=None):
    """exact tier; launch False: the host half only (the wrong references differ from the right one where they should)"""
    for kind in ("big", "int") if launch else ("big",):           # (|int| <= |big|: its exactness condition is implied)
        o = _fwd_operands(c, kind, dev)
        R = _fwd_refs(c, o, wrongs=kind == "big")
        cond = R["abs"] + o.bias64.abs() + o.base64.abs()
        assert float(cond.max()) < LIM, f"{c.id}: the exactness condition fails: {float(cond.max())} >= 2^24"
        for en in _epis(c):
            e = EPIS[en]
            what = f"{c.id}/{en}/{kind}"
            odt = F32 if e.out32 else BF
            right = _epi(c, e, o, R["ok"])[0].to(odt)
            wrongs = {}
            if kind == "big":
                for n in GEOM:
                    if n in R:
                        wrongs[n] = _epi(c, e, o, R[n])[0].to(odt)
                        _assert_differs_in_bands(c, right, wrongs[n], f"{what} {n}")
                for n in _epi_wrongs(c, e, True):
                    wrongs[n] = _epi(c, e, o, R["ok"], variant=n)[0].to(odt)
                    _assert_differs_in_bands(c, right, wrongs[n], f"{what} {n}", ("first z tile", "last z tile"))
            if not launch:
                continue
            r = _launch(c, e, o)
            assert bool(torch.isfinite(r.y.float()).all()), f"{what}: non-finite output (NaN padding read?)"
            bad = _bits(r.y) != _bits(right)
            assert not bool(bad.any()), (f"{what} [{_plan(c, e, mode).name}]: {int(bad.sum())} elements differ from the float64 result rounded once, "
                                         f"first at {torch.nonzero(bad)[0].tolist()}")
            _assert_guard(r, what)
            for n, w in wrongs.items():
                assert not torch.equal(r.y, w), f"{what}: the kernel wrote the wrong result '{n}'"
            if e.stats:
                _assert_stats(c, r, what)
            if save is not None and en in SAVE_EPIS and kind == "big":
                save[what] = _bits(r.y).cpu()
            if not e.acc:                               # a second call: bit for bit
                r2 = _launch(c, e, o)
                assert torch.equal(_bits(r2.y), _bits(r.y))
                if e.stats:
                    assert torch.equal(r2.mean, r.mean) and torch.equal(r2.rstd, r.rstd)


# ============================================================================================== forward: Tier 2
FAMS = ("randn", "offset", "exp")


def _tier2_fwd(c, mode, dev, save=None):
    pools = {en: Pool(f"{c.id}/{en}") for en in _epis(c)}
    for fam in FAMS:
        o = _fwd_operands(c, fam, dev)
        R = _fwd_refs(c, o)
        for en in _epis(c):
            e = EPIS[en]
            p = _plan(c, e, mode)
            d = p.steps + 32
            r = _launch(c, e, o)
            what = f"{c.id}/{en}/{fam}"
            assert bool(torch.isfinite(r.y.float()).all()), f"{what}: non-finite output (NaN padding read?)"
            _assert_guard(r, what)
            v, tol = _epi(c, e, o, R["ok"], R["abs"], d)
            wrongs = {n: _epi(c, e, o, R[n], R["abs"], d)[0] for n in GEOM if n in R}
            for n in _epi_wrongs(c, e, False):
                wrongs[n] = _epi(c, e, o, R["ok"], R["abs"], d, variant=n)[0]
            pools[en].check(f"{p.name} {'fp32' if e.out32 else 'bf16'}", r.y, v, tol, wrongs)
            if e.stats and fam != "exp":
                _assert_stats(c, r, what)
            if save is not None and en in SAVE_EPIS and fam == "randn":
                save[what] = _bits(r.y).cpu()
    for p in pools.values():
        p.done()


FWD_IDS = [c.id for c in FWD]
assert len(set(FWD_IDS)) == len(FWD_IDS)


@gpu
@pytest.mark.parametrize("c", FWD, ids=FWD_IDS)
def test_conv_fwd_exact(c):
    _witness(c, _mode())
    _tier1_fwd(c, _mode(), DEV)


@gpu
@pytest.mark.parametrize("c", FWD, ids=FWD_IDS)
def test_conv_fwd_bounds(c):
    _witness(c, _mode())
    _tier2_fwd(c, _mode(), DEV)


@gpu
def test_conv_default_mode_selects_by_size():
    """the 512-workgroup thresholds, in this process (no hook): one shape per column family at the threshold, one just below"""
    want = [("strip-fast-share", 4, 8, 512), ("tile", 2, 8, 0), ("mc1", 2, 8, 512), ("tile", 2, 4, 0), ("strip-fast", 4, 8, 576)]
    for c, (name, tx, ty, rows) in zip(SEL, want):
        p = _plan(c, EPIS["stats"], 1)
        assert (p.name, p.TX, p.TY) == (name, tx, ty), f"{c.id}: {p}"
        assert _stats_rows(c, False, 1) == (_cdiv(c.X, tx) * _cdiv(c.Y, ty) * 4 if rows else 0)
        _witness(c, _mode())
    assert _stats_rows(SEL[4], False, 1) > 512                # the two-stage fold of ucfvit_instnorm_cl_stats_fold


# ============================================================================================== weight gradient
def _w_operands(c, kind, dev):
    g = torch.Generator().manual_seed(_seed(c, kind))
    exact = kind in ("int", "big")
    o = O()
    x = _values(g, kind, (c.B, c.X, c.Y, c.Z, c.cin)).to(BF)
    dy = _values(g, kind if exact else "randn", (c.B, c.X, c.Y, c.Z, c.cout), 1.0 if exact else 0.05).to(BF)
    _, o.x = _carve(x, float("nan"), dev)
    _, o.dy = _carve(dy, float("nan"), dev)
    o.x64, o.dy64 = x.double().to(dev), dy.double().to(dev)
    return o


def _w_launch(c, o):
    ops, conv = _ops(), _conv()
    if c.via == "conv3":
        return conv.conv3_wgrad(o.x, o.dy, c.cin, c.cout)
    if c.via == "pw":
        return conv._pointwise_wgrad(o.x, o.dy).reshape(c.cout, c.cin, 1, 1, 1)
    return conv.unpack_conv_wgrad(ops.conv3d_wgrad(o.x, o.dy, ksize=c.ks), c.cin, c.cout, c.ks)


def _w_refs(c, o):
    R = {"ok": _wgrad64(o.x64, o.dy64, c.ks), "abs": _wgrad64(o.x64.abs(), o.dy64.abs(), c.ks)}
    if c.ks == 3:
        R["mirror"] = R["ok"].flip(2, 3, 4)
        R["replicate"] = _wgrad64(o.x64, o.dy64, 3, "replicate")
    for ax, n in (("x", 1), ("y", 2), ("z", 3)):                  # x and dy offset by one voxel
        if o.x64.shape[n] > 1:
            R["shift_" + ax] = _wgrad64(o.x64.roll(1, n), o.dy64, c.ks)
    if c.Z > 1:                                                   # the last z plane (the ragged end of the 32-deep tile) left out
        dz = o.dy64.clone()
        dz[:, :, :, -1] = 0
        R["drop_last_z"] = _wgrad64(o.x64, dz, c.ks)
    return R


W_WRONG = ("mirror", "replicate", "shift_x", "shift_y", "shift_z", "drop_last_z")


def _tier1_w(c, dev, launch=True):
    for kind in ("big", "int"):
        o = _w_operands(c, kind, dev)
        R = _w_refs(c, o)
        assert float(R["abs"].max()) < LIM, f"{c.id}: the exactness condition fails over all voxels: {float(R['abs'].max())} >= 2^24"
        right = R["ok"].float()
        for n in W_WRONG:
            if n in R:
                assert not torch.equal(R[n].float(), right), f"{c.id}/{kind}: the wrong gradient '{n}' equals the right one"
        if not launch:
            continue
        got = _w_launch(c, o)
        assert tuple(got.shape) == tuple(right.shape) and got.dtype == F32
        bad = got != right
        assert not bool(bad.any()), f"{c.id}/{kind}: {int(bad.sum())} elements differ from float64, first at {torch.nonzero(bad)[0].tolist()}"
        for n in W_WRONG:
            if n in R:
                assert not torch.equal(got, R[n].float()), f"{c.id}/{kind}: the kernel wrote the wrong gradient '{n}'"
        assert torch.equal(_w_launch(c, o), got)                  # a second call: the fold has a fixed order


def _tier2_w(c, dev):
    n_wg, p = _witness_w(c)
    pool = Pool(c.id)
    for fam in FAMS:
        o = _w_operands(c, fam, dev)
        R = _w_refs(c, o)
        got = _w_launch(c, o)
        assert bool(torch.isfinite(got).all()), f"{c.id}/{fam}: non-finite gradient (NaN padding read?)"
        t = p["d"] * U * R["abs"]
        tol = t + U * (R["ok"].abs() + t)
        pool.check(f"wgrad k{c.ks}" + (" swapped" if c.swapped else ""), got, R["ok"], tol, {n: R[n] for n in W_WRONG if n in R})
    pool.done()


W_IDS = [c.id for c in WGRAD]


@gpu
@pytest.mark.parametrize("c", WGRAD, ids=W_IDS)
def test_conv_wgrad_exact(c):
    _witness_w(c)
    _tier1_w(c, DEV)


@gpu
@pytest.mark.parametrize("c", WGRAD, ids=W_IDS)
def test_conv_wgrad_bounds(c):
    _tier2_w(c, DEV)


def test_conv_wgrad_plan_and_tiles_per_workgroup():
    """CPU: the workspace query against the restated conv_wgrad_route on every case; the cases the table names for tiles_per_wg > 1 have it (n_wg
    from the QUERY below the tile count), the role-swapped calls hand the kernel the exchanged channel counts"""
    multi = []
    for c in WGRAD:
        n_wg, p = _witness_w(c)
        assert n_wg == p["n_wg"]
        if n_wg < p["tiles"]:
            multi.append((c.ks, p["tpw"]))
    assert (3, 2) in multi and (1, 2) in multi and len(multi) == 3, multi
    big = _wplan(WC(2, 8, 12, 40, 256, 128))
    assert big["tiles"] == 48 and big["n_wg"] == 24 and big["tpw"] == 2
    assert {(_wplan(c)["MB"], _wplan(c)["cpc"], c.ks) for c in WGRAD} >= {(m, k, s) for m in (1, 2) for k in (8, 16, 32) for s in (3, 1)}
    assert [c.kdims for c in WGRAD if c.swapped] == [(16, 32), (16, 64), (8, 32)]


# ============================================================================================== symmetries
@gpu
def test_fused_res_block_forward_equals_the_chain_bit_for_bit():
    """unet_res_block with an identity residual against conv3x3x3 -> instnorm_act_cl -> conv3x3x3 -> instnorm_act_cl(+ inp) at a size the tile
    kernel serves: the same kernels in the same order, the same bits"""
    conv = _conv()
    g = torch.Generator().manual_seed(5)
    inp = torch.randn(2, 3, 7, 17, 16, generator=g).bfloat16().to(DEV)
    w1 = (torch.randn(16, 16, 3, 3, 3, generator=g) * 0.07).to(DEV)
    w2 = (torch.randn(16, 16, 3, 3, 3, generator=g) * 0.07).to(DEV)
    fused = conv.unet_res_block(inp, w1, w2)
    y1 = conv.instnorm_act_cl(conv.conv3x3x3(inp, w1))
    chain = conv.instnorm_act_cl(conv.conv3x3x3(y1, w2), inp)
    assert bool(torch.isfinite(fused.float()).all()) and torch.equal(fused, chain)


# ============================================================================================== refusals
def test_conv_refuses_unsupported_channel_counts_on_the_host():
    conv = _conv()
    with pytest.raises(ValueError, match="Cin must be 8, 16 or a multiple of 32"):
        conv.pack_conv_weight(torch.zeros(16, 24, 3, 3, 3))
    with pytest.raises(ValueError, match="kernel size must be 1 or 3"):
        conv.pack_conv_weight(torch.zeros(16, 16, 2, 2, 2))
    from UCF_VIT._hip import lib
    L = lib.load()
    assert L.ucfvit_conv3d_fwd_stats_rows(2, 4, 8, 32, 24, 16, 3, 0) == 0 and L.ucfvit_conv3d_fwd_stats_rows(2, 4, 8, 32, 16, 24, 3, 0) == 0
    assert L.ucfvit_conv3d_wgrad_workspace(2, 4, 8, 32, 24, 16, 3) == 0 and L.ucfvit_conv3d_wgrad_workspace(2, 4, 8, 32, 16, 24, 3) == 0


@gpu
def test_conv_refusals():
    ops, conv = _ops(), _conv()
    from UCF_VIT._hip import lib
    L = lib.load()
    x24 = torch.zeros(1, 2, 4, 17, 24, dtype=BF, device=DEV)
    x16 = torch.zeros(1, 2, 4, 17, 16, dtype=BF, device=DEV)
    with pytest.raises(lib.HipLibraryError, match="Cin must be 8, 16 or a multiple of 32"):
        ops.conv3d_fwd(x24, torch.zeros(ops.conv_packed_numel(24, 16, 3), dtype=BF, device=DEV), 16)
    with pytest.raises(lib.HipLibraryError, match="Cout must be a multiple of 16"):
        ops.conv3d_fwd(x16, torch.zeros(ops.conv_packed_numel(16, 24, 3), dtype=BF, device=DEV), 24)
    with pytest.raises(ValueError, match="Cout must be a multiple of 16"):
        conv.conv3x3x3(x16, torch.zeros(24, 16, 3, 3, 3, device=DEV))
    with pytest.raises(ValueError, match="unsupported channel counts"):
        ops.conv3d_wgrad(x24, x16)
    wp = conv.pack_conv_weight(torch.zeros(16, 16, 3, 3, 3)).to(DEV)
    # statistics on an output that is not dense bf16: ops refuses each form, and so does the library
    buf = torch.zeros(1, 2, 4, 17, 24, dtype=BF, device=DEV)
    for kw in (dict(out=buf[..., :16]), dict(cout_store=12), dict(out_dtype=F32), dict(accumulate_into=torch.zeros(1, 2, 4, 17, 16, dtype=BF, device=DEV))):
        with pytest.raises(ValueError, match="statistics need a dense bf16 output"):
            ops.conv3d_fwd(x16, wp, 16, stats_eps=EPS, **kw)
    part = torch.full((1 << 16,), SENT, dtype=F32, device=DEV)
    y = torch.full((1, 2, 4, 17, 24), SENT, dtype=BF, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(lib.HipLibraryError, match="statistics need a dense bf16 output"):
        lib.check(L.ucfvit_conv3d_fwd(x16.data_ptr(), wp.data_ptr(), None, y.data_ptr(), 1, 2, 4, 17, 16, 16, 3, 24, 16, lib.BF16, 0, part.data_ptr(), st), "fwd")
    # statistics handed to a launch whose kernel has no epilogue for them (the tile kernel: Z <= 16, or any size under UCFVIT_CONV_STRIP=0)
    x_t = torch.zeros(1, 2, 4, 16, 16, dtype=BF, device=DEV)
    y_t = torch.full((1, 2, 4, 16, 16), SENT, dtype=BF, device=DEV)
    assert L.ucfvit_conv3d_fwd_stats_rows(1, 2, 4, 16, 16, 16, 3, 0) == 0
    with pytest.raises(lib.HipLibraryError, match="no statistics epilogue"):
        lib.check(L.ucfvit_conv3d_fwd(x_t.data_ptr(), wp.data_ptr(), None, y_t.data_ptr(), 1, 2, 4, 16, 16, 16, 3, 16, 16, lib.BF16, 0, part.data_ptr(), st), "fwd")
    torch.cuda.synchronize()
    assert bool((part == SENT).all()) and bool((y == SENT).all()) and bool((y_t == SENT).all())       # a refused launch writes nothing


# ============================================================================================== around the kernels
def _bound_check(family, what, got, ref, absref, d, out_dtype, wrongs):
    t = d * U * absref
    tol = t + (U if out_dtype == F32 else UB) * (ref.abs() + t)
    _ratio(family, what, got, ref, tol)
    for n, w in wrongs.items():
        assert not _within(got, w, tol), f"{what}: the bound does not reject the wrong reference '{n}'"


def _d2s64(cols, B, X, Y, Z, C):
    """cols [B X Y Z, 8 C], column blocks (dx, dy, dz) -> [B, 2X, 2Y, 2Z, C]"""
    return cols.reshape(B, X, Y, Z, 2, 2, 2, C).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(B, 2 * X, 2 * Y, 2 * Z, C)


@gpu
@pytest.mark.parametrize("cin,cout,route", [(32, 8, "1x1x1 kernel"), (16, 16, "1x1x1 kernel"), (768, 32, "gemm"), (128, 64, "gemm")])
def test_tconv2x2x2_per_element(cin, cout, route):
    conv = _conv()
    assert (cin < conv.GEMM_MIN) == (route == "1x1x1 kernel")
    B, X, Y, Z = 2, 3, 5, 7
    V = B * X * Y * Z
    for kind in ("big", "randn", "offset"):
        g = torch.Generator().manual_seed(cin + cout + len(kind))
        exact = kind == "big"
        x = _values(g, kind, (B, X, Y, Z, cin)).to(BF)
        w = _values(g, kind if exact else "randn", (cin, cout, 2, 2, 2), 1.0 if exact else cin ** -0.5).to(BF)
        skip = _values(g, "randn", (B, 2 * X, 2 * Y, 2 * Z, cout)).to(BF)        # (C + Cs) / 8 must be a power of two
        dy = _values(g, kind if exact else "randn", (B, 2 * X, 2 * Y, 2 * Z, cout), 1.0 if exact else 0.1).to(BF)
        x64, w64, dy64 = x.double().to(DEV), w.double().to(DEV), dy.double().to(DEV)
        w2 = w64.permute(2, 3, 4, 1, 0).reshape(8 * cout, cin)                 # rows (dx, dy, dz, co)
        ref = _d2s64(x64.reshape(V, cin) @ w2.T, B, X, Y, Z, cout)
        aref = _d2s64(x64.abs().reshape(V, cin) @ w2.abs().T, B, X, Y, Z, cout)
        swapped = _d2s64(x64.reshape(V, cin) @ w64.permute(4, 3, 2, 1, 0).reshape(8 * cout, cin).T, B, X, Y, Z, cout)    # (dz, dy, dx) blocks
        _, xv = _carve(x, float("nan"), DEV)
        xv.requires_grad_(True)
        wv = w.float().to(DEV).requires_grad_(True)
        out = conv.tconv2x2x2(xv, wv)
        cat = conv.tconv2x2x2(xv.detach(), wv.detach(), skip.to(DEV))
        assert torch.equal(cat[..., :cout], out) and torch.equal(cat[..., cout:], skip.to(DEV))
        out.backward(dy.to(DEV))
        dcols = dy64.reshape(B, X, 2, Y, 2, Z, 2, cout).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(V, 8 * cout)
        dx_ref, dx_abs = (dcols @ w2).reshape(x.shape), (dcols.abs() @ w2.abs()).reshape(x.shape)
        dw2, dw2_abs = dcols.T @ x64.reshape(V, cin), dcols.abs().T @ x64.abs().reshape(V, cin)
        to_w = lambda m: m.reshape(2, 2, 2, cout, cin).permute(4, 3, 0, 1, 2)
        if exact:
            assert float(aref.max()) < LIM and float(dx_abs.max()) < LIM and float(dw2_abs.max()) < LIM
            assert torch.equal(out, ref.to(BF)) and not torch.equal(out, swapped.to(BF))
            assert torch.equal(xv.grad, dx_ref.to(BF)) and torch.equal(wv.grad, to_w(dw2).float())
        else:
            fam = f"tconv2 {route}"
            _bound_check(fam + " fwd", f"tconv2x2x2 {cin}->{cout} {kind}", out, ref, aref, _cdiv(cin, 32) + 32, BF, {"blocks (dz, dy, dx)": swapped})
            _bound_check(fam + " dx", f"tconv2x2x2 dx {cin}->{cout} {kind}", xv.grad, dx_ref, dx_abs, _cdiv(8 * cout, 32) + 32, BF,
                         {"dy of the neighbouring voxel": (dcols.roll(1, 0) @ w2).reshape(x.shape)})
            # 1x1x1 weight gradient: its plan; GEMM: ceil(V / 32) + 32 and up to 8 split-K slices
            d = _wplan(WC(B, X, Y, Z, cin, 8 * cout, 1, via="pw"))["d"] if route != "gemm" else _cdiv(V, 32) + 32 + 8
            _bound_check(fam + " dw", f"tconv2x2x2 dw {cin}->{cout} {kind}", wv.grad, to_w(dw2), to_w(dw2_abs), d, F32,
                         {"x of the neighbouring voxel": to_w(dcols.T @ x64.reshape(V, cin).roll(1, 0))})


@gpu
@pytest.mark.parametrize("cin,cout,bias,fp32,route", [(16, 4, True, True, "1x1x1 kernel"), (16, 3, True, True, "1x1x1 kernel"), (32, 16, False, False, "1x1x1 kernel"),
                                                      (8, 16, True, False, "1x1x1 kernel"), (256, 32, True, False, "1x1x1 kernel"),
                                                      (128, 128, True, False, "gemm"), (256, 128, False, True, "gemm")])
def test_conv1x1x1_per_element(cin, cout, bias, fp32, route):
    conv = _conv()
    assert (cin >= conv.GEMM_MIN and cout >= conv.GEMM_MIN) == (route == "gemm")
    B, X, Y, Z = 2, 3, 5, 33
    V = B * X * Y * Z
    odt = F32 if fp32 else BF
    for kind in ("big", "randn", "offset"):
        g = torch.Generator().manual_seed(3 * cin + cout + len(kind))
        exact = kind == "big"
        x = _values(g, kind, (B, X, Y, Z, cin)).to(BF)
        w = _values(g, kind if exact else "randn", (cout, cin, 1, 1, 1), 1.0 if exact else cin ** -0.5).to(BF)
        b = _values(g, "int4" if exact else "randn", (cout,), 0.5).to(BF)
        dy = _values(g, kind if exact else "randn", (B, X, Y, Z, cout), 1.0 if exact else 0.1).to(BF)
        x64, w64, b64, dy64 = x.double().to(DEV), w.double().reshape(cout, cin).to(DEV), b.double().to(DEV), dy.double().to(DEV)
        ref = x64 @ w64.T + (b64 if bias else 0.0)
        aref = x64.abs() @ w64.abs().T + (b64.abs() if bias else 0.0)
        _, xv = _carve(x, float("nan"), DEV)
        xv.requires_grad_(True)
        wv = w.float().to(DEV).requires_grad_(True)
        bv = b.float().to(DEV).requires_grad_(True) if bias else None
        out = conv.conv1x1x1(xv, wv, bv, out_fp32=fp32)
        assert out.dtype == odt and tuple(out.shape) == (B, X, Y, Z, cout) and bool(torch.isfinite(out.float()).all())
        out.backward(dy.to(DEV).to(odt))
        d2 = dy64.reshape(V, cout)
        dx_ref, dx_abs = (d2 @ w64).reshape(x.shape), (d2.abs() @ w64.abs()).reshape(x.shape)
        dw, dw_abs = d2.T @ x64.reshape(V, cin), d2.abs().T @ x64.abs().reshape(V, cin)
        if exact:
            assert float(aref.max()) < LIM and float(dx_abs.max()) < LIM and float(dw_abs.max()) < LIM and float(d2.abs().sum(0).max()) < LIM
            assert torch.equal(out, ref.to(odt))
            if bias:
                assert not torch.equal(out, (ref - b64 + b64.roll(1)).to(odt))
                assert torch.equal(bv.grad, d2.sum(0).float())
            assert torch.equal(xv.grad, dx_ref.to(BF)) and torch.equal(wv.grad.reshape(cout, cin), dw.float())
        else:
            fam = f"conv1 {route}"
            wrongs = {"last input channel dropped": ref - x64[..., -1:] @ w64[:, -1:].T}
            if bias:
                wrongs["bias of the neighbouring channel"] = ref - b64 + b64.roll(1)
            _bound_check(f"{fam} fwd {'fp32' if fp32 else 'bf16'}", f"conv1x1x1 {cin}->{cout} {kind}", out, ref, aref, _cdiv(cin, 32) + 32 + 1, odt, wrongs)
            _bound_check(fam + " dx", f"conv1x1x1 dx {cin}->{cout} {kind}", xv.grad, dx_ref, dx_abs, _cdiv(max(cout, 8), 32) + 32, BF,
                         {"dy of the neighbouring voxel": (d2.roll(1, 0) @ w64).reshape(x.shape)})
            if route == "gemm":
                d = _cdiv(V, 32) + 32 + 8
            else:               # the kernel's operands: x as it is, dy padded to an input width; roles swapped when the padded Cout is 8
                d = _wplan(WC(B, X, Y, Z, cin, conv._pad_cin(cout), 1, via="pw"))["d"]
            _bound_check(fam + " dw", f"conv1x1x1 dw {cin}->{cout} {kind}", wv.grad.reshape(cout, cin), dw, dw_abs, d, F32,
                         {"x of the neighbouring voxel": d2.T @ x64.reshape(V, cin).roll(1, 0)})
            if bias:
                s, sa = d2.sum(0), d2.abs().sum(0)
                assert bool(((bv.grad.double() - s).abs() <= V * U * sa + U * s.abs()).all()), "conv1x1x1: bias gradient out of the bound of a V-long fp32 sum"


@gpu
@pytest.mark.parametrize("cin,cout,cs", [(32, 16, 0), (64, 32, 16), (16, 16, 8)])
def test_tconv1x1x1_per_element(cin, cout, cs):
    conv = _conv()
    B, X, Y, Z = 2, 3, 5, 17
    V = B * X * Y * Z
    for kind in ("big", "randn", "offset"):
        g = torch.Generator().manual_seed(5 * cin + cout + len(kind))
        exact = kind == "big"
        x = _values(g, kind, (B, X, Y, Z, cin)).to(BF)
        w = _values(g, kind if exact else "randn", (cin, cout, 1, 1, 1), 1.0 if exact else cin ** -0.5).to(BF)
        dy = _values(g, kind if exact else "randn", (B, X, Y, Z, cout + cs), 1.0 if exact else 0.1).to(BF)
        skip = _values(g, "randn", (B, X, Y, Z, cs)).to(BF).to(DEV) if cs else None
        x64, w64, dy64 = x.double().to(DEV), w.double().reshape(cin, cout).to(DEV), dy.double().to(DEV)
        ref, aref = x64 @ w64, x64.abs() @ w64.abs()
        _, xv = _carve(x, float("nan"), DEV)
        xv.requires_grad_(True)
        wv = w.float().to(DEV).requires_grad_(True)
        sv = skip.clone().requires_grad_(True) if cs else None
        out = conv.tconv1x1x1(xv, wv, sv)
        assert tuple(out.shape) == (B, X, Y, Z, cout + cs) and bool(torch.isfinite(out.float()).all())
        out.backward(dy.to(DEV))
        if cs:
            assert torch.equal(out[..., cout:], skip) and torch.equal(sv.grad, dy.to(DEV)[..., cout:])
        d2 = dy64[..., :cout].reshape(V, cout)
        dx_ref, dx_abs = (d2 @ w64.T).reshape(x.shape), (d2.abs() @ w64.abs().T).reshape(x.shape)
        dw, dw_abs = x64.reshape(V, cin).T @ d2, x64.abs().reshape(V, cin).T @ d2.abs()
        got_dw = wv.grad.reshape(cin, cout)
        if exact:
            assert float(aref.max()) < LIM and float(dx_abs.max()) < LIM and float(dw_abs.max()) < LIM
            assert torch.equal(out[..., :cout], ref.to(BF)) and torch.equal(xv.grad, dx_ref.to(BF)) and torch.equal(got_dw, dw.float())
        else:
            _bound_check("tconv1 fwd", f"tconv1x1x1 {cin}->{cout} {kind}", out[..., :cout], ref, aref, _cdiv(cin, 32) + 32, BF,
                         {"last input channel dropped": ref - x64[..., -1:] @ w64[-1:]})
            _bound_check("tconv1 dx", f"tconv1x1x1 dx {cin}->{cout} {kind}", xv.grad, dx_ref, dx_abs, _cdiv(cout, 32) + 32, BF,
                         {"dy of the neighbouring voxel": (d2.roll(1, 0) @ w64.T).reshape(x.shape)})
            _bound_check("tconv1 dw", f"tconv1x1x1 dw {cin}->{cout} {kind}", got_dw, dw, dw_abs, _wplan(WC(B, X, Y, Z, cin, cout, 1))["d"], F32,
                         {"x of the neighbouring voxel": x64.reshape(V, cin).roll(1, 0).T @ d2})


@gpu
@pytest.mark.parametrize("C,Cs,extra", [(8, 0, 0), (16, 0, 16), (8, 8, 0), (16, 16, 32), (8, 24, 0)])
def test_depth_to_space_and_back_are_exact_rearrangements(C, Cs, extra):
    """depth_to_space2 into a channel slice (with and without skip), space_to_depth2 out of one: torch.equal to the index arithmetic, every
    sentinel of the wider buffer untouched"""
    ops = _ops()
    B, X, Y, Z = 2, 3, 1, 5
    g = torch.Generator().manual_seed(C + Cs)
    cols = torch.randn(B * X * Y * Z, 8 * C, generator=g).to(BF)
    skip = torch.randn(B, 2 * X, 2 * Y, 2 * Z, Cs, generator=g).to(BF).to(DEV) if Cs else None
    _, cv = _carve(cols, float("nan"), DEV)
    ref = _d2s64(cols.to(DEV), B, X, Y, Z, C)
    ld = C + Cs + extra
    V8 = B * X * Y * Z * 8
    buf = torch.full((V8 + 2, ld), SENT, dtype=BF, device=DEV)
    out = ops.depth_to_space2(cv, B, X, Y, Z, C, out=buf[:V8].view(B, 2 * X, 2 * Y, 2 * Z, ld)[..., :C], skip=skip)
    assert torch.equal(out, ref)
    if Cs:
        assert torch.equal(buf[:V8, C:C + Cs].reshape(skip.shape), skip)
    assert bool((buf[:V8, C + Cs:] == SENT).all()) and bool((buf[V8:] == SENT).all())
    if not Cs and not extra:
        assert torch.equal(ops.depth_to_space2(cv, B, X, Y, Z, C), ref)
    back = ops.space_to_depth2(buf[:V8].view(B, 2 * X, 2 * Y, 2 * Z, ld)[..., :C])      # out of the slice, NaN-free: the sentinels stay out
    assert torch.equal(back, cols.to(DEV))


@gpu
def test_pad_channels8_and_pad_rows8_are_exact():
    ops = _ops()
    g = torch.Generator().manual_seed(2)
    for C in (1, 3, 8):
        vol = torch.randn(2, C, 3, 5, 7, generator=g)
        _, vv = _carve(vol, float("nan"), DEV)
        ref = torch.zeros(2, 3, 5, 7, 8, dtype=BF)
        ref[..., :C] = vol.permute(0, 2, 3, 4, 1).to(BF)
        assert torch.equal(ops.pad_channels8(vv).cpu(), ref)
    for dt in (F32, BF):
        for C, ld in ((3, 3), (4, 8), (1, 5), (8, 8), (5, 16)):
            rows = torch.randn(2, 3, 7, ld, generator=g).to(dt)
            buf = torch.full((2 * 3 * 7 + 1, ld), float("nan"), dtype=dt, device=DEV)
            buf[:-1] = rows.reshape(-1, ld).to(DEV)
            buf[:, C:] = float("nan")                                  # the columns behind the slice are never read
            ref = torch.zeros(2, 3, 7, 8, dtype=BF)
            ref[..., :C] = rows[..., :C].to(BF)
            assert torch.equal(ops.pad_rows8(buf[:-1].view(2, 3, 7, ld)[..., :C]).cpu(), ref)


# ============================================================================================== CPU: routing and the host half of Tier 1
def _required_branches():
    """every branch the table must reach, as (plan name, CPC, KS, NB, TX, TY, DEPTH, fp32 output) or a looser tuple; see the docstring"""
    seen = {m: set() for m in range(4)}
    for m in range(4):
        for c in FWD:
            for en in _epis(c):
                e = EPIS[en]
                p = _plan(c, e, m)
                seen[m].add((p.name, min(c.cin, 32), c.ks, p.NB, p.TX, p.TY, p.depth, e.out32, c.cin if c.cin > 32 else 0))
    return seen


def test_conv_table_reaches_every_branch():
    seen = _required_branches()

    def has(m, **kw):
        keys = ("name", "cpc", "ks", "NB", "TX", "TY", "depth", "out32", "cin")
        return any(all(dict(zip(keys, s))[k] == v for k, v in kw.items()) for s in seen[m])

    for m in (0, 1):                                                  # the tile kernel at small sizes
        for cpc in (8, 16, 32):
            for ks in (3, 1):
                assert has(m, name="tile", cpc=cpc, ks=ks, out32=False) and has(m, name="tile", cpc=cpc, ks=ks, out32=True), (m, cpc, ks)
        for nb in (4, 2, 1):
            assert has(m, name="tile", NB=nb)
        for cin in (64, 128, 256):
            assert has(m, name="tile", cin=cin)
    assert not any(s[0] != "tile" for s in seen[0])
    assert {s[0] for s in seen[1]} == {"tile", "strip-fast", "strip-fast-share", "mc1"}       # the default reaches the column kernels by size only
    for cpc, depth in ((8, 2), (16, 2), (32, 1)):
        for ks in (3, 1):
            name = "strip-fast-share" if (cpc == 16 and ks == 3) else "strip-fast"
            assert has(2, name=name, cpc=cpc, ks=ks, depth=depth, out32=False) and has(2, name=name, cpc=cpc, ks=ks, depth=depth, out32=True)
            assert not has(2, name=name, cpc=cpc, ks=ks, depth=3 - depth)
            bname = name.replace("fast", "branching")
            assert has(3, name=bname, cpc=cpc, ks=ks, depth=1) and has(2, name=bname, cpc=cpc, ks=ks)      # 2: by cout_store / the odd slice
    for tx, ty, nb in ((2, 4, 4), (2, 8, 2), (2, 8, 1), (4, 8, 1)):
        for m, pre in ((2, "strip-fast"), (3, "strip-branching")):
            assert any(s[0].startswith(pre) and s[3:6] == (nb, tx, ty) for s in seen[m]), (m, tx, ty, nb)
    assert not any(s[0].startswith("strip-fast") for s in seen[3])
    for tzt in (1, 2, 4):
        assert has(2, name=f"mc{tzt}") and has(3, name=f"mc{tzt}")
    for cin in (64, 128, 256):
        assert any(s[0].startswith("mc") and s[8] == cin for s in seen[2])
    for m in range(4):
        assert all(_plan(MC48, EPIS[en], m).kind == 0 for en in MC48.epis), "Z = 48 must fall back to the tile kernel"
    # the odd slice and the odd cout_store reach the branching kernel in mode 2
    c = next(c for c in FWD if c.fam == "strip" and "slice_odd" in _epis(c))
    for en in ("slice_odd", "cs3", "cs3_ld8", "cs5_ld8", "csm11_o32"):
        cc = c if en in _epis(c) else FWD[0]
        assert not _plan(cc, EPIS[en], 2).fast and _plan(cc, EPIS[en], 2).kind == 1
    assert _plan(c, EPIS["slice"], 2).fast
    assert {c.Z for c in FWD if c.fam == "strip"} >= {17, 31, 32, 33, 53} and {c.Z for c in FWD if c.fam == "tile"} >= {1, 15, 16}
    assert {c.Z for c in WGRAD} >= {31, 32, 33, 65}


def _route_table():
    """both size queries against the restated plans over the whole table under this process's UCFVIT_CONV_STRIP -> kinds of the dense launches"""
    m = _mode()
    kinds = [0, 0, 0]
    for c in FWD:
        _witness(c, m)
        kinds[_plan(c, EPIS["stats"], m).kind] += 1
    for c in WGRAD:
        _witness_w(c)
    return kinds


@pytest.mark.parametrize("mode", ["0", "1", "2", "3"])
def test_conv_route_queries_every_mode(mode):
    """strip_mode() reads UCFVIT_CONV_STRIP once per process: the whole table in one child per mode"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "routes"], env=dict(os.environ, UCFVIT_CONV_STRIP=mode), capture_output=True,
                       text=True, timeout=ROUTE_TIMEOUT, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
    got = [int(v) for v in r.stdout.split("kinds:")[1].split()[:3]]
    want = [0, 0, 0]
    for c in FWD:
        want[_plan(c, EPIS["stats"], int(mode)).kind] += 1
    assert got == want, (got, want)
    if mode == "0":
        assert got[1] == got[2] == 0
    elif mode == "1":
        assert got[1] == 2 and got[2] == 1                            # only the selection cases
    else:
        assert got[1] > 20 and got[2] >= 5


def _route_text(pass_, B, X, Y, Z, cin, cout, ks, bias=False, out32=False, ldy=None, cs=None, mode=-1, cap=160):
    """ucfvit_conv3d_route: pass 0 the forward launch of these arguments, 1 the weight gradient; mode = the hook value to assume, -1 the process's"""
    import ctypes
    from UCF_VIT._hip import lib
    buf = ctypes.create_string_buffer(cap)
    n = lib.load().ucfvit_conv3d_route(pass_, B, X, Y, Z, cin, cout, ks, int(bias), lib.F32 if out32 else lib.BF16, ldy or cout, cs or cout, mode, buf, cap)
    assert 0 < n < cap and len(buf.value) == n, f"ucfvit_conv3d_route returned {n}: {lib.load().ucfvit_last_error()}"
    return buf.value.decode()


def _plan_text(c, e, mode):
    """the restated plan in the words of ucfvit_conv3d_route; rows: the statistics rows of the plan's own kernel and tile"""
    p = _plan(c, e, mode)
    rows = _cdiv(c.X, p.TX) * _cdiv(c.Y, p.TY) * 4 if p.kind else 0
    return f"{p.name} cpc{min(c.cin, 32)} ks{c.ks} nb{p.NB} {p.TX}x{p.TY} depth{p.depth} rows{rows}"


def test_conv_route_text_equals_the_restated_plan():
    """CPU, one process: for every case, every epilogue it runs and every hook value 0 .. 3 handed in as an argument, the library names the
    kernel, CPC, KS, NB, tile, DEPTH and statistics rows that _plan restates; a dense bf16 launch has the rows of ucfvit_conv3d_fwd_stats_rows
    as restated; mode -1 is this process's own hook value"""
    seen = set()
    for c in FWD:
        for en in _epis(c):
            e = EPIS[en]
            for mode in range(4):
                said = _route_text(0, *c.shape, c.cin, c.cout, c.ks, e.bias, e.out32, e.ld_of(c), e.cs_of(c), mode)
                assert said == _plan_text(c, e, mode), f"{c.id} {en} mode {mode}: ucfvit_conv3d_route says '{said}', the restated plan '{_plan_text(c, e, mode)}'"
                if not e.out32 and e.cs_of(c) == c.cout and e.ld_of(c) == c.cout:
                    assert said.endswith(f" rows{_stats_rows(c, e.bias, mode)}"), (c.id, en, mode, said)
                seen.add(said.split()[0])
            assert _route_text(0, *c.shape, c.cin, c.cout, c.ks, e.bias, e.out32, e.ld_of(c), e.cs_of(c)) == _plan_text(c, e, _mode())
    assert seen == {"tile", "strip-fast", "strip-fast-share", "strip-branching", "strip-branching-share", "mc1", "mc2", "mc4"}, seen


def test_conv_wgrad_route_text_equals_the_restated_plan():
    """CPU: for every weight-gradient case, with the channel counts the kernel sees (role-swapped ones included), the library names the MB,
    n_wg, tiles_per_wg, slots and n_out that _wplan restates, and both size queries are fields of the same route"""
    from UCF_VIT._hip import lib
    L = lib.load()
    for c in WGRAD:
        (kin, kout), p = c.kdims, _wplan(c)
        said = _route_text(1, c.B, c.X, c.Y, c.Z, kin, kout, c.ks)
        want = f"wgrad cpc{p['cpc']} ks{c.ks} mb{p['MB']} n_wg{p['n_wg']} tiles_per_wg{p['tpw']} slots{p['slots']} n_out{p['n_out']}"
        assert said == want, f"{c.id}: ucfvit_conv3d_route says '{said}', the restated plan '{want}'"
        assert said == _route_text(1, c.B, c.X, c.Y, c.Z, kin, kout, c.ks, bias=True, out32=True, ldy=7, cs=99, mode=3)     # pass 1 ignores the epilogue
        assert L.ucfvit_conv3d_wgrad_workspace(c.B, c.X, c.Y, c.Z, kin, kout, c.ks) == p["n_wg"] * p["slots"] * p["n_out"] * 4
        assert L.ucfvit_conv3d_wgrad_size(kin, kout, c.ks) == p["n_out"]


def test_conv_route_query_cuts_the_text_to_the_room_given():
    """the length returned is the whole text's, the text is cut to cap - 1 characters and terminated, cap 0 writes nothing; arguments the
    entry points refuse are an error"""
    import ctypes
    from UCF_VIT._hip import lib as L
    lib = L.load()
    args = (0, 2, 3, 9, 17, 16, 16, 3, 0, L.BF16, 16, 16, 2)
    name = b"strip-fast-share cpc16 ks3 nb1 4x8 depth2 rows8"
    assert _route_text(*args[:8], mode=2).encode() == name
    for cap, want in ((4, b"str\0x"), (1, b"\0xxxx"), (len(name), name[:-1] + b"\0x"), (len(name) + 1, name + b"\0x")):
        buf = ctypes.create_string_buffer(b"x" * 64, 64)
        assert lib.ucfvit_conv3d_route(*args, buf, cap) == len(name)
        assert buf.raw[:len(want)] == want, (cap, buf.raw)
    buf = ctypes.create_string_buffer(b"x" * 64, 64)
    assert lib.ucfvit_conv3d_route(*args, buf, 0) == len(name) and buf.raw == b"x" * 64
    for bad in ((0, 2, 3, 9, 17, 24, 16, 3, 0, L.BF16, 16, 16, 2), (1, 2, 3, 9, 17, 16, 24, 3, 0, L.BF16, 16, 16, 2), (0, 2, 3, 9, 17, 16, 16, 3, 0, L.BF16, 16, 17, 2),
                (2, 2, 3, 9, 17, 16, 16, 3, 0, L.BF16, 16, 16, 2), (0, 2, 3, 9, 17, 16, 16, 3, 0, L.BF16, 16, 16, 4)):
        assert lib.ucfvit_conv3d_route(*bad, buf, 64) < 0 and b"ucfvit_conv3d_route" in lib.ucfvit_last_error()
    assert buf.raw == b"x" * 64


@pytest.mark.parametrize("part", range(4))
def test_conv_tier1_wrong_references_differ_on_the_host(part):
    """CPU: the host half of Tier 1 over the whole table, a quarter per case (the selection cases and the two 140 000-voxel weight
    gradients are the same code at a larger volume: left to the GPU run): the exactness condition holds, and every wrong alternative differs
    from the right result in the faces and z-tile bands it guards"""
    for c in [c for c in FWD if c.forced][part::4]:
        _tier1_fwd(c, 1, "cpu", launch=False)
    for c in [c for c in WGRAD if c.B * c.X * c.Y * c.Z < 20000][part::4]:
        _tier1_w(c, "cpu", launch=False)


# ============================================================================================== forced modes
_CHILD = {"failed": None, "res": {}, "secs": {}}


def _run_payload(path):
    """child process: both tiers over the forced table under this process's UCFVIT_CONV_STRIP; the outputs of SAVE_EPIS go to the parent"""
    m = _mode()
    save = {}
    for c in FWD:
        if c.forced:
            _witness(c, m)
            _tier1_fwd(c, m, DEV, save=save)
            _tier2_fwd(c, m, DEV, save=save)
    torch.cuda.synchronize()
    for k in sorted(RATIOS):
        print(f"RATIO SUMMARY mode {m} {k}: {RATIOS[k]:.3f}")
    assert all(r <= 1.0 for r in RATIOS.values())
    torch.save(save, path)


@pytest.fixture(scope="module")
def child_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("conv_forced")


@gpu
@pytest.mark.parametrize("mode", ["0", "2", "3"])
def test_conv_forced_mode(mode, child_dir):
    """UCFVIT_CONV_STRIP = 0 / 2 / 3: the forced table, both tiers, in one fresh child each (a new process, never a replaced one)"""
    if _CHILD["failed"] is not None:
        pytest.fail(f"the forced child of mode {_CHILD['failed']} failed: no further child is started")
    f = child_dir / f"mode{mode}.pt"
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "run", str(f)], env=dict(os.environ, UCFVIT_CONV_STRIP=mode),
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _CHILD["failed"] = mode
        raise
    _CHILD["secs"][mode] = time.time() - t0
    print(f"CHILD mode {mode}: {_CHILD['secs'][mode]:.1f} s")
    print("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("RATIO SUMMARY")))
    if r.returncode != 0:
        _CHILD["failed"] = mode
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    _CHILD["res"][mode] = torch.load(f, weights_only=True)


@gpu
def test_conv_forced_modes_agree():
    """the parent's half: every Tier 1 output of every child against the float64 reference computed HERE, and the real-valued outputs of
    mode 0 against 2 against 3 bit for bit wherever no SHARE instantiation serves the case (the same MFMA order per output element)"""
    res = _CHILD["res"]
    assert sorted(res) == ["0", "2", "3"], "the three forced children must have run (test_conv_forced_mode) before this test"
    keys = sorted(res["0"])
    assert len(keys) > 100 and all(sorted(res[m]) == keys for m in res)
    n_exact = n_bits = n_share = 0
    for c in FWD:
        if not c.forced:
            continue
        o = _fwd_operands(c, "big", DEV)
        S = _conv64(o.x64, o.w64)
        for en in _epis(c):
            if en not in SAVE_EPIS:
                continue
            e = EPIS[en]
            right = _bits(_epi(c, e, o, S)[0].to(F32 if e.out32 else BF)).cpu()
            for m in res:
                assert torch.equal(res[m][f"{c.id}/{en}/big"], right), f"{c.id}/{en}: the child of mode {m} differs from the float64 result"
                n_exact += 1
            k = f"{c.id}/{en}/randn"
            share = any(_plan(c, e, m).share for m in (2, 3))
            assert torch.equal(res["2"][k], res["3"][k]), f"{k}: modes 2 and 3 (the same instantiation, FAST or branching) differ"
            if share:
                n_share += 1
            else:
                assert torch.equal(res["0"][k], res["2"][k]), f"{k}: modes 0 and 2 differ"
                n_bits += 1
    print(f"FORCED: {n_exact} exact comparisons, {n_bits} bit-identical triples, {n_share} SHARE cases (bounded in the children)")
    assert n_bits > 50 and n_share >= 4


@gpu
def test_conv_ratios_report():
    """last test of the file: the worst err / bound per kernel family seen by this process"""
    for k in sorted(RATIOS):
        print(f"RATIO SUMMARY {k}: {RATIOS[k]:.3f}")
    assert all(r <= 1.0 for r in RATIOS.values())


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        _run_payload(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "routes":
        print("kinds:", *_route_table())
    else:
        sys.exit("usage: test_conv3d_ops.py run OUT.pt | routes")
