"""Every kernel of csrc/quadtree.hip (the fixed-length quadtree / octree patcher: the INPUT of every adaptive-patching workload) element by
element: the tree builders bit for bit against the integer oracle, the two serializers against float64 references of the same formula, through
UCF_VIT._hip.ops (and UCF_VIT._hip.lib where outputs are carved from sentinel buffers or a raw refusal is wanted).  The references are numpy
float64 / Python ints written here; they never call the project's kernels.  The trees reuse oracle/quadtree_ref.py's build_tree / build_octree
(pinned to the reference's fixtures) through test_fast_tree_reference_is_the_oracle: ref_tree below is the same greedy rule on a summed-area
table, so that L = 6394 takes milliseconds.  The oracle's serialize (fp32, square only) is not used.  All inputs are drawn on the CPU from
seeds; B >= 2 throughout, so a batch-stride error lands in the other image.  U = 2^-24.

Kernels and the cases that reach them (test_tables_reach_every_branch asserts this list from the restated host rules smem_q / smem_o).  The
two builders are csrc/patcher_tree.h's tree_refine<ND> / tree_write<ND> for ND = 2 and 3: every branch of that one refinement is reached in
both dimensions by the q-* and the o-* cases below.
    quadtree_build_kernel      test_tree_build[q-*]: 12x20, 20x12, 7x5, 28x28, 96x160, 3x3, 2x2, 1x1 at L = 1, 4 and an L that stops early,
                               224x224 at L = 1024, 128x128 dense at L = 2728 (65,568 B of LDS: the first L above 64 KiB, hipFuncSetAttribute),
                               256x256 at L = 6394 (153,552 B: the largest accepted L); maps: all 0 (every step a tie), all 255, random 0 / 255,
                               arbitrary uint8 (so that / 255 floors); n > 256 (the strided scan / copy loops) from L = 1024 on
    sat3_x / _y / _z,          test_tree_build[o-*]: N = 1, 2, 6, 12, 20, 32 at L = 1, 8, 120, 225 (norm 255), N = 6 and 12 with norm 85 and 1,
      octree_build_kernel      N = 32 at L = 2045 (65,696 B: first above 64 KiB; B = 3, different densities), N = 32 and 64 at L = 4789 (153,504 B:
                               the largest accepted L; N = 32 has 4096 leaves at most and stops before L, N = 64 reaches it)
    quadtree_serialize_kernel  test_serialize[q2-*] (Tier 2) / [q1-*] (Tier 1): hand-made node lists in a 300 x 260 image (W x H), B = 2, leaves
                               (w, h) = (1,1) (2,2) (3,3) (1,5) (5,1) (3,7) (8,8) (13,9) (24,24) (127,64) (256,256), each at the top-left corner,
                               the bottom-right corner and in the interior; p = 8, 3, 16; C = 1, 3, 5 (p p C = 9 ... 1280: below and above the 256
                               threads); empty leaves (w = 0, h = 0, w < 0: the `w <= 0` branch), count below the number of valid-looking rows,
                               count = 0 (test_serialize_count_zero)
    octree_serialize_kernel    test_serialize[o2-*] / [o1-*]: extents (nx, ny, nz) = (1,1,1) (2,2,2) (3,1,2) (5,5,5) (12,7,3) (64,64,64)
                               (128,128,128) in an N = 128 volume (B = 2, C = 1), the first five also in an N = 20 volume with C = 2; p = 1 (inv = 0),
                               2, 4, 7; the same empty-leaf and count rows
    both pairs chained         test_build_then_serialize: 12x20 (L = 100) and 12^3 (L = 120), maps and images of their own

Tier 1, exact (np.array_equal on the bits; the conditions are computed in float64 from the operands and asserted by t1_conditions; the
*_on_the_host tests run the same cases through an fp32 numpy emulation of the kernels' expression order, which must then be exact too):
    bicubic, leaf extent an odd multiple of p (p, 3p, 5p, rectangular mixes): every sample lands on a pixel centre, the weights are exactly
        (0, 1, 0, 0) and the output is the centre pixel bit for bit for any finite fp32 image (randn * 1000 here; no -0, whose sign 0 + -0 drops)
    bicubic, even multiple (2p, 4p): t = 1/2, weights exactly (-3, 19, 19, -3) / 32; pixels are integers in [-64, 64], so all 16 products are
        multiples of 2^-10 with a magnitude sum below 2^24 of them: every partial sum in any order (and with or without fma) is an fp32 number
    trilinear p = 1: voxel (z1, y1, x1); p = 2: the eight corners; any finite image
    trilinear, p - 1 a power of two: n = 9 -> p = 3, 5, 9 (p - 1 divides n - 1: integer positions; p = n is the identity) and n = 6 -> 3,
        n = 4 -> 5, n = 7 -> 9 (fractional dyadic weights): inv, positions and weights are dyadic, integer voxels give exact results
    padding rows (s >= count[b]) and empty leaves (any extent <= 0) are exactly zero in both tiers

Tier 2, per-element bound on real-valued images (uniform [0, 255), randn, randn + 1000): |got - ref| <= t, ref the float64 value of the same
formula, t read off the kernel:
    bicubic: t = [8 U S(|wy|, |wx|) + S(dwy, |wx|) + S(|wy|, dwx) + dfy Sy(|wy'|, |wx|) + dfx Sx(|wy|, |wx'|)] (1 + 2^-10),
        S(a, b) = sum over the 16 taps of a b |tap|; Sx / Sy the same with |tap - the tap of column 1 in its row| / |tap - the tap of row 1 in
        its column|: the four w' sum to zero, so a constant per row (column) drops out of d out / d t, which tightens the issue's |tap| form.  8: product, 3 additions (0 + x is exact), product, 3 additions.  dw = (9 | 8) U ptilde(x):
        the outer / inner weight polynomials in Horner form take 6 / 5 roundings, their argument (t + 1, 1 - t, 2 - t) one more, which costs at
        most 3 U ptilde (x ptilde' <= 3 ptilde for a cubic with the coefficients' magnitudes, ptilde).  df = U (2 (px + 1/2) w / p + |f| + 1): the
        rounded sx, the product, the subtraction, and t = f - floor(f) (rounds only for f in (-1/2, 0)).  w' is the analytic derivative.
        1 + 2^-10 covers the second-order terms.
    trilinear: t = [9 U S(w) + sum over the axes of df (weighted |differences| of the four corner pairs along the axis)] (1 + 2^-10): per level
        1 - t, a product and the addition, three levels; d out / d t_axis is exactly that weighted difference;
        df = 3 U f (the rounded inv and two products; f - (int) f is exact).
    Where a position lies within df of an integer, floorf / (int) may pick the other cell; both choices are continuous neighbours.  The reference
    is therefore formed for every cell choice floor(f +- df) per axis (4 / 8 candidates) and an element passes if one of them satisfies the bound;
    such output elements are counted (printed as `ambiguous`; the aligned-corner positions that are exact integers are among them).  A bound that is infinite or exceeds the image's range fails the case.
Each d was validated before any GPU run: test_serialize_on_the_host runs the same cases on the fp32 emulation (err / bound <= 1).

Wrong references, all through Pool.check: over every Tier 2 case each applicable one must differ from every candidate of the right reference
by more than the bound somewhere (shown on the host) and be rejected by what the kernel wrote:
    A = -0.5 for -0.75; align_corners swapped (bicubic with aligned corners, trilinear with half-pixel centres); the x and y extents exchanged
    (rectangular leaves; trilinear: p > 1 only, at p = 1 the position is 0 whatever the extent); the leaf shifted by one pixel; border reflected
    (reflect-101) instead of clamped and clamping to the image instead of to the leaf (bicubic only: the aligned-corner trilinear rule never
    leaves the leaf); the trilinear scale n for n - 1 (p > 2: at p = 2 the far sample is clamped onto the same corner); channel c + 1 (C > 1);
    batch element b + 1.
    Trees (test_tree_build, test_tree_wrong_references_differ): the children order lt / rt / lb / rb permuted (every case with a split) and the
    LAST maximum instead of the first (every case with a split whose all-zero map ties at every step, and wherever else it differs).

Guards.  Images are carved from NaN-filled allocations, node lists and outputs from sentinel-filled ones; every call is made twice, once through
ops and once through the library into the carved outputs: both must agree bit for bit and the bytes beyond [B, L, ...] must be untouched.
test_refusals_write_nothing pins, with sentinel outputs and nothing launched: L = 0, 2, 3, 6397 (quadtree), L = 2, 7, 4796 (octree), N = 257,
norm_factor 0 and 256, H W 255 >= 2^32 and H = 32768 (through the argument check alone: tiny dummy allocations), N = 204 with norm_factor 1
(N^3 255 / norm >= 2^31: the int32 node value would go negative, no `v > bv` would fire and cur[0x7fffffff] would be read; refused since this
file; N = 203 is accepted and compared), B = 0 with null pointers (OK), p = 0 / L = 0 on the serializers; test_ops_refusals the same as ops
raises them plus wrong dtypes, wrong ranks, a non-cubic volume and non-contiguous tensors; test_patchify_refuses_bad_lengths the two modules.
Not covered: H or W above 300 in the serializer (the index arithmetic is int64 throughout), B L >= 2^31.

Measured on an MI355X: 105 GPU tests + 161 CPU tests, 5.4 s for the file; no test takes half a second (the 128^3 trilinear cases and the
largest L stay below 0.1 s each).  Every Tier 1 comparison and every tree was exact.  The offset family (randn + 1000) uses little of the
bicubic bound: what remains there is the rounding of the weights (the Horner bound, 8 - 9 U of a polynomial of magnitude up to 36) times |tap|.
Mutation check (nothing of it committed), one line each, the GPU half of this file against the mutated library:
    `oi < bi` -> `oi <= bi` in the wave reduction (both builders): all 105 passed; an equivalent mutant: lanes hold distinct indices (equal only
        when both are the empty 0x7fffffff), so the extra assignment copies a lane onto itself
    `h - 1` -> `H - 1` in the bicubic clamp (the wrong reference "image" on y): 22 failed, test_serialize on all 15 q2-* and all 6 q1-* cases
        and test_build_then_serialize[q-12x20-L100-B3]
    `nz - 1` -> `nz` in the trilinear scale (the wrong reference "scale"): 12 failed, test_serialize on all 8 o2-* cases with p > 2, the 3
        o1-dyadic-* cases, and test_build_then_serialize[o-12-L120-B3]; p = 1 and p = 2 cannot tell (position 0, and the clamped far corner)
  worst err / bound (host emulation | MI355X)      uniform          randn            randn + 1000
  quadtree_serialize, p = 8, 3, 16                 0.101 | 0.102    0.180 | 0.179    0.017 | 0.014
  octree_serialize, N = 128, C = 1                 0.351 | 0.351    0.332 | 0.215    0.327 | 0.338
  octree_serialize, N = 20, C = 2                  -                0.271 | 0.271    0.312 | 0.312
  build -> serialize, 12x20 / 12^3                 0.006 | 0.005 / 0.364 | 0.373
No defect found in the kernels' arithmetic: no ratio above 1, no sentinel touched, both LDS opt-in paths work up to 150 KiB.  Two changes to
the product belong with this file: ucfvit_octree_build refuses N^3 * 255 / norm_factor >= 2^31, and Patchify / Patchify_3D refuse a
fixed_length below 1 (-2 % 3 == 1 in Python let it through to the library).
"""
import functools
import math
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from oracle import quadtree_ref as QR

gpu = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
LIM = 2.0 ** 24
PAD = 64                                   # sentinel elements in front of and behind every carved tensor
ISENT = -77777                             # int32 sentinel
FSENT = -12352.0                           # fp32 sentinel
RATIOS = {}


def _ops():
    from UCF_VIT._hip import ops
    return ops


def _lib():
    from UCF_VIT._hip import lib
    return lib


# ---- csrc/quadtree.hip restated: node sizes, the LDS rule, the thread count ----------------------------------------------------------------
NT = 256
QNODE, ONODE = 12, 16                      # csrc/patcher_tree.h: sizeof(Node<2>) = 4 shorts + int, sizeof(Node<3>) = 6 shorts + int


def smem_q(L):
    return 2 * (L + 4) * QNODE


def smem_o(L):
    return 2 * (L + 8) * ONODE


LDS_OPT_IN, LDS_CAP = 64 * 1024, 150 * 1024


def _seed(*parts):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate("|".join(str(p) for p in parts))) % (2 ** 31)


def _rng(*parts):
    return np.random.Generator(np.random.PCG64(_seed(*parts)))


# ============================================================================================== trees: reference
def ref_tree(dom, L, norm=255, order=None, last=False):
    """the greedy refinement of FixedQuadTree / FixedOctTree (oracle/quadtree_ref.py build_tree / build_octree) on a summed-area table, in Python
    ints / int64.  dom uint8 [H, W] or [N, N, N] -> (nodes int64 [n, 4 | 6], values int64 [n]).  order: a permutation of the children (wrong
    reference); last: the last maximum instead of the first (wrong reference)."""
    dim = dom.ndim
    sat = np.pad(dom.astype(np.int64), [(1, 0)] * dim)
    for a in range(dim):
        sat = sat.cumsum(a)

    def val(k):
        if dim == 2:
            x1, x2, y1, y2 = k
            s = sat[y2, x2] - sat[y1, x2] - sat[y2, x1] + sat[y1, x1]
        else:
            x1, x2, y1, y2, z1, z2 = k
            s = (sat[z2, y2, x2] - sat[z1, y2, x2] - sat[z2, y1, x2] - sat[z2, y2, x1] + sat[z1, y1, x2] + sat[z1, y2, x1] + sat[z2, y1, x1]
                 - sat[z1, y1, x1])
        return int(s) // norm
    nk = 4 if dim == 2 else 8
    root = [0, dom.shape[1], 0, dom.shape[0]] if dim == 2 else [0, dom.shape[0], 0, dom.shape[1], 0, dom.shape[2]]
    nodes = np.zeros((L + nk, 2 * dim), np.int64)
    vals = np.zeros(L + nk, np.int64)
    nodes[0], vals[0], n = root, val(root), 1
    while n < L:
        idx = int(np.argmax(vals[:n])) if not last else n - 1 - int(np.argmax(vals[:n][::-1]))
        q = [int(v) for v in nodes[idx]]
        if q[1] - q[0] == 2:
            break
        if dim == 2:
            x1, x2, y1, y2 = q
            mx, my = (x1 + x2) // 2, (y1 + y2) // 2
            kids = [[x1, mx, my, y2], [mx, x2, my, y2], [x1, mx, y1, my], [mx, x2, y1, my]]                 # lt, rt, lb, rb
        else:
            x1, x2, y1, y2, z1, z2 = q
            mx, my, mz = (x1 + x2) // 2, (y1 + y2) // 2, (z1 + z2) // 2
            kids = [[xa, xb, ya, yb, za, zb] for (za, zb) in ((z1, mz), (mz, z2)) for (ya, yb) in ((y1, my), (my, y2))
                    for (xa, xb) in ((x1, mx), (mx, x2))]
        if order is not None:
            kids = [kids[o] for o in order]
        nodes[idx + nk:n + nk - 1] = nodes[idx + 1:n].copy()
        vals[idx + nk:n + nk - 1] = vals[idx + 1:n].copy()
        nodes[idx:idx + nk] = kids
        vals[idx:idx + nk] = [val(k) for k in kids]
        n += nk - 1
    return nodes[:n].copy(), vals[:n].copy()


def make_map(kind, shape, rng):
    if kind == "zero":
        return np.zeros(shape, np.uint8)
    if kind == "full":
        return np.full(shape, 255, np.uint8)
    if kind == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return (rng.random(shape) < float(kind[1:])).astype(np.uint8) * 255            # "r0.3": random 0 / 255 of that density


@dataclass(frozen=True)
class TreeC:
    dim: int
    shape: tuple             # (H, W) or (N,)
    L: int
    maps: tuple = ("zero", "full", "r0.3", "u8")
    norm: int = 255
    expect: frozenset = frozenset()        # edges this case is in the table for, asserted from the oracle's output

    @property
    def id(self):
        s = "x".join(str(v) for v in self.shape)
        return f"{'q' if self.dim == 2 else 'o'}-{s}-L{self.L}" + (f"-n{self.norm}" if self.norm != 255 else "") + f"-B{len(self.maps)}"

    @property
    def full_shape(self):
        return self.shape if self.dim == 2 else self.shape * 3


def _E(*names):
    return frozenset(names)


# expect: "w1" leaves of width 1, "nonsq" non-square (non-cubic) leaves, "zerow" a zero-width leaf, "early" stops before L, "big" more than 256 nodes
TREES = [
    TreeC(2, (12, 20), 1), TreeC(2, (12, 20), 4, expect=_E("nonsq")), TreeC(2, (12, 20), 100, expect=_E("w1", "nonsq", "early")),
    TreeC(2, (20, 12), 1), TreeC(2, (20, 12), 4, expect=_E("nonsq")), TreeC(2, (20, 12), 100, expect=_E("w1", "nonsq", "early")),
    TreeC(2, (7, 5), 1), TreeC(2, (7, 5), 4, expect=_E("nonsq")), TreeC(2, (7, 5), 40, expect=_E("w1", "nonsq", "early")),
    TreeC(2, (28, 28), 1), TreeC(2, (28, 28), 4), TreeC(2, (28, 28), 196, expect=_E("w1", "nonsq", "early")),
    TreeC(2, (96, 160), 1), TreeC(2, (96, 160), 4, expect=_E("nonsq")), TreeC(2, (96, 160), 4000, expect=_E("nonsq", "early", "big")),
    TreeC(2, (3, 3), 1), TreeC(2, (3, 3), 4, expect=_E("w1", "nonsq")), TreeC(2, (3, 3), 40, expect=_E("w1", "zerow")),
    TreeC(2, (2, 2), 1), TreeC(2, (2, 2), 4, expect=_E("early")), TreeC(2, (2, 2), 40, expect=_E("early")),
    TreeC(2, (1, 1), 1), TreeC(2, (1, 1), 4, expect=_E("zerow")), TreeC(2, (1, 1), 40, expect=_E("zerow")),
    TreeC(2, (224, 224), 1024, ("zero", "r0.05", "u8"), expect=_E("big")),
    TreeC(2, (128, 128), 2728, ("full", "r0.9"), expect=_E("big")),
    TreeC(2, (256, 256), 6394, ("full", "r0.5", "zero"), expect=_E("big", "early")),
]
for _N in (1, 2, 6, 12, 20, 32):
    for _L in (1, 8, 120, 225):
        TREES.append(TreeC(3, (_N,), _L))
TREES += [TreeC(3, (6,), 120, norm=85), TreeC(3, (6,), 120, norm=1), TreeC(3, (12,), 120, norm=85), TreeC(3, (12,), 225, norm=1),
          TreeC(3, (32,), 2045, ("full", "r0.5", "r0.05"), expect=_E("big")),
          TreeC(3, (32,), 4789, ("full", "r0.5"), expect=_E("big", "early")),
          TreeC(3, (64,), 4789, ("full", "u8"), expect=_E("big"))]
O_EXPECT = {"o-12-L120-B4": _E("w1"), "o-1-L8-B4": _E("zerow"), "o-2-L8-B4": _E("early"), "o-6-L120-B4": _E("w1", "nonsq")}
PERM2, PERM3 = (1, 0, 2, 3), (0, 2, 1, 3, 4, 5, 6, 7)          # rt before lt; y before x


def _pad_tree(nodes, vals, L, dim):
    """what the kernels write for one image: [L, 2 dim] nodes, [L] values, count, [L, 1 + dim] (size, centres); padding 0 / 0 / (0, -1, ...)"""
    n = len(nodes)
    no = np.zeros((L, 2 * dim), np.int32)
    va = np.zeros(L, np.int32)
    sp = np.zeros((L, 1 + dim), np.float32)
    sp[:, 1:] = -1.0
    no[:n], va[:n] = nodes, vals
    sp[:n, 0] = (nodes[:, 1] - nodes[:, 0]).astype(np.float32)
    for a in range(dim):
        sp[:n, 1 + a] = (nodes[:, 2 * a + 1] + nodes[:, 2 * a]).astype(np.float32) * np.float32(0.5)
    return no, va, n, sp


@functools.lru_cache(maxsize=None)
def tree_ref(c):
    rng = _rng("tree", c.id)
    maps = np.stack([make_map(k, c.full_shape, rng) for k in c.maps])
    out = {"maps": maps}
    for name, kw in (("right", {}), ("perm", {"order": PERM2 if c.dim == 2 else PERM3}), ("last", {"last": True})):
        parts = [_pad_tree(*ref_tree(m, c.L, c.norm, **kw), c.L, c.dim) for m in maps]
        out[name] = tuple(np.stack([p[i] for p in parts]) if i != 2 else np.array([p[2] for p in parts], np.int32) for i in range(4))
    return out


def tree_flags(c):
    """the edges the oracle's output of this case shows, over its batch"""
    nodes, _, count, _ = tree_ref(c)["right"]
    f = set()
    for b in range(len(count)):
        n = nodes[b, :count[b]].astype(np.int64)
        ext = n[:, 1::2] - n[:, 0::2]
        if (ext[:, 0] == 1).any():
            f.add("w1")
        if (ext != ext[:, :1]).any():
            f.add("nonsq")
        if (ext == 0).any():
            f.add("zerow")
        if count[b] < c.L:
            f.add("early")
        if count[b] > 256:
            f.add("big")
    return f


def _expect(c):
    return c.expect | O_EXPECT.get(c.id, frozenset())


# ============================================================================================== serializers: one sampler per kernel
def cubic_weights(t, A, ft):
    """cubic_coeffs of the kernel in its expression order, in the float type ft -> [4, ...]"""
    A, one, two = ft(A), ft(1), ft(2)
    f5, f8, f4, a2, a3 = ft(5) * A, ft(8) * A, ft(4) * A, A + ft(2), A + ft(3)
    x0, x1, x2, x3 = t + one, t, one - t, two - t
    return np.stack([((A * x0 - f5) * x0 + f8) * x0 - f4, (a2 * x1 - a3) * x1 * x1 + one, (a2 * x2 - a3) * x2 * x2 + one,
                     ((A * x3 - f5) * x3 + f8) * x3 - f4])


def cubic_bounds(t, A):
    """float64: (|dw / dt| [4, ...], rounding bound of the fp32 weights [4, ...])"""
    a, a2, a3 = abs(A), A + 2, A + 3
    dpo = lambda x: 3 * A * x * x - 10 * A * x + 8 * A                                   # noqa: E731
    dpi = lambda x: 3 * a2 * x * x - 2 * a3 * x                                          # noqa: E731
    pto = lambda x: a * x ** 3 + 5 * a * x * x + 8 * a * x + 4 * a                       # noqa: E731
    pti = lambda x: a2 * x ** 3 + a3 * x * x + 1                                         # noqa: E731
    x0, x1, x2, x3 = np.abs(t + 1), np.abs(t), np.abs(1 - t), np.abs(2 - t)
    dw = np.abs(np.stack([dpo(t + 1), dpi(t), dpi(1 - t), dpo(2 - t)]))
    rb = U * np.stack([9 * pto(x0), 8 * pti(x1), 8 * pti(x2), 9 * pto(x3)])
    return dw, rb


def _reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    per = 2 * (n - 1)
    m = np.mod(i, per)
    return np.where(m >= n, per - m, m)


def bicubic_leaf(img, node, p, ft=np.float64, A=-0.75, align=False, swap=False, shift=0, border="leaf", chan=0, bias=(0, 0), bound=False):
    """one leaf of quadtree_serialize_kernel: img [H, W, C] fp32, node (x1, x2, y1, y2) -> out [p, p, C] in ft (+ the bound, + the cells).
    ft = float32 with the defaults is the emulation of the kernel; float64 the reference; the other arguments form the wrong references;
    bias (ex, ey) in {-1, 0, 1}: the cell is floor(f + e df)."""
    H, W, C = img.shape
    x1, x2, y1, y2 = (int(v) for v in node)
    w, h = x2 - x1, y2 - y1
    if swap:
        w, h = h, w
    x1 += shift
    k = np.arange(p)

    def axis(n, e, lo, size):
        kf = k.astype(ft)
        if align:
            f = kf * ft(n - 1) / ft(max(p - 1, 1))
        else:
            f = (kf + ft(0.5)) * (ft(n) / ft(p)) - ft(0.5)
        df = U * (2 * (k + 0.5) * n / p + np.abs(f.astype(np.float64)) + 1)
        fl = np.floor(f + ft(e) * df.astype(ft)) if e else np.floor(f)
        t = f - fl
        i = fl.astype(np.int64)[None, :] - 1 + np.arange(4)[:, None]                      # [4 taps, p]
        if border == "leaf":
            i = np.clip(i, 0, n - 1)
        elif border == "reflect":
            i = _reflect101(i, n)
        return t, df, np.clip(i + lo, 0, size - 1), fl.astype(np.int64)                  # "image": only the clip to the image
    tx, dfx, X, cx = axis(w, bias[0], x1, W)
    ty, dfy, Y, cy = axis(h, bias[1], y1, H)
    wx, wy = cubic_weights(tx, A, ft), cubic_weights(ty, A, ft)                           # [4, p]
    taps = img[Y[:, :, None, None], X[None, None, :, :], :]                               # [4, p(y), 4, p(x), C]
    if chan:
        taps = taps[..., (np.arange(C) + chan) % C]
    taps = taps.astype(ft)
    acc = np.zeros((p, p, C), ft)
    for a in range(4):
        r = np.zeros((p, p, C), ft)
        for d in range(4):
            r = r + wx[d][None, :, None] * taps[a, :, d, :, :]
        acc = acc + wy[a][:, None, None] * r
    if not bound:
        return acc
    S = lambda ay, ax, v=np.abs(taps): np.einsum("ap,dq,apdqc->pqc", ay, ax, v)           # noqa: E731
    dtx, dty = np.abs(taps - taps[:, :, 1:2]), np.abs(taps - taps[1:2])                   # sum of w' is 0: any constant per row / column drops out
    dwx, rbx = cubic_bounds(tx, A)
    dwy, rby = cubic_bounds(ty, A)
    awx, awy = np.abs(wx), np.abs(wy)
    t = (8 * U * S(awy, awx) + S(rby, awx) + S(awy, rbx) + S(dwy * dfy[None, :], awx, dty) + S(awy, dwx * dfx[None, :], dtx)) * (1 + 2.0 ** -10)
    return acc, t, (cx, cy)


def trilinear_leaf(img, node, p, ft=np.float64, align=True, swap=False, shift=0, chan=0, scale_n=False, bias=(0, 0, 0), bound=False):
    """one leaf of octree_serialize_kernel: img [N, N, N, C] fp32 indexed [z][y][x], node (x1, x2, y1, y2, z1, z2) -> out [p(z), p(y), p(x), C]"""
    N, C = img.shape[0], img.shape[-1]
    x1, x2, y1, y2, z1, z2 = (int(v) for v in node)
    nx, ny, nz = x2 - x1, y2 - y1, z2 - z1
    if swap:
        nx, ny = ny, nx
    x1 += shift
    k = np.arange(p)

    def axis(n, e, lo):
        kf = k.astype(ft)
        if align:
            inv = ft(1) / ft(p - 1) if p > 1 else ft(0)
            f = kf * ft(n if scale_n else n - 1) * inv                                 # scale_n: n for n - 1 (wrong reference)
        else:
            f = np.maximum((kf + ft(0.5)) * (ft(n) / ft(p)) - ft(0.5), ft(0))
        df = 3 * U * f.astype(np.float64)
        i0 = np.clip(np.floor(f + ft(e) * df.astype(ft)).astype(np.int64), 0, n - 1)
        t = f - i0.astype(ft)
        i1 = np.minimum(i0 + 1, n - 1)
        return t, df, np.clip(i0 + lo, 0, N - 1), np.clip(i1 + lo, 0, N - 1), i0
    tx, dfx, X0, X1, cx = axis(nx, bias[0], x1)
    ty, dfy, Y0, Y1, cy = axis(ny, bias[1], y1)
    tz, dfz, Z0, Z1, cz = axis(nz, bias[2], z1)

    def at(Z, Y, X):
        v = img[Z[:, None, None], Y[None, :, None], X[None, None, :], :]
        if chan:
            v = v[..., (np.arange(C) + chan) % C]
        return v.astype(ft)
    one = ft(1)
    TX, TY, TZ = tx[None, None, :, None], ty[None, :, None, None], tz[:, None, None, None]
    corner = {(a, b, d): at((Z0, Z1)[a], (Y0, Y1)[b], (X0, X1)[d]) for a in (0, 1) for b in (0, 1) for d in (0, 1)}
    c00 = corner[0, 0, 0] * (one - TX) + corner[0, 0, 1] * TX
    c01 = corner[0, 1, 0] * (one - TX) + corner[0, 1, 1] * TX
    c10 = corner[1, 0, 0] * (one - TX) + corner[1, 0, 1] * TX
    c11 = corner[1, 1, 0] * (one - TX) + corner[1, 1, 1] * TX
    c0 = c00 * (one - TY) + c01 * TY
    c1 = c10 * (one - TY) + c11 * TY
    out = c0 * (one - TZ) + c1 * TZ
    if not bound:
        return out
    WX, WY, WZ = (np.abs(one - TX), np.abs(TX)), (np.abs(one - TY), np.abs(TY)), (np.abs(one - TZ), np.abs(TZ))
    DX, DY, DZ = dfx[None, None, :, None], dfy[None, :, None, None], dfz[:, None, None, None]
    t = 0.0
    for (a, b, d), v in corner.items():
        t = t + np.abs(v) * 9 * U * WZ[a] * WY[b] * WX[d]
    for a in (0, 1):                                                                      # d out / d t_axis = the weighted differences of the corner pairs
        for b in (0, 1):
            t = t + DX * WZ[a] * WY[b] * np.abs(corner[a, b, 1] - corner[a, b, 0])
            t = t + DY * WZ[a] * WX[b] * np.abs(corner[a, 1, b] - corner[a, 0, b])
            t = t + DZ * WY[a] * WX[b] * np.abs(corner[1, a, b] - corner[0, a, b])
    return out, t * (1 + 2.0 ** -10), (cx, cy, cz)


def serialize_all(dim, imgs, nodes, count, p, ft=np.float64, batch=0, bias=None, bound=False, **variant):
    """the whole launch: imgs [B, ...] fp32, nodes [B, S, 2 dim], count [B] -> [B, S, p .. p, C] in ft; zero patches for s >= count[b] and for
    leaves with an extent <= 0.  batch: read the image of batch element b + batch (wrong reference)"""
    B, S = nodes.shape[:2]
    C = imgs.shape[-1]
    leaf = bicubic_leaf if dim == 2 else trilinear_leaf
    out = np.zeros((B, S) + (p,) * dim + (C,), ft)
    tol = np.zeros(out.shape, np.float64) if bound else None
    cells = {}
    for b in range(B):
        for s in range(min(int(count[b]), S)):
            nd = nodes[b, s]
            if ((nd[1::2] - nd[0::2]) <= 0).any():
                continue
            kw = dict(variant)
            if bias is not None:
                kw["bias"] = bias
            r = leaf(imgs[(b + batch) % B], nd, p, ft, bound=bound, **kw)
            if bound:
                out[b, s], tol[b, s], cells[b, s] = r
            else:
                out[b, s] = r
    return (out, tol, cells) if bound else out


# ---- node lists
QW, QH = 300, 260
Q_EXT = [(1, 1), (2, 2), (3, 3), (1, 5), (5, 1), (3, 7), (8, 8), (13, 9), (24, 24), (127, 64), (256, 256)]
O_EXT = [(1, 1, 1), (2, 2, 2), (3, 1, 2), (5, 5, 5), (12, 7, 3), (64, 64, 64), (128, 128, 128)]


def _place(ext, size, where):
    """where 0: at the origin (touches the left / top borders), 1: at the far corner (right / bottom), 2: interior (where there is room)"""
    out = []
    for a, (e, n) in enumerate(zip(ext, size)):
        room = n - e
        lo = 0 if where == 0 else (room if where == 1 else min(room // 2, 17 + 5 * a))
        out += [lo, lo + e]
    return out


def _empties(dim):
    if dim == 2:
        return [[5, 5, 3, 9], [5, 9, 3, 3], [9, 5, 3, 9], [0, 0, 0, 0]]                  # w = 0, h = 0, w < 0, the padding row
    return [[5, 5, 3, 9, 2, 4], [5, 9, 3, 3, 2, 4], [5, 9, 3, 9, 4, 2], [0, 0, 0, 0, 0, 0]]


def node_list(dim, exts, size):
    """B = 2: every extent at three places, the empty leaves in between; batch element 1 has the list reversed; count[0] leaves the last three
    (valid-looking) rows out, count[1] takes all"""
    rows = [_place(e, size, wh) for e in exts for wh in (0, 1, 2)]
    em = _empties(dim)
    for i, r in enumerate(em):
        rows.insert(2 * i + 1, r)
    a = np.array(rows, np.int32)
    nodes = np.stack([a, a[::-1].copy()])
    return nodes, np.array([len(rows) - 3, len(rows)], np.int32)


@dataclass(frozen=True)
class SerC:
    dim: int
    tier: int
    kind: str                # node list: "t2" | "t2small" (octree, N = 20) | "odd" | "even" | "p1" | "p2" | "dyadic"
    p: int
    C: int
    fam: str                 # "uniform" | "randn" | "randn1000" | "int" | "wild"

    @property
    def id(self):
        return f"{'q' if self.dim == 2 else 'o'}{self.tier}-{self.kind}-p{self.p}-C{self.C}-{self.fam}"

    @property
    def size(self):
        if self.dim == 2:
            return (QW, QH)
        return (128,) * 3 if self.kind == "t2" else (20,) * 3


FAMS = ("uniform", "randn", "randn1000")
SERS = [SerC(2, 2, "t2", 8, C, f) for C in (1, 3, 5) for f in FAMS]
SERS += [SerC(2, 2, "t2", p, (1, 3, 5)[(i + j) % 3], f) for i, p in enumerate((3, 16)) for j, f in enumerate(FAMS)]
SERS += [SerC(3, 2, "t2", p, 1, FAMS[i % 3]) for i, p in enumerate((1, 2, 4, 7))] + [SerC(3, 2, "t2", 7, 1, f) for f in FAMS[1:]]
SERS += [SerC(3, 2, "t2small", p, 2, f) for p in (1, 2, 4, 7) for f in FAMS[(p % 3):(p % 3) + 2]]
SERS += [SerC(2, 1, "odd", p, C, "wild") for p, C in ((8, 3), (3, 5), (16, 1))]
SERS += [SerC(2, 1, "even", p, C, "int") for p, C in ((8, 5), (3, 1), (16, 3))]
SERS += [SerC(3, 1, "p1", 1, 2, "wild"), SerC(3, 1, "p2", 2, 2, "wild"), SerC(3, 1, "p1", 1, 1, "wild")]
SERS += [SerC(3, 1, "dyadic", p, C, "int") for p, C in ((3, 2), (5, 1), (9, 2))]


def ser_exts(c):
    p = c.p
    if c.kind == "t2":
        return Q_EXT if c.dim == 2 else O_EXT
    if c.kind == "t2small":
        return O_EXT[:5]
    if c.kind == "odd":
        return [(p, p), (3 * p, p), (5 * p, 3 * p), (p, 5 * p), (3 * p, 3 * p)]
    if c.kind == "even":
        return [(2 * p, 2 * p), (4 * p, 2 * p), (2 * p, 4 * p), (4 * p, 4 * p)]
    if c.kind in ("p1", "p2"):
        return O_EXT[:5]
    return [(9, 9, 9), ({3: 6, 5: 4, 9: 7}[p],) * 3, (9, {3: 6, 5: 4, 9: 7}[p], 1)]       # dyadic


def make_images(c):
    B = 2
    shape = (B, QH, QW, c.C) if c.dim == 2 else (B,) + c.size + (c.C,)
    g = torch.Generator().manual_seed(_seed("img", c.id))
    if c.fam == "uniform":
        v = torch.rand(shape, generator=g, dtype=torch.float32) * 255
    elif c.fam == "int":
        v = torch.randint(-64, 65, shape, generator=g).float()
    else:
        v = torch.randn(shape, generator=g, dtype=torch.float32)
        v = v + 1000.0 if c.fam == "randn1000" else (v * 1000.0 if c.fam == "wild" else v)
    v = v.numpy()
    v[v == 0] = 0.0                                                                      # no -0: the kernels' 0.f + (0 * x) drops its sign
    return v


def _biases(dim):
    return [tuple(b) for b in np.array(np.meshgrid(*[(-1, 1)] * dim)).T.reshape(-1, dim)]


def wrong_variants(c):
    """name -> keyword arguments of serialize_all for every wrong reference that applies to the case"""
    w = {"align": {"align": c.dim == 2}, "shift": {"shift": 1}, "batch": {"batch": 1}}
    if c.C > 1:
        w["chan"] = {"chan": 1}
    if c.dim == 2:
        w.update({"A": {"A": -0.5}, "swap": {"swap": True}, "reflect": {"border": "reflect"}, "image": {"border": "image"}})
    elif c.p > 1:
        w["swap"] = {"swap": True}
        if c.p > 2:                                                                       # at p = 2 the far sample is clamped onto the same corner
            w["scale"] = {"scale_n": True}
    return w


@functools.lru_cache(maxsize=None)
def ser_ref(c):
    imgs = make_images(c)
    nodes, count = node_list(c.dim, ser_exts(c), c.size)
    cands, tol, seen = [], None, {}
    for bias in _biases(c.dim):
        o, t, cells = serialize_all(c.dim, imgs, nodes, count, c.p, bias=bias, bound=True)
        cands.append(o)
        tol = t if tol is None else np.maximum(tol, t)
        for k, cs in cells.items():
            seen.setdefault(k, []).append(cs)
    amb = 0                                                                               # output elements with more than one cell choice on some axis
    for k, lst in seen.items():
        per_axis = [np.any([cs[a] != lst[0][a] for cs in lst], axis=0) for a in range(c.dim)]             # [p] per axis (x, y(, z))
        grid = np.zeros((c.p,) * c.dim, bool)
        for a, m in enumerate(per_axis):
            grid |= m.reshape([-1 if i == c.dim - 1 - a else 1 for i in range(c.dim)])
        amb += int(grid.sum()) * c.C
    wrongs = {n: serialize_all(c.dim, imgs, nodes, count, c.p, **kw) for n, kw in wrong_variants(c).items()} if c.tier == 2 else {}
    return dict(imgs=imgs, nodes=nodes, count=count, cands=cands, tol=tol, wrongs=wrongs, ambiguous=amb)


class Pool:
    """every comparison of the serializers goes through check(): the result must be within the bound of one candidate of the right reference per
    element, and every wrong reference must (a) differ from all candidates by more than the bound somewhere and (b) be rejected"""

    def __init__(self, what, backend):
        self.what, self.backend, self.rej, self.differs = what, backend, {}, {}

    @staticmethod
    def _err(x, cands):
        return np.min(np.stack([np.abs(x.astype(np.float64) - r) for r in cands]), axis=0)

    def check(self, kernel, family, got, cands, tol, wrongs=None):
        assert got.shape == cands[0].shape, f"{self.what}: shape {got.shape} against {cands[0].shape}"
        assert not np.isnan(got).any(), f"{self.what} {kernel} {family}: NaN in the result"
        assert np.isfinite(tol).all(), f"{self.what} {kernel} {family}: the bound is vacuous (infinite)"
        err = self._err(got, cands)
        q = np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))
        r = float(q.max())
        key = f"{kernel} {family} [{self.backend}]"
        RATIOS[key] = max(RATIOS.get(key, 0.0), r)
        print(f"RATIO {key} {self.what}: worst err/bound {r:.3f}")
        bad = err > tol
        assert not bad.any(), (f"{self.what} {kernel} {family}: {int(bad.sum())} of {bad.size} elements out of bound, worst err/bound {r:.3g}, "
                               f"first at {np.argwhere(bad)[0].tolist()}")
        for name, w in (wrongs or {}).items():
            self.differs[name] = bool((self._err(w, cands) > tol).any())
            self.rej[name] = bool((np.abs(got.astype(np.float64) - w) > tol).any())

    def done(self, need=()):
        assert set(need) <= set(self.rej), f"{self.what}: wrong references never formed: {sorted(set(need) - set(self.rej))}"
        same = [k for k, d in self.differs.items() if not d]
        assert not same, f"{self.what}: wrong references within the bound of the right one: {same}"
        missed = [k for k, r in self.rej.items() if not r]
        assert not missed, f"{self.what}: the bound does not reject the wrong references {missed}"


def t1_conditions(c, R):
    """the exactness conditions of a Tier 1 case, computed in float64 from the operands"""
    imgs, nodes, count = R["imgs"], R["nodes"], R["count"]
    assert np.isfinite(imgs).all() and not np.signbit(imgs[imgs == 0]).any()
    assert all(np.array_equal(R["cands"][0], k) for k in R["cands"][1:]), f"{c.id}: a position is not exactly on its cell"
    assert float(R["tol"].max()) < math.inf
    p = c.p
    k = np.arange(p, dtype=np.float64)
    for b in range(2):
        for s in range(int(count[b])):
            ext = (nodes[b, s, 1::2] - nodes[b, s, 0::2]).astype(np.int64)
            if (ext <= 0).any():
                continue
            for n in ext:
                if c.dim == 2:
                    f = (k + 0.5) * (float(n) / p) - 0.5
                    t = f - np.floor(f)
                    w = cubic_weights(t, -0.75, np.float64)
                    if c.kind == "odd":
                        assert n % (2 * p) == p and (t == 0).all() and (w == np.array([0.0, 1, 0, 0])[:, None]).all()
                    else:
                        assert n % (2 * p) == 0 and (t == 0.5).all() and (w * 32 == np.array([-3.0, 19, 19, -3])[:, None]).all()
                elif c.kind == "p1":
                    assert p == 1
                elif c.kind == "p2":
                    assert p == 2                                                        # positions 0 and (n - 1) * 1.f: the corners
                else:
                    assert (p - 1) & (p - 2) == 0                                         # inv = 1 / (p - 1) is a power of two
                    f = k * (n - 1) / (p - 1)
                    assert (f * (p - 1) == np.round(f * (p - 1))).all() and np.float32(1) / np.float32(p - 1) == 1.0 / (p - 1)
    if c.fam == "int":
        # every product is a multiple of q with the magnitude sum below 2^24 q: any order of fp32 additions, fused or not, is exact
        q = 2.0 ** -10 if c.dim == 2 else 1.0 / (p - 1) ** 3
        assert (imgs == np.round(imgs)).all()
        mag = 4.0 * np.abs(imgs).max() if c.dim == 2 else np.abs(imgs).max()            # sum |wy| |wx| = (44 / 32)^2 < 4; trilinear weights sum to 1
        assert mag / q < LIM


def _check_case(c, got, backend):
    R = ser_ref(c)
    kern = "quadtree_serialize" if c.dim == 2 else "octree_serialize"
    B, S = R["nodes"].shape[:2]
    # rows that must be exactly zero: padding and empty leaves
    for b in range(B):
        for s in range(S):
            nd = R["nodes"][b, s]
            if s >= R["count"][b] or ((nd[1::2] - nd[0::2]) <= 0).any():
                assert not got[b, s].any() and not np.signbit(got[b, s]).any(), f"{c.id}: row {b},{s} is not exactly zero"
    if c.tier == 1:
        t1_conditions(c, R)
        want = R["cands"][0].astype(np.float32)
        assert np.array_equal(want.astype(np.float64), R["cands"][0]), f"{c.id}: the float64 result is no fp32 number"
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), \
            f"{c.id} [{backend}]: not bit for bit, {int((got != want).sum())} elements differ, worst {np.abs(got - want).max()}"
        return
    span = float(R["imgs"].max() - R["imgs"].min())
    assert float(R["tol"].max()) < span, f"{c.id}: the bound {R['tol'].max()} exceeds the image's range {span}"
    pool = Pool(c.id, backend)
    pool.check(kern, c.fam, got, R["cands"], R["tol"], R["wrongs"])
    pool.done(wrong_variants(c))
    print(f"{c.id}: {R['ambiguous']} of {int((R['tol'] > 0).sum())} elements ambiguous (a position within its error of an integer)")


# ============================================================================================== the library on carved buffers
def _carve(a, fill):
    """numpy array -> (view on the device in the middle of a sentinel-filled allocation, the allocation)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device=DEV)
    buf[PAD:PAD + t.numel()] = t.reshape(-1).to(DEV)
    return buf[PAD:PAD + t.numel()].view(t.shape), buf


def _carve_out(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    return buf[PAD:PAD + n].view(shape), buf


def _guards_ok(buf, fill):
    n = buf.numel() - 2 * PAD
    return bool((buf[:PAD] == fill).all()) and bool((buf[PAD + n:] == fill).all())


def _untouched(buf, fill):
    return bool((buf == fill).all())


def _bits_equal(a, b):
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    return a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                              b.view(torch.int32) if b.dtype == torch.float32 else b)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tree_outs(B, L, dim):
    return [_carve_out((B, L, 2 * dim), torch.int32, ISENT), _carve_out((B, L), torch.int32, ISENT), _carve_out((B,), torch.int32, ISENT),
            _carve_out((B, L, 1 + dim), torch.float32, FSENT)]


def _raw_build(dim, dom, L, norm, outs, shape=None, ws=None):
    """the library call as ops makes it, into the given outputs -> return code.  shape: (B, H, W) / (B, N) to claim instead of dom's own"""
    lib, ops = _lib().load(), _ops()
    o = [v.data_ptr() for v, _ in outs]
    if dim == 2:
        B, H, W = shape or dom.shape
        ws = ws if ws is not None else ops.workspace(lib.ucfvit_quadtree_workspace(B, H, W), dom.device)
        return lib.ucfvit_quadtree_build(dom.data_ptr(), *o, B, H, W, L, ws.data_ptr(), _stream())
    B, N = shape or dom.shape[:2]
    ws = ws if ws is not None else ops.workspace(lib.ucfvit_octree_workspace(B, N), dom.device)
    return lib.ucfvit_octree_build(dom.data_ptr(), *o, B, N, L, norm, ws.data_ptr(), _stream())


def hip_build(c, maps):
    """ops.*_build, then the library into sentinel-carved outputs: both bit for bit the same, nothing written beyond [B, L, ...]"""
    ops = _ops()
    dom, _ = _carve(maps, 7)
    a = ops.quadtree_build(dom, c.L) if c.dim == 2 else ops.octree_build(dom, c.L, c.norm)
    outs = _tree_outs(len(maps), c.L, c.dim)
    assert _raw_build(c.dim, dom, c.L, c.norm, outs) == 0, _lib().load().ucfvit_last_error()
    torch.cuda.synchronize()
    for (v, buf), x, fill in zip(outs, a, (ISENT, ISENT, ISENT, FSENT)):
        assert _bits_equal(v, x), f"{c.id}: a second build on the same maps differs"
        assert _guards_ok(buf, fill), f"{c.id}: bytes beyond the outputs were written"
    return [x.cpu().numpy() for x in a]


def hip_serialize(c, imgs, nodes, count, flat=True):
    """ops.*_serialize on carved inputs (in its [B, C, S, p^dim] view unless flat=False), then the library into a sentinel-carved output"""
    ops, lib = _ops(), _lib().load()
    B, S, p, C, dim = nodes.shape[0], nodes.shape[1], c.p, imgs.shape[-1], c.dim
    im, _ = _carve(imgs, float("nan"))
    nd, _ = _carve(nodes, ISENT)
    ct, _ = _carve(count, ISENT)
    if dim == 2:
        a = ops.quadtree_serialize(im, nd, ct, p)
        assert tuple(a.shape) == (B, C, S, p * p)
    else:
        a = ops.octree_serialize(im, nd, ct, p, flat=flat)
        assert tuple(a.shape) == ((B, C, S, p ** 3) if flat else (B, S, p, p, p, C))
    out, buf = _carve_out((B, S) + (p,) * dim + (C,), torch.float32, FSENT)
    if dim == 2:
        rc = lib.ucfvit_quadtree_serialize(im.data_ptr(), nd.data_ptr(), ct.data_ptr(), out.data_ptr(), B, imgs.shape[1], imgs.shape[2], C, S, p,
                                           _stream())
    else:
        rc = lib.ucfvit_octree_serialize(im.data_ptr(), nd.data_ptr(), ct.data_ptr(), out.data_ptr(), B, imgs.shape[1], C, S, p, _stream())
    assert rc == 0, lib.ucfvit_last_error()
    torch.cuda.synchronize()
    assert _bits_equal(out.view(a.shape), a), f"{c.id}: a second call on the same inputs differs"
    assert _guards_ok(buf, FSENT), f"{c.id}: bytes beyond the output were written"
    return a.cpu().numpy()


def as_view(ref, dim, flat=True):
    """what np.reshape([S, p .. p, C] -> [C, S, p^dim]) of the patch list holds per batch element (transform.py:44-48, :123-126), built by explicit
    indexing: element (c', s', j') of the result is element number (c' S + s') p^dim + j' of the list in its own row-major order, i.e. list element
    (s, pixel, c) with s = e // (p^dim C), pixel = (e // C) % p^dim, c = e % C"""
    if not flat:
        return ref
    B, S, C = ref.shape[0], ref.shape[1], ref.shape[-1]
    P = int(np.prod(ref.shape[2:-1]))
    lst = np.stack([ref[..., c].reshape(B, S, P) for c in range(C)], axis=-1)             # [B, S, pixel, C] with the pixels of a patch numbered row-major
    cv, sv, jv = np.indices((C, S, P))
    e = (cv * S + sv) * P + jv
    return lst[:, e // (P * C), (e // C) % P, e % C]


def from_view(got, like):
    """undo as_view (the same memory order) so that rows and leaves can be addressed"""
    return got.reshape(like.shape)


# ============================================================================================== tests: trees
_T_IDS = [c.id for c in TREES]


def test_fast_tree_reference_is_the_oracle():
    """ref_tree == oracle.quadtree_ref.build_tree / build_octree (pinned to the reference's fixtures) on every case the oracle does quickly"""
    n = 0
    for c in TREES:
        if c.L > 1024 or np.prod(c.full_shape) > 60000:
            continue
        R = tree_ref(c)
        for b, m in enumerate(R["maps"]):
            on, ov = QR.build_tree(m, c.L) if c.dim == 2 else QR.build_octree(m, c.L, c.norm)
            cnt = int(R["right"][2][b])
            assert cnt == len(on), (c.id, b)
            assert np.array_equal(R["right"][0][b, :cnt], np.array(on, np.int32).reshape(cnt, -1)), (c.id, b)
            assert np.array_equal(R["right"][1][b, :cnt], np.array(ov, np.int64)), (c.id, b)
            n += 1
    assert n > 150


@pytest.mark.parametrize("c", TREES, ids=_T_IDS)
def test_tree_table_shows_its_edges(c):
    """the table cannot drift away from the edges it names: they are asserted from the oracle's output"""
    have = tree_flags(c)
    assert _expect(c) <= have, f"{c.id}: expected {sorted(_expect(c))}, the oracle shows {sorted(have)}"
    print(f"FLAGS {c.id}: {sorted(have)} counts {tree_ref(c)['right'][2].tolist()}")


def _tree_wrong_applies(c, name):
    R = tree_ref(c)
    split = R["right"][2] > 1
    if name == "perm":
        return split
    return (R["right"][2] > (4 if c.dim == 2 else 8)) & np.array([k == "zero" for k in c.maps])          # two splits at least


@pytest.mark.parametrize("c", TREES, ids=_T_IDS)
def test_tree_wrong_references_differ(c):
    R = tree_ref(c)
    for name in ("perm", "last"):
        diff = np.array([not np.array_equal(R[name][0][b], R["right"][0][b]) for b in range(len(c.maps))])
        need = _tree_wrong_applies(c, name)
        assert (diff | ~need).all(), f"{c.id}: the wrong reference {name} builds the right tree for maps {np.nonzero(need & ~diff)[0].tolist()}"


@gpu
@pytest.mark.parametrize("c", TREES, ids=_T_IDS)
def test_tree_build(c):
    R = tree_ref(c)
    got = hip_build(c, R["maps"])
    for g, w, what in zip(got, R["right"], ("nodes", "values", "count", "seq_ps")):
        assert g.dtype == w.dtype and np.array_equal(g, w), f"{c.id}: {what} differ from the oracle, first at {np.argwhere(g != w)[0].tolist()}"
    for name in ("perm", "last"):
        for b in np.nonzero(_tree_wrong_applies(c, name))[0]:
            assert not np.array_equal(got[0][b], R[name][0][b]), f"{c.id}: the wrong reference {name} is not rejected for map {b}"


# ============================================================================================== tests: serializers
_S_IDS = [c.id for c in SERS]


@pytest.mark.parametrize("c", SERS, ids=_S_IDS)
def test_serialize_on_the_host(c):
    """the fp32 emulation of the kernel's expression order against the float64 reference: validates every d (err / bound <= 1), the wrong
    references' distance and the Tier 1 conditions without a GPU"""
    R = ser_ref(c)
    emu = serialize_all(c.dim, R["imgs"], R["nodes"], R["count"], c.p, ft=np.float32)
    assert emu.dtype == np.float32
    _check_case(c, emu, "emu")


@gpu
@pytest.mark.parametrize("c", SERS, ids=_S_IDS)
def test_serialize(c):
    R = ser_ref(c)
    flat = not (c.dim == 3 and c.p == 4)                                                  # the p = 4 octree cases take the flat=False list
    got = hip_serialize(c, R["imgs"], R["nodes"], R["count"], flat)
    want_shape = as_view(R["cands"][0], c.dim, flat).shape
    assert got.shape == want_shape
    # element by element in the returned layout against the explicitly indexed reshape of the reference's patch list, then leaf by leaf
    err = Pool._err(got, [as_view(k, c.dim, flat) for k in R["cands"]])
    assert (err <= as_view(R["tol"], c.dim, flat)).all(), f"{c.id}: the returned view is not the plain reshape of the patch list"
    if flat and c.C > 1:                                                                  # named elements: channel c of pixel j of leaf s sits at flat element (s P + j) C + c
        P, C, S = c.p ** c.dim, c.C, R["nodes"].shape[1]
        lst = from_view(got, R["cands"][0]).reshape(2, S, P, C)
        for (s, j, ch) in ((0, 0, 1), (S - 1, P - 1, C - 1), (S // 2, P // 2, 0)):
            e = (s * P + j) * C + ch
            assert got[1, e // (S * P), (e // P) % S, e % P] == lst[1, s, j, ch]
    _check_case(c, from_view(got, R["cands"][0]), "hip")


@gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_serialize_count_zero(dim):
    c = SerC(dim, 2, "t2" if dim == 2 else "t2small", 4, 2, "randn")
    R = ser_ref(c)
    got = hip_serialize(c, R["imgs"], R["nodes"], np.zeros(2, np.int32))
    assert not got.any() and not np.signbit(got).any()


E2E = [TreeC(2, (12, 20), 100, ("full", "r0.3", "u8")), TreeC(3, (12,), 120, ("full", "r0.1", "u8"))]


@functools.lru_cache(maxsize=None)
def e2e_ref(c, p, C):
    T = tree_ref(c)
    B = len(c.maps)
    g = torch.Generator().manual_seed(_seed("e2e", c.id))
    imgs = (torch.rand((B,) + c.full_shape + (C,), generator=g, dtype=torch.float32) * 255).numpy()
    nodes, _, count, _ = T["right"]
    cands, tol = [], None
    for bias in _biases(c.dim):
        o, t, _ = serialize_all(c.dim, imgs, nodes, count, p, bias=bias, bound=True)
        cands.append(o)
        tol = t if tol is None else np.maximum(tol, t)
    return imgs, nodes, count, cands, tol


@pytest.mark.parametrize("c", E2E, ids=[c.id for c in E2E])
def test_build_then_serialize_on_the_host(c):
    imgs, nodes, count, cands, tol = e2e_ref(c, 4, 3)
    emu = serialize_all(c.dim, imgs, nodes, count, 4, ft=np.float32)
    Pool(c.id, "emu").check("e2e", "uniform", emu, cands, tol)
    for b in range(len(count)):
        assert not emu[b, count[b]:].any()


@gpu
@pytest.mark.parametrize("c", E2E, ids=[c.id for c in E2E])
def test_build_then_serialize(c):
    """build -> serialize on the device as Patchify / Patchify_3D chain them, against oracle tree -> float64 resampling"""
    ops = _ops()
    imgs, nodes, count, cands, tol = e2e_ref(c, 4, 3)
    dom, _ = _carve(tree_ref(c)["maps"], 7)
    im, _ = _carve(imgs, float("nan"))
    n, _, ct, _ = ops.quadtree_build(dom, c.L) if c.dim == 2 else ops.octree_build(dom, c.L)
    assert np.array_equal(n.cpu().numpy(), nodes) and np.array_equal(ct.cpu().numpy(), count)
    seq = ops.quadtree_serialize(im, n, ct, 4) if c.dim == 2 else ops.octree_serialize(im, n, ct, 4)
    got = from_view(seq.cpu().numpy(), cands[0])
    Pool(c.id, "hip").check("e2e", "uniform", got, cands, tol)
    for b in range(len(count)):
        assert not got[b, count[b]:].any()


# ============================================================================================== tests: the tables
def test_tables_reach_every_branch():
    """the header's kernel-to-case list, from the restated host rules"""
    q = [c for c in TREES if c.dim == 2]
    o = [c for c in TREES if c.dim == 3]
    for cs, smem, step in ((q, smem_q, 3), (o, smem_o, 7)):
        Ls = sorted({c.L for c in cs})
        assert all(L % step == 1 and smem(L) <= LDS_CAP for L in Ls)
        assert any(smem(L) <= LDS_OPT_IN for L in Ls) and any(smem(L) > LDS_OPT_IN for L in Ls)
        first = min(L for L in range(1, 10000, step) if smem(L) > LDS_OPT_IN)
        last = max(L for L in range(1, 10000, step) if smem(L) <= LDS_CAP)
        assert first in Ls and last in Ls, (first, last)
        assert smem(last + step) > LDS_CAP
        big = [c for c in cs if int(tree_ref(c)["right"][2].max()) > NT]                  # n > 256: the strided scan and copy loops
        assert big and any(int(tree_ref(c)["right"][2].max()) <= NT for c in cs)
        assert any(smem(c.L) > LDS_OPT_IN and int(tree_ref(c)["right"][2].max()) == c.L for c in cs)      # above 64 KiB AND the list filled
    assert (min(L for L in range(1, 10000, 3) if smem_q(L) > LDS_OPT_IN), smem_q(2728), smem_q(6394)) == (2728, 65568, 153552)
    assert (min(L for L in range(1, 10000, 7) if smem_o(L) > LDS_OPT_IN), smem_o(2045), smem_o(4789)) == (2045, 65696, 153504)
    assert smem_q(6397) > LDS_CAP and smem_o(4796) > LDS_CAP and 6397 % 3 == 1 and 4796 % 7 == 1
    flags = {f for c in TREES for f in _expect(c)}
    assert flags == {"w1", "nonsq", "zerow", "early", "big"}
    assert {k for c in TREES for k in c.maps if not k.startswith("r")} == {"zero", "full", "u8"}
    assert {c.norm for c in o} == {255, 85, 1} and min(len(c.maps) for c in TREES) >= 2
    for dim in (2, 3):
        cs = [c for c in SERS if c.dim == dim]
        assert {c.tier for c in cs} == {1, 2}
        assert any(c.p == 1 for c in cs) == (dim == 3) and any(c.p > 1 for c in cs)      # p == 1 (inv = 0) is the octree's branch
        assert {c.fam for c in cs if c.tier == 2} == set(FAMS)
        t2 = [c for c in cs if c.tier == 2]
        assert {c.p for c in t2} == ({8, 3, 16} if dim == 2 else {1, 2, 4, 7})
        assert {c.C for c in t2} == ({1, 3, 5} if dim == 2 else {1, 2})
        assert any(c.p ** dim * c.C < NT for c in cs) and any(c.p ** dim * c.C > NT and (c.p ** dim * c.C) % NT for c in cs)
        for c in cs:
            nodes, count = node_list(dim, ser_exts(c), c.size)
            ext = nodes[..., 1::2] - nodes[..., 0::2]
            assert (ext == 0).any() and (ext < 0).any()                                   # the `w <= 0` branch
            assert count[0] < nodes.shape[1] and (ext[0, count[0]:] > 0).all()            # valid-looking rows beyond count
            lo, hi = nodes[..., 0::2].min(), (nodes[..., 1::2] - np.array(c.size, np.int32)).max()
            assert lo >= 0 and hi <= 0                                                    # every leaf lies inside the image: nothing reads out of bounds
            if c.tier == 2 and c.kind == "t2":
                real = ext[(ext > 0).all(-1)]
                assert {tuple(e) for e in real.tolist()} == set(Q_EXT if dim == 2 else O_EXT)
                assert (nodes[..., 0::2] == 0).any() and (nodes[0, :, 1] == c.size[0]).any() and (nodes[0, :, 3] == c.size[1]).any()
                assert dim == 2 or ((nodes[0, :, 5] == c.size[2]).any() and (nodes[..., 4] == 0).any())
    assert any(c.kind == "t2" and c.dim == 3 and c.size == (128,) * 3 and c.C == 1 for c in SERS)


# ============================================================================================== tests: refusals
def _refused(rc, needle):
    msg = _lib().load().ucfvit_last_error().decode()
    assert rc != 0, f"accepted; expected a refusal naming {needle!r}"
    assert needle in msg, f"refused with {msg!r}; expected {needle!r}"


@gpu
def test_refusals_write_nothing():
    lib = _lib().load()
    B = 2
    dummy = torch.zeros(64, dtype=torch.uint8, device=DEV)

    def fresh(L, dim):
        return _tree_outs(B, max(L, 1), dim)

    def clean(outs):
        torch.cuda.synchronize()
        return all(_untouched(buf, fill) for (_, buf), fill in zip(outs, (ISENT, ISENT, ISENT, FSENT)))
    e = torch.zeros((B, 16, 16), dtype=torch.uint8, device=DEV)
    for L, needle in ((0, "3n+1"), (2, "3n+1"), (3, "3n+1"), (6397, "does not fit")):
        outs = fresh(L, 2)
        _refused(_raw_build(2, e, L, 255, outs), needle)
        assert clean(outs), L
    for shape in ((B, 4105, 4105), (B, 32768, 8), (B, 8, 32768), (B, 0, 8)):
        outs = fresh(4, 2)
        _refused(_raw_build(2, dummy, 4, 255, outs, shape=shape, ws=dummy), "out of range")
        assert clean(outs), shape
    d = torch.zeros((B, 8, 8, 8), dtype=torch.uint8, device=DEV)
    for L, needle in ((0, "7n+1"), (2, "7n+1"), (7, "7n+1"), (4796, "does not fit")):
        outs = fresh(L, 3)
        _refused(_raw_build(3, d, L, 255, outs), needle)
        assert clean(outs), L
    for norm in (0, 256, -1):
        outs = fresh(8, 3)
        _refused(_raw_build(3, d, 8, norm, outs), "norm_factor")
        assert clean(outs), norm
    outs = fresh(8, 3)
    _refused(_raw_build(3, dummy, 8, 255, outs, shape=(B, 257), ws=dummy), "1..256")
    assert clean(outs)
    # the int32 node value: N^3 * 255 / norm_factor must stay below 2^31; N = 204 with norm 1 is the first that does not
    assert 204 ** 3 * 255 // 1 >= 2 ** 31 > 203 ** 3 * 255 // 1 and 256 ** 3 * 255 // 1 >= 2 ** 31 > 256 ** 3 * 255 // 2
    for N, norm in ((204, 1), (256, 1)):
        outs = fresh(8, 3)
        _refused(_raw_build(3, dummy, 8, norm, outs, shape=(B, N), ws=dummy), f"N={N} with norm_factor={norm}")
        assert clean(outs), (N, norm)
    # serializers
    out, buf = _carve_out((B, 4, 2, 2, 1), torch.float32, FSENT)
    nd = torch.zeros((B, 4, 6), dtype=torch.int32, device=DEV)
    ct = torch.zeros(B, dtype=torch.int32, device=DEV)
    im = torch.zeros((B, 4, 4, 4, 1), dtype=torch.float32, device=DEV)
    for (L, p) in ((0, 2), (4, 0)):
        _refused(lib.ucfvit_quadtree_serialize(im.data_ptr(), nd.data_ptr(), ct.data_ptr(), out.data_ptr(), B, 4, 4, 1, L, p, _stream()), "bad shape")
        _refused(lib.ucfvit_octree_serialize(im.data_ptr(), nd.data_ptr(), ct.data_ptr(), out.data_ptr(), B, 4, 1, L, p, _stream()), "bad shape")
    torch.cuda.synchronize()
    assert _untouched(buf, FSENT)
    # B = 0: nothing to do, OK with null pointers
    assert lib.ucfvit_quadtree_build(None, None, None, None, None, 0, 16, 16, 4, None, _stream()) == 0
    assert lib.ucfvit_octree_build(None, None, None, None, None, 0, 8, 8, 255, None, _stream()) == 0
    assert lib.ucfvit_quadtree_serialize(None, None, None, None, 0, 16, 16, 1, 4, 2, _stream()) == 0
    assert lib.ucfvit_octree_serialize(None, None, None, None, 0, 8, 1, 8, 2, _stream()) == 0
    # a refusal leaves the library usable
    outs = fresh(4, 2)
    assert _raw_build(2, e, 4, 255, outs) == 0
    torch.cuda.synchronize()
    assert outs[2][0].tolist() == [4, 4]


@gpu
def test_octree_value_limit_neighbour_is_accepted():
    """N = 203 with norm_factor 1: the root value 203^3 * 255 = 2,133,183,885 is the largest accepted family; dense maps, against the oracle"""
    c = TreeC(3, (203,), 8, ("full", "full"), norm=1)
    maps = np.full((2, 203, 203, 203), 255, np.uint8)
    maps[1, :7, :5, :3] = 11
    got = hip_build(c, maps)
    for b in range(2):
        n, v = ref_tree(maps[b], 8, 1)
        assert v.max() < 2 ** 31 and v[0] > 2 ** 27
        assert got[2][b] == 8 and np.array_equal(got[0][b], n) and np.array_equal(got[1][b].astype(np.int64), v)
    with pytest.raises(_lib().HipLibraryError, match="N=204 with norm_factor=1"):
        _ops().octree_build(torch.zeros((1, 204, 204, 204), dtype=torch.uint8, device=DEV), 8, 1)


@gpu
def test_ops_refusals():
    ops, Err = _ops(), _lib().HipLibraryError
    e = torch.zeros((2, 16, 16), dtype=torch.uint8, device=DEV)
    d = torch.zeros((2, 8, 8, 8), dtype=torch.uint8, device=DEV)
    for L in (0, 2, 3, 6397):
        with pytest.raises(Err):
            ops.quadtree_build(e, L)
    for L in (0, 2, 7, 4796):
        with pytest.raises(Err):
            ops.octree_build(d, L)
    for norm in (0, 256):
        with pytest.raises(Err, match="norm_factor"):
            ops.octree_build(d, 8, norm)
    with pytest.raises(Err, match="1..256"):
        ops.octree_build(torch.zeros((1, 257, 257, 257), dtype=torch.uint8, device=DEV), 8)
    # dtypes, ranks, shapes
    for bad in (e.float(), e.to(torch.int32), e[0], e.unsqueeze(0)):
        with pytest.raises(TypeError):
            ops.quadtree_build(bad, 4)
    for bad in (d.float(), d[0], torch.zeros((2, 8, 8, 4), dtype=torch.uint8, device=DEV)):
        with pytest.raises(TypeError):
            ops.octree_build(bad, 8)
    img = torch.zeros((2, 16, 16, 3), dtype=torch.float32, device=DEV)
    vol = torch.zeros((2, 8, 8, 8, 1), dtype=torch.float32, device=DEV)
    n2, n3 = torch.zeros((2, 4, 4), dtype=torch.int32, device=DEV), torch.zeros((2, 8, 6), dtype=torch.int32, device=DEV)
    ct = torch.zeros(2, dtype=torch.int32, device=DEV)
    for args in ((img.double(), n2, ct), (img.bfloat16(), n2, ct), (img, n2.long(), ct), (img, n2, ct.long()), (img[0], n2, ct)):
        with pytest.raises(TypeError):
            ops.quadtree_serialize(*args, 4)
    for args in ((vol.double(), n3, ct), (vol, n3.long(), ct), (vol, n3, ct.long()), (vol[0], n3, ct)):
        with pytest.raises(TypeError):
            ops.octree_serialize(*args, 2)
    # non-contiguous tensors and tensors on the host
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.quadtree_build(e.transpose(1, 2)[:, :, :8], 4)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.octree_build(d.transpose(1, 3), 8)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.quadtree_serialize(img[..., :2], n2, ct, 4)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.quadtree_serialize(img, n2[:, ::2], ct, 4)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.octree_serialize(vol.transpose(1, 2), n3, ct, 2)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.quadtree_build(e.cpu(), 4)
    # and the accepted neighbours still work
    assert ops.quadtree_build(e, 4)[2].tolist() == [4, 4] and ops.octree_build(d, 8)[2].tolist() == [8, 8]


def test_patchify_refuses_bad_lengths():
    from UCF_VIT.dataloaders.transform import Patchify, Patchify_3D
    for L in (0, 2, 3, 195, -2, -5):
        with pytest.raises(ValueError, match="3n\\+1"):
            Patchify(L, 8, 3)
    for L in (0, 2, 7, 728, -6, -13):
        with pytest.raises(ValueError, match="7n\\+1"):
            Patchify_3D(L, 8, 1)
    assert Patchify(196, 8, 3).fixed_length == 196 and Patchify_3D(729, 8, 1).norm_factor == 255
    assert Patchify_3D(8, 4, 255).norm_factor == 1                                        # the norm the value limit of the octree is about
