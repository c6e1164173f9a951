"""The kernels of csrc/patcher_labels.hip (labels_kernel<ND, T> for ND = 2, 3: the label serializers; quadtree_ / octree_deserialize_kernel over one
leaf walker: the tree deserializers; every case family below exists in both dimensions) element by element, through
UCF_VIT._hip.ops and, into outputs carved from sentinel-filled allocations, through UCF_VIT._hip.lib.  The references are numpy integer /
float64 code written here (restating the rules of csrc/resample_rules.h); they never call the project's kernels.  B >= 2 throughout.  U = 2^-24.

Parity.  The 3-D rules are pinned against the reference: tests/golden/tree_labels.npz holds serialize_labels / deserialize of the reference's
FixedOctTree (scipy RegularGridInterpolator) for N = 16, 32 at p = 2, 4, 8 (even p: the reference has no exact ties).  The 2-D rules are
PARITY UNPINNED, like the existing bicubic serializer: the reference's cv2.resize is not available to record from.  The nearest rules coincide
with any implementation whenever w / p or p / w is whole (every leaf of a power-of-two image).

Label serializers (np.array_equal on class indices and one-hot):
    2-D  hand-made node lists in a 300 x 260 label image (W x H), leaves (1,1) (2,2) (3,3) (5,1) (8,8) (13,9) (24,24) (256,256), each at the
         origin, the far corner and in the interior, empty leaves (w = 0, h = 0, w < 0) and a padding row in between, count[0] below the number
         of valid-looking rows; p = 3, 8, 16 x nc = 1, 4, 255, uint8 and int64 labels; rule min((px w) // p, w - 1)
    3-D  extents (1,1,1) (2,2,2) (3,1,2) (5,5,5) (12,7,3) (64,64,64) in N = 64; p = 1, 2, 4, 7; the integer grid rule (ties to the lower index)
    the octree fixtures bit for bit; padding rows are class 0; count = 0; labels >= nc, < 0 and 2^40: index unchanged, all-zero one-hot column
Deserializers, nearest mode (bit for bit): leaf tables of the same extents laid out WITHOUT overlap (a tree never overlaps; the 64^3 leaf is a
    volume of its own), random integer patches; uncovered pixels exactly 0 (partial lists); the round trip through a built tree (12x20 at
    L = 100, 12^3 at L = 120).  The round trip deserialize_nearest(serialize_labels(x)) == x holds for ANY x only where the leaf is as wide as
    the patch (both rules are then the identity); for the other leaves with p | w nearest resampling keeps one sample per block (2-D) and the
    3-D grid rule does not even map blocks onto blocks (n = 16, p = 4: voxel 12 reads patch cell 2), so those leaves are compared on an x that is
    constant on every block of every leaf (2-D) / on every leaf (3-D).  Both are asserted; the issue's wording (any x, every p | w) is not a
    property of nearest resampling.
Deserializers, bicubic / trilinear.  Exact tier (bits): w = p is the identity on any finite input (bicubic: t = 0, weights (0, 1, 0, 0);
    trilinear for p - 1 a power of two, where k (p - 1) fl(1 / (p - 1)) == k: asserted); w = p / 3, p / 5 land on patch centres (p = 15, 9, 3);
    trunc on +-2.7 gives +-2.  Bounded tier on uniform [0, 255), randn, randn + 1000 patches: |got - ref64| <= t with t re-derived from
    the kernels as written, which evaluate the expressions of the existing serializers with source and destination extents exchanged:
        bicubic    f = (x + 1/2) (p / w) - 1/2, cell floor(f), t = f - floor(f), cubic_coeffs(t) on both axes, 4 x (4 products summed from 0) then
                   4 products summed from 0, taps clamped to the patch (and truncated first with trunc, which is exact):
                   t = [8 U S(|wy|, |wx|) + S(dwy, |wx|) + S(|wy|, dwx) + dfy Sy(|wy'|, |wx|) + dfx Sx(|wy|, |wx'|)] (1 + 2^-10), S(a, b) = sum over
                   the 16 taps of a b |tap|, Sx / Sy with |tap - tap of column / row 1| (the w' sum to zero); dw = (9 | 8) U ptilde (Horner
                   roundings of the outer / inner polynomial incl. their argument); df = U (2 (x + 1/2) p / w + |f| + 1)
        trilinear  f = z (p - 1) fl(1 / (n - 1)), cell (int) f clamped to p - 1, three lerps a (1 - t) + b t:
                   t = [9 U S(w |corner|) + sum over axes of df (weighted |corner differences| along the axis)] (1 + 2^-10), df = 3 U f
    Where a position lies within df of an integer either neighbouring cell is accepted (references for floor(f +- df) per axis); such elements are
    counted and may be at most 5 % of a case's elements: the leaf tables are chosen for that (62^3 instead of 64^3: gcd(61, p - 1) = 1, so only the
    last sample of an axis is whole; 2-D: w = p, 3p are few pixels next to the 256^2 leaves), shown on the host.
    The 3-D fixtures within the same bound.  Both strided input layouts ([B, L, p.., C] and [B, C, L, p^d]) and both output layouts give
    identical bits.  Wrong references are rejected (and shown on the host to differ by more than the bound): A = -0.5, extents exchanged, leaf
    shifted by one, ties upward (3-D nearest rules), batch element b + 1, channel c + 1.
Refusals (nothing written, sentinels intact): p = 0, nc = 0 and 256, N = 257, H = 32768, wrong label dtype code, unknown mode, non-dense
    output strides; B = 0 with null pointers returns OK; through ops: wrong dtypes, wrong ranks, non-contiguous labels, bad mode strings.

worst err / bound (host fp32 emulation | MI355X) and the ambiguous share of the painted elements, from a run of this file.  The translation unit
is built without fma contraction, so the kernels evaluate exactly what the emulation evaluates: both columns agree to every printed digit.
    quadtree_deserialize  uniform 0.040 | 0.040   randn 0.044 | 0.044   randn + 1000 0.025 | 0.025   uniform + trunc 0.036 | 0.036   ambiguous <= 0.93 %
    octree_deserialize    uniform 0.474 | 0.474   randn 0.436 | 0.436   randn + 1000 0.325 | 0.325                                    ambiguous <= 4.80 %
    octree fixtures (N = 16, 32; p = 2, 4, 8)     0.444 | 0.444
The bicubic bound is loose here because the leaves are magnified (p = 8 -> 256): the position error df, scaled by the tap differences, dominates
it and the positions of a power-of-two leaf are exact.  It still tells every wrong reference apart.  The whole file: 61 GPU tests in 7.8 s, 54
host tests in 24 s (the float64 references of the 256^2 and 62^3 leaves for every cell choice; no GPU test above 1.3 s).
"""
import functools
import os
from dataclasses import dataclass

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
PAD = 64                                   # sentinel elements in front of and behind every carved tensor
ISENT = -77777                             # int32 sentinel
LSENT = -7777777777                        # int64 sentinel
FSENT = -12352.0                           # fp32 sentinel
AMB_CAP = 0.05
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_labels.npz")


def _ops():
    from UCF_VIT._hip import ops
    return ops


def _lib():
    from UCF_VIT._hip import lib
    return lib


def _seed(*parts):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate("|".join(str(p) for p in parts))) % (2 ** 31)


def _rng(*parts):
    return np.random.Generator(np.random.PCG64(_seed(*parts)))


# ============================================================================================== the integer rules (csrc/resample_rules.h restated)
def nearest_floor(j, n_src, n_dst):
    """cv2.resize(INTER_NEAREST): source index of destination index j"""
    return np.minimum((np.asarray(j, np.int64) * n_src) // n_dst, n_src - 1)


def nearest_grid(j, n_src, n_dst, ties_up=False):
    """scipy RegularGridInterpolator('nearest') on linspace(0, n, n_src) queried at linspace(0, n, n_dst), in integers; ties to the lower index
    (ties_up: the wrong reference)"""
    j = np.asarray(j, np.int64)
    if n_src < 2 or n_dst < 2:
        return np.zeros_like(j)
    num, den = j * (n_src - 1), n_dst - 1
    i = np.minimum(num // den, n_src - 2)
    r2 = 2 * (num - i * den)
    return np.where((r2 < den) if ties_up else (r2 <= den), i, i + 1)


def _valid(nodes, count, b, s):
    nd = nodes[b, s].astype(np.int64)
    return s < count[b] and not ((nd[1::2] - nd[0::2]) <= 0).any()


def labels_all(dim, labels, nodes, count, p, ties_up=False, swap=False, shift=0, batch=0):
    """labels [B, H, W] or [B, N, N, N] -> class indices int64 [B, S, p .. p]; class 0 for padding rows and empty leaves"""
    B, S = nodes.shape[:2]
    out = np.zeros((B, S) + (p,) * dim, np.int64)
    k = np.arange(p)
    for b in range(B):
        lab = labels[(b + batch) % B]
        for s in range(S):
            if not _valid(nodes, count, b, s):
                continue
            nd = nodes[b, s].astype(np.int64)
            lo, ext = nd[0::2].copy(), nd[1::2] - nd[0::2]
            if shift:
                lo[0] += shift if nd[1] + shift <= lab.shape[-1] else (-shift if nd[0] - shift >= 0 else 0)
            if swap:
                ext = ext[[1, 0] + list(range(2, dim))]
            if dim == 2:
                ix, iy = lo[0] + nearest_floor(k, ext[0], p), lo[1] + nearest_floor(k, ext[1], p)
                out[b, s] = lab[np.minimum(iy, lab.shape[0] - 1)[:, None], np.minimum(ix, lab.shape[1] - 1)[None, :]]
            else:
                ix, iy, iz = (np.minimum(lo[a] + nearest_grid(k, ext[a], p, ties_up), lab.shape[0] - 1) for a in range(3))
                out[b, s] = lab[iz[:, None, None], iy[None, :, None], ix[None, None, :]]
    return out


def onehot_of(idx, nc):
    """[B, S, p ..] -> fp32 [B, nc, S * p^d]: the collate's F.one_hot(...).permute in the memory order of the plain reshape; labels outside
    [0, nc) give an all-zero column"""
    B = idx.shape[0]
    return (idx.reshape(B, 1, -1) == np.arange(nc)[None, :, None]).astype(np.float32)


# ============================================================================================== the smooth rules
def cubic_weights(t, A, ft):
    """cubic_coeffs of the kernel in its expression order, in the float type ft -> [4, ...]"""
    A, one, two = ft(A), ft(1), ft(2)
    f5, f8, f4, a2, a3 = ft(5) * A, ft(8) * A, ft(4) * A, A + ft(2), A + ft(3)
    x0, x1, x2, x3 = t + one, t, one - t, two - t
    return np.stack([((A * x0 - f5) * x0 + f8) * x0 - f4, (a2 * x1 - a3) * x1 * x1 + one, (a2 * x2 - a3) * x2 * x2 + one,
                     ((A * x3 - f5) * x3 + f8) * x3 - f4])


def cubic_bounds(t, A):
    """float64: (|dw / dt| [4, ...], rounding bound of the fp32 weights [4, ...]): 6 / 5 Horner roundings of the outer / inner polynomial, one
    for the argument, which costs at most 3 U ptilde (x ptilde' <= 3 ptilde); ptilde: the polynomial of the coefficients' magnitudes"""
    a, a2, a3 = abs(A), A + 2, A + 3
    dpo = lambda x: 3 * A * x * x - 10 * A * x + 8 * A                                   # noqa: E731
    dpi = lambda x: 3 * a2 * x * x - 2 * a3 * x                                          # noqa: E731
    pto = lambda x: a * x ** 3 + 5 * a * x * x + 8 * a * x + 4 * a                       # noqa: E731
    pti = lambda x: a2 * x ** 3 + a3 * x * x + 1                                         # noqa: E731
    x0, x1, x2, x3 = np.abs(t + 1), np.abs(t), np.abs(1 - t), np.abs(2 - t)
    dw = np.abs(np.stack([dpo(t + 1), dpi(t), dpi(1 - t), dpo(2 - t)]))
    rb = U * np.stack([9 * pto(x0), 8 * pti(x1), 8 * pti(x2), 9 * pto(x3)])
    return dw, rb


def bicubic_paint(patch, w, h, ft=np.float64, A=-0.75, swap=False, bias=(0, 0), trunc=False, bound=False):
    """one leaf of quadtree_deserialize_kernel: patch [p(y), p(x), C] -> [h, w, C] in ft (+ the bound, + the cells [h, w, 2]).  ft = float32 with
    the defaults is the emulation of the kernel; float64 the reference; bias (ex, ey) in {-1, 0, 1}: the cell is floor(f + e df)"""
    p, C = patch.shape[0], patch.shape[-1]

    def axis(n, n_scale, e):
        k = np.arange(n)
        f = (k.astype(ft) + ft(0.5)) * (ft(p) / ft(n_scale)) - ft(0.5)
        df = U * (2 * (k + 0.5) * p / n_scale + np.abs(f.astype(np.float64)) + 1)
        fl = np.floor(f + ft(e) * df.astype(ft)) if e else np.floor(f)
        return f - fl, df, np.clip(fl.astype(np.int64)[None, :] - 1 + np.arange(4)[:, None], 0, p - 1), fl.astype(np.int64)
    tx, dfx, X, cx = axis(w, h if swap else w, bias[0])
    ty, dfy, Y, cy = axis(h, w if swap else h, bias[1])
    wx, wy = cubic_weights(tx, A, ft), cubic_weights(ty, A, ft)                           # [4, w], [4, h]
    src = np.trunc(patch) if trunc else patch
    taps = src[Y[:, :, None, None], X[None, None, :, :], :].astype(ft)                    # [4, h, 4, w, C]
    acc = np.zeros((h, w, C), ft)
    for a in range(4):
        r = np.zeros((h, w, C), ft)
        for d in range(4):
            r = r + wx[d][None, :, None] * taps[a, :, d, :, :]
        acc = acc + wy[a][:, None, None] * r
    if not bound:
        return acc
    S = lambda ay, ax, v=np.abs(taps): np.einsum("ap,dq,apdqc->pqc", ay, ax, v)           # noqa: E731
    dtx, dty = np.abs(taps - taps[:, :, 1:2]), np.abs(taps - taps[1:2])
    dwx, rbx = cubic_bounds(tx, A)
    dwy, rby = cubic_bounds(ty, A)
    awx, awy = np.abs(wx), np.abs(wy)
    t = (8 * U * S(awy, awx) + S(rby, awx) + S(awy, rbx) + S(dwy * dfy[None, :], awx, dty) + S(awy, dwx * dfx[None, :], dtx)) * (1 + 2.0 ** -10)
    return acc, t, np.stack(np.broadcast_arrays(cx[None, :], cy[:, None]), -1)


def trilinear_paint(patch, nx, ny, nz, ft=np.float64, swap=False, bias=(0, 0, 0), bound=False):
    """one leaf of octree_deserialize_kernel: patch [p(z), p(y), p(x), C] -> [nz, ny, nx, C]"""
    p = patch.shape[0]

    def axis(n, n_scale, e):
        k = np.arange(n)
        inv = ft(1) / ft(n_scale - 1) if n_scale > 1 else ft(0)
        f = k.astype(ft) * ft(p - 1) * inv
        df = 3 * U * f.astype(np.float64)
        i0 = np.clip(np.floor(f + ft(e) * df.astype(ft)).astype(np.int64), 0, p - 1)
        return f - i0.astype(ft), df, i0, np.minimum(i0 + 1, p - 1)
    tx, dfx, X0, X1 = axis(nx, ny if swap else nx, bias[0])
    ty, dfy, Y0, Y1 = axis(ny, nx if swap else ny, bias[1])
    tz, dfz, Z0, Z1 = axis(nz, nz, bias[2])
    at = lambda Z, Y, X: patch[Z[:, None, None], Y[None, :, None], X[None, None, :], :].astype(ft)       # noqa: E731
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
    for a in (0, 1):
        for b in (0, 1):
            t = t + DX * WZ[a] * WY[b] * np.abs(corner[a, b, 1] - corner[a, b, 0])
            t = t + DY * WZ[a] * WX[b] * np.abs(corner[a, 1, b] - corner[a, 0, b])
            t = t + DZ * WY[a] * WX[b] * np.abs(corner[1, a, b] - corner[0, a, b])
    cells = np.stack(np.broadcast_arrays(X0[None, None, :], Y0[None, :, None], Z0[:, None, None]), -1)
    return out, t * (1 + 2.0 ** -10), cells


def deser_all(dim, seq, nodes, count, shape, mode="smooth", ft=np.float64, bias=None, bound=False, trunc=False, A=-0.75, swap=False, shift=0,
              ties_up=False, batch=0, chan=0):
    """the whole launch: seq [B, S, p .. p, C] fp32, nodes [B, S, 2 dim], count [B] -> the image [B, *shape, C] (shape = (H, W) or (N, N, N)) in
    ft, zero where no valid leaf paints (+ the bound and the painted cells).  swap / shift / ties_up / batch / chan / A: the wrong references"""
    B, S = nodes.shape[:2]
    p, C = seq.shape[2], seq.shape[-1]
    out = np.zeros((B,) + tuple(shape) + (C,), ft)
    tol = np.zeros(out.shape, np.float64) if bound else None
    cells = np.full((B,) + tuple(shape) + (dim,), -1, np.int64) if bound else None
    for b in range(B):
        for s in range(S):
            if not _valid(nodes, count, b, s):
                continue
            nd = nodes[b, s].astype(np.int64)
            lo, ext = nd[0::2].copy(), nd[1::2] - nd[0::2]
            if shift:
                lo[0] += shift if nd[1] + shift <= shape[-1] else (-shift if nd[0] - shift >= 0 else 0)
            patch = seq[(b + batch) % B, s]
            if chan:
                patch = patch[..., (np.arange(C) + chan) % C]
            sw = ext[[1, 0] + list(range(2, dim))] if swap else ext           # the extents the rule is evaluated with
            sl = (b,) + tuple(slice(lo[a], lo[a] + ext[a]) for a in reversed(range(dim)))
            if mode == "nearest":
                if dim == 2:
                    ix, iy = nearest_floor(np.arange(ext[0]), p, sw[0]), nearest_floor(np.arange(ext[1]), p, sw[1])
                    out[sl] = patch[iy[:, None], ix[None, :]]
                else:
                    ix, iy, iz = (np.minimum(nearest_grid(np.arange(ext[a]), p, sw[a], ties_up), p - 1) for a in range(3))
                    out[sl] = patch[iz[:, None, None], iy[None, :, None], ix[None, None, :]]
                continue
            kw = dict(ft=ft, swap=swap, bound=bound)
            if bias is not None:
                kw["bias"] = bias
            r = bicubic_paint(patch, ext[0], ext[1], A=A, trunc=trunc, **kw) if dim == 2 else trilinear_paint(patch, ext[0], ext[1], ext[2], **kw)
            if bound:
                out[sl], tol[sl], cells[sl] = r
            else:
                out[sl] = r
    return (out, tol, cells) if bound else out


# ============================================================================================== node lists
QW, QH, ON = 300, 260, 64
Q_EXT = [(1, 1), (2, 2), (3, 3), (5, 1), (8, 8), (13, 9), (24, 24), (256, 256)]
O_EXT = [(1, 1, 1), (2, 2, 2), (3, 1, 2), (5, 5, 5), (12, 7, 3), (64, 64, 64)]


def _place(ext, size, where):
    """where 0: at the origin, 1: at the far corner, 2: interior (where there is room)"""
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


def _with_empties(rows, dim):
    rows = [list(r) for r in rows]
    for i, r in enumerate(_empties(dim)):
        rows.insert(min(2 * i + 1, len(rows)), r)
    return rows


def read_list(dim):
    """the serializers' list (leaves may overlap: they only read), B = 2: every extent at three places, the empty leaves in between; batch element
    1 has the list reversed; count[0] leaves the last three (valid-looking) rows out, count[1] takes all"""
    size = (QW, QH) if dim == 2 else (ON,) * 3
    rows = _with_empties([_place(e, size, wh) for e in (Q_EXT if dim == 2 else O_EXT) for wh in (0, 1, 2)], dim)
    a = np.array(rows, np.int32)
    return np.stack([a, a[::-1].copy()]), np.array([len(rows) - 3, len(rows)], np.int32)


def _box(lo, ext):
    return [v for a in range(len(lo)) for v in (lo[a], lo[a] + ext[a])]


# painting lists: no two leaves of one batch element overlap; every extent touches a border or corner somewhere and lies in the interior somewhere
Q_PAINT = [
    [_box((0, 0), (256, 256)), _box((276, 0), (24, 24)), _box((260, 30), (13, 9)), _box((270, 50), (8, 8)), _box((258, 70), (5, 1)),
     _box((297, 257), (3, 3)), _box((0, 258), (2, 2)), _box((290, 100), (1, 1)), _box((262, 120), (24, 24)), _box((299, 259), (1, 1))],
    [_box((44, 4), (256, 256)), _box((0, 0), (1, 1)), _box((298, 0), (2, 2)), _box((20, 0), (3, 3)), _box((30, 2), (5, 1)),
     _box((0, 236), (24, 24)), _box((5, 100), (13, 9)), _box((20, 50), (8, 8)), _box((25, 251), (13, 9)), _box((10, 20), (2, 2)),
     _box((292, 0), (5, 1)), _box((30, 150), (3, 3)), _box((36, 4), (8, 8))],
]
O_PAINT_FULL = [
    [_box((0, 0, 0), (64, 64, 64))],
    [_box((0, 0, 0), (1, 1, 1)), _box((62, 62, 62), (2, 2, 2)), _box((10, 20, 30), (3, 1, 2)), _box((20, 5, 40), (5, 5, 5)),
     _box((40, 50, 10), (12, 7, 3)), _box((59, 0, 0), (5, 5, 5)), _box((0, 57, 61), (12, 7, 3)), _box((30, 30, 30), (2, 2, 2)),
     _box((63, 63, 0), (1, 1, 1)), _box((20, 63, 62), (3, 1, 2))],
]
# bounded tier: 62^3 for 64^3 (gcd(61, p - 1) = 1 for p <= 8: only the last sample of an axis is a whole position); the small leaves in the margin
O_PAINT_T2 = [
    [_box((0, 0, 0), (62, 62, 62)), _box((62, 62, 62), (2, 2, 2)), _box((63, 0, 0), (1, 1, 1)), _box((62, 10, 20), (2, 2, 2))],
    [_box((2, 2, 2), (62, 62, 62)), _box((0, 0, 0), (2, 2, 2)), _box((0, 10, 20), (2, 5, 7)), _box((5, 0, 5), (12, 2, 3)), _box((30, 30, 0), (3, 1, 2)),
     _box((0, 40, 40), (1, 1, 1)), _box((20, 20, 0), (5, 2, 2))],
]


def paint_list(table, dim):
    """B = 2 from a painting table: the empty leaves in between, rows padded to one length with padding rows; count[0] leaves the last valid row
    of element 0 out (its region stays 0), count[1] takes all"""
    rows = [_with_empties(r, dim) for r in table]
    S = max(len(r) for r in rows)
    count = np.array([len(rows[0]) - 1, len(rows[1])], np.int32)
    for r in rows:
        r += [[0] * (2 * dim)] * (S - len(r))
    return np.array(rows, np.int32), count


def exact_list(p, dim, exts):
    """leaves of the exact tier next to each other along x, B = 2 (element 1 reversed and moved by one pixel)"""
    rows, x = [], 0
    for e in exts:
        rows.append(_box((x,) + (0,) * (dim - 1), e))
        x += e[0]
    a = np.array(rows, np.int32)
    b = a[::-1].copy()
    b[:, 0:2] += 1
    b[:, 2:4] += 2
    return np.stack([a, b]), np.array([len(rows), len(rows)], np.int32), x + 1


def check_paint_table(nodes, count, shape):
    """inside the image, and no two valid leaves of a batch element overlap"""
    dim = len(shape)
    for b in range(nodes.shape[0]):
        cover = np.zeros(shape, np.int32)
        for s in range(nodes.shape[1]):
            if not _valid(nodes, count, b, s):
                continue
            nd = nodes[b, s]
            assert all(nd[2 * a] >= 0 and nd[2 * a + 1] <= shape[dim - 1 - a] for a in range(dim)), (b, s)
            cover[tuple(slice(nd[2 * a], nd[2 * a + 1]) for a in reversed(range(dim)))] += 1
        assert cover.max() == 1, f"batch element {b}: leaves overlap"


# ============================================================================================== cases
@dataclass(frozen=True)
class LabC:
    dim: int
    p: int
    nc: int
    dtype: str

    @property
    def id(self):
        return f"{'q' if self.dim == 2 else 'o'}-p{self.p}-nc{self.nc}-{self.dtype}"


LABS = [LabC(2, p, nc, ("u8", "i64")[(i * 3 + j) % 2]) for i, p in enumerate((3, 8, 16)) for j, nc in enumerate((1, 4, 255))]
LABS += [LabC(3, p, (1, 4, 255)[i % 3], ("u8", "i64")[i % 2]) for i, p in enumerate((1, 2, 4, 7))] + [LabC(3, 7, 4, "u8"), LabC(3, 2, 255, "u8"),
                                                                                                     LabC(3, 4, 1, "i64")]


@functools.lru_cache(maxsize=None)
def lab_ref(c):
    nodes, count = read_list(c.dim)
    shape = (2, QH, QW) if c.dim == 2 else (2, ON, ON, ON)
    labels = _rng("lab", c.id).integers(0, c.nc, shape).astype(np.uint8 if c.dtype == "u8" else np.int64)
    idx = labels_all(c.dim, labels, nodes, count, c.p)
    wrongs = {"swap": labels_all(c.dim, labels, nodes, count, c.p, swap=True), "shift": labels_all(c.dim, labels, nodes, count, c.p, shift=1),
              "batch": labels_all(c.dim, labels, nodes, count, c.p, batch=1)}
    if c.dim == 3 and c.p == 7:
        wrongs["ties"] = labels_all(c.dim, labels, nodes, count, c.p, ties_up=True)
    return dict(labels=labels, nodes=nodes, count=count, idx=idx, wrongs=wrongs)


@dataclass(frozen=True)
class DesC:
    dim: int
    tier: str                # "near" | "exact" | "bound"
    p: int
    C: int
    fam: str                 # "int" | "wild" | "uniform" | "randn" | "randn1000" | "pm27"
    trunc: bool = False
    table: str = "paint"     # "paint" | "t2" | "id" (w = p) | "centre" (w = p / 3, p / 5)

    @property
    def id(self):
        return f"{'q' if self.dim == 2 else 'o'}-{self.tier}-{self.table}-p{self.p}-C{self.C}-{self.fam}" + ("-trunc" if self.trunc else "")


FAMS = ("uniform", "randn", "randn1000")
DESS = [DesC(2, "near", p, C, "int") for p, C in ((3, 1), (8, 3), (16, 2))] + [DesC(3, "near", p, C, "int") for p, C in ((1, 2), (2, 1), (4, 3), (7, 1))]
DESS += [DesC(2, "exact", p, C, "wild", table="id") for p, C in ((8, 3), (3, 1), (16, 2))]
DESS += [DesC(2, "exact", p, 2, "wild", table="centre") for p in (15, 9, 3)]
DESS += [DesC(2, "exact", 8, 2, "pm27", trunc=True, table="id")]
DESS += [DesC(3, "exact", p, C, "wild", table="id") for p, C in ((1, 2), (2, 1), (3, 2), (5, 1), (9, 1))]
DESS += [DesC(2, "bound", 8, 2, f) for f in FAMS] + [DesC(2, "bound", 3, 1, "randn"), DesC(2, "bound", 16, 3, "uniform"),
                                                     DesC(2, "bound", 8, 2, "uniform", trunc=True)]
DESS += [DesC(3, "bound", 5, 1, f, table="t2") for f in FAMS] + [DesC(3, "bound", 2, 2, "randn", table="t2"), DesC(3, "bound", 8, 1, "uniform", table="t2")]


def des_table(c):
    """-> (nodes, count, shape)"""
    p = c.p
    if c.table == "id":
        exts = [(p,) * c.dim] * 3
    elif c.table == "centre":
        exts = [(p // 3, p // 3), (p, p // 3), (p // 3, p)] + ([(p // 5, p // 5), (p // 5, p // 3)] if p % 5 == 0 else [])
    else:
        exts = None
    if exts is not None:
        nodes, count, wid = exact_list(p, c.dim, exts)
        shape = (p + 3, wid + 2) if c.dim == 2 else (max(p + 3, wid + 2),) * 3
        return nodes, count, shape
    if c.dim == 2:
        return paint_list(Q_PAINT, 2) + ((QH, QW),)
    return paint_list(O_PAINT_T2 if c.table == "t2" else O_PAINT_FULL, 3) + ((ON,) * 3,)


def make_seq(c, S):
    shape = (2, S) + (c.p,) * c.dim + (c.C,)
    g = torch.Generator().manual_seed(_seed("seq", c.id))
    if c.fam == "uniform":
        v = torch.rand(shape, generator=g, dtype=torch.float32) * 255
    elif c.fam == "int":
        v = torch.randint(0, 256, shape, generator=g).float()
    elif c.fam == "pm27":
        v = (torch.randint(0, 2, shape, generator=g).float() * 2 - 1) * 2.7
    else:
        v = torch.randn(shape, generator=g, dtype=torch.float32)
        v = v + 1000.0 if c.fam == "randn1000" else (v * 1000.0 if c.fam == "wild" else v)
    v = v.numpy()
    v[v == 0] = 0.0                                                                      # no -0: the kernels' 0.f + (0 * x) drops its sign
    return v


def _biases(dim):
    return [tuple(b) for b in np.array(np.meshgrid(*[(-1, 1)] * dim)).T.reshape(-1, dim)]


def wrong_variants(c):
    w = {"shift": {"shift": 1}, "batch": {"batch": 1}}
    if c.p > 1:
        w["swap"] = {"swap": True}
    if c.C > 1:
        w["chan"] = {"chan": 1}
    if c.dim == 2 and c.tier == "bound":
        w["A"] = {"A": -0.5}
    if c.dim == 3 and c.tier == "near" and c.p > 1:
        w["ties"] = {"ties_up": True}
    return w


@functools.lru_cache(maxsize=None)
def des_ref(c):
    nodes, count, shape = des_table(c)
    seq = make_seq(c, nodes.shape[1])
    mode = "nearest" if c.tier == "near" else "smooth"
    if c.tier == "near":
        want = deser_all(c.dim, seq, nodes, count, shape, mode)
        wrongs = {n: deser_all(c.dim, seq, nodes, count, shape, mode, **kw) for n, kw in wrong_variants(c).items()}
        return dict(seq=seq, nodes=nodes, count=count, shape=shape, cands=[want], tol=np.zeros(want.shape), wrongs=wrongs, ambiguous=0.0)
    cands, tol, cell0, amb = [], None, None, None
    for bias in _biases(c.dim):
        o, t, cells = deser_all(c.dim, seq, nodes, count, shape, mode, bias=bias, bound=True, trunc=c.trunc)
        cands.append(o)
        tol = t if tol is None else np.maximum(tol, t)
        if cell0 is None:
            cell0, amb = cells, np.zeros(cells.shape[:-1], bool)
        amb |= (cells != cell0).any(-1)
    painted = (cell0[..., 0] >= 0)
    wrongs = {n: deser_all(c.dim, seq, nodes, count, shape, mode, trunc=c.trunc, **kw) for n, kw in wrong_variants(c).items()} if c.tier == "bound" else {}
    return dict(seq=seq, nodes=nodes, count=count, shape=shape, cands=cands, tol=tol, wrongs=wrongs, ambiguous=float(amb.sum()) / max(int(painted.sum()), 1))


RATIOS = {}


def check_des(c, got, backend):
    """got [B, *shape, C] against the references of the case: exact tiers on the bits, the bounded tier per element against the nearest candidate;
    uncovered pixels exactly 0; every wrong reference differs from all candidates by more than the bound somewhere and is rejected by `got`"""
    R = des_ref(c)
    cands, tol = R["cands"], R["tol"]
    assert got.shape == cands[0].shape and not np.isnan(got).any()
    if c.tier != "bound":
        assert all(np.array_equal(cands[0], k) for k in cands[1:]), f"{c.id}: a position is not exactly on its cell"
        want = cands[0].astype(np.float32)
        assert np.array_equal(want.astype(np.float64), cands[0]), f"{c.id}: the float64 result is no fp32 number"
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), \
            f"{c.id} [{backend}]: not bit for bit, {int((got != want).sum())} elements differ, worst {np.abs(got - want).max()}"
    else:
        span = float(R["seq"].max() - R["seq"].min())
        assert np.isfinite(tol).all() and float(tol.max()) < span, f"{c.id}: the bound {tol.max()} is vacuous against the range {span}"
        assert R["ambiguous"] <= AMB_CAP, f"{c.id}: {R['ambiguous']:.3%} of the painted elements are ambiguous"
        err = np.min(np.stack([np.abs(got.astype(np.float64) - r) for r in cands]), axis=0)
        q = np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))
        key = f"{'quadtree' if c.dim == 2 else 'octree'}_deserialize {c.fam}{' trunc' if c.trunc else ''} [{backend}]"
        RATIOS[key] = max(RATIOS.get(key, 0.0), float(q.max()))
        print(f"RATIO {key} {c.id}: worst err/bound {q.max():.3f}, ambiguous {R['ambiguous']:.3%}")
        bad = err > tol
        assert not bad.any(), f"{c.id} [{backend}]: {int(bad.sum())} of {bad.size} elements out of bound, worst err/bound {q.max():.3g} at {np.argwhere(bad)[0].tolist()}"
    for name, w in R["wrongs"].items():
        differs = (np.min(np.stack([np.abs(w - r) for r in cands]), axis=0) > tol).any()
        assert differs, f"{c.id}: the wrong reference '{name}' lies within the bound of the right one"
        assert (np.abs(got.astype(np.float64) - w) > tol).any(), f"{c.id} [{backend}]: the wrong reference '{name}' is not rejected"
    assert set(wrong_variants(c)) <= set(R["wrongs"]) or c.tier == "exact"


# ============================================================================================== host half
SCIPY_N, SCIPY_P = (2, 3, 4, 5, 6, 7, 8, 12, 16, 20, 32, 64), (2, 3, 4, 5, 7, 8, 16)


def test_integer_nearest_rule_against_scipy():
    """equal to RegularGridInterpolator(method='nearest') for every even p; for odd p different only at exact ties (where the rule takes the lower
    index and scipy's double arithmetic may go up); the header's example n = 4, p = 3"""
    from scipy.interpolate import RegularGridInterpolator
    ties = 0
    for n in SCIPY_N:
        for p in SCIPY_P:
            want = RegularGridInterpolator(points=[np.linspace(0, n, n)], values=np.arange(n, dtype=np.float64), method="nearest")(
                np.linspace(0, n, p)[:, None]).astype(np.int64)
            j = np.arange(p)
            got = nearest_grid(j, n, p)
            tie = 2 * (j * (n - 1) - np.minimum(j * (n - 1) // (p - 1), n - 2) * (p - 1)) == p - 1
            assert np.array_equal(got[~tie], want[~tie]), (n, p)
            assert ((want[tie] == got[tie]) | (want[tie] == got[tie] + 1)).all(), (n, p)
            if p % 2 == 0:
                assert not tie.any() and np.array_equal(got, want), (n, p)
            ties += int((want != got).sum())
    assert ties > 0                                                                       # scipy does send some midpoints up
    assert nearest_grid(np.arange(3), 4, 3).tolist() == [0, 1, 3]
    assert nearest_grid(np.arange(4), 1, 4).tolist() == [0] * 4 and nearest_grid(np.arange(1), 9, 1).tolist() == [0]
    assert nearest_floor(np.arange(8), 3, 8).tolist() == [0, 0, 0, 1, 1, 1, 2, 2] and nearest_floor(np.arange(2), 5, 2).tolist() == [0, 2]


def test_tables_are_what_they_claim():
    for table, dim, shape, exts in ((Q_PAINT, 2, (QH, QW), Q_EXT), (O_PAINT_FULL, 3, (ON,) * 3, O_EXT), (O_PAINT_T2, 3, (ON,) * 3, None)):
        nodes, count = paint_list(table, dim)
        check_paint_table(nodes, count, shape)
        have = {tuple(int(v) for v in (nd[1::2] - nd[0::2])) for b in range(2) for nd in nodes[b]}
        assert exts is None or set(exts) <= have
    for c in DESS:
        nodes, count, shape = des_table(c)
        check_paint_table(nodes, count, shape)
    nodes, count = read_list(2)
    assert nodes.shape[0] == 2 and count[0] == nodes.shape[1] - 3
    for c in DESS:
        if c.tier == "exact" and c.dim == 3:                                              # identity of the trilinear rule: whole positions in fp32
            k = np.arange(c.p, dtype=np.float32)
            inv = np.float32(1) / np.float32(c.p - 1) if c.p > 1 else np.float32(0)
            assert np.array_equal(k * np.float32(c.p - 1) * inv, k if c.p > 1 else 0 * k), c.id


@pytest.mark.parametrize("c", [c for c in DESS if c.tier != "near"], ids=lambda c: c.id)
def test_deserialize_on_the_host(c):
    """the fp32 emulation of the kernels' expression order through the same check as the GPU result: exact tiers on the bits, the bounded tier
    within the bound, the ambiguous share below the cap, the wrong references told apart"""
    R = des_ref(c)
    got = deser_all(c.dim, R["seq"], R["nodes"], R["count"], R["shape"], "smooth", ft=np.float32, trunc=c.trunc)
    assert got.dtype == np.float32
    check_des(c, got, "host")


@pytest.mark.parametrize("c", [c for c in DESS if c.tier == "near"], ids=lambda c: c.id)
def test_nearest_wrong_references_differ_on_the_host(c):
    R = des_ref(c)
    for name, w in R["wrongs"].items():
        assert not np.array_equal(w, R["cands"][0]), (c.id, name)
    assert set(wrong_variants(c)) == set(R["wrongs"])


@pytest.mark.parametrize("c", LABS, ids=lambda c: c.id)
def test_label_wrong_references_differ_on_the_host(c):
    R = lab_ref(c)
    for name, w in R["wrongs"].items():
        assert not np.array_equal(w, R["idx"]) or c.nc == 1, (c.id, name)
    oh = onehot_of(R["idx"], c.nc)
    assert oh.shape == (2, c.nc, R["idx"][0].size) and (oh.sum(1) == 1).all()


def _golden():
    return np.load(GOLDEN)


def _golden_case(G, i, p):
    """B = 2 from one fixture tree: element 0 the whole list, element 1 the first half of it (what the reference gives with the other rows and
    regions zero, since leaves do not overlap)"""
    L, n = int(G[f"L{i}"]), len(G[f"nodes{i}"])
    nodes = np.zeros((2, L, 6), np.int32)
    nodes[:, :n] = G[f"nodes{i}"]
    count = np.array([n, n // 2], np.int32)
    labels = np.stack([G[f"labels{i}"]] * 2)
    idx = np.zeros((2, L, p, p, p), np.int64)
    idx[0, :n] = G[f"seq_labels{i}_p{p}"]
    idx[1, :n // 2] = G[f"seq_labels{i}_p{p}"][:n // 2]
    seq = np.stack([G[f"patches{i}_p{p}"]] * 2)
    painted = np.stack([G[f"painted{i}_p{p}"]] * 2)[..., None].copy()
    for nd in G[f"nodes{i}"][n // 2:]:
        painted[1, nd[4]:nd[5], nd[2]:nd[3], nd[0]:nd[1]] = 0
    return nodes, count, labels, idx, seq, painted


GOLD = [(i, p) for i in (0, 1) for p in (2, 4, 8)]


@pytest.mark.parametrize("i,p", GOLD)
def test_rules_reproduce_the_reference_fixtures_on_the_host(i, p):
    """the integer rule == the reference's serialize_labels bit for bit; the float64 trilinear rule == its deserialize to 1e-9; the fp32 emulation
    within the bound of the reference"""
    G = _golden()
    nodes, count, labels, idx, seq, painted = _golden_case(G, i, p)
    N = labels.shape[1]
    assert np.array_equal(labels_all(3, labels, nodes, count, p), idx)
    ref, tol, _ = deser_all(3, seq, nodes, count, (N,) * 3, bound=True)
    assert np.abs(ref - painted).max() <= 1e-9
    emu = deser_all(3, seq, nodes, count, (N,) * 3, ft=np.float32)
    _check_fixture(emu, painted, seq, nodes, count, "host")


def _check_fixture(got, painted, seq, nodes, count, backend):
    N = painted.shape[1]
    tol = None
    for bias in _biases(3):
        _, t, _ = deser_all(3, seq, nodes, count, (N,) * 3, bias=bias, bound=True)
        tol = t if tol is None else np.maximum(tol, t)
    err = np.abs(got.astype(np.float64) - painted)
    q = np.where(err == 0, 0.0, err / np.maximum(tol + 1e-9, 1e-300))
    key = f"octree fixtures [{backend}]"
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(q.max()))
    print(f"RATIO {key} N={N}: worst err/bound {q.max():.3f}")
    assert (err <= tol + 1e-9).all(), f"[{backend}] worst err/bound {q.max():.3g}"
    assert not got[painted == 0][tol[painted == 0] == 0].any()


# ============================================================================================== the library on carved buffers
def _carve(a, fill):
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


def _raw_labels(dim, lab, nd, ct, idx, oh, p, nc, dtcode=None, shape=None):
    lib = _lib().load()
    dtcode = (_lib().LABEL_U8 if lab.dtype == torch.uint8 else _lib().LABEL_I64) if dtcode is None else dtcode
    shape = tuple(lab.shape) if shape is None else shape
    B, S = shape[0], nd.shape[1]
    ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    if dim == 2:
        return lib.ucfvit_quadtree_serialize_labels(lab.data_ptr(), nd.data_ptr(), ct.data_ptr(), ptr(idx), ptr(oh), B, shape[1], shape[2], S, p, nc, dtcode,
                                                    _stream())
    return lib.ucfvit_octree_serialize_labels(lab.data_ptr(), nd.data_ptr(), ct.data_ptr(), ptr(idx), ptr(oh), B, shape[1], S, p, nc, dtcode, _stream())


def hip_labels(dim, labels, nodes, count, p, nc):
    """ops.*_serialize_labels on carved inputs, then the library into sentinel-carved outputs, both at once and each alone: all bit for bit the same,
    nothing written beyond the outputs -> (idx, onehot) as numpy"""
    ops = _ops()
    lab, _ = _carve(labels, 3)
    nd, _ = _carve(nodes, ISENT)
    ct, _ = _carve(count, ISENT)
    fn = ops.quadtree_serialize_labels if dim == 2 else ops.octree_serialize_labels
    idx_a, oh_a = fn(lab, nd, ct, p, nc)
    B, S = nodes.shape[:2]
    assert tuple(idx_a.shape) == (B, S) + (p,) * dim and idx_a.dtype == torch.int64
    assert tuple(oh_a.shape) == (B, nc, S * p ** dim) and oh_a.dtype == torch.float32
    for want_idx, want_oh in ((True, True), (True, False), (False, True)):
        idx_o, ibuf = _carve_out(idx_a.shape, torch.int64, LSENT)
        oh_o, obuf = _carve_out(oh_a.shape, torch.float32, FSENT)
        rc = _raw_labels(dim, lab, nd, ct, idx_o if want_idx else None, oh_o if want_oh else None, p, nc)
        assert rc == 0, _lib().load().ucfvit_last_error()
        torch.cuda.synchronize()
        assert _bits_equal(idx_o, idx_a) if want_idx else _untouched(ibuf, LSENT)
        assert _bits_equal(oh_o, oh_a) if want_oh else _untouched(obuf, FSENT)
        assert _guards_ok(ibuf, LSENT) and _guards_ok(obuf, FSENT), "bytes beyond the outputs were written"
    only_idx, none = fn(lab, nd, ct, p, nc, want_onehot=False)
    assert none is None and _bits_equal(only_idx, idx_a)
    return idx_a.cpu().numpy(), oh_a.cpu().numpy()


def hip_deserialize(dim, seq, nodes, count, shape, p, mode, trunc=False):
    """ops.*_deserialize from the patch list [B, S, p.., C] into channels-last and from the model layout [B, C, S, p^d] into planar, then the library
    with the layouts crossed into sentinel-carved outputs: identical bits everywhere -> the channels-last image as numpy"""
    ops, lib, L = _ops(), _lib().load(), _lib()
    B, S, C, P = seq.shape[0], seq.shape[1], seq.shape[-1], p ** dim
    npix = int(np.prod(shape))
    sq, _ = _carve(seq, float("nan"))
    sm, _ = _carve(np.ascontiguousarray(np.moveaxis(seq.reshape(B, S, P, C), 3, 1)), float("nan"))
    nd, _ = _carve(nodes, ISENT)
    ct, _ = _carve(count, ISENT)
    size = tuple(shape) if dim == 2 else shape[0]
    smooth = "bicubic" if dim == 2 else "trilinear"
    kw = dict(mode="nearest" if mode == "nearest" else smooth)
    if dim == 2:
        kw["truncate"] = trunc
    fn = ops.quadtree_deserialize if dim == 2 else ops.octree_deserialize
    a = fn(sq, nd, ct, size, p, channels_last=True, **kw)
    b = fn(sm, nd, ct, size, p, channels_last=False, **kw)
    assert tuple(a.shape) == (B,) + tuple(shape) + (C,) and tuple(b.shape) == (B, C) + tuple(shape)
    assert _bits_equal(a, b.movedim(1, -1)), "the two layouts give different bits"
    m = L.RESAMPLE_NEAREST if mode == "nearest" else L.RESAMPLE_SMOOTH
    list_str, model_str = (S * P * C, 1, P * C, C), (C * S * P, S * P, P, 1)
    for src, sstr, planar in ((sq, list_str, True), (sm, model_str, False)):
        out, buf = _carve_out((B, C) + tuple(shape) if planar else (B,) + tuple(shape) + (C,), torch.float32, FSENT)
        ostr = (npix * C, npix, 1) if planar else (npix * C, 1, C)
        if dim == 2:
            rc = lib.ucfvit_quadtree_deserialize(src.data_ptr(), nd.data_ptr(), ct.data_ptr(), out.data_ptr(), B, shape[0], shape[1], C, S, p, *sstr, *ostr, m,
                                                 int(trunc), _stream())
        else:
            rc = lib.ucfvit_octree_deserialize(src.data_ptr(), nd.data_ptr(), ct.data_ptr(), out.data_ptr(), B, shape[0], C, S, p, *sstr, *ostr, m, _stream())
        assert rc == 0, lib.ucfvit_last_error()
        torch.cuda.synchronize()
        assert _bits_equal(out, b if planar else a), "the library call differs from ops"
        assert _guards_ok(buf, FSENT), "bytes beyond the output were written"
    return a.cpu().numpy()


# ============================================================================================== GPU half
@gpu
@pytest.mark.parametrize("c", LABS, ids=lambda c: c.id)
def test_serialize_labels(c):
    R = lab_ref(c)
    idx, oh = hip_labels(c.dim, R["labels"], R["nodes"], R["count"], c.p, c.nc)
    assert np.array_equal(idx, R["idx"]), f"{c.id}: {int((idx != R['idx']).sum())} class indices differ"
    assert np.array_equal(oh, onehot_of(R["idx"], c.nc)), f"{c.id}: the one-hot block differs"
    B, S = R["nodes"].shape[:2]
    for b in range(B):
        for s in range(S):
            if not _valid(R["nodes"], R["count"], b, s):
                assert not idx[b, s].any(), f"{c.id}: row {b},{s} is not class 0"
    for name, w in R["wrongs"].items():
        assert c.nc == 1 or not np.array_equal(idx, w), f"{c.id}: the wrong reference '{name}' is not rejected"


@gpu
@pytest.mark.parametrize("dim", (2, 3))
def test_serialize_labels_count_zero_and_out_of_range(dim):
    """count = 0: everything class 0.  Labels >= nc (uint8 7 at nc = 4; int64 -3, 2^40, 4): written unchanged to the index output, all-zero
    one-hot column, sentinels intact (hip_labels)"""
    p, nc = 2, 4
    shape = (2, 9, 11) if dim == 2 else (2, 6, 6, 6)
    box = [[1, 3, 2, 4], [0, 11, 0, 9]] if dim == 2 else [[1, 3, 2, 4, 0, 2], [0, 6, 0, 6, 0, 6]]
    nodes = np.array([box + [[0] * (2 * dim)], box[::-1] + [[0] * (2 * dim)]], np.int32)
    for dtype, bad in ((np.uint8, (7, 255, 4)), (np.int64, (-3, 2 ** 40, 4))):
        labels = _rng("oor", dim, dtype).integers(0, nc, shape).astype(dtype)
        labels[0, 2, 1] = bad[0] if dim == 2 else labels[0, 2, 1]
        if dim == 2:
            labels[0, 3, 2], labels[1, 0, 0] = bad[1], bad[2]
        else:
            labels[0, 0, 2, 1], labels[0, 1, 3, 2], labels[1, 0, 0, 0] = bad
        count = np.array([2, 2], np.int32)
        want = labels_all(dim, labels, nodes, count, p)
        assert sum(int((want == v).sum()) > 0 for v in bad) == 3, "the out-of-range labels are not sampled"
        idx, oh = hip_labels(dim, labels, nodes, count, p, nc)
        assert np.array_equal(idx, want) and np.array_equal(oh, onehot_of(want, nc))
        cols = oh.sum(1).reshape(want.shape)
        assert (cols[(want < 0) | (want >= nc)] == 0).all() and (cols[(want >= 0) & (want < nc)] == 1).all()
        idx, oh = hip_labels(dim, labels, nodes, np.zeros(2, np.int32), p, nc)
        assert not idx.any() and (oh[:, 0] == 1).all() and not oh[:, 1:].any()


@gpu
@pytest.mark.parametrize("i,p", GOLD)
def test_octree_fixtures(i, p):
    """the reference's serialize_labels bit for bit (uint8 and int64 labels) and its deserialize within the bound, both layouts"""
    G = _golden()
    nodes, count, labels, idx, seq, painted = _golden_case(G, i, p)
    for lab in (labels, labels.astype(np.int64)):
        got, oh = hip_labels(3, lab, nodes, count, p, 4)
        assert np.array_equal(got, idx) and np.array_equal(oh, onehot_of(idx, 4))
    N = labels.shape[1]
    got = hip_deserialize(3, seq, nodes, count, (N,) * 3, p, "smooth")
    _check_fixture(got, painted, seq, nodes, count, "MI355X")
    # nearest mode paints the reference's label patches back: where the leaf is as wide as the patch this is the label volume itself
    back = hip_deserialize(3, idx.astype(np.float32)[..., None], nodes, count, (N,) * 3, p, "nearest")
    assert np.array_equal(back, deser_all(3, idx.astype(np.float32)[..., None], nodes, count, (N,) * 3, "nearest"))
    for nd in nodes[0, :count[0]]:
        if nd[1] - nd[0] == p:
            sl = (0, slice(nd[4], nd[5]), slice(nd[2], nd[3]), slice(nd[0], nd[1]))
            assert np.array_equal(back[sl][..., 0], labels[sl])


@gpu
@pytest.mark.parametrize("c", DESS, ids=lambda c: c.id)
def test_deserialize(c):
    R = des_ref(c)
    got = hip_deserialize(c.dim, R["seq"], R["nodes"], R["count"], R["shape"], c.p, "nearest" if c.tier == "near" else "smooth", c.trunc)
    check_des(c, got, "MI355X")
    if c.fam == "pm27":
        assert set(np.unique(got).tolist()) == {-2.0, 0.0, 2.0}


def _block_constant(dim, nodes, count, shape, p, rng):
    """a label map that is constant on every block of every leaf (2-D: the (w / p) x (h / p) blocks where p divides both; else and in 3-D the leaf)"""
    x = rng.integers(0, 4, (nodes.shape[0],) + tuple(shape)).astype(np.int64)
    for b in range(nodes.shape[0]):
        for s in range(int(count[b])):
            nd = nodes[b, s].astype(np.int64)
            ext = nd[1::2] - nd[0::2]
            if (ext <= 0).any():
                continue
            sl = (b,) + tuple(slice(nd[2 * a], nd[2 * a + 1]) for a in reversed(range(dim)))
            if dim == 2 and (ext % p == 0).all():
                blocks = rng.integers(0, 4, (p, p))
                x[sl] = np.repeat(np.repeat(blocks, ext[1] // p, 0), ext[0] // p, 1)
            else:
                x[sl] = rng.integers(0, 4)
    return x


@gpu
@pytest.mark.parametrize("dim,p", [(2, 1), (2, 2), (3, 1), (3, 2), (3, 3)])
def test_round_trip_through_a_built_tree(dim, p):
    """deserialize_nearest(serialize_labels(x)) == x on the tree the builder makes (12x20 at L = 100, 12^3 at L = 120; B = 3 maps): on any x for the
    leaves as wide as the patch, on a block-constant x for every leaf with p | w (see the docstring); class indices and one-hot planes"""
    ops = _ops()
    rng = _rng("trip", dim, p)
    shape, L = ((12, 20), 100) if dim == 2 else ((12, 12, 12), 120)
    maps = np.stack([np.zeros(shape, np.uint8), (rng.random(shape) < 0.3).astype(np.uint8) * 255, (rng.random(shape) < 0.05).astype(np.uint8) * 255])
    dom = torch.from_numpy(maps).to(DEV)
    nodes_t, _, count_t, _ = ops.quadtree_build(dom, L) if dim == 2 else ops.octree_build(dom, L)
    nodes, count = nodes_t.cpu().numpy(), count_t.cpu().numpy()
    size = shape if dim == 2 else shape[0]
    ser = ops.quadtree_serialize_labels if dim == 2 else ops.octree_serialize_labels
    des = ops.quadtree_deserialize if dim == 2 else ops.octree_deserialize
    seen = {"same": 0, "multiple": 0}
    for kind in ("any", "block"):
        x = rng.integers(0, 4, (3,) + shape).astype(np.int64) if kind == "any" else _block_constant(dim, nodes, count, shape, p, rng)
        idx, oh = ser(torch.from_numpy(x).to(DEV), nodes_t, count_t, p, 4)
        assert np.array_equal(idx.cpu().numpy(), labels_all(dim, x, nodes, count, p))
        back = des(idx.float().unsqueeze(-1), nodes_t, count_t, size, p, mode="nearest")[..., 0].cpu().numpy()
        planes = des(oh.view(3, 4, L, p ** dim), nodes_t, count_t, size, p, mode="nearest", channels_last=False).cpu().numpy()
        for b in range(3):
            for s in range(int(count[b])):
                nd = nodes[b, s].astype(np.int64)
                ext = nd[1::2] - nd[0::2]
                if (ext <= 0).any() or (ext % p != 0).any() or (kind == "any" and (ext != p).any()):
                    continue
                sl = tuple(slice(nd[2 * a], nd[2 * a + 1]) for a in reversed(range(dim)))
                assert np.array_equal(back[b][sl], x[b][sl]), (kind, b, s, nd.tolist())
                assert np.array_equal(planes[b].argmax(0)[sl], x[b][sl]) and (planes[b].sum(0)[sl] == 1).all()
                seen["same" if (ext == p).all() else "multiple"] += 1
    assert seen["same"] > 0 and (seen["multiple"] > 0 or p > 2), seen


@gpu
def test_refusals_write_nothing():
    lib, L = _lib().load(), _lib()
    lab, _ = _carve(np.zeros((2, 8, 8), np.uint8), 3)
    vol, _ = _carve(np.zeros((2, 4, 4, 4), np.uint8), 3)
    nd2, _ = _carve(np.tile(np.array([0, 8, 0, 8], np.int32), (2, 1, 1)), ISENT)
    nd3, _ = _carve(np.tile(np.array([0, 4, 0, 4, 0, 4], np.int32), (2, 1, 1)), ISENT)
    ct, _ = _carve(np.ones(2, np.int32), ISENT)
    idx, ibuf = _carve_out((2, 1, 4, 4, 4), torch.int64, LSENT)
    oh, obuf = _carve_out((2, 4, 64), torch.float32, FSENT)
    bad = [(2, lab, nd2, 0, 4, None, None), (2, lab, nd2, 2, 0, None, None), (2, lab, nd2, 2, 256, None, None), (2, lab, nd2, 2, 4, 2, None),
           (2, lab, nd2, 2, 4, None, (2, 32768, 8)), (2, lab, nd2, 2, 4, None, (2, 8, 32768)),
           (3, vol, nd3, 0, 4, None, None), (3, vol, nd3, 2, 0, None, None), (3, vol, nd3, 2, 256, None, None), (3, vol, nd3, 2, 4, -1, None),
           (3, vol, nd3, 2, 4, None, (2, 257, 257, 257))]
    for dim, la, nd, p, nc, code, shape in bad:
        rc = _raw_labels(dim, la, nd, ct, idx, oh, p, nc, code, shape)
        assert rc == -1 and lib.ucfvit_last_error(), (dim, p, nc, code, shape)
    assert _raw_labels(2, lab, nd2, ct, None, None, 2, 4) == -1                          # nothing to write
    seq, _ = _carve(np.zeros((2, 1, 2, 2, 2, 1), np.float32), 0.0)
    out, fbuf = _carve_out((2, 8, 8, 8, 1), torch.float32, FSENT)
    s = _stream()
    q = lambda B=2, H=8, W=8, C=1, S=1, p=2, sstr=(4, 1, 4, 1), ostr=(64, 1, 1), mode=0, tr=0: lib.ucfvit_quadtree_deserialize(      # noqa: E731
        seq.data_ptr(), nd2.data_ptr(), ct.data_ptr(), out.data_ptr(), B, H, W, C, S, p, *sstr, *ostr, mode, tr, s)
    o = lambda B=2, N=8, C=1, S=1, p=2, sstr=(8, 1, 8, 1), ostr=(512, 1, 1), mode=0: lib.ucfvit_octree_deserialize(                   # noqa: E731
        seq.data_ptr(), nd3.data_ptr(), ct.data_ptr(), out.data_ptr(), B, N, C, S, p, *sstr, *ostr, mode, s)
    for rc in (q(p=0), q(H=32768), q(W=32768), q(C=0), q(C=256), q(S=0), q(mode=2), q(ostr=(64, 1, 2)), q(ostr=(128, 64, 1)), q(sstr=(4, 1, 4, 0)),
               o(p=0), o(N=257), o(N=0), o(C=0), o(mode=-1), o(ostr=(512, 2, 1)), o(sstr=(8, 0, 8, 1))):
        assert rc == -1 and lib.ucfvit_last_error()
    torch.cuda.synchronize()
    assert _untouched(ibuf, LSENT) and _untouched(obuf, FSENT) and _untouched(fbuf, FSENT)
    # B = 0 with null pointers is a no-op
    assert lib.ucfvit_quadtree_serialize_labels(None, None, None, None, None, 0, 8, 8, 1, 2, 4, L.LABEL_U8, s) == 0
    assert lib.ucfvit_octree_serialize_labels(None, None, None, None, None, 0, 4, 1, 2, 4, L.LABEL_I64, s) == 0
    assert lib.ucfvit_quadtree_deserialize(None, None, None, None, 0, 8, 8, 1, 1, 2, 4, 1, 4, 1, 64, 1, 1, 0, 0, s) == 0
    assert lib.ucfvit_octree_deserialize(None, None, None, None, 0, 8, 1, 1, 2, 8, 1, 8, 1, 512, 1, 1, 0, s) == 0
    # the accepted neighbours of the refusals do run
    assert q() == 0 and o() == 0
    torch.cuda.synchronize()
    assert _guards_ok(fbuf, FSENT)


@gpu
def test_ops_refusals():
    ops = _ops()
    from UCF_VIT.dataloaders.transform import Patchify, Patchify_3D
    lab = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    vol = torch.zeros((2, 4, 4, 4), dtype=torch.int64, device=DEV)
    nd2 = torch.tensor([[[0, 8, 0, 8]]] * 2, dtype=torch.int32, device=DEV)
    nd3 = torch.tensor([[[0, 4, 0, 4, 0, 4]]] * 2, dtype=torch.int32, device=DEV)
    ct = torch.ones(2, dtype=torch.int32, device=DEV)
    seq2, seq3 = torch.zeros((2, 1, 2, 2, 1), device=DEV), torch.zeros((2, 1, 2, 2, 2, 1), device=DEV)
    with pytest.raises(TypeError):
        ops.quadtree_serialize_labels(lab.int(), nd2, ct, 2, 4)                          # wrong label dtype
    with pytest.raises(TypeError):
        ops.quadtree_serialize_labels(lab[0], nd2, ct, 2, 4)                             # wrong rank
    with pytest.raises(TypeError):
        ops.quadtree_serialize_labels(lab, nd3, ct, 2, 4)                                # octree nodes
    with pytest.raises(TypeError):
        ops.quadtree_serialize_labels(lab, nd2.long(), ct, 2, 4)
    with pytest.raises(TypeError):
        ops.octree_serialize_labels(vol[:, :, :, :3].contiguous(), nd3, ct, 2, 4)        # not cubic
    with pytest.raises(TypeError):
        ops.octree_serialize_labels(vol.float(), nd3, ct, 2, 4)
    with pytest.raises(RuntimeError):
        ops.quadtree_serialize_labels(lab.transpose(1, 2), nd2, ct, 2, 4)                # non-contiguous labels
    with pytest.raises(RuntimeError):
        ops.octree_serialize_labels(vol.transpose(1, 3), nd3, ct, 2, 4)
    with pytest.raises(RuntimeError):
        ops.quadtree_serialize_labels(lab.cpu(), nd2, ct, 2, 4)
    for bad in (dict(patch=0, num_classes=4), dict(patch=2, num_classes=0), dict(patch=2, num_classes=256)):
        with pytest.raises(ValueError):
            ops.quadtree_serialize_labels(lab, nd2, ct, **bad)
        with pytest.raises(ValueError):
            ops.octree_serialize_labels(vol, nd3, ct, **bad)
    with pytest.raises(ValueError):
        ops.quadtree_serialize_labels(lab, nd2, ct, 2, 4, want_idx=False, want_onehot=False)
    with pytest.raises(TypeError):
        ops.quadtree_deserialize(seq2.double(), nd2, ct, (8, 8), 2)
    with pytest.raises(TypeError):
        ops.quadtree_deserialize(seq2[0], nd2, ct, (8, 8), 2)                            # wrong rank
    with pytest.raises(TypeError):
        ops.quadtree_deserialize(seq3, nd2, ct, (8, 8), 2)
    with pytest.raises(ValueError):
        ops.quadtree_deserialize(seq2, nd2, ct, (8, 8), 2, mode="trilinear")
    with pytest.raises(ValueError):
        ops.octree_deserialize(seq3, nd3, ct, 4, 2, mode="bicubic")
    with pytest.raises(ValueError):
        ops.octree_deserialize(seq3, nd3, ct, (4, 4, 5), 2)
    with pytest.raises(ValueError):
        ops.quadtree_deserialize(seq2, nd2[:, :0], ct, (8, 8), 2)                        # sequence lengths disagree
    with pytest.raises(RuntimeError):
        ops.quadtree_deserialize(seq2.expand(2, 1, 2, 2, 3), nd2, ct, (8, 8), 2)         # zero-stride channel axis
    with pytest.raises(RuntimeError):
        ops.octree_deserialize(seq3, nd3, ct, 257, 2)                                    # the library's N <= 256
    with pytest.raises(ValueError):
        Patchify_3D(8, 2, 1).deserialize(seq3, nd3, ct, 4, truncate=True)
    # the modules: labels through forward's tree, shapes and the default modes
    pq, po = Patchify(4, 2, 1), Patchify_3D(8, 2, 1)
    nd2b, nd3b = nd2.repeat(1, 4, 1), nd3.repeat(1, 8, 1)
    assert tuple(pq.serialize_labels(lab, nd2b, ct, 3).shape) == (2, 3, 4 * 4) and tuple(pq.serialize_labels(lab, nd2b, ct, 3, one_hot=False).shape) == (2, 4, 2, 2)
    assert tuple(po.serialize_labels(vol, nd3b, ct, 3).shape) == (2, 3, 8 * 8)
    assert tuple(pq.deserialize(torch.zeros((2, 3, 4, 4), device=DEV), nd2b, ct, (8, 8), channels_last=False).shape) == (2, 3, 8, 8)
    assert tuple(po.deserialize(torch.zeros((2, 8, 2, 2, 2, 1), device=DEV), nd3b, ct, 4, mode="nearest").shape) == (2, 4, 4, 4, 1)
