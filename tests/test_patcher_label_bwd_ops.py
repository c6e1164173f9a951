"""The adjoints of the tree deserializers (csrc/patcher_labels_bwd.hip: deserialize_bwd_kernel<ND, RULE> and deserialize_bwd_sum_kernel<ND>) element
by element, through UCF_VIT._hip.ops, through UCF_VIT._hip.lib into outputs carved from sentinel-filled allocations, and through autograd
(HF.deserialize, Patchify.deserialize).  The host emulation of the forward and the node tables are those of tests/test_patcher_label_ops.py,
imported, not copied.  U = 2^-24.

Reference.  Per leaf and axis a matrix W[x, k]: the sum, in float64, of the fp32 weights with which leaf position x reads token index k in the
forward (axis_weights: the forward's position expression in fp32, cubic_weights of the sibling file, the clamped taps; the unit is built
without contraction, so these are the device's weights).  The adjoint is dseq[c, k] = sum_x prod_axes W[x_a, k_a] dout[c, x] in float64.  That
this is the adjoint of the forward the sibling file pins is shown on the host: <paint(seq), g> = <seq, adjoint(g)> for every case table, to
1024 U sum over taps |seq| |g| (paint evaluates its weights in float64; cubic_bounds gives at most 9 U ptilde <= 324 U for a coefficient and
df |dw / dt| <= 75 U for its position, per axis).  References with the axes' extents exchanged, without the half-pixel bias and with ties sent
up are shown to fall outside the bound.

Bound of the per-element tier: the kernel adds, innermost axis first, products w g (one rounding each), multiplies a row's sum by the row's
weight (one rounding; once more for a plane in 3-D) and adds the rows; a leaf of more than 1024 pixels is cut into at most 16 slices whose
partial sums are added in order.  Every term therefore passes through at most 3 product roundings and through at most
Kx + Ky + Kz + 16 <= K + 2 + 16 additions, K the number of tap terms of the element:
    |got - ref64| <= (K + 21) U sum |w| |g| (1 + 2^-10).
Exact tiers (bits): nearest mode with integer dout, |g| <= 8 (an int64 sum); leaves whose weights are all 0 or 1 (bicubic at extent = p,
trilinear at extent = p where k (p - 1) fl(1 / (p - 1)) == k) on wild dout: dseq is the gathered dout; leaves whose weights are multiples
of 2^-q, q <= 10 (bicubic at extent 2 p: q = 8; trilinear at extent 2 p - 1 for p - 1 a power of two: q = 1) with dout in -2 .. 2, where
sum |w| |g| 2^(d q) < 2^24 makes every partial sum an fp32 number.  Each premise is asserted on the emulated weights.

worst err / bound on an MI355X, from a run of this file (-s prints a RATIO line per case): 2-D bicubic 0.055 .. 0.105 (p = 3, 8, 16; uniform,
randn, randn + 1000), 3-D trilinear 0.008 .. 0.073 (p = 1, 2, 4, 7); against the per-leaf F.interpolate loop under autograd 0.004 (2-D) and
0.002 (3-D).  The bound counts every tap term as one sequential addition while the kernel's sums are nested, so it is loose by construction;
it still tells every wrong reference apart.  The whole file: 44 GPU tests in 4 s, 36 host tests in 7 s.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_patcher_label_ops import (DEV, FSENT, ISENT, O_EXT, O_PAINT_FULL, ON, Q_EXT, Q_PAINT, QH, QW, U, _bits_equal, _carve, _carve_out,  # noqa: E402
                                    _guards_ok, _lib, _ops, _rng, _stream, _untouched, _with_empties, cubic_bounds, cubic_weights, deser_all,
                                    exact_list, nearest_floor, nearest_grid)            # deser_all: bicubic_paint / trilinear_paint per leaf

gpu = pytest.mark.gpu
SLICES, SLICE_PIXELS = 16, 1024                     # csrc/patcher_gather.h: BWD_SLICES, BWD_SLICE_PIXELS
CB = 3 + SLICES + 2                                 # see the docstring
RATIOS = {}


# ============================================================================================== the reference
def axis_weights(rule, n, p, n_scale=None, half=True, ties_up=False):
    """rule 'cubic' | 'linear' | 'floor' | 'grid': n leaf positions against p token indices -> (W, Wabs, T) [n, p]: the float64 sum of the emulated
    fp32 taps of x on k, of their magnitudes, and their number.  n_scale: the extent the rule is evaluated with (the wrong reference 'swap');
    half=False drops the half-pixel bias; ties_up sends the grid rule's ties up"""
    f32 = np.float32
    ns = n if n_scale is None else n_scale
    x = np.arange(n)
    W, Wabs, T = np.zeros((n, p)), np.zeros((n, p)), np.zeros((n, p), np.int64)

    def put(idx, w):
        np.add.at(W, (x, idx), w.astype(np.float64))
        np.add.at(Wabs, (x, idx), np.abs(w.astype(np.float64)))
        np.add.at(T, (x, idx), 1)
    if rule == "cubic":
        scale = f32(p) / f32(ns)
        f = (x.astype(f32) + f32(0.5)) * scale - f32(0.5) if half else x.astype(f32) * scale
        fl = np.floor(f)
        w = cubic_weights(f - fl, -0.75, f32)
        assert w.dtype == f32
        for d in range(4):
            put(np.clip(fl.astype(np.int64) - 1 + d, 0, p - 1), w[d])
    elif rule == "linear":
        inv = f32(1) / f32(ns - 1) if ns > 1 else f32(0)
        f = x.astype(f32) * f32(p - 1) * inv
        i0 = np.minimum(f.astype(np.int64), p - 1)
        t = f - i0.astype(f32)
        put(i0, f32(1) - t)
        put(np.minimum(i0 + 1, p - 1), t)
    elif rule == "floor":
        put(nearest_floor(x, p, ns), np.ones(n, f32))
    else:
        put(np.minimum(nearest_grid(x, p, ns, ties_up), p - 1), np.ones(n, f32))
    return W, Wabs, T


def _rule(dim, mode):
    return {(2, "smooth"): "cubic", (2, "nearest"): "floor", (3, "smooth"): "linear", (3, "nearest"): "grid"}[dim, mode]


def _contract(mats, g):
    """mats per axis x, y(, z) [n_a, p]; g [(nz,) ny, nx, C] -> [(p,) p, p, C]"""
    out = g
    for a, M in enumerate(mats):                     # axis a of the leaf is array axis dim - 1 - a
        ax = len(mats) - 1 - a
        out = np.moveaxis(np.tensordot(M.T, out, axes=([1], [ax])), 0, ax)
    return out


def adjoint_leaf(dim, mode, g, ext, p, swap=False, half=True, ties_up=False, taps=False):
    """g float64 [(nz,) ny, nx, C] of one leaf of extents ext = (nx, ny(, nz)) -> (dseq [(p,) p, p, C], sum |w| |g|, K tap terms [(p,) p, p, 1])"""
    sw = [ext[1], ext[0]] + list(ext[2:]) if swap else list(ext)
    ws = [axis_weights(_rule(dim, mode), ext[a], p, sw[a], half, ties_up) for a in range(dim)]
    one = np.ones(tuple(reversed(ext)) + (1,))
    if taps:                                         # sum over the tap terms of |g|, unweighted
        return _contract([w[2].astype(np.float64) for w in ws], np.abs(g))
    return (_contract([w[0] for w in ws], g), _contract([w[1] for w in ws], np.abs(g)), _contract([w[2].astype(np.float64) for w in ws], one))


def live(nodes, count, b, s, shape):
    """a row the kernels read: below count, no empty extent, the box inside the image (shape (H, W) or (N, N, N))"""
    nd = nodes[b, s].astype(np.int64)
    dim = len(shape)
    if s >= count[b] or ((nd[1::2] - nd[0::2]) <= 0).any():
        return False
    return all(nd[2 * a] >= 0 and nd[2 * a + 1] <= shape[dim - 1 - a] for a in range(dim))


def adjoint_all(dim, mode, g, nodes, count, p, taps=False, **wrong):
    """g [B, *shape, C] -> (dseq float64 [B, S, p .. p, C], bound [same], sum |w| |g| [same]); rows that are not live are 0 with bound 0.
    taps: (the sum of |g| over an element's tap terms, None, None) instead"""
    B, S = nodes.shape[:2]
    shape, C = g.shape[1:-1], g.shape[-1]
    out = np.zeros((B, S) + (p,) * dim + (C,))
    tol, absum = np.zeros_like(out), np.zeros_like(out)
    g = g.astype(np.float64)
    for b in range(B):
        for s in range(S):
            if not live(nodes, count, b, s, shape):
                continue
            nd = nodes[b, s].astype(np.int64)
            ext = nd[1::2] - nd[0::2]
            sl = (b,) + tuple(slice(nd[2 * a], nd[2 * a + 1]) for a in reversed(range(dim)))
            if taps:
                out[b, s] = adjoint_leaf(dim, mode, g[sl], ext, p, taps=True)
                continue
            d, ab, K = adjoint_leaf(dim, mode, g[sl], ext, p, **wrong)
            out[b, s], tol[b, s], absum[b, s] = d, (K + CB) * U * ab * (1 + 2.0 ** -10), ab
    return (out, None, None) if taps else (out, tol, absum)


# ============================================================================================== cases
OUTSIDE = {2: [[290, 310, 0, 8], [-2, 3, 5, 9], [10, 20, 255, 265]], 3: [[60, 66, 0, 4, 0, 4], [-1, 3, 5, 9, 5, 9], [0, 4, 0, 4, 62, 65]]}


def bwd_list(dim):
    """B = 2 from the sibling's painting tables (every extent of Q_EXT / O_EXT, the 256^2 and 64^3 leaves of several slices): empty leaves and
    boxes that leave the image in between, padded to one length with padding rows; count[0] leaves the last valid row of element 0 out"""
    rows = []
    for r in (Q_PAINT if dim == 2 else O_PAINT_FULL):
        r = _with_empties(r, dim)
        for i, o in enumerate(OUTSIDE[dim]):
            r.insert(min(3 * i + 2, len(r) - 1), o)
        rows.append(r)
    S = max(len(r) for r in rows) + 1
    count = np.array([len(rows[0]) - 1, len(rows[1])], np.int32)
    for r in rows:
        r += [[0] * (2 * dim)] * (S - len(r))
    return np.array(rows, np.int32), count, ((QH, QW) if dim == 2 else (ON,) * 3)


CASES = [(2, p, C) for p in (3, 8, 16) for C in (1, 3)] + [(3, 1, 2), (3, 2, 1), (3, 4, 3), (3, 7, 1)]
FAMS = ("uniform", "randn", "randn1000")
BOUNDED = [(dim, p, C, FAMS[i % 3]) for i, (dim, p, C) in enumerate(CASES)] + [(2, 8, 3, "randn"), (2, 8, 3, "randn1000"), (3, 4, 3, "uniform"),
                                                                              (3, 4, 3, "randn1000")]
_id = lambda c: "-".join(str(v) for v in c)          # noqa: E731


def make_g(fam, shape, *key):
    g = torch.Generator().manual_seed(int(_rng("g", fam, shape, *key).integers(1 << 30)))
    if fam == "uniform":
        v = torch.rand(shape, generator=g, dtype=torch.float32) * 255
    elif fam == "int8":
        v = torch.randint(-8, 9, shape, generator=g).float()
    elif fam == "int2":
        v = torch.randint(-2, 3, shape, generator=g).float()
    else:
        v = torch.randn(shape, generator=g, dtype=torch.float32)
        v = v + 1000.0 if fam == "randn1000" else (v * 1000.0 if fam == "wild" else v)
    return v.numpy()


@functools.lru_cache(maxsize=None)
def bwd_ref(dim, p, C, fam, mode):
    nodes, count, shape = bwd_list(dim)
    g = make_g(fam, (2,) + tuple(shape) + (C,), dim, p, mode)
    want, tol, _ = adjoint_all(dim, mode, g, nodes, count, p)
    return dict(g=g, nodes=nodes, count=count, shape=shape, want=want, tol=tol)


def wrongs_of(dim, mode, p):
    w = {}
    if p > 1:
        w["swap"] = dict(swap=True)
    if dim == 2 and mode == "smooth":
        w["bias"] = dict(half=False)
    if dim == 3 and mode == "nearest" and p > 1:
        w["ties"] = dict(ties_up=True)
    return w


def check_bounded(key, got, R, dim, mode, p, backend):
    want, tol = R["want"], R["tol"]
    assert got.shape == want.shape and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - want)
    q = np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))
    RATIOS[f"{key} [{backend}]"] = float(q.max())
    print(f"RATIO deserialize_bwd {key} [{backend}]: worst err/bound {q.max():.3f}")
    bad = err > tol
    assert not bad.any(), f"{key} [{backend}]: {int(bad.sum())} of {bad.size} elements out of bound, worst err/bound {q.max():.3g} at {np.argwhere(bad)[0].tolist()}"
    for name, kw in wrongs_of(dim, mode, p).items():
        w, _, _ = adjoint_all(dim, mode, R["g"], R["nodes"], R["count"], p, **kw)
        assert (np.abs(w - want) > tol).any(), f"{key}: the wrong reference '{name}' lies within the bound of the right one"
        assert (np.abs(got.astype(np.float64) - w) > tol).any(), f"{key} [{backend}]: the wrong reference '{name}' is not rejected"


# ---- exact tiers: the leaf tables and their premises
def exact_case(dim, kind, p):
    """kind 'id': extent p; 'half': bicubic extent 2 p, trilinear extent 2 p - 1 -> (nodes, count, shape, q) with every weight a multiple of 2^-q"""
    e = p if kind == "id" else (2 * p if dim == 2 else 2 * p - 1)
    nodes, count, wid = exact_list(p, dim, [(e,) * dim] * 3)
    shape = (e + 3, wid + 2) if dim == 2 else (max(e + 3, wid + 2),) * 3
    W, _, _ = axis_weights(_rule(dim, "smooth"), e, p)
    q = next((k for k in range(11) if np.array_equal(W * 2.0 ** k, np.round(W * 2.0 ** k))), None)
    return nodes, count, shape, q, W


EXACT = [(2, "id", p) for p in (3, 8, 16)] + [(3, "id", p) for p in (1, 2, 3, 5, 9)] + [(2, "half", p) for p in (3, 8, 16)] + \
        [(3, "half", p) for p in (2, 3, 5)]


def exact_inputs(dim, kind, p, C=2):
    nodes, count, shape, q, W = exact_case(dim, kind, p)
    if kind == "id":
        assert q == 0 and np.array_equal(W, np.eye(p)), f"extent = p is not the identity for {dim}-D p = {p}"
    else:
        assert q is not None and q <= 10, f"the weights at the doubled extent are no multiples of 2^-10 ({dim}-D p = {p})"
    g = make_g("wild" if kind == "id" else "int2", (2,) + tuple(shape) + (C,), dim, kind, p)
    want, tol, absum = adjoint_all(dim, "smooth", g, nodes, count, p)
    if kind == "half":                               # every partial sum is a multiple of 2^-(dim q) below 2^(24 - dim q): an fp32 number
        assert float(absum.max()) * 2.0 ** (dim * q) < 2.0 ** 24
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want), "the float64 result is no fp32 number"
    return nodes, count, shape, g, want.astype(np.float32)


# ============================================================================================== host half
@pytest.mark.parametrize("dim", (2, 3))
def test_the_table_has_every_kind_of_row(dim):
    nodes, count, shape = bwd_list(dim)
    kinds = {"live": 0, "padding": 0, "empty": 0, "outside": 0, "sliced": 0}
    for b in range(2):
        for s in range(nodes.shape[1]):
            nd = nodes[b, s].astype(np.int64)
            ext = nd[1::2] - nd[0::2]
            if s >= count[b]:
                kinds["padding"] += 1
            elif (ext <= 0).any():
                kinds["empty"] += 1
            elif not live(nodes, count, b, s, shape):
                kinds["outside"] += 1
            else:
                kinds["live"] += 1
                kinds["sliced"] += int(np.prod(ext)) > SLICE_PIXELS
    assert all(v > 0 for v in kinds.values()), kinds
    have = {tuple(int(v) for v in (nd[1::2] - nd[0::2])) for b in range(2) for nd in nodes[b]}
    assert set(Q_EXT if dim == 2 else O_EXT) <= have
    assert count[0] != count[1]


@pytest.mark.parametrize("dim,p,C", CASES, ids=[_id(c) for c in CASES])
@pytest.mark.parametrize("mode", ("smooth", "nearest"))
def test_reference_is_the_adjoint_of_the_forward(dim, p, C, mode):
    """<paint(seq), g> = <seq, adjoint(g)> with the sibling file's float64 forward on the rows both sides read"""
    nodes, count, shape = bwd_list(dim)
    for b in range(2):                               # the sibling's forward does not test for boxes outside the image: take them out
        for s in range(nodes.shape[1]):
            if not live(nodes, count, b, s, shape):
                nodes[b, s] = 0
    rng = _rng("adj", dim, p, C, mode)
    seq = rng.random((2, nodes.shape[1]) + (p,) * dim + (C,)) + 0.5                      # positive: the two sides do not cancel to nothing
    g = rng.random((2,) + tuple(shape) + (C,)) + 0.5
    out = deser_all(dim, seq, nodes, count, shape, mode)
    adj, tol, _ = adjoint_all(dim, mode, g, nodes, count, p)
    lhs, rhs = float((out * g).sum()), float((seq * adj).sum())
    scale = float((seq * adjoint_all(dim, mode, g, nodes, count, p, taps=True)[0]).sum())
    assert abs(lhs - rhs) <= 1024 * U * scale, (lhs, rhs, scale)
    assert abs(lhs) > 100 * 1024 * U * scale, "the identity is vacuous on these inputs"
    for name, kw in wrongs_of(dim, mode, p).items():
        w, _, _ = adjoint_all(dim, mode, g, nodes, count, p, **kw)
        assert (np.abs(w - adj) > tol).any(), f"the wrong reference '{name}' lies within the bound"


@pytest.mark.parametrize("dim,kind,p", EXACT, ids=[_id(c) for c in EXACT])
def test_exact_tier_premises_hold_on_the_emulated_weights(dim, kind, p):
    nodes, count, shape, g, want = exact_inputs(dim, kind, p)
    if kind == "id":                                 # dseq is the gathered dout
        for b in range(2):
            for s in range(int(count[b])):
                nd = nodes[b, s]
                sl = (b,) + tuple(slice(nd[2 * a], nd[2 * a + 1]) for a in reversed(range(dim)))
                assert np.array_equal(want[b, s], g[sl])


# ============================================================================================== the library and the ops
def _raw_bwd(dim, dout, nd, ct, dseq, ws, B, shape, C, S, p, sstr, ostr, mode):
    lib = _lib().load()
    ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    if dim == 2:
        return lib.ucfvit_quadtree_deserialize_bwd(ptr(dout), ptr(nd), ptr(ct), ptr(dseq), B, shape[0], shape[1], C, S, p, *sstr, *ostr, mode, ptr(ws),
                                                   _stream())
    return lib.ucfvit_octree_deserialize_bwd(ptr(dout), ptr(nd), ptr(ct), ptr(dseq), B, shape[0], C, S, p, *sstr, *ostr, mode, ptr(ws), _stream())


def _ws(dim, B, shape, C, S, p):
    lib = _lib().load()
    n = lib.ucfvit_quadtree_deserialize_bwd_workspace(B, shape[0], shape[1], C, S, p) if dim == 2 else \
        lib.ucfvit_octree_deserialize_bwd_workspace(B, shape[0], C, S, p)
    assert n >= 0, lib.ucfvit_last_error()
    return torch.full((n // 4 + 1,), float("nan"), dtype=torch.float32, device=DEV)


def hip_bwd(dim, g, nodes, count, p, mode):
    """ops.*_deserialize_bwd from channels-last dout into the patch list [B, S, p.., C] and from planar dout into the model layout [B, C, S, p^d],
    each twice; then the library with the layouts crossed into sentinel-carved outputs and a NaN-filled workspace: identical bits everywhere, all
    rows written, guards intact -> the patch list as numpy"""
    ops, L = _ops(), _lib()
    B, S, C, P = g.shape[0], nodes.shape[1], g.shape[-1], p ** dim
    shape = g.shape[1:-1]
    npix = int(np.prod(shape))
    gl, _ = _carve(g, float("nan"))
    gp, _ = _carve(np.ascontiguousarray(np.moveaxis(g, -1, 1)), float("nan"))
    nd, _ = _carve(nodes, ISENT)
    ct, _ = _carve(count, ISENT)
    kw = dict(mode="nearest" if mode == "nearest" else ("bicubic" if dim == 2 else "trilinear"))
    fn = ops.quadtree_deserialize_bwd if dim == 2 else ops.octree_deserialize_bwd
    list_shape, model_shape = (B, S) + (p,) * dim + (C,), (B, C, S, P)
    a = fn(gl, nd, ct, list_shape, p, channels_last=True, **kw)
    b = fn(gp, nd, ct, model_shape, p, channels_last=False, **kw)
    assert tuple(a.shape) == list_shape and tuple(b.shape) == model_shape and a.dtype == torch.float32
    as_list = lambda t: t.view(B, C, S, P).movedim(1, 3).reshape(list_shape)          # noqa: E731
    assert _bits_equal(a, as_list(b)), "the two layouts give different bits"
    assert _bits_equal(a, fn(gl, nd, ct, list_shape, p, channels_last=True, **kw)) and _bits_equal(b, fn(gp, nd, ct, b, p, channels_last=False, **kw)), \
        "the same call twice gives different bits"
    m = L.RESAMPLE_NEAREST if mode == "nearest" else L.RESAMPLE_SMOOTH
    list_str, model_str = (S * P * C, 1, P * C, C), (C * S * P, S * P, P, 1)
    ws = _ws(dim, B, shape, C, S, p)
    for dout, planar, sstr, oshape in ((gl, False, model_str, model_shape), (gp, True, list_str, list_shape)):
        out, buf = _carve_out(oshape, torch.float32, FSENT)
        ostr = (npix * C, npix, 1) if planar else (npix * C, 1, C)
        rc = _raw_bwd(dim, dout, nd, ct, out, ws, B, shape, C, S, p, sstr, ostr, m)
        assert rc == 0, L.load().ucfvit_last_error()
        torch.cuda.synchronize()
        assert _bits_equal(out, a if oshape == list_shape else b), "the library call differs from ops"
        assert _guards_ok(buf, FSENT), "bytes beyond dseq were written"
    got = a.cpu().numpy()
    for bb in range(B):
        for s in range(S):
            if not live(nodes, count, bb, s, shape):
                assert not got[bb, s].any() and not np.signbit(got[bb, s]).any(), f"row {bb},{s} is not exactly 0"
    return got


@gpu
@pytest.mark.parametrize("dim,p,C", CASES, ids=[_id(c) for c in CASES])
def test_bwd_nearest_with_integer_dout_is_an_integer_sum(dim, p, C):
    R = bwd_ref(dim, p, C, "int8", "nearest")
    want = R["want"]
    assert np.array_equal(want, np.round(want)) and np.abs(want).max() < 2 ** 24
    got = hip_bwd(dim, R["g"], R["nodes"], R["count"], p, "nearest")
    assert np.array_equal(got.astype(np.int64), want.astype(np.int64)) and np.array_equal(got, np.round(got)), \
        f"{int((got != want).sum())} elements differ from the int64 sum"
    for name, kw in wrongs_of(dim, "nearest", p).items():
        w, _, _ = adjoint_all(dim, "nearest", R["g"], R["nodes"], R["count"], p, **kw)
        assert not np.array_equal(w, want) and not np.array_equal(got, w), name


@gpu
@pytest.mark.parametrize("dim,kind,p", EXACT, ids=[_id(c) for c in EXACT])
def test_bwd_exact_tiers(dim, kind, p):
    nodes, count, shape, g, want = exact_inputs(dim, kind, p)
    got = hip_bwd(dim, g, nodes, count, p, "smooth")
    want = want + np.float32(0)                      # a float64 sum may be -0; the kernel's 0.f + ... never is
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), \
        f"not bit for bit: {int((got != want).sum())} elements differ, worst {np.abs(got - want).max()}"


@gpu
@pytest.mark.parametrize("dim,p,C,fam", BOUNDED, ids=[_id(c) for c in BOUNDED])
def test_bwd_against_float64(dim, p, C, fam):
    R = bwd_ref(dim, p, C, fam, "smooth")
    got = hip_bwd(dim, R["g"], R["nodes"], R["count"], p, "smooth")
    check_bounded(_id((dim, p, C, fam)), got, R, dim, "smooth", p, "MI355X")


@gpu
@pytest.mark.parametrize("dim", (2, 3))
def test_count_zero_gives_zeros(dim):
    nodes, _, shape = bwd_list(dim)
    g = make_g("randn", (2,) + tuple(shape) + (2,), dim, "zero")
    for mode in ("smooth", "nearest"):
        got = hip_bwd(dim, g, nodes, np.zeros(2, np.int32), 4, mode)
        assert not got.any()


@gpu
def test_refusals_write_nothing():
    lib = _lib().load()
    nd2, _ = _carve(np.tile(np.array([0, 8, 0, 8], np.int32), (2, 1, 1)), ISENT)
    nd3, _ = _carve(np.tile(np.array([0, 4, 0, 4, 0, 4], np.int32), (2, 1, 1)), ISENT)
    ct, _ = _carve(np.ones(2, np.int32), ISENT)
    dout, _ = _carve(np.ones((2, 64, 32, 1), np.float32), 0.0)
    dseq, buf = _carve_out((2, 1, 2, 2, 2, 1), torch.float32, FSENT)
    ws = torch.zeros(1 << 16, device=DEV)
    q = lambda B=2, H=64, W=32, C=1, S=1, p=2, sstr=(4, 1, 4, 1), ostr=(2048, 1, 1), mode=0, d=dout, n=nd2, o=dseq, w=ws: _raw_bwd(      # noqa: E731
        2, d, n, ct, o, w, B, (H, W), C, S, p, sstr, ostr, mode)
    o = lambda B=2, N=8, C=1, S=1, p=2, sstr=(8, 1, 8, 1), ostr=(512, 1, 1), mode=0, d=dout, n=nd3, out=dseq, w=ws: _raw_bwd(           # noqa: E731
        3, d, n, ct, out, w, B, (N,), C, S, p, sstr, ostr, mode)
    for rc in (q(p=0), q(H=32768), q(W=32768), q(C=0), q(C=256), q(S=0), q(mode=2), q(ostr=(2048, 1, 2)), q(ostr=(1024, 2048, 1)), q(sstr=(4, 1, 4, 0)),
               q(sstr=(0, 1, 4, 1)), q(d=None), q(n=None), q(o=None), q(w=None), q(p=1025),
               o(p=0), o(N=257), o(N=0), o(C=0), o(mode=-1), o(ostr=(512, 2, 1)), o(sstr=(8, 0, 8, 1)), o(sstr=(0, 1, 8, 1)), o(d=None), o(p=257)):
        assert rc == -1 and lib.ucfvit_last_error()
    torch.cuda.synchronize()
    assert _untouched(buf, FSENT)
    assert lib.ucfvit_quadtree_deserialize_bwd_workspace(2, 8, 8, 1, 1, 0) == -1 and lib.ucfvit_octree_deserialize_bwd_workspace(2, 257, 1, 1, 2) == -1
    assert lib.ucfvit_quadtree_deserialize_bwd_workspace(2, 32, 32, 3, 5, 4) == 0                       # no leaf of 1024 pixels has two slices
    assert lib.ucfvit_quadtree_deserialize_bwd_workspace(2, 32, 33, 3, 5, 4) == 2 * 5 * SLICES * 3 * 16 * 4
    assert lib.ucfvit_octree_deserialize_bwd_workspace(0, 64, 3, 5, 4) == 0
    # B = 0 with null pointers is a no-op
    s = _stream()
    assert lib.ucfvit_quadtree_deserialize_bwd(None, None, None, None, 0, 8, 8, 1, 1, 2, 4, 1, 4, 1, 64, 1, 1, 0, None, s) == 0
    assert lib.ucfvit_octree_deserialize_bwd(None, None, None, None, 0, 8, 1, 1, 2, 8, 1, 8, 1, 512, 1, 1, 0, None, s) == 0
    # the accepted neighbours of the refusals do run; an image of at most 1024 pixels needs no workspace
    assert q() == 0 and o() == 0 and o(w=None) == 0 and q(H=8, W=8, ostr=(64, 1, 1), mode=1, w=None) == 0
    torch.cuda.synchronize()
    assert _guards_ok(buf, FSENT) and (dseq.flatten()[:8] == 16.0).all()                  # the last call: 8 x 8 ones gathered by 2 x 2 tokens


@gpu
def test_ops_refusals():
    ops = _ops()
    from UCF_VIT.dataloaders.transform import Patchify, Patchify_3D
    nd2 = torch.tensor([[[0, 8, 0, 8]]] * 2, dtype=torch.int32, device=DEV)
    nd3 = torch.tensor([[[0, 4, 0, 4, 0, 4]]] * 2, dtype=torch.int32, device=DEV)
    ct = torch.ones(2, dtype=torch.int32, device=DEV)
    d2, d3 = torch.zeros((2, 8, 8, 1), device=DEV), torch.zeros((2, 4, 4, 4, 1), device=DEV)
    s2, s3 = (2, 1, 2, 2, 1), (2, 1, 2, 2, 2, 1)
    with pytest.raises(TypeError):
        ops.quadtree_deserialize_bwd(d2.double(), nd2, ct, s2, 2)
    with pytest.raises(TypeError):
        ops.quadtree_deserialize_bwd(d2[0], nd2, ct, s2, 2)                               # wrong rank
    with pytest.raises(TypeError):
        ops.quadtree_deserialize_bwd(d2, nd3, ct, s2, 2)
    with pytest.raises(TypeError):
        ops.quadtree_deserialize_bwd(d2, nd2, ct, s3, 2)                                  # the shape of a 3-D sequence
    with pytest.raises(TypeError):
        ops.octree_deserialize_bwd(d3, nd3, ct.long(), s3, 2)
    with pytest.raises(ValueError):
        ops.quadtree_deserialize_bwd(d2, nd2, ct, s2, 2, mode="trilinear")
    with pytest.raises(ValueError):
        ops.octree_deserialize_bwd(d3, nd3, ct, s3, 2, mode="bicubic")
    with pytest.raises(ValueError):
        ops.octree_deserialize_bwd(d3[:, :, :, :3].contiguous(), nd3, ct, s3, 2)          # not cubic
    with pytest.raises(ValueError):
        ops.quadtree_deserialize_bwd(d2, nd2[:, :0], ct, s2, 2)                           # sequence lengths disagree
    with pytest.raises(ValueError):
        ops.quadtree_deserialize_bwd(d2, nd2, ct, (2, 1, 2, 2, 3), 2)                     # channels disagree
    with pytest.raises(ValueError):
        ops.quadtree_deserialize_bwd(d2, nd2, ct, s2, 0)
    with pytest.raises(RuntimeError):
        ops.quadtree_deserialize_bwd(d2.cpu(), nd2, ct, s2, 2)
    with pytest.raises(RuntimeError):
        ops.quadtree_deserialize_bwd(d2.transpose(1, 2), nd2, ct, s2, 2)                  # non-dense dout
    like = torch.zeros(1, device=DEV).expand(s3)                                          # shaped like an expanded view: a dense gradient
    assert ops.octree_deserialize_bwd(d3, nd3, ct, like, 2).is_contiguous()
    with pytest.raises(TypeError):
        ops.octree_deserialize_bwd(d3, nd3, ct, like.double(), 2)
    seq = torch.zeros(s2, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match="truncate"):
        Patchify(4, 2, 1).deserialize(seq, nd2, ct, (8, 8), truncate=True)
    with pytest.raises(ValueError):
        Patchify_3D(8, 2, 1).deserialize(torch.zeros(s3, device=DEV, requires_grad=True), nd3, ct, 4, truncate=True)
    out = Patchify(4, 2, 1).deserialize(seq.detach(), nd2, ct, (8, 8), truncate=True)      # without a gradient: the path of before
    assert not out.requires_grad
    with torch.no_grad():
        assert not Patchify(4, 2, 1).deserialize(seq, nd2, ct, (8, 8)).requires_grad


# ============================================================================================== autograd
def _built_tree(dim):
    ops = _ops()
    n, L = (32, 16) if dim == 2 else (16, 8)
    ax = np.arange(n) - n / 2 + 0.5
    r = np.sqrt(sum(np.meshgrid(*([ax] * dim), indexing="ij")[a] ** 2 * (1 + 0.3 * a) for a in range(dim)))
    contour = (np.abs(r - n / 4) < 0.8).astype(np.uint8) * 255
    dom = torch.from_numpy(np.stack([contour, np.roll(contour, 3, axis=-1)])).to(DEV)
    nodes, _, count, _ = ops.quadtree_build(dom, L) if dim == 2 else ops.octree_build(dom, L)
    return nodes, count, n, L


def _interp_loop(dim, seq, nodes, count, n):
    """the per-leaf torch loop under autograd: seq [B, C, L, P] -> [B, C, *img]"""
    F = torch.nn.functional
    B, C, L, P = seq.shape
    p = round(P ** (1.0 / dim))
    out = torch.zeros((B, C) + (n,) * dim, device=seq.device)
    nl, cl = nodes.cpu().numpy(), count.cpu().numpy()
    for b in range(B):
        for s in range(int(cl[b])):
            nd = nl[b, s]
            ext = [int(nd[2 * a + 1] - nd[2 * a]) for a in reversed(range(dim))]
            patch = seq[b, :, s].reshape((1, C) + (p,) * dim)
            leaf = F.interpolate(patch, size=ext, mode="bicubic", align_corners=False) if dim == 2 else \
                F.interpolate(patch, size=ext, mode="trilinear", align_corners=True)
            sl = (b, slice(None)) + tuple(slice(int(nd[2 * a]), int(nd[2 * a + 1])) for a in reversed(range(dim)))
            out[sl] = leaf[0]
    return out


def _weight_error(dim, ext, p):
    """per axis [n, p]: how far two fp32 evaluations of the forward's weights can lie apart: both sides' coefficient roundings and positions"""
    outs = []
    for n in ext:
        x = np.arange(n, dtype=np.float64)
        E = np.zeros((n, p))
        if dim == 2:
            f = (x + 0.5) * p / n - 0.5
            fl = np.floor(f)
            df = U * (2 * (x + 0.5) * p / n + np.abs(f) + 1)
            dw, rb = cubic_bounds(f - fl, -0.75)
            for d in range(4):
                np.add.at(E, (np.arange(n), np.clip(fl.astype(np.int64) - 1 + d, 0, p - 1)), 2 * (rb[d] + dw[d] * df))
        else:
            f = x * (p - 1) / max(n - 1, 1)
            i0 = np.minimum(np.floor(f).astype(np.int64), p - 1)
            for i in (i0, np.minimum(i0 + 1, p - 1)):
                np.add.at(E, (np.arange(n), i), 2 * (3 * U * f + 2 * U))
        outs.append(E)
    return outs


def loop_tolerance(dim, g, nodes, count, n, p, g_other=None):
    """how far the gradient [B, C, L, p^d] of the HIP adjoint and of the per-leaf F.interpolate loop may lie apart for the upstream gradient g
    [B, C, *img]: both sides' summation bounds, (K + 21) U sum |w| |g| each, and the distance of two fp32 evaluations of the weights
    (_weight_error); g_other: the loop's own upstream gradient where it differs from g, whose difference is carried through |w|"""
    nl, cl, gn = nodes.cpu().numpy(), count.cpu().numpy(), g.detach().cpu().numpy().astype(np.float64)
    go = None if g_other is None else g_other.detach().cpu().numpy().astype(np.float64)
    B, C, L = gn.shape[0], gn.shape[1], nl.shape[1]
    tol = np.zeros((B, C, L, p ** dim))
    for b in range(B):
        for s in range(L):
            if not live(nl, cl, b, s, (n,) * dim):
                continue
            nd = nl[b, s].astype(np.int64)
            ext = nd[1::2] - nd[0::2]
            sl = (b, slice(None)) + tuple(slice(nd[2 * a], nd[2 * a + 1]) for a in reversed(range(dim)))
            gl = np.moveaxis(gn[sl], 0, -1)
            _, ab, K = adjoint_leaf(dim, "smooth", gl, ext, p)
            ws = [axis_weights(_rule(dim, "smooth"), ext[a], p)[1] for a in range(dim)]
            es = _weight_error(dim, ext, p)
            t = 2 * (K + CB) * U * ab * (1 + 2.0 ** -10)
            for a in range(dim):
                t = t + _contract([es[i] if i == a else ws[i] for i in range(dim)], np.abs(gl))
            if go is not None:
                t = t + _contract(ws, np.abs(np.moveaxis(go[sl], 0, -1) - gl)) * (1 + 2.0 ** -10)
            tol[b, :, s] = np.moveaxis(t.reshape(p ** dim, C), 1, 0)
    return tol


@gpu
@pytest.mark.parametrize("dim", (2, 3))
def test_autograd_matches_the_raw_op_and_the_interpolate_loop(dim):
    from UCF_VIT._hip import functional as HF
    from UCF_VIT.dataloaders.transform import Patchify, Patchify_3D
    ops = _ops()
    nodes, count, n, L = _built_tree(dim)
    p, C, B = (4, 3, 2) if dim == 2 else (2, 3, 2)
    size = (n, n) if dim == 2 else n
    gen = torch.Generator().manual_seed(7 + dim)
    seq0 = torch.randn((B, C, L, p ** dim), generator=gen).to(DEV)
    g = torch.randn((B, C) + (n,) * dim, generator=gen).to(DEV)
    seq = seq0.clone().requires_grad_(True)
    out = HF.deserialize(seq, nodes, count, size, p, dim, channels_last=False)
    fwd = ops.quadtree_deserialize if dim == 2 else ops.octree_deserialize
    assert out.requires_grad and _bits_equal(out.detach(), fwd(seq0, nodes, count, size, p, channels_last=False))
    out.backward(g)
    bwd = ops.quadtree_deserialize_bwd if dim == 2 else ops.octree_deserialize_bwd
    raw = bwd(g, nodes, count, seq0, p, channels_last=False)
    assert _bits_equal(seq.grad, raw) and seq.grad.stride() == seq0.stride()
    # the module takes the same path when seq requires grad
    seq_m = seq0.clone().requires_grad_(True)
    (Patchify if dim == 2 else Patchify_3D)(L, p, C).deserialize(seq_m, nodes, count, size, channels_last=False).backward(g)
    assert _bits_equal(seq_m.grad, raw)
    # the patch-list layout, channels-last image
    seq_l = seq0.view(B, C, L, p ** dim).movedim(1, 3).reshape((B, L) + (p,) * dim + (C,)).contiguous().requires_grad_(True)
    HF.deserialize(seq_l, nodes, count, size, p, dim).backward(g.movedim(1, -1).contiguous())
    assert _bits_equal(seq_l.grad.reshape(B, L, p ** dim, C).movedim(3, 1), raw)
    # the torch loop
    seq_t = seq0.clone().requires_grad_(True)
    _interp_loop(dim, seq_t, nodes, count, n).backward(g)
    tol = loop_tolerance(dim, g, nodes, count, n, p)
    err = (seq.grad - seq_t.grad).abs().double().cpu().numpy()
    q = np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))
    print(f"RATIO autograd vs interpolate loop {dim}-D: worst err/bound {q.max():.3f}")
    assert (err <= tol).all(), f"worst err/bound {q.max():.3g}"
    assert float(seq_t.grad.abs().max()) > 1e3 * float(tol.max())
    # bf16 in, bf16 gradient out: the cast happens under autograd
    seq_h = seq0.bfloat16().requires_grad_(True)
    HF.deserialize(seq_h, nodes, count, size, p, dim, channels_last=False).backward(g)
    assert seq_h.grad.dtype == torch.bfloat16 and torch.equal(seq_h.grad, raw.bfloat16())
    with pytest.raises(TypeError):
        HF.DeserializeFn.apply(seq0.bfloat16(), nodes, count, size, p, dim, "nearest", False)
