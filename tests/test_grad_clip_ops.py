"""ucfvit_grad_sqnorm / ucfvit_grad_clip_coef / ucfvit_adamw_clipped on the MI355X (csrc/grad_clip.hip).

Real-valued tier: NORM against the float64 norm of the fp32 products fl(g * k) within grad_clip_ref.norm_bound, which is derived there for
the structure built (squares accumulated in double from the first add: the half ulp of the final rounding to fp32 plus (n + partials) / 2
double roundings), not measured; COEF against the float64 coefficient within coef_bound where it is below 1.
Exact tier: COEF is 1.0f when the threshold is not exceeded; 0 for an Inf norm and NaN for a NaN norm; FOUND_INF is what
ucfvit_grad_nonfinite sets; two runs give the same bits; with COEF = 1 ucfvit_adamw_clipped leaves the bits of the entry point without
clipping in p, m, v, shadow and ema, and with COEF = c < 1 those of that entry point called with grad_scale = fl32(gscale * c).

Sizes: tail only (1, 3), one 16-byte vector, vector + tail (5, 7, 1027 and vector + 1, + 3 for bf16, whose vector holds 8), and one full pass of
the capped grid with its unroll plus 1027 (GC_MAX_GRID x GC_BLOCK x GC_UNROLL vectors, read from the source), where the unrolled loop, the
remainder loop and the tail all run."""
import math
import os
import re

import numpy as np
import pytest
import torch

import grad_clip_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
MULT = 0.37                       # not a power of two: the product g * k rounds
SCALE = 3.0                       # nor is 1 / 3


def _consts():
    txt = open(os.path.join(ROOT, "ucf-vit_amd", "csrc", "grad_clip.hip")).read()
    return {k: int(re.search(rf"constexpr int {k} = (\d+);", txt).group(1)) for k in ("GC_BLOCK", "GC_MAX_GRID", "GC_UNROLL")}


def _epv(dtype):
    return 4 if dtype == torch.float32 else 8


def _sizes(dtype):
    c, epv = _consts(), _epv(dtype)
    return sorted({1, 3, epv, 5, 7, epv + 1, epv + 3, 1027, c["GC_MAX_GRID"] * c["GC_BLOCK"] * c["GC_UNROLL"] * epv + 1027})


def _ops():
    from UCF_VIT._hip import ops
    return ops


def _lib():
    from UCF_VIT._hip import lib
    return lib


def _grad(n, dtype, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.standard_normal(n).astype(np.float32) * np.exp2(g.integers(-6, 7, n)).astype(np.float32) * np.float32(scale)
    return torch.from_numpy(x).to(DEV).to(dtype)


def _np(t):
    return t.float().cpu().numpy()


def _gs_state(scale=SCALE, found_inf=0.0, applied=0.0):
    s = torch.zeros(16, dtype=torch.float32)
    s[0], s[1], s[2], s[4] = scale, float(np.float32(1.0) / np.float32(scale)), found_inf, applied
    return s.to(DEV)


def _gc_state(max_norm, coef=0.0):
    s = torch.zeros(8, dtype=torch.float32)
    s[0], s[1], s[2], s[3:] = max_norm, -7.0, coef, 5.0                 # stale NORM / spare values must not matter
    return s.to(DEV)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _norm_coef(segs, max_norm, gs=None, mult=MULT, ws=None):
    """the optimizer's sequence over a list of segments -> (NORM, COEF, number of partials, workspace)"""
    ops, lib = _ops(), _lib()
    counts = [ops.grad_sqnorm_partials(g.numel(), g.dtype) for g in segs]
    total = sum(counts)
    if ws is None:
        ws = torch.full((total + 5,), float("nan"), dtype=torch.float64, device=DEV)
    gc = _gc_state(max_norm)
    off = 0
    for g, c in zip(segs, counts):
        if c:
            assert ops.grad_sqnorm(g, ws[off:off + c], mult, gs) == c
        off += c
    ops.grad_clip_coef(ws, total, gc)
    out = gc.cpu()
    assert out[lib.GC_MAX_NORM].item() == float(np.float32(max_norm)) and (out[3:] == 5.0).all()
    return out[lib.GC_NORM].item(), out[lib.GC_COEF].item(), total, ws


# ============================================================================================== 1. the norm
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_norm_against_float64(dtype, scaled):
    lib = _lib()
    worst = 0.0
    for n in _sizes(dtype):
        g = _grad(n, dtype, 1000 + n % 997)
        gs = _gs_state() if scaled else None
        inv = float(np.float32(1.0) / np.float32(SCALE)) if scaled else None
        ref = R.norm64([_np(g)], MULT, inv)
        norm, coef, count, ws = _norm_coef([g], 0.25 * ref, gs)
        assert count == min((n + _epv(dtype) * 256 - 1) // (_epv(dtype) * 256), _consts()["GC_MAX_GRID"])
        assert bool(torch.isnan(ws[count:]).all()) and bool(torch.isfinite(ws[:count]).all())        # exactly `count` partials were written
        bound = R.norm_bound(ref, n, count)
        worst = max(worst, abs(norm - ref) / bound)
        assert abs(norm - ref) <= bound, (n, norm, ref)
        # wrong references the bound must reject: a norm two ulps off, and the one without the scaler's factor
        assert abs(norm - ref * (1 + 4 * R.U32)) > bound
        if scaled:
            assert abs(norm - R.norm64([_np(g)], MULT)) > bound
        cref = R.coef64(ref, 0.25 * ref)
        assert abs(coef - cref) <= R.coef_bound(cref, n, count), (n, coef, cref)
        if scaled:
            assert gs[lib.GS_FOUND_INF].item() == 0.0
    print(f"{dtype} scaled={scaled}: worst NORM err / bound {worst:.3f}")


def test_several_segments_share_one_workspace_and_stale_partials_are_not_read():
    """three segments of mixed dtype with an empty one among them, in a NaN-poisoned workspace that a larger layout used before: the
    second fold must read exactly its own `count` partials (the stale ones behind them are finite, the rest NaN)"""
    ops = _ops()
    ws = torch.full((64,), float("nan"), dtype=torch.float64, device=DEV)
    big = [_grad(5000, torch.float32, 1), _grad(3000, torch.float32, 2), _grad(2049, torch.bfloat16, 3)]
    ref = R.norm64([_np(g) for g in big], MULT)
    norm, _, count, _ = _norm_coef(big, 1.0, ws=ws)
    assert count == 5 + 3 + 2 and abs(norm - ref) <= R.norm_bound(ref, 10049, count)
    stale = ws.clone()
    small = [_grad(1027, torch.float32, 4), torch.empty(0, dtype=torch.float32, device=DEV), _grad(7, torch.bfloat16, 5)]
    assert [ops.grad_sqnorm_partials(g.numel(), g.dtype) for g in small] == [2, 0, 1]
    ref = R.norm64([_np(g) for g in small], MULT)
    norm, coef, count, _ = _norm_coef(small, 0.5 * ref, ws=ws)
    assert count == 3 and abs(norm - ref) <= R.norm_bound(ref, 1034, count), (norm, ref)
    assert _same(ws[3:], stale[3:]) and bool(torch.isfinite(ws[:10]).all()) and bool(torch.isnan(ws[10:]).all())
    assert abs(coef - R.coef64(ref, 0.5 * ref)) <= R.coef_bound(0.5, 1034, count)
    # no segment at all: norm 0, coefficient 1
    assert _norm_coef([], 1.0, ws=ws)[:3] == (0.0, 1.0, 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_give_the_same_bits(dtype):
    n = _sizes(dtype)[-1]
    g = _grad(n, dtype, 77)
    runs = []
    for _ in range(2):
        gs = _gs_state()
        norm, coef, count, ws = _norm_coef([g, g[:1027]], 1.0, gs)
        runs.append((np.float32(norm).tobytes(), np.float32(coef).tobytes(), ws[:count].clone()))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and _same(runs[0][2], runs[1][2])


# ============================================================================================== 2. the coefficient
def test_coefficient_is_exactly_one_at_or_below_the_threshold():
    """far below: exactly 1.0f.  At the threshold clip_grad_norm_'s formula gives max / (norm + 1e-6), which is 1.0f exactly when 1e-6 is
    below half an ulp of the norm, i.e. from 32 upwards: the gradients are drawn with a norm of about 1000.  A threshold 2^-20 below the norm
    clips (16 ulps of the quotient: no rounding of the division can hide it)."""
    g = _grad(1027, torch.float32, 5, scale=4.0)
    norm, coef, _, _ = _norm_coef([g], 1e6)
    assert coef == 1.0 and norm > 32.0
    assert _norm_coef([g], norm)[:2] == (norm, 1.0)
    below = float(np.float32(norm * (1.0 - 2.0 ** -20)))
    n2, c2, _, _ = _norm_coef([g], below)
    assert n2 == norm and c2 < 1.0 and abs(c2 - below / norm) <= 3 * R.U32
    # small norms: still 1.0f whenever max > norm + 1e-6
    g = _grad(7, torch.float32, 6, scale=1e-3)
    norm, coef, _, _ = _norm_coef([g], 1.0)
    assert 0.0 < norm < 0.1 and coef == 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_all_zero_gradients(dtype):
    for n in (1, 1027):
        g = torch.zeros(n, dtype=dtype, device=DEV)
        g[n // 2] = -0.0
        assert _norm_coef([g], 1.0)[:2] == (0.0, 1.0)
        assert _norm_coef([g], 1.0, _gs_state())[:2] == (0.0, 1.0)
    norm, coef, _, _ = _norm_coef([g], 1e-7)                   # a threshold below 1e-6 clips even a zero gradient, as torch's formula does
    assert norm == 0.0 and abs(coef - 0.1) <= 0.1 * 4 * R.U32


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_non_finite_gradients_propagate(dtype, scaled):
    """Inf anywhere: NORM = Inf, COEF = 0; NaN anywhere: both NaN (torch's clamp keeps a NaN); first element, the middle (the second
    workgroup), the scalar tail; and in every load of the unrolled loop at the large size"""
    lib = _lib()
    for n in (1027, _sizes(dtype)[-1]):
        g = _grad(n, dtype, 9)
        epv = _epv(dtype)
        spots = [0, n // 2, n - 1]
        if n > 1027:
            stride = _consts()["GC_MAX_GRID"] * _consts()["GC_BLOCK"] * epv
            spots = [u * stride + 7 * epv + u for u in range(_consts()["GC_UNROLL"])] + [n - 1029, n - 1]
        for i in spots:
            keep = g[i].clone()
            for bad in (float("inf"), float("-inf"), float("nan")):
                g[i] = bad
                gs = _gs_state() if scaled else None
                norm, coef, _, _ = _norm_coef([g], 1.0, gs)
                if math.isnan(bad):
                    assert math.isnan(norm) and math.isnan(coef), (n, i)
                else:
                    assert norm == float("inf") and coef == 0.0, (n, i, bad)
                if scaled:
                    assert gs[lib.GS_FOUND_INF].item() == 1.0, (n, i, bad)
            g[i] = keep
        assert math.isfinite(_norm_coef([g], 1.0)[0])


# ============================================================================================== 3. the flag
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_flag_equals_grad_nonfinite(dtype):
    ops, lib = _ops(), _lib()
    ws = torch.empty(2048, dtype=torch.float64, device=DEV)

    def flags(g, mult, scale, preset=0.0):
        a, b = _gs_state(scale, preset), _gs_state(scale, preset)
        ops.grad_nonfinite(g, a, mult)
        ops.grad_sqnorm(g, ws, mult, b)
        assert _same(a, b)                                               # nothing else of the state moves
        return a[lib.GS_FOUND_INF].item(), b[lib.GS_FOUND_INF].item()

    for n in (1, 3, 1027, _sizes(dtype)[-1]):
        g = _grad(n, dtype, 21)
        assert flags(g, 1.0, 1.0) == (0.0, 0.0)
        assert flags(g, 1.0, 1.0, preset=1.0) == (1.0, 1.0), "the pass cleared the flag"
        i = n // 2
        for bad in (float("inf"), float("nan")):
            keep = g[i].clone()
            g[i] = bad
            assert flags(g, 1.0, 1.0) == (1.0, 1.0)
            g[i] = keep
        g[i] = 1e30
        assert flags(g, 1.0, 1.0) == (0.0, 0.0), "1e30 itself is finite"
        assert flags(g, 1e10, 1.0) == (1.0, 1.0), "1e30 * 1e10 overflows"
        assert flags(g, 1.0, 2.0 ** -40) == (1.0, 1.0), "1e30 * 2^40 overflows"
        assert flags(g, 1e-10, 2.0 ** -40) == (0.0, 0.0), "1e30 * 1e-10 * 2^40 is finite"
        g[i] = torch.finfo(dtype).max
        assert flags(g, 1.0, 1.0) == (0.0, 0.0), "the largest finite value, multiplier 1"
        # ... and its square, which is not an fp32 number, does not overflow the double sum: the norm is finite
        ref = R.norm64([_np(g)], 1.0, 1.0)
        norm = _norm_coef([g], 1.0, _gs_state(1.0), mult=1.0)[0]
        assert math.isfinite(norm) and abs(norm - ref) <= R.norm_bound(ref, n, 1024)
    # an Inf stays in the partial of the workgroup that read it
    g = _grad(4099, dtype, 22)
    g[5] = float("inf")
    assert ops.grad_sqnorm(g, ws, 1.0, None) >= 3 and ws[0].item() == float("inf") and math.isfinite(ws[1].item())


# ============================================================================================== 4. AdamW with the coefficient
ADAMW_SIZES = [1, 3, 4, 5, 7, 1027, 2 ** 21 + 1027]          # test_ema_ops.py's: tails, one vector, and past one pass of AdamW's 2048 x 256 x 4 grid
HP = (1e-3, 0.9, 0.95, 1e-8, 0.01)                           # lr, beta1, beta2, eps, weight decay
STEP = 3
GSCALE = 0.37
RATE = 0.01


def _inputs(n, gdtype, shadow, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    f = lambda a: torch.from_numpy(a.astype(np.float32)).to(DEV)           # noqa: E731
    d = dict(p=f(g.standard_normal(n)), g=f(g.standard_normal(n) * 0.1).to(gdtype), m=f(g.standard_normal(n) * 0.01),
             v=f(g.uniform(0.0, 0.01, n)), sh=torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV) if shadow else None,
             ema=f(g.standard_normal(n)))
    d["p"][::11] = 0.0
    return d


def _clone(d):
    return {k: None if v is None else v.clone() for k, v in d.items()}


def _sibling(d, ema, scaled, gscale, found_inf=0.0):
    """the entry point without clipping, on d in place"""
    ops = _ops()
    a = (d["p"], d["g"], d["m"], d["v"], d["sh"])
    st = _gs_state(4.0, found_inf, float(STEP - 1))                       # 4.0 / 0.25: test_ema_ops.py's state
    if not scaled:
        ops.adamw_ema(*a, d["ema"], *HP, STEP, RATE, gscale) if ema else ops.adamw(*a, *HP, STEP, gscale)
    elif ema:
        ops.adamw_scaled_ema(*a, d["ema"], *HP, st, RATE, gscale)
    else:
        ops.adamw_scaled(*a, *HP, st, gscale)


def _clipped(d, ema, scaled, gc, found_inf=0.0):
    _ops().clipped_adamw(d["p"], d["g"], d["m"], d["v"], d["sh"], d["ema"] if ema else None, *HP, STEP, RATE if ema else None, gc,
                         _gs_state(4.0, found_inf, float(STEP - 1)) if scaled else None, GSCALE)


def _assert_same(a, b, what):
    for k in ("p", "m", "v", "sh", "ema"):
        if a[k] is not None:
            assert _same(a[k], b[k]), (what, k)


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16])
def test_adamw_clipped_exact_tier(gdtype, ema, scaled):
    lib = _lib()
    for n in ADAMW_SIZES:
        d0 = _inputs(n, gdtype, n % 2 == 1, 500 + n % 97)
        # COEF = 1.0f: the bits of the entry point without clipping
        base, got = _clone(d0), _clone(d0)
        _sibling(base, ema, scaled, GSCALE)
        assert not _same(base["p"], d0["p"]) and (_same(base["ema"], d0["ema"]) != ema)
        _clipped(got, ema, scaled, _gc_state(1.0, coef=1.0))
        _assert_same(base, got, f"coef 1 n={n}")
        # COEF = c < 1 as the device wrote it: the entry point without clipping at grad_scale = fl32(gscale * c)
        gs = _gs_state(4.0, 0.0, float(STEP - 1)) if scaled else None
        ws = torch.empty(2048, dtype=torch.float64, device=DEV)
        gc = _gc_state(1.0)
        cnt = _ops().grad_sqnorm(d0["g"], ws, GSCALE, gs)
        norm = R.norm64([_np(d0["g"])], GSCALE, 0.25 if scaled else None)
        gc[lib.GC_MAX_NORM] = 0.3 * norm
        _ops().grad_clip_coef(ws, cnt, gc)
        c = gc[lib.GC_COEF].item()
        assert 0.29 < c < 0.31
        base, got = _clone(d0), _clone(d0)
        _sibling(base, ema, scaled, float(np.float32(GSCALE) * np.float32(c)))
        _clipped(got, ema, scaled, gc)
        _assert_same(base, got, f"coef {c} n={n}")
        unclipped = _clone(d0)
        _sibling(unclipped, ema, scaled, GSCALE)
        assert not _same(unclipped["m"], got["m"])                         # the coefficient did reach the gradients
        # the check fired: nothing moves
        if scaled:
            got = _clone(d0)
            _clipped(got, ema, scaled, gc, found_inf=1.0)
            _assert_same(d0, got, f"skipped n={n}")


def test_refusals_return_before_any_launch():
    from UCF_VIT._hip.lib import HipLibraryError
    ops = _ops()
    d0 = _inputs(64, torch.float32, True, 7)
    got = _clone(d0)
    gc = _gc_state(1.0, 1.0)
    pad = torch.zeros(65, device=DEV)
    a = (got["p"], got["g"], got["m"], got["v"], got["sh"])
    ws = torch.zeros(8, dtype=torch.float64, device=DEV)
    with pytest.raises(HipLibraryError, match="ema_rate"):
        ops.clipped_adamw(*a, got["ema"], *HP, STEP, 1.5, gc)
    with pytest.raises(HipLibraryError, match="aligned"):
        ops.clipped_adamw(*a, pad[1:], *HP, STEP, 0.1, gc)
    with pytest.raises(ValueError, match="clip state"):
        ops.clipped_adamw(*a, None, *HP, STEP, None, gc[:4])
    with pytest.raises(ValueError, match="loss-scaler state"):
        ops.clipped_adamw(*a, None, *HP, STEP, None, gc, gc)
    with pytest.raises(ValueError, match="partials"):
        ops.grad_sqnorm(_grad(5000, torch.float32, 1), ws[:4])
    with pytest.raises(ValueError, match="partials"):
        ops.grad_sqnorm(got["g"], ws.float())
    with pytest.raises(ValueError, match="partials"):
        ops.grad_clip_coef(ws, 9, gc)
    with pytest.raises(HipLibraryError, match="16-byte aligned"):
        ops.grad_sqnorm(pad[1:], ws)
    with pytest.raises(TypeError):
        ops.grad_sqnorm_partials(8, torch.float16)
    torch.cuda.synchronize()
    _assert_same(d0, got, "refused")
    assert not ws.any() and not pad.any() and gc[2].item() == 1.0
