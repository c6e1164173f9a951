"""The DDPM kernels on the MI355X, element by element against float64 (tests/diffusion_ref.py), each with an exact tier: ucfvit_ddpm_q_sample,
ucfvit_time_tokens_fwd / _bwd, ucfvit_relu_dropout / _bwd, ucfvit_ddpm_step.

Roundoff bounds, u = 2^-24 (fp32 unit roundoff), every product and sum of the kernels being rounded on its own (no fma contraction):
  q_sample   fl(fl(a x) + fl(b e)): two products and one sum, |err| <= (2u + u^2)(|a x| + |b e|) < 3u (|a x| + |b e|).
  time tokens fl(fl(p + pos) + temb): two sums, |err| < 3u (|p| + |pos| + |temb|); a bf16 result adds half an ulp of the output.
  dtemb      a sum of N terms in any fixed order: |err| <= gamma_{N-1} sum|dout| <= gamma_N sum|dout|, gamma_N = N u / (1 - N u).
  relu_dropout fl(f x): one product, |err| <= u |f x| < 2u |f x|; exact for f = 2 (p = 0.5) and without a factor (p = 0).
  ddpm_step  fl(fl(c1 fl(x - fl(c2 e))) + fl(sigma z)): five roundings, each term passes at most four of them:
             |err| < 4u (|c1| (|x| + |c2 e|) + |sigma z|) to first order; the u^2 terms are below 1e-7 of that.
"""
import numpy as np
import pytest
import torch

import diffusion_ref as DRF

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
DTYPES = [torch.float32, torch.bfloat16]


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.Generator(np.random.PCG64(seed)).standard_normal(tuple(shape)) * scale).astype(np.float32))


def ints(shape, seed, lo=-8, hi=9):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).integers(lo, hi, tuple(shape)).astype(np.float32))


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def half_ulp(v, dtype):
    """half an ulp of the output format at |v| (0 for fp32: its rounding is inside the u-bounds)"""
    if dtype == torch.float32:
        return np.zeros_like(v)
    _, e = np.frexp(np.abs(v))                        # |v| in [2^(e-1), 2^e): ulp = 2^(e-1-7)
    return np.where(v == 0, 0.0, np.ldexp(1.0, e - 1 - 8))


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.view(view), b.view(view))


# ---------------------------------------------------------------------------------------------------------------- q_sample
@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (3, 3, 8, 8)])          # 105 elements per sample: element path; 192: 16-byte path
def test_q_sample(shape):
    from UCF_VIT._hip import ops
    T = 10
    x0, eps = rnd(shape, 1), rnd(shape, 2)
    g = np.random.Generator(np.random.PCG64(3))
    sa, sb = torch.from_numpy(g.uniform(0.05, 1.0, T).astype(np.float32)), torch.from_numpy(g.uniform(0.05, 1.0, T).astype(np.float32))
    for t in ([0, T - 1, 4], [T + 5, -3, 4]):                            # the second: out of range on both sides, clamped to T-1 and 0
        tt = torch.tensor(t, dtype=torch.int64)
        out = ops.ddpm_q_sample(x0.to(DEV), eps.to(DEV), tt.to(DEV), sa.to(DEV), sb.to(DEV))
        ax, be = DRF.q_sample(x0.numpy(), eps.numpy(), t, sa.numpy(), sb.numpy())
        err = np.abs(f64(out) - (ax + be))
        bound = 3 * U * (np.abs(ax) + np.abs(be))
        print(f"q_sample {shape} t={t}: worst err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert (err <= bound).all()
        clamped = ops.ddpm_q_sample(x0.to(DEV), eps.to(DEV), tt.clamp(0, T - 1).to(DEV), sa.to(DEV), sb.to(DEV))
        assert same_bits(out, clamped)
        xin = x0.to(DEV).clone()
        assert ops.ddpm_q_sample(xin, eps.to(DEV), tt.to(DEV), sa.to(DEV), sb.to(DEV), out=xin) is xin and same_bits(xin, out)
    # exact tier: tables of powers of two, integer data
    pa = torch.tensor([2.0 ** -(k % 5) for k in range(T)])
    pb = torch.tensor([2.0 ** -((k + 2) % 4) for k in range(T)])
    xi, ei, tt = ints(shape, 4), ints(shape, 5), torch.tensor([0, T - 1, 4])
    out = ops.ddpm_q_sample(xi.to(DEV), ei.to(DEV), tt.to(DEV), pa.to(DEV), pb.to(DEV))
    ax, be = DRF.q_sample(xi.numpy(), ei.numpy(), tt.numpy(), pa.numpy(), pb.numpy())
    assert same_bits(out, torch.from_numpy((ax + be).astype(np.float32)))


# ---------------------------------------------------------------------------------------------------------------- time tokens
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,D", [(5, 24), (16, 64)])
@pytest.mark.parametrize("has_cls", [0, 1])
@pytest.mark.parametrize("has_pos", [0, 1])
def test_time_tokens_fwd(dtype, L, D, has_cls, has_pos):
    from UCF_VIT._hip import ops
    B, N = 3, L + has_cls
    patches, temb = rnd((B, L, D), 11).to(dtype), rnd((B, D), 12).to(dtype)
    cls = rnd((D,), 13).to(dtype) if has_cls else None
    pos = rnd((N, D), 14).to(dtype) if has_pos else None
    dev = lambda t: None if t is None else t.to(DEV)
    out = ops.time_tokens_fwd(dev(patches).view(B * L, D), dev(cls), dev(pos), dev(temb), B, L, D)
    assert out.shape == (B, N, D) and out.dtype == dtype
    a, p, te = DRF.time_tokens_terms(f64(patches), None if cls is None else f64(cls), None if pos is None else f64(pos), f64(temb))
    if dtype == torch.float32:                                           # bit for bit: the same two fp32 adds on the host
        a32 = torch.from_numpy(a.astype(np.float32))
        want = ((a32 + torch.from_numpy(p.astype(np.float32))) if has_pos else a32) + torch.from_numpy(te.astype(np.float32))
        assert same_bits(out, want)
    exact = a + p + te
    err = np.abs(f64(out) - exact)
    bound = half_ulp(np.maximum(np.abs(exact), np.abs(f64(out))), dtype) + 3 * U * (np.abs(a) + np.abs(p) + np.abs(te))
    assert (err <= bound).all()
    # a zero time row: the token kernel's bits
    zero = ops.time_tokens_fwd(dev(patches).view(B * L, D), dev(cls), dev(pos), torch.zeros(B, D, dtype=dtype, device=DEV), B, L, D)
    assert same_bits(zero, ops.tokens_fwd(dev(patches).view(B * L, D), dev(cls), dev(pos), B, L, D))


def _time_tokens_bwd_case(dtype, B, L, D, has_cls, seed, integer=False):
    from UCF_VIT._hip import ops
    N = L + has_cls
    dout = (ints((B, N, D), seed, -4, 5) if integer else rnd((B, N, D), seed)).to(dtype)
    d = dout.to(DEV)
    for accumulate in (False, True):
        init_pos, init_cls = rnd((N, D), seed + 1).to(DEV), rnd((D,), seed + 2).to(DEV)
        kw = lambda: dict(dpos=init_pos.clone(), dcls=init_cls.clone() if has_cls else None, accumulate=accumulate)
        dp, dpos, dcls, dtemb = ops.time_tokens_bwd(d, B, L, D, bool(has_cls), True, **kw())
        rp, rpos, rcls = ops.tokens_bwd(d, B, L, D, bool(has_cls), True, **kw())
        assert same_bits(dp.view(B, L, D), dout[:, has_cls:]) and same_bits(dp, rp)
        assert same_bits(dpos, rpos) and (not has_cls or same_bits(dcls, rcls))
        _, pos64, cls64, temb64 = DRF.time_tokens_bwd(f64(dout), has_cls)
        base = f64(init_pos) if accumulate else 0.0
        gam = (B + 1) * U / (1 - (B + 1) * U)
        assert (np.abs(f64(dpos) - (base + pos64)) <= gam * (np.abs(base) + np.abs(f64(dout)).sum(0))).all()
        assert dtemb.dtype == torch.float32 and dtemb.shape == (B, D)
        if integer:
            assert same_bits(dtemb, torch.from_numpy(temb64.astype(np.float32)))
        gam = N * U / (1 - N * U)
        err, bound = np.abs(f64(dtemb) - temb64), gam * np.abs(f64(dout)).sum(1)
        assert (err <= bound).all()
        again = ops.time_tokens_bwd(d, B, L, D, bool(has_cls), True, **kw())
        assert same_bits(again[3], dtemb) and same_bits(again[1], dpos) and same_bits(again[0], dp)
    # no position gradient wanted, no patch gradient wanted: the other results do not change
    dp2, dpos2, _, dtemb2 = ops.time_tokens_bwd(d, B, L, D, bool(has_cls), False, want_patches=False)
    assert dp2 is None and dpos2 is None and same_bits(dtemb2, dtemb)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,D", [(5, 24), (16, 64)])
@pytest.mark.parametrize("has_cls", [0, 1])
def test_time_tokens_bwd(dtype, L, D, has_cls):
    _time_tokens_bwd_case(dtype, 3, L, D, has_cls, 21)
    _time_tokens_bwd_case(dtype, 3, L, D, has_cls, 24, integer=True)


def test_time_tokens_bwd_folds_many_row_chunks():
    """N = 197 rows of D = 1024: 25 row chunks, several workgroups"""
    _time_tokens_bwd_case(torch.bfloat16, 2, 196, 1024, 1, 31)
    _time_tokens_bwd_case(torch.float32, 2, 196, 1024, 1, 34, integer=True)


# ---------------------------------------------------------------------------------------------------------------- relu + dropout
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [24, 64, 7])                               # 7: the element path
@pytest.mark.parametrize("p", [0.0, 0.5, 0.1])
def test_relu_dropout(dtype, D, p):
    from UCF_VIT._hip import ops
    rows, seed = 5, 0x1234_5678_9ABC_DEF1
    x = rnd((rows, D), 41)
    x[0, 0], x[0, 1], x[1, 2] = 0.0, -0.0, 0.0
    keep_ref, f, _ = DRF.relu_dropout(x.numpy(), p, seed)
    dropped = np.argwhere(~keep_ref)
    assert p == 0 or len(dropped) >= 1
    for (r, c), poison in zip(dropped, (float("nan"), float("inf"))):    # under dropped elements: must not pass
        x[r, c] = poison
    x = x.to(dtype)
    xs = np.nan_to_num(f64(x), nan=-1.0, posinf=1.0)                     # the two poisoned elements are dropped: any finite stand-in
    active = keep_ref & (xs > 0)
    dy = rnd((rows, D), 42)
    for (r, c), poison in zip(np.argwhere(~active), (float("nan"), float("inf"), float("-inf"))):
        dy[r, c] = poison                                                # the backward's selects: under a dropped or inactive element
    dy = dy.to(dtype)
    y = ops.relu_dropout(x.to(DEV), p, seed)
    dx = ops.relu_dropout_bwd(x.to(DEV), dy.to(DEV), p, seed)
    dys = np.nan_to_num(f64(dy), nan=1.0, posinf=1.0, neginf=-1.0)       # they sit where nothing passes: any finite stand-in
    for got, src, name in ((y, xs, "fwd"), (dx, dys, "bwd")):
        g = f64(got)
        assert np.isfinite(g).all(), name
        assert ((g != 0) == (active & (src != 0))).all(), name         # the mask of dropout_ref, bit for bit, and the ReLU gate
        want = np.where(active, f * src, 0.0)
        if p in (0.0, 0.5):                                              # f = 1 (no product) or 2: exact in either format
            assert (g == want).all(), name
            assert not np.signbit(g[~active]).any(), name               # +0 where nothing passes
        else:
            assert (np.abs(g - want) <= half_ulp(np.maximum(np.abs(want), np.abs(g)), dtype) + 2 * U * np.abs(want)).all(), name
    xin = x.to(DEV).clone()
    assert ops.relu_dropout(xin, p, seed, out=xin) is xin and same_bits(xin, y)
    din = dy.to(DEV).clone()
    assert ops.relu_dropout_bwd(x.to(DEV), din, p, seed, out=din) is din and same_bits(din, dx)
    if p > 0:
        other = ops.relu_dropout(x.to(DEV), p, seed + 1)
        assert not same_bits(other, y)


# ---------------------------------------------------------------------------------------------------------------- reverse step
STEP_SHAPES = [((2, 3, 12, 20), 4), ((2, 1, 8, 8), 2), ((2, 3, 32, 32), 16), ((2, 2, 8, 12, 4), 4)]


def _pred_shape(shape, p):
    nd = len(shape) - 2
    L = int(np.prod([s // p for s in shape[2:]]))
    return (shape[0], L, shape[1] * p ** nd)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,p", STEP_SHAPES)
def test_ddpm_step(dtype, shape, p):
    from UCF_VIT._hip import ops
    ps = _pred_shape(shape, p)
    C, dims = shape[1], shape[2:]
    # index tier: every element of pred lands on its pixel
    idx = (torch.arange(int(np.prod(ps))) % 251 - 125).float().reshape(ps).to(dtype)
    out = ops.ddpm_step(torch.zeros(shape, device=DEV), idx.to(DEV), None, p, 1.0, 1.0, 0.0)
    want = -DRF.unpatchify(f64(idx), C, dims, p)
    assert out.dtype == torch.float32 and (f64(out) == want).all()
    # arithmetic tier: power-of-two coefficients, integer data
    x, z, pr = ints(shape, 51), ints(shape, 52), ints(ps, 53).to(dtype)
    out = ops.ddpm_step(x.to(DEV), pr.to(DEV), z.to(DEV), p, 2.0, 0.5, 0.25)
    want, _ = DRF.ddpm_step(x.numpy(), f64(pr), z.numpy(), p, 2.0, 0.5, 0.25)
    assert (f64(out) == want).all()
    # general
    x, z, pr = rnd(shape, 54), rnd(shape, 55), rnd(ps, 56).to(dtype)
    c1, c2, sigma = 1.0101525, 0.0870388, 0.1414213
    for zz, sg in ((z, sigma), (None, 0.0)):
        out = ops.ddpm_step(x.to(DEV), pr.to(DEV), None if zz is None else zz.to(DEV), p, c1, c2, sg)
        want, terms = DRF.ddpm_step(x.numpy(), f64(pr), None if zz is None else zz.numpy(), p, c1, c2, sg)
        err = np.abs(f64(out) - want)
        print(f"ddpm_step {shape} p={p} {dtype}: worst err/bound {np.max(err / (4 * U * terms)):.3f}")
        assert (err <= 4 * U * terms).all()
        xin = x.to(DEV).clone()
        assert ops.ddpm_step(xin, pr.to(DEV), None if zz is None else zz.to(DEV), p, c1, c2, sg, out=xin) is xin and same_bits(xin, out)
