"""The two kernels of csrc/qk_norm.hip per element against float64, in the manner of the LayerNorm cases of tests/test_rowwise_ops.py.

Bit-for-bit tier: the V third of qkv and of dqkv (filled with NaN / Inf patterns) is not touched, saved_qk holds the input bits, two calls
give the same bits, and the in-place result does not depend on whether saved_qk is asked for.

Bounded tier: normal operands; the reference sees the same rounded inputs and runs in float64 on the device.  A segment has dh elements,
W = 16 bytes of them per lane, summed along a chain of W terms and then log2(dh / W) butterfly levels: a sum of depth h = W + log2(dh / W)
is off by at most h * 2^-24 * sum|terms|.  The bounds are those of the LayerNorm test with that h; a bf16 output adds 2^-8 of its value.
The sums over rows and heads follow the kernel's order: rows per wave, the 4 waves pairwise, the heads and column tiles in ascending
order, then ucfvit_reduce_rows over the row chunks.  Each bound is shown to reject plausibly wrong references: statistics over the whole
row instead of per head, gamma_q applied to K, the unbiased variance, eps dropped, a missing last row chunk in the sums.

The coarse-grid case the exact tier could hold (every segment is +p and -p in equal numbers for a power of two p, eps = 0: mean 0 and
variance p^2 are exact) is NOT exact in this kernel: rstd comes from rsqrtf, which is within 2 ulp but not correctly rounded.  It is
checked in the bounded tier, with the bound that follows from that: 3 * 2^-24 relative on the product, plus the output rounding."""
import math

import pytest
import torch

import qk_norm_ref as QR

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
UB = 2.0 ** -8
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def _ops():
    from UCF_VIT._hip import ops
    return ops


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=_gen(seed), device=DEV, dtype=torch.float32) * scale


def _quarters(shape, seed, dtype, k=8):
    return (torch.randint(-k, k + 1, shape, generator=_gen(seed), device=DEV).float() * 0.25).to(dtype)


def _ou(dtype):
    return UB if dtype == torch.bfloat16 else U


def _within(got, ref, tol):
    return bool(((got.double() - ref).abs() <= tol).all())


def _check(got, ref, tol, wrong, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, "
                                 f"worst excess {float((err - tol)[bad].max()):.3e}")
    for i, w in enumerate(wrong):
        assert not _within(got, w, tol), f"{what}: the bound does not reject wrong reference {i}"


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _depth(dh, dtype):
    W = 8 if dtype == torch.bfloat16 else 4
    return W, W + int(math.log2(dh // W))


def _inputs(rows, H, dh, dtype, seed):
    """qkv [rows, 3 H dh]: per segment a scale in [1, 3] (every fifth segment 1e-3: variance 1e-6, where eps decides) and a mean offset
    of order 1, different per head; the V third carries NaN / Inf / finite patterns that must come back bit for bit"""
    x = _randn((rows, 3, H, dh), seed)
    sc = 1.0 + 2.0 * torch.rand((rows, 3, H, 1), generator=_gen(seed + 1), device=DEV)
    small = (torch.arange(rows * 3 * H, device=DEV).view(rows, 3, H, 1) % 5) == 1
    sc = torch.where(small, torch.full_like(sc, 1e-3), sc)
    off = torch.randn((rows, 3, H, 1), generator=_gen(seed + 2), device=DEV)
    x = (x * sc + torch.where(small, torch.zeros_like(off), off)).to(dtype)
    v = x[:, 2].clone().reshape(-1)
    v[0::3] = float("nan")
    v[1::3] = float("inf")
    v[4::6] = float("-inf")
    x[:, 2] = v.view(rows, H, dh)
    gq, gk = 1.0 + 0.5 * _randn(dh, seed + 3), 1.0 + 0.5 * _randn(dh, seed + 4)
    bq, bk = _randn(dh, seed + 5, 0.5), _randn(dh, seed + 6, 0.5)
    return x.view(rows, 3 * H * dh).contiguous(), gq, bq, gk, bk


def _stats(x64, H, dh, whole_row=False):
    """x64 [rows, 2, H, dh] -> mu, var [rows, 2, H, 1]"""
    dims = (2, 3) if whole_row else (3,)
    mu = x64.mean(dims, keepdim=True)
    var = ((x64 - mu) ** 2).mean(dims, keepdim=True)
    return mu.expand(-1, -1, H, 1), var.expand(-1, -1, H, 1)


def _fwd_check(ops, rows, H, dh, dtype, eps, seed, sample=None):
    """runs the forward kernel on fresh inputs, checks statistics and output per element (on the rows `sample`, default all), and returns
    what the backward check needs"""
    W, h = _depth(dh, dtype)
    ou = _ou(dtype)
    x, gq, bq, gk, bk = _inputs(rows, H, dh, dtype, seed)
    qkv = x.clone()
    saved, mean, rstd = ops.qk_norm_fwd(qkv, gq, bq, gk, bk, H, dh, eps)
    D = H * dh
    # ---- bit-for-bit: the V third, the saved copy, independence of the saved copy, repeatability
    assert torch.equal(_bits(qkv[:, 2 * D:]), _bits(x[:, 2 * D:])), "the V third was written"
    assert torch.equal(_bits(saved), _bits(x[:, :2 * D])), "saved_qk is not the input bits"
    q2 = x.clone()
    assert ops.qk_norm_fwd(q2, gq, bq, gk, bk, H, dh, eps, save=False) == (None, None, None)
    assert torch.equal(_bits(q2), _bits(qkv)), "the in-place result depends on saved_qk"
    q3 = x.clone()
    s3, m3, r3 = ops.qk_norm_fwd(q3, gq, bq, gk, bk, H, dh, eps)
    assert torch.equal(_bits(q3), _bits(qkv)) and torch.equal(m3, mean) and torch.equal(r3, rstd) and torch.equal(_bits(s3), _bits(saved))
    # ---- bounded: statistics and output
    rsel = slice(None) if sample is None else sample
    n = rows if sample is None else len(sample)
    x64 = x[rsel][:, :2 * D].double().view(n, 2, H, dh)
    g64 = torch.stack([gq, gk]).double().view(1, 2, 1, dh)
    b64 = torch.stack([bq, bk]).double().view(1, 2, 1, dh)
    mu, var = _stats(x64, H, dh)
    rs = 1.0 / torch.sqrt(var + eps)
    mk, rk = mean[rsel].double().view(n, 2, H, 1), rstd[rsel].double().view(n, 2, H, 1)
    tol_mu = (h + 2) * U * x64.abs().mean(3, keepdim=True) + U * mu.abs()
    mu_w, var_w = _stats(x64, H, dh, whole_row=True)
    _check(mk, mu, tol_mu, [mu_w] if H > 1 else [], f"mean rows={rows} H={H}")
    delta = mk - mu
    rel_rs = 0.5 * ((h + 6) * U * (var + delta ** 2) / (var + eps) + delta ** 2 / (var + eps)) + 3 * U
    wrong_rs = [1.0 / torch.sqrt(var * dh / (dh - 1) + eps), 1.0 / torch.sqrt(var)]          # unbiased variance; eps dropped
    if H > 1:
        wrong_rs.append(1.0 / torch.sqrt(var_w + eps))
    _check(rk, rs, rel_rs * rs, wrong_rs, f"rstd rows={rows} H={H}")
    eps_rs = (rk / rs - 1.0).abs()
    d = x64 - mu
    yref = d * rs * g64 + b64
    t = g64.abs() * (delta.abs() * rk) + (d * g64).abs() * (rs * eps_rs)
    t = t + 4 * U * ((d - delta) * rk * g64).abs() + 4 * U * b64.abs()
    tol_y = t + ou * (yref.abs() + t)
    flat = lambda a: a.reshape(n, 2 * D)
    g_sw = torch.stack([gq, gq]).double().view(1, 2, 1, dh)
    wrong_y = [flat(d * rs * g_sw + b64),                                                     # gamma_q applied to K
               flat(d / torch.sqrt(var * dh / (dh - 1) + eps) * g64 + b64),                   # unbiased variance
               flat(d / torch.sqrt(var) * g64 + b64)]                                         # eps dropped
    if H > 1:
        wrong_y.append(flat((x64 - mu_w) / torch.sqrt(var_w + eps) * g64 + b64))              # statistics over the whole row
    _check(qkv[rsel][:, :2 * D], flat(yref), flat(tol_y), wrong_y, f"y rows={rows} H={H}")
    # the restatement the Block tests use says the same
    if sample is None:
        full = QR.qk_norm64(torch.nan_to_num(x.double(), 0.0, 0.0, 0.0), gq.double(), bq.double(), gk.double(), bk.double(), eps, H, dh)
        assert _within(qkv[:, :2 * D], full[:, :2 * D], flat(tol_y))
    return x, saved, mean, rstd, gq, gk


def _sum_depth(ops, rows, H, dh, dtype):
    """depth of the evaluation tree of the sums over rows (and heads): rows per wave of a chunk, 2 levels over the 4 waves, the heads of all
    column tiles one after the other, then ucfvit_reduce_rows over the R chunk rows (its partial rows per thread, 2, 16, 1 as in the
    LayerNorm test)"""
    from UCF_VIT._hip import lib
    R = lib.load().ucfvit_qk_norm_partial_rows(rows, H, dh)
    rpc = -(-rows // R)
    return R, rpc, -(-rpc // 4) + 2 + 2 * H + -(-R // 64) + 2 + 16 + 1


def _bwd_check(ops, rows, H, dh, dtype, seed, fwd, chunk_rows=None):
    x, saved, mean, rstd, gq, gk = fwd
    W, h = _depth(dh, dtype)
    ou = _ou(dtype)
    D = H * dh
    dy = _quarters((rows, 3 * D), seed + 10, dtype)
    vpat = dy[:, 2 * D:].clone().reshape(-1)
    vpat[0::2] = float("nan")
    vpat[1::4] = float("inf")
    dy[:, 2 * D:] = vpat.view(rows, D)
    R, rpc, hs = _sum_depth(ops, rows, H, dh, dtype)
    # ---- the kernel: plain, with both sums, with each alone; dx must not depend on the sums, and two calls give the same bits
    dA = ops.qk_norm_bwd(dy.clone(), saved, gq, gk, mean, rstd, H, dh)
    pg, cs = torch.full((4, dh), float("nan"), device=DEV), torch.full((2 * D,), float("nan"), device=DEV)
    dB = ops.qk_norm_bwd(dy.clone(), saved, gq, gk, mean, rstd, H, dh, param_grads=pg, c_colsum=cs)
    pg2, cs2 = torch.empty_like(pg), torch.empty_like(cs)
    dC = ops.qk_norm_bwd(dy.clone(), saved, gq, gk, mean, rstd, H, dh, param_grads=pg2)
    dD = ops.qk_norm_bwd(dy.clone(), saved, gq, gk, mean, rstd, H, dh, c_colsum=cs2)
    for other in (dB, dC, dD):
        assert torch.equal(_bits(other), _bits(dA)), "dx depends on which sums are taken"
    assert torch.equal(pg2, pg) and torch.equal(cs2, cs), "the sums depend on each other"
    assert torch.equal(_bits(dA[:, 2 * D:]), _bits(dy[:, 2 * D:])), "the V third of dqkv was written"
    pg0, cs0 = _randn((4, dh), seed + 11), _randn((2 * D,), seed + 12)       # accumulate on top of non-zero buffers: one more addition
    pg3, cs3 = pg0.clone(), cs0.clone()
    ops.qk_norm_bwd(dy.clone(), saved, gq, gk, mean, rstd, H, dh, param_grads=pg3, param_accumulate=True, c_colsum=cs3,
                    c_colsum_accumulate=True)
    for got, base, fresh in ((pg3, pg0, pg), (cs3, cs0, cs)):
        want = base.double() + fresh.double()
        assert _within(got, want, 2 * U * (base.double().abs() + fresh.double().abs() + want.abs())), "accumulate"
    # ---- float64, in row blocks (the large case does not fit at once); per-element checks on every row, sums accumulated
    g64 = torch.stack([gq, gk]).double().view(1, 2, 1, dh)
    g_sw = torch.stack([gq, gq]).double().view(1, 2, 1, dh)
    last_from = (R - 1) * rpc                                          # first row of the last row chunk
    acc = {k: torch.zeros((2, dh) if k[0] in "gb" else (2 * D,), dtype=torch.float64, device=DEV)
           for k in ("g", "g_abs", "g_rnd", "g_wrong", "b", "b_wrong", "c", "c_abs", "c_t", "c_wrong")}
    step = chunk_rows or rows
    for r0 in range(0, rows, step):
        r1 = min(rows, r0 + step)
        n = r1 - r0
        x64 = saved[r0:r1].double().view(n, 2, H, dh)
        dy64 = dy[r0:r1, :2 * D].double().view(n, 2, H, dh)
        m_in, r_in = mean[r0:r1].double().view(n, 2, H, 1), rstd[r0:r1].double().view(n, 2, H, 1)
        xh = (x64 - m_in) * r_in
        g = dy64 * g64
        c1, c2 = g.mean(3, keepdim=True), (g * xh).mean(3, keepdim=True)
        dx0 = r_in * (g - c1 - xh * c2)
        e_c1 = (h + 3) * U * g.abs().mean(3, keepdim=True)
        e_c2 = (h + 7) * U * (g * xh).abs().mean(3, keepdim=True)
        inner = g.abs() + c1.abs() + (xh * c2).abs()
        t32 = r_in * (e_c1 + xh.abs() * e_c2 + c2.abs() * 4 * U * xh.abs() + 8 * U * inner)
        if chunk_rows is None or r0 == 0 or r1 == rows:                # the large case: its first and last row block per element
            gw = dy64 * g_sw
            wrong = [(r_in * (gw - gw.mean(3, keepdim=True) - xh * (gw * xh).mean(3, keepdim=True))).reshape(n, 2 * D)]     # gamma_q on K
            if H > 1:                                                  # the two segment means taken over the whole row
                wrong.append((r_in * (g - g.mean((2, 3), keepdim=True) - xh * (g * xh).mean((2, 3), keepdim=True))).reshape(n, 2 * D))
            _check(dA[r0:r1, :2 * D], dx0.reshape(n, 2 * D), (t32 + ou * (dx0.abs() + t32)).reshape(n, 2 * D), wrong,
                   f"dx rows={rows} H={H} block {r0}")
        keep = (torch.arange(r0, r1, device=DEV) < last_from).double().view(n, 1, 1, 1)
        acc["g"] += (dy64 * xh).sum((0, 2))
        acc["g_abs"] += (dy64 * xh).abs().sum((0, 2))
        acc["g_rnd"] += (dy64.abs() * 4 * U * xh.abs()).sum((0, 2))
        acc["g_wrong"] += (dy64 * xh * keep).sum((0, 2))
        acc["b"] += dy64.sum((0, 2))
        acc["b_wrong"] += (dy64 * keep).sum((0, 2))
        acc["c"] += dx0.sum(0).reshape(-1)
        acc["c_abs"] += dx0.abs().sum(0).reshape(-1)
        acc["c_t"] += t32.sum(0).reshape(-1)
        acc["c_wrong"] += (dx0 * keep).sum(0).reshape(-1)
    got_g, got_b = pg.view(2, 2, dh)[:, 0], pg.view(2, 2, dh)[:, 1]      # [q / k][dgamma / dbeta][dh]
    tol_g = (hs + 6) * U * acc["g_abs"] + acc["g_rnd"]
    _check(got_g, acc["g"], tol_g, [acc["g_wrong"], acc["g"].flip(0)], f"dgamma rows={rows} H={H}")
    assert torch.equal(got_b.double(), acc["b"]), f"dbeta rows={rows} H={H} is an exact sum of multiples of 1/4"
    assert not torch.equal(got_b.double(), acc["b_wrong"]) and not torch.equal(got_b.double(), acc["b"].flip(0))
    _check(cs, acc["c"], acc["c_t"] + (hs + 6) * U * acc["c_abs"], [acc["c_wrong"]], f"colsum rows={rows} H={H}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dh", [32, 64, 128])
def test_qk_norm_fwd_bwd_vs_fp64(dh, dtype):
    """dh x H in {1, 3, 16} x rows in {1, 5, 3 * 197} (H 3, dh 32: a part-filled wave; 3 * 197 rows: more than one row chunk and a ragged
    last one); eps 1e-5 with segments of variance 1e-6, so that a dropped eps shows"""
    ops = _ops()
    for H in (1, 3, 16):
        for rows in (1, 5, 3 * 197):
            seed = 1000 * dh + 37 * H + rows
            fwd = _fwd_check(ops, rows, H, dh, dtype, 1e-5, seed)
            _bwd_check(ops, rows, H, dh, dtype, seed, fwd)
    R, rpc, _ = _sum_depth(ops, 3 * 197, 16, dh, dtype)
    assert R > 1 and (3 * 197) % rpc != 0                              # several chunks, the last one ragged


def test_qk_norm_vit_l_stream_bf16():
    """[665 * 197, 16, 64] bf16, the ViT-L stream: every workgroup loops over its rows.  Statistics and output on a sample of rows (the
    first and last of the stream and of chunks in between), dx on the first and last row block, all sums over all rows."""
    ops = _ops()
    rows, H, dh = 665 * 197, 16, 64
    R, rpc, _ = _sum_depth(ops, rows, H, dh, torch.bfloat16)
    sample = sorted({0, 1, 2, 3, 4, rpc - 1, rpc, rpc + 1, 17 * rpc + 5, rows // 2, (R - 1) * rpc - 1, (R - 1) * rpc, rows - 2, rows - 1})
    fwd = _fwd_check(ops, rows, H, dh, torch.bfloat16, 1e-6, 99, sample=sample)
    _bwd_check(ops, rows, H, dh, torch.bfloat16, 99, fwd, chunk_rows=8192)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_coarse_grid_is_bounded_not_exact(dtype):
    """every segment holds +p and -p in equal numbers (p a power of two per segment), eps = 0: mean 0 and variance p^2 are exact in the
    kernel, xhat = +-1 up to rsqrtf (2 ulp, not correctly rounded), so y = +-gamma + beta within 3 U |gamma| + U |y| and the output
    rounding: the bounded tier (see the module docstring)"""
    ops = _ops()
    rows, H, dh = 37, 3, 64
    sign = torch.where(torch.rand((rows, 3, H, dh), generator=_gen(5), device=DEV).argsort(3) % 2 == 0, 1.0, -1.0)
    p = torch.pow(2.0, torch.randint(-6, 7, (rows, 3, H, 1), generator=_gen(6), device=DEV).float())
    x = (sign * p).to(dtype).view(rows, 3 * H * dh).contiguous()
    gq, gk, bq, bk = 1.0 + 0.5 * _randn(dh, 7), 1.0 + 0.5 * _randn(dh, 8), _randn(dh, 9, 0.5), _randn(dh, 10, 0.5)
    qkv = x.clone()
    saved, mean, rstd = ops.qk_norm_fwd(qkv, gq, bq, gk, bk, H, dh, 0.0)
    assert torch.equal(mean, torch.zeros_like(mean))                  # exact
    assert _within(rstd.view(rows, 2, H, 1), 1.0 / p[:, :2].double(), 3 * U / p[:, :2].double())
    g64 = torch.stack([gq, gk]).double().view(1, 2, 1, dh)
    b64 = torch.stack([bq, bk]).double().view(1, 2, 1, dh)
    yref = sign[:, :2].double() * g64 + b64
    tol = 3 * U * g64.abs() + U * yref.abs()
    tol = tol + _ou(dtype) * (yref.abs() + tol)
    D = H * dh
    _check(qkv[:, :2 * D], yref.reshape(rows, 2 * D), tol.expand_as(yref).reshape(rows, 2 * D), [(-yref).reshape(rows, 2 * D)], "coarse grid")
    assert torch.equal(_bits(qkv[:, 2 * D:]), _bits(x[:, 2 * D:]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,dh", [(197, 64), (300, 32)])
def test_k_norm_bias_gradient_through_attention_is_zero(N, dh, dtype):
    """A key bias shifts every score of a query alike, so through a real attention dbeta_k = sum over rows and heads of dK is
    mathematically 0 (N 197, dh 64: the fused short route; N 300: the streaming route).  What the kernels return is round-off, compared
    absolutely: every dK[k] is a sum over the N queries accumulated in fp32 (depth <= N, plus 64 for the softmax and exp arithmetic in
    front of it) and rounded once to the output type, so each carries at most (u_out + (N + 64) U) of the magnitudes summed, and the sum
    of the dK errors is bounded by (2 u_out + (N + 64) U) * sum|dK| (the second u_out: bf16 kernels also round the probabilities they
    multiply).  The same bound rejects the q_norm bias gradient, which is not zero."""
    ops = _ops()
    B, H = 2, 3
    D = H * dh
    rows = B * N
    qkv = _randn((rows, 3 * D), 21).to(dtype)
    gq, gk, bq, bk = 1.0 + 0.3 * _randn(dh, 22), 1.0 + 0.3 * _randn(dh, 23), _randn(dh, 24, 0.3), _randn(dh, 25, 0.3)
    saved, mean, rstd = ops.qk_norm_fwd(qkv, gq, bq, gk, bk, H, dh, 1e-6)
    o, lse = ops.attention_fwd(qkv, B, N, H, dh, dh ** -0.5)
    do = _randn((rows, D), 26).to(dtype)
    dqkv = ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, dh ** -0.5)
    sum_abs_dk = dqkv[:, D:2 * D].double().abs().view(rows, H, dh).sum((0, 1))
    pg = torch.empty((4, dh), device=DEV)
    ops.qk_norm_bwd(dqkv, saved, gq, gk, mean, rstd, H, dh, param_grads=pg)
    tol = (2 * _ou(dtype) + (N + 64) * U) * sum_abs_dk
    print("max |dbeta_k|", float(pg[3].abs().max()), "bound", float(tol.min()), "max |dbeta_q|", float(pg[1].abs().max()))
    assert bool((pg[3].double().abs() <= tol).all())
    assert float(pg[1].abs().max()) > float(tol.max())                  # not a bound anything passes


def test_wrapper_refusals():
    ops = _ops()
    H, dh = 2, 32
    qkv = torch.zeros((4, 3 * H * dh), device=DEV)
    g = torch.ones(dh, device=DEV)
    st = torch.zeros((4, 2 * H), device=DEV)
    sv = torch.zeros((4, 2 * H * dh), device=DEV)
    with pytest.raises(TypeError, match=r"\[rows, 3 H dh\]"):
        ops.qk_norm_fwd(qkv[:, :-1].contiguous(), g, g, g, g, H, dh, 1e-6)
    with pytest.raises(ValueError, match="dh=48"):
        ops.qk_norm_fwd(torch.zeros((4, 3 * 2 * 48), device=DEV), g, g, g, g, 2, 48, 1e-6)
    with pytest.raises(TypeError, match="fp32 tensors of dh"):
        ops.qk_norm_fwd(qkv, g.bfloat16(), g, g, g, H, dh, 1e-6)
    with pytest.raises(TypeError, match="fp32 tensors of dh"):
        ops.qk_norm_fwd(qkv, g, g, g[:16], g, H, dh, 1e-6)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.qk_norm_fwd(torch.zeros((4, 6 * H * dh), device=DEV)[:, ::2], g, g, g, g, H, dh, 1e-6)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ops.qk_norm_fwd(qkv.cpu(), g, g, g, g, H, dh, 1e-6)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ops.qk_norm_fwd(qkv, g.cpu(), g, g, g, H, dh, 1e-6)
    with pytest.raises(TypeError, match="dqkv's dtype"):
        ops.qk_norm_bwd(qkv, sv.bfloat16(), g, g, st, st, H, dh)
    with pytest.raises(TypeError, match=r"fp32 \[rows, 2 H\]"):
        ops.qk_norm_bwd(qkv, sv, g, g, st[:2], st, H, dh)
    with pytest.raises(TypeError, match="4 dh elements"):
        ops.qk_norm_bwd(qkv, sv, g, g, st, st, H, dh, param_grads=torch.zeros(dh, device=DEV))
    with pytest.raises(TypeError, match="2 H dh elements"):
        ops.qk_norm_bwd(qkv, sv, g, g, st, st, H, dh, c_colsum=torch.zeros(H * dh, device=DEV))
    with pytest.raises(RuntimeError, match="ucfvit_qk_norm_fwd.*bad eps"):
        ops.qk_norm_fwd(qkv, g, g, g, g, H, dh, -1.0)
    empty = torch.zeros((0, 3 * H * dh), device=DEV)
    assert ops.qk_norm_fwd(empty, g, g, g, g, H, dh, 1e-6)[0].shape == (0, 2 * H * dh)
    with pytest.raises(ValueError, match="empty input"):
        ops.qk_norm_bwd(empty, sv[:0], g, g, st[:0], st[:0], H, dh, param_grads=torch.zeros((4, dh), device=DEV))
