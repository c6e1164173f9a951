"""The row-wise, reduction, copy and optimizer kernels of csrc/norm.hip and csrc/elementwise.hip against float64 references, at the widths
and batch sizes of the bench workloads (bench.WORKLOADS) and at the edges of their code paths: every LayerNorm NV instantiation, grids that
loop many times over their rows, the colsum chunk cap, the scalar fallbacks, the grid-stride loops and n % 4 tails of cast / AdamW.

Exact tier: copies and permutations are compared bit for bit.  Sums are fed multiples of 1/4 (or small integers) whose partial sums stay
below 2^22, exact in fp32 whatever the summation order, so a correct kernel equals the fp64 reference exactly.

Real-valued tier: normal operands; the reference sees the same rounded inputs and runs in float64 on the device.  Every bound is per element
and follows the kernel's arithmetic: a sum whose evaluation tree has depth h (sequential chain per lane / wave / workgroup, then the tree or
chain of the cross-lane and cross-workgroup reductions) is off by at most h * 2^-24 * sum|terms|; a bf16 output adds 2^-8 of its value (RNE).
Each bound is also shown to reject a plausibly wrong reference (a dropped last vector, a missing chunk, a shifted token, a missing bias
correction, a swapped patch axis ...), so it is tight enough to catch the bug it is meant for."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24          # fp32 unit roundoff
UB = 2.0 ** -8          # bf16 unit roundoff (RNE: |fl(x) - x| <= 2^-8 |x|)
EPS_LN = 1e-6


def _ops():
    from UCF_VIT._hip import ops
    return ops


def _wl(name):
    import bench
    return bench.WORKLOADS[name]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, seed, dtype=torch.float32, scale=1.0):
    return (torch.randn(shape, generator=_gen(seed), device=DEV, dtype=torch.float32) * scale).to(dtype)


def _quarters(shape, seed, dtype, k=8):
    """multiples of 1/4 in [-k/4, k/4]: exact in bf16, and every partial sum of fewer than 2^21 of them is exact in fp32"""
    return (torch.randint(-k, k + 1, shape, generator=_gen(seed), device=DEV).float() * 0.25).to(dtype)


def _out_u(dtype):
    return UB if dtype == torch.bfloat16 else U


def _within(got, ref, tol):
    return bool(((got.double() - ref).abs() <= tol).all())


def _check(got, ref, tol, wrong, what):
    """got within tol of ref everywhere, and the same tol rejects every reference in `wrong`"""
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, "
                                 f"worst excess {float((err - tol)[bad].max()):.3e}")
    for w in (wrong if isinstance(wrong, (list, tuple)) else [wrong]):
        assert not _within(got, w, tol), f"{what}: the bound does not reject a wrong reference"


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


# ============================================================================================== LayerNorm
def _ln_nv(D, dtype):
    epv = 16 // torch.tensor([], dtype=dtype).element_size()
    nvec = D // epv
    return epv, next(nv for nv in (1, 2, 4, 8) if nvec <= 64 * nv)


def _ln_grid(rows, backward):
    return max(1, min((rows + 3) // 4, 768 if backward else 2048))


def _ln_inputs(rows, D, dtype, seed):
    x = _randn((rows, D), seed) * (1.0 + 2.0 * torch.rand((rows, 1), generator=_gen(seed + 1), device=DEV))
    x = x + torch.randn((rows, 1), generator=_gen(seed + 2), device=DEV)
    if dtype == torch.float32:               # rows 2, 6, 10 ...: |mean| = 1000 standard deviations (what the two-pass variance is for)
        x[2::4] += 1000.0 * torch.sign(torch.randn((x[2::4].shape[0], 1), generator=_gen(seed + 3), device=DEV))
    gamma = (1.0 + 0.5 * _randn(D, seed + 4)).to(dtype)
    beta = _randn(D, seed + 5, scale=0.5).to(dtype)
    return x.to(dtype), gamma, beta


def _ln_stats(x64, keep=None):
    xs = x64 if keep is None else x64[:, :keep]
    D = x64.shape[1]
    mu = xs.sum(1) / D
    var = ((xs - mu[:, None]) ** 2).sum(1) / D
    return mu, var


LN_CASES = ([(torch.bfloat16, D) for D in (192, 512, 576, 768, 1024, 2048, 4096)]
            + [(torch.float32, D) for D in (64, 256, 576, 768, 1024, 2048)])


def _ln_rows(dtype, D):
    w = _wl("vit_l16_224")
    vit_l_rows = w["batch"] * ((w["img"] // w["patch"]) ** 2 + 1)        # 665 x 197 = 131005
    big = vit_l_rows if (dtype == torch.bfloat16 and D == w["dim"]) else 32773   # > 4 passes of the forward grid (2048 wg x 4 rows)
    return [1, 3, 5, big]


@pytest.mark.parametrize("dtype,D", LN_CASES, ids=[f"{'bf16' if d == torch.bfloat16 else 'fp32'}-D{D}" for d, D in LN_CASES])
def test_layernorm_fwd_bwd_vs_fp64(dtype, D):
    """y, mean, rstd; dx without and with dres; dgamma / dbeta fresh and accumulated; the dx column sums (DXS) fresh and accumulated.
    Bounds: mean and the centred sum of squares are sums of depth k + 6 (k = elements per lane, 6 shuffle levels); the variance error
    also carries delta^2 (delta = the kernel's mean error, centring about a wrong mean adds delta^2 exactly); rsqrtf is within 2 ulp.
    dgamma: depth = rows per wave + 3 (waves) + partial rows per reduce thread + 2 + 16 (+1 accumulate).  dbeta is an exact sum."""
    ops = _ops()
    epv, nv = _ln_nv(D, dtype)
    k = nv * epv
    bwd_ok = D <= (1024 if dtype == torch.float32 else 2048)
    ou = _out_u(dtype)
    for rows in _ln_rows(dtype, D):
        seed = rows * 31 + D
        x, gamma, beta = _ln_inputs(rows, D, dtype, seed)
        y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, EPS_LN)
        x64, g64, b64 = x.double(), gamma.double(), beta.double()
        mu, var = _ln_stats(x64)
        rs = 1.0 / torch.sqrt(var + EPS_LN)
        mu_w, var_w = _ln_stats(x64, D - epv)                           # wrong: the last 16-byte vector of each row left out
        rs_w = 1.0 / torch.sqrt(var_w + EPS_LN)
        absx = x64.abs().sum(1)
        tol_mu = (k + 8) * U * absx / D + U * mu.abs()
        _check(mean, mu, tol_mu, mu_w, f"mean rows={rows}")
        delta = mean.double() - mu
        rel_rs = 0.5 * ((k + 12) * U * (var + delta ** 2) / (var + EPS_LN) + delta ** 2 / (var + EPS_LN)) + 3 * U
        wrong_rs = [rs_w, 1.0 / torch.sqrt(var * D / (D - 1) + EPS_LN)]
        if dtype == torch.float32 and rows >= 3:                       # one-pass E[x^2] - mu^2 in fp32 on the |mean| = 1000 sigma rows
            xf = x.float()
            wrong_rs.append(1.0 / torch.sqrt(((xf * xf).mean(1) - xf.mean(1) ** 2).clamp_min(0).double() + EPS_LN))
        _check(rstd, rs, rel_rs * rs, wrong_rs, f"rstd rows={rows}")
        eps_rs = (rstd.double() / rs - 1.0).abs()
        d = x64 - mu[:, None]
        yref = d * rs[:, None] * g64 + b64
        t = g64.abs() * (delta.abs() * rstd.double())[:, None] + (d * g64).abs() * (rs * eps_rs)[:, None]
        t = t + 4 * U * ((d - delta[:, None]) * rstd.double()[:, None] * g64).abs() + 4 * U * b64.abs()
        tol_y = t + ou * (yref.abs() + t)
        y_w = (x64 - mu_w[:, None]) * rs_w[:, None] * g64 + b64
        _check(y, yref, tol_y, y_w, f"y rows={rows}")
        del d, yref, t, tol_y, y_w
        if not bwd_ok:
            continue
        # ---- backward, with the forward's (checked) statistics as its inputs
        dy = _quarters((rows, D), seed + 10, dtype)
        dres = _randn((rows, D), seed + 11, dtype)
        m_in, r_in = mean.double()[:, None], rstd.double()[:, None]
        xh = (x64 - m_in) * r_in
        dy64 = dy.double()
        g = dy64 * g64
        c1, c2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
        dx0 = r_in * (g - c1 - xh * c2)
        c1w, c2w = g[:, :D - epv].sum(1, keepdim=True) / D, (g * xh)[:, :D - epv].sum(1, keepdim=True) / D
        dx0_w = r_in * (g - c1w - xh * c2w)                             # wrong: the last vector left out of the row sums
        e_c1 = (k + 9) * U * g.abs().mean(1, keepdim=True)
        e_c2 = (k + 13) * U * (g * xh).abs().mean(1, keepdim=True)
        inner = g.abs() + c1.abs() + (xh * c2).abs()
        t32 = r_in * (e_c1 + xh.abs() * e_c2 + c2.abs() * 4 * U * xh.abs() + 8 * U * inner)   # fp32 value of r before dres
        dres64 = dres.double()
        # call A: no dres, no column sums, fresh dgamma / dbeta
        dxA, dgA, dbA = ops.layernorm_bwd(dy, x, gamma, mean, rstd)
        _check(dxA, dx0, t32 + ou * (dx0.abs() + t32), dx0_w, f"dx rows={rows}")
        gb = _ln_grid(rows, True)
        h = -(-rows // (4 * gb)) + 3 + -(-gb // 64) + 2 + 16 + 1
        dg = (dy64 * xh).sum(0)
        last = (torch.arange(rows, device=DEV) // 4) % gb != gb - 1     # wrong: the partial row of the last workgroup left out
        tol_dg = (h + 6) * U * (dy64 * xh).abs().sum(0) + (dy64.abs() * 4 * U * xh.abs()).sum(0)
        _check(dgA, dg, tol_dg, (dy64 * xh)[last].sum(0), f"dgamma rows={rows}")
        assert torch.equal(dbA.double(), dy64.sum(0)), f"dbeta rows={rows} is an exact sum"
        # call B: dres, dgamma / dbeta accumulated into non-zero buffers, dx column sums accumulated
        dg0, db0 = _randn(D, seed + 12), _quarters((D,), seed + 13, torch.float32)
        cs0 = _randn(D, seed + 14)
        dgB, dbB, csB = dg0.clone(), db0.clone(), cs0.clone()
        dxB, _, _ = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dres=dres, dgamma=dgB, dbeta=dbB, accumulate=True, dx_colsum=csB,
                                      dx_colsum_accumulate=True)
        dx1 = dx0 + dres64
        t1 = t32 + 2 * U * (dx1.abs() + dres64.abs())
        _check(dxB, dx1, t1 + ou * (dx1.abs() + t1), dx0_w + dres64, f"dx+dres rows={rows}")
        _check(dgB, dg0.double() + dg, tol_dg + 2 * U * (dg0.double().abs() + (dg0.double() + dg).abs()), dg0.double() + (dy64 * xh)[last].sum(0),
               f"dgamma accumulate rows={rows}")
        assert torch.equal(dbB.double(), db0.double() + dy64.sum(0)), f"dbeta accumulate rows={rows}"
        cs = dx1.sum(0)
        tol_cs = t1.sum(0) + (h + 6) * U * dx1.abs().sum(0)
        _check(csB, cs0.double() + cs, tol_cs + 2 * U * (cs0.double().abs() + (cs0.double() + cs).abs()), cs0.double() + dx1[last].sum(0),
               f"dx_colsum accumulate rows={rows}")
        # call C: column sums written fresh (no dres); dx must not depend on whether the sums are taken
        csC = torch.full((D,), float("nan"), device=DEV)
        dxC, _, _ = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx_colsum=csC)
        assert torch.equal(dxC, dxA)
        _check(csC, dx0.sum(0), t32.sum(0) + (h + 6) * U * dx0.abs().sum(0), dx0[last].sum(0), f"dx_colsum rows={rows}")


@pytest.mark.parametrize("dtype,D,backward,limit", [
    (torch.bfloat16, 100, False, "multiple of 8"), (torch.float32, 66, False, "multiple of 4"), (torch.bfloat16, 100, True, "multiple of 8"),
    (torch.bfloat16, 4104, False, "4096"), (torch.float32, 2052, False, "2048"),
    (torch.float32, 2048, True, "1024"), (torch.bfloat16, 4096, True, "2048")])
def test_layernorm_rejects_unsupported_widths(dtype, D, backward, limit):
    ops = _ops()
    x = _randn((4, D), 1, dtype)
    one, zero = torch.ones(D, dtype=dtype, device=DEV), torch.zeros(D, dtype=dtype, device=DEV)
    with pytest.raises(RuntimeError, match=limit):
        if backward:
            mean, rstd = torch.zeros(4, device=DEV), torch.ones(4, device=DEV)
            ops.layernorm_bwd(x, x, one, mean, rstd)
        else:
            ops.layernorm_fwd(x, one, zero, EPS_LN)
    torch.cuda.synchronize()


# ============================================================================================== column sums / partial-row reduction
def _colsum_depth(M, vector):
    if not vector:
        return M + 2
    chunks = max(1, min(256, -(-M // 128)))
    rpc = -(-M // chunks)
    return -(-rpc // 4) + 4 + -(-chunks // 64) + 2 + 16 + 1


def _colsum_missing_last_chunk(x64, M):
    """the column sums without the last non-empty row chunk (at M = 32769 the 256th chunk of 129 rows is empty)"""
    chunks = max(1, min(256, -(-M // 128)))
    rpc = -(-M // chunks)
    return x64[:(M - 1) // rpc * rpc].sum(0)


COLSUM = [(torch.bfloat16, 1, 1024), (torch.float32, 127, 3072), (torch.bfloat16, 32769, 4096), (torch.float32, 32769, 1024),
          (torch.bfloat16, 131005, 1024), (torch.bfloat16, 131005, 3072), (torch.float32, 131005, 4096)]


@pytest.mark.parametrize("dtype,M,N", COLSUM)
def test_colsum_vector_path(dtype, M, N):
    """chunk cap (256 chunks of up to 512 rows at M = 131005), exact tier (quarters) and real-valued tier, fresh and accumulated"""
    ops = _ops()
    xq = _quarters((M, N), M + N, dtype)
    assert torch.equal(ops.colsum(xq).double(), xq.double().sum(0))
    acc0 = _quarters((N,), 7, torch.float32)
    assert torch.equal(ops.colsum(xq, out=acc0.clone(), accumulate=True).double(), acc0.double() + xq.double().sum(0))
    x = _randn((M, N), M + N + 1, dtype)
    x64 = x.double()
    ref = x64.sum(0)
    tol = _colsum_depth(M, True) * U * x64.abs().sum(0)
    _check(ops.colsum(x), ref, tol, _colsum_missing_last_chunk(x64, M), f"colsum M={M}")


def test_colsum_strided_qkv_third_and_scalar_fallbacks():
    """the V third of a ViT-L qkv buffer [M, 3D] (ldx = 3D); odd N; a view 2 bytes off 16-byte alignment; M = 0 (regression: the
    NULL data pointer of an empty input was refused)"""
    ops = _ops()
    w = _wl("vit_l16_224")
    D = w["dim"]
    M = w["batch"] * ((w["img"] // w["patch"]) ** 2 + 1)
    qkv = _quarters((M, 3 * D), 3, torch.bfloat16)
    v = qkv[:, 2 * D:]
    assert torch.equal(ops.colsum(v).double(), v.double().sum(0))
    qkv = _randn((M, 3 * D), 4, torch.bfloat16)
    v64 = qkv[:, 2 * D:].double()
    _check(ops.colsum(qkv[:, 2 * D:]), v64.sum(0), _colsum_depth(M, True) * U * v64.abs().sum(0), _colsum_missing_last_chunk(v64, M),
           "colsum strided")
    for dtype, M, N, off in [(torch.bfloat16, 5000, 1001, 0), (torch.float32, 777, 333, 0), (torch.bfloat16, 3000, 1024, 1),
                             (torch.float32, 129, 64, 1)]:
        base = _quarters((M, N + off), M + N, dtype)
        xq = base[:, off:]
        assert torch.equal(ops.colsum(xq).double(), xq.double().sum(0))
        acc0 = _quarters((N,), 9, torch.float32)
        assert torch.equal(ops.colsum(xq, out=acc0.clone(), accumulate=True).double(), acc0.double() + xq.double().sum(0))
        base = _randn((M, N + off), M + N + 1, dtype)
        x64 = base[:, off:].double()
        _check(ops.colsum(base[:, off:]), x64.sum(0), _colsum_depth(M, False) * U * x64.abs().sum(0), x64[:-1].sum(0),
               f"colsum scalar M={M} N={N} off={off}")
    for dtype in (torch.float32, torch.bfloat16):
        e = torch.empty((0, 1024), dtype=dtype, device=DEV)
        assert torch.equal(ops.colsum(e), torch.zeros(1024, device=DEV))
        acc0 = _randn(1024, 5)
        assert torch.equal(ops.colsum(e, out=acc0.clone(), accumulate=True), acc0)


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 63, 64, 65, 768])
def test_reduce_rows(rows):
    """reduce_partials_kernel: 16 row groups, 4 loads in flight (64-row steps), N = 1000 (not a multiple of the 16-column workgroup)"""
    ops = _ops()
    N = 1000
    pq = _quarters((rows, N), rows, torch.float32, k=4096)
    assert torch.equal(ops.reduce_rows(pq, torch.empty(N, device=DEV)).double(), pq.double().sum(0))
    acc0 = _quarters((N,), 3, torch.float32)
    assert torch.equal(ops.reduce_rows(pq, acc0.clone(), accumulate=True).double(), acc0.double() + pq.double().sum(0))
    p = _randn((rows, N), rows + 1)
    p64 = p.double()
    h = -(-rows // 64) + 2 + 16 + 1
    _check(ops.reduce_rows(p, torch.empty(N, device=DEV)), p64.sum(0), h * U * p64.abs().sum(0), p64[:-1].sum(0), f"reduce_rows {rows}")


# ============================================================================================== token assembly
def _tok_cases():
    w = _wl("vit_l16_224")
    L = (w["img"] // w["patch"]) ** 2
    return [(torch.bfloat16, w["batch"], L, w["dim"], True, True), (torch.bfloat16, w["batch"], L, w["dim"], False, False),
            (torch.float32, 7, 49, 192, True, False), (torch.float32, 6, 64, 192, False, True), (torch.bfloat16, 3, 16, 192, True, True)]


@pytest.mark.parametrize("dtype,B,L,D,has_cls,has_pos", _tok_cases())
def test_tokens_fwd_bwd(dtype, B, L, D, has_cls, has_pos):
    """forward and dpatches bit-exact; dpos / dcls: exact tier (quarters) and real-valued tier (a sequential sum over B, depth B + 1),
    fresh and accumulated; want_patches=False"""
    ops = _ops()
    pre = 1 if has_cls else 0
    N = L + pre
    patches = _randn((B * L, D), B + L + D, dtype)
    cls = _randn(D, 2, dtype) if has_cls else None
    pos = _randn((N, D), 3, dtype) if has_pos else None
    out = ops.tokens_fwd(patches, cls, pos, B, L, D)
    tok = patches.view(B, L, D)
    if has_cls:
        tok = torch.cat([cls.view(1, 1, D).expand(B, 1, D), tok], 1)
    ref = tok.double() + (pos.double() if has_pos else 0.0)
    assert torch.equal(out, ref.float().to(dtype))                     # the sum of two bf16 is exact in fp32: one RNE either way
    for exact in (True, False):
        dout = _quarters((B, N, D), 5, dtype) if exact else _randn((B, N, D), 6, dtype)
        d64 = dout.double()
        dpatches, dpos, dcls = ops.tokens_bwd(dout, B, L, D, has_cls, True)
        assert torch.equal(dpatches, dout[:, pre:].reshape(B * L, D))
        ref = d64.sum(0)
        tol = 0 * ref if exact else (B + 1) * U * d64.abs().sum(0)
        wrong = torch.roll(ref, 1, 0)                                   # dpos shifted by one token
        _check(dpos, ref, tol, wrong, "dpos")
        if has_cls:
            _check(dcls, ref[0], tol[0], ref[1], "dcls")
        p0, c0 = _randn((N, D), 7), _randn(D, 8)
        dpatches, dpos, dcls = ops.tokens_bwd(dout, B, L, D, has_cls, True, dpos=p0.clone(), dcls=c0.clone(), accumulate=True,
                                              want_patches=False)
        assert dpatches is None
        tol_a = tol + 2 * U * (p0.double().abs() + (p0.double() + ref).abs())
        _check(dpos, p0.double() + ref, tol_a, p0.double() + wrong, "dpos accumulate")
        if has_cls:
            tol_c = tol[0] + 2 * U * (c0.double().abs() + (c0.double() + ref[0]).abs())
            _check(dcls, c0.double() + ref[0], tol_c, c0.double() + ref[1], "dcls accumulate")


# ============================================================================================== MAE row gathers / scatters, unshuffle
def _shuffle(B, L, seed):
    noise = torch.rand((B, L), generator=_gen(seed), device=DEV)
    ids_shuffle = torch.argsort(noise, dim=1)
    return ids_shuffle, torch.argsort(ids_shuffle, dim=1)


@pytest.mark.parametrize("dtype,B,L,R,D", [(torch.bfloat16, 1002, 196, 49, 1024), (torch.bfloat16, 5, 196, 49, 12), (torch.float32, 4, 50, 13, 3),
                                           (torch.float32, 3, 64, 64, 192), (torch.bfloat16, 4, 16, 0, 64), (torch.bfloat16, 0, 16, 4, 64)])
def test_gather_scatter_rows_bit_exact(dtype, B, L, R, D):
    """16-B vector path and the 2-byte fallback (row bytes not a multiple of 16); idx = ids_shuffle[:, :R] with row stride L;
    R = 0 and B = 0; the scatter zeroes every row no index names.  Regression: an empty tensor's data pointer is NULL, and rows_copy
    checked for NULL pointers before it returned on B = 0 / R = 0 (a scatter with R = 0 must still zero its output)."""
    ops = _ops()
    ids_shuffle, _ = _shuffle(max(B, 1), L, B + L + R)
    ids_shuffle = ids_shuffle[:B].contiguous()
    src = _randn((B, L, D), 11, dtype)
    out = ops.gather_rows(src, ids_shuffle, R, L)
    ref = torch.gather(src, 1, ids_shuffle[:, :R, None].expand(B, R, D))
    assert out.shape == (B, R, D) and torch.equal(_bits(out), _bits(ref))
    dout = _randn((B, R, D), 12, dtype)
    dsrc = ops.scatter_rows(dout, ids_shuffle, L, L)
    ref = torch.zeros((B, L, D), dtype=dtype, device=DEV).scatter_(1, ids_shuffle[:, :R, None].expand(B, R, D), dout)
    assert torch.equal(_bits(dsrc), _bits(ref))


def _unshuffle_cases():
    w = _wl("mae_vit_l16_224")
    L = (w["img"] // w["patch"]) ** 2
    R = int(L * (1 - w["mask_ratio"]))
    B = w["batch"]
    return [(torch.bfloat16, B, L, R, w["dec_dim"], True), (torch.bfloat16, B, L, R, 576, False), (torch.float32, 9, L, R, 576, True),
            (torch.float32, 4, 20, 5, 64, False)]


@pytest.mark.parametrize("dtype,B,L,R,D,has_pos", _unshuffle_cases())
def test_unshuffle_fwd_bwd(dtype, B, L, R, D, has_pos):
    """forward and dx bit-exact; dmask_token = sum over b and the masked positions (per-b chain over L, then a chain over B: depth
    L + B + 1) and dpos = sum over b (depth B + 1) in the exact and the real-valued tier, fresh and accumulated"""
    ops = _ops()
    _, ids_restore = _shuffle(B, L, B + D)
    x = _randn((B, R, D), 21, dtype)
    mtok = _randn(D, 22, dtype)
    pos = _randn((L, D), 23, dtype) if has_pos else None
    out = ops.unshuffle_fwd(x, mtok, ids_restore, pos)
    full = torch.cat([x, mtok.view(1, 1, D).expand(B, L - R, D)], 1)
    tok = torch.gather(full, 1, ids_restore[:, :, None].expand(B, L, D))
    assert torch.equal(out, (tok.double() + (pos.double() if has_pos else 0.0)).float().to(dtype))
    masked = (ids_restore >= R).double()[:, :, None]
    for exact in (True, False):
        dout = _quarters((B, L, D), 24, dtype) if exact else _randn((B, L, D), 25, dtype)
        d64 = dout.double()
        dx, dmask, dpos = ops.unshuffle_bwd(dout, ids_restore, R, has_pos)
        ids_shuffle = torch.argsort(ids_restore, dim=1)
        assert torch.equal(dx, torch.gather(dout, 1, ids_shuffle[:, :R, None].expand(B, R, D)))
        ref_m = (d64 * masked).sum((0, 1))
        tol_m = 0 * ref_m if exact else (L + B + 2) * U * (d64.abs() * masked).sum((0, 1))
        wrong_m = (d64 * masked)[:-1].sum((0, 1))                       # the last batch element left out
        _check(dmask, ref_m, tol_m, wrong_m, "dmask_token")
        ref_p = d64.sum(0)
        tol_p = 0 * ref_p if exact else (B + 1) * U * d64.abs().sum(0)
        if has_pos:
            _check(dpos, ref_p, tol_p, torch.roll(ref_p, 1, 0), "dpos")
        m0, p0 = _randn(D, 26), _randn((L, D), 27)
        _, dmask, dpos = ops.unshuffle_bwd(dout, ids_restore, R, has_pos, dmask=m0.clone(), dpos=p0.clone() if has_pos else None,
                                           accumulate=True)
        _check(dmask, m0.double() + ref_m, tol_m + 2 * U * (m0.double().abs() + (m0.double() + ref_m).abs()), m0.double() + wrong_m,
               "dmask_token accumulate")
        if has_pos:
            _check(dpos, p0.double() + ref_p, tol_p + 2 * U * (p0.double().abs() + (p0.double() + ref_p).abs()),
                   p0.double() + torch.roll(ref_p, 1, 0), "dpos accumulate")


# ============================================================================================== cast
CAST_N = [0, 1, 2, 3, 4, 5, 3 * 2 ** 20 + 3]      # 3*2^20+3: 786432 vectors > 2048 x 256 threads (a second grid-stride pass) + a 3-tail


@pytest.mark.parametrize("src_dt,dst_dt", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.float32),
                                           (torch.bfloat16, torch.bfloat16)])
@pytest.mark.parametrize("scale", [1.0, 0.125, 3.0])
def test_cast_bit_exact(src_dt, dst_dt, scale):
    """bit-exact against (src.float() * scale).to(dst): +-0, +-inf, NaN (stays NaN, payload not compared), values that overflow bf16.
    No subnormals: they are left out of this comparison.  Regression: n = 0 (NULL data pointers) was refused as a null pointer."""
    ops = _ops()
    specials = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan"), 3.4e38, -3.39e38, 1.0, -2.5, 65504.0])
    for n in CAST_N:
        src = _randn(n, n + 1) * 10.0
        if n >= 16:
            src[-len(specials):] = specials.to(DEV)                     # the specials also land in the tail
            src[:len(specials)] = specials.to(DEV)
        elif n:
            src[:n] = specials[(torch.arange(n) * 3 + n) % len(specials)].to(DEV)
        src = src.to(src_dt)
        dst = torch.full((n,), 7.0, dtype=dst_dt, device=DEV)
        ops.cast(src, dst, scale)
        ref = (src.float() * scale).to(dst_dt)
        nan = torch.isnan(ref)
        assert torch.equal(torch.isnan(dst), nan), f"n={n}: NaN positions differ"
        assert torch.equal(_bits(dst)[~nan], _bits(ref)[~nan]), f"n={n}"


# ============================================================================================== transpose_batched
def _transpose_table(shapes):
    rows, off, tiles = [], 0, 0
    for r, c in shapes:
        rows.append([off, off, r, c, tiles])
        off += (r * c + 63) // 64 * 64
        tiles += -(-r // 64) * -(-c // 64)
    return torch.tensor(rows, dtype=torch.int64, device=DEV), off, tiles


def test_transpose_batched_bit_exact():
    """one table with the ViT-L weight shapes (qkv 3072x1024, proj 1024^2, fc1 4096x1024, fc2 1024x4096, the 1000x1024 head) and a
    matrix whose extents are multiples of 8 but not of 64; and a table of one matrix"""
    ops = _ops()
    w = _wl("vit_l16_224")
    D = w["dim"]
    for shapes in ([(3 * D, D), (D, D), (4 * D, D), (D, 4 * D), (w["classes"], D), (200, 328)], [(200, 328)], [(D, 4 * D)]):
        table, total, tiles = _transpose_table(shapes)
        src = _randn(total, len(shapes), torch.bfloat16)
        dst = torch.zeros(total, dtype=torch.bfloat16, device=DEV)
        ops.transpose_batched(src, dst, table, len(shapes), tiles)
        for (o, _, r, c, _) in table.tolist():
            assert torch.equal(_bits(dst[o:o + r * c].view(c, r)), _bits(src[o:o + r * c].view(r, c).t()))


def test_param_store_transposed_shadow_vit_b():
    """after refresh_shadow() on a ViT-B: every shadow is the RNE bf16 of its master weight and every transposed shadow its transpose"""
    from UCF_VIT._hip.params import HipParamStore
    from UCF_VIT.simple.arch import VIT
    w = _wl("vit_b16_224")
    torch.manual_seed(0)
    m = VIT(img_size=[w["img"], w["img"]], patch_size=w["patch"], in_chans=3, num_classes=w["classes"], embed_dim=w["dim"],
            depth=w["depth"], num_heads=w["heads"]).to(DEV)
    st = HipParamStore(m)
    st.refresh_shadow()
    n_t = 0
    for p, o in zip(st.params, st.offsets):
        s = st.shadow_view(p, o, p.numel())
        assert torch.equal(_bits(s), _bits(p.detach().to(torch.bfloat16)))
        if getattr(p, "_ucf_has_t", False):
            assert torch.equal(_bits(st.shadow_t_view(p, o, p.numel())), _bits(s.t()))
            n_t += 1
    assert n_t >= 4 * w["depth"] + 1                                   # at least qkv, proj, fc1, fc2 per block and the head


# ============================================================================================== AdamW
def _adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, gs):
    """fp64 torch.optim.AdamW update from the kernel's fp32 state (hyper-parameters as the fp32 values the kernel receives);
    returns the new state, its per-element bounds and wrong references: moments with beta and 1 - beta swapped, p without the
    v bias correction, p moved along the previous first moment"""
    f = lambda a: float(torch.tensor(a, dtype=torch.float32))          # noqa: E731
    bc1, bc2 = f(1.0 - b1 ** step), f(1.0 - b2 ** step)                # ops.adamw forms them in double, the ABI takes fp32
    lr, b1, b2, eps, wd, gs = map(f, (lr, b1, b2, eps, wd, gs))
    p, g, m, v = p.double(), g.double() * gs, m.double(), v.double()
    m1 = b1 * m + (1 - b1) * g
    v1 = b2 * v + (1 - b2) * g * g
    sq = torch.sqrt(v1)
    den = sq / math.sqrt(bc2) + eps
    pd = p * (1 - lr * wd)
    p1 = pd - (lr / bc1) * m1 / den
    w = dict(m=(1 - b1) * m + b1 * g, v=(1 - b2) * v + b2 * g * g, p_nobc2=pd - (lr / bc1) * m1 / (sq + eps),
             p_oldm=pd - (lr / bc1) * m / den)
    e_m = 4 * U * (b1 * m.abs() + (1 - b1) * g.abs())
    e_v = 6 * U * (b2 * v + (1 - b2) * g * g)
    e_den = sq / math.sqrt(bc2) * (0.5 * e_v / v1.clamp_min(1e-300) + 6 * U) + U * den
    upd = (lr / bc1) * m1.abs() / den
    e_p = (lr / bc1) * (e_m + m1.abs() * (e_den / den + 6 * U)) / den + 4 * U * p.abs() + 2 * U * (upd + p1.abs())
    return p1, m1, v1, e_p, e_m, e_v, w


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("gs", [1.0, 0.125])
@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("with_shadow", [True, False])
def test_adamw_vs_fp64(gdt, gs, wd, with_shadow):
    """steps 1 .. 5 and step 1000, each compared per element with an fp64 step from the same fp32 state; n covers the n % 4 tails, the
    vector body and (3*2^20+3) a second grid-stride pass; the bf16 shadow is the RNE of p bit for bit.  The bound of p also rejects p
    moved along the previous first moment and (t <= 5, where 1 - beta2^t is far from 1) p updated without the v bias correction."""
    ops = _ops()
    lr, b1, b2, eps = 1e-3, 0.9, 0.95, 1e-8
    for n in [1, 2, 3, 4, 5, 1003, 3 * 2 ** 20 + 3]:
        p = _randn(n, n)
        m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        sh = torch.empty(n, dtype=torch.bfloat16, device=DEV) if with_shadow else None
        for step in [1, 2, 3, 4, 5, 1000]:
            g = _randn(n, n * 7 + step, gdt, scale=1e-2 * step if step < 10 else 1e-2)
            p1, m1, v1, e_p, e_m, e_v, w = _adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, gs)
            ops.adamw(p, g, m, v, sh, lr, b1, b2, eps, wd, step, grad_scale=gs)
            _check(m, m1, e_m + U * m1.abs(), w["m"], f"m n={n} step={step}")
            _check(v, v1, e_v + U * v1, w["v"], f"v n={n} step={step}")
            _check(p, p1, e_p, [w["p_oldm"]] + ([w["p_nobc2"]] if step <= 5 else []), f"p n={n} step={step}")
            if with_shadow:
                assert torch.equal(_bits(sh), _bits(p.to(torch.bfloat16))), f"shadow n={n} step={step}"


# ============================================================================================== patchify-MSE
def _seq_target(img):
    B, C, S, P = img.shape
    return img.permute(0, 2, 3, 1).reshape(B, S, P * C)               # 'b c s p -> b s (p c)'


def _patch_cases():
    w = _wl("mae_vit_l16_224")
    return [("2d", torch.bfloat16, w["batch"], 3, (w["img"], w["img"]), w["patch"], w["mask_ratio"], 1.0),
            ("2d", torch.float32, 5, 3, (32, 48), 8, 0.0, 0.5), ("2d", torch.bfloat16, 3, 2, (24, 16), 4, 0.5, 1.0),
            ("3d", torch.float32, 2, 2, (16, 24, 32), 8, 0.75, 1.0), ("3d", torch.bfloat16, 3, 3, (8, 8, 16), 4, 0.0, 0.25),
            ("seq", torch.float32, 4, 3, (196, 64), None, 0.75, 1.0), ("seq", torch.bfloat16, 2, 2, (50, 27), None, 0.0, 2.0)]


@pytest.mark.parametrize("kind,dtype,B,C,sp,p,ratio,gs", _patch_cases())
def test_patch_mse_vs_fp64(kind, dtype, B, C, sp, p, ratio, gs):
    """nd = 2, 3 and the token-sequence target (nd = 1) with C > 1; masked and unmasked; targets from oracle.ucf_vit_ref.patchify.
    Loss: per-thread chains of ceil(total / (256 nb)) terms, an 8-level LDS tree, a chain over the nb <= 1024 partials (the MAE
    size reaches the cap).  dpred: 2 gs / (P sum(mask)) in fp32 (3 roundings) times (pred - target) (1 rounding) and the mask.
    Wrong references: the target with two patch axes swapped (3-D: pw and pd; 2-D: ph and pw; sequence: (c p) for (p c))."""
    from oracle import ucf_vit_ref as R
    ops = _ops()
    img = _randn((B, C) + tuple(sp), B + C, torch.float32)
    if kind == "seq":
        tgt, tgt_w = _seq_target(img), img.permute(0, 2, 1, 3).reshape(B, sp[0], C * sp[1])
    elif kind == "2d":
        tgt = R.patchify(img, p, twoD=True)
        tgt_w = R.patchify(img.transpose(2, 3), p, twoD=True).view(B, sp[1] // p, sp[0] // p, -1).transpose(1, 2).reshape(tgt.shape)
    else:
        tgt = R.patchify(img, p, twoD=False)
        tgt_w = R.patchify(img.transpose(3, 4), p, twoD=False).view(B, sp[0] // p, sp[2] // p, sp[1] // p, -1).transpose(2, 3).reshape(tgt.shape)
    L, P = tgt.shape[1], tgt.shape[2]
    pred = (tgt + 0.1 * _randn(tgt.shape, 3)).to(dtype)
    mask = None
    if ratio:
        _, ids_restore = _shuffle(B, L, 5)
        mask = (ids_restore >= L - int(L * ratio)).float()
    loss, dpred = ops.patch_mse(pred, img, p, mask, grad_scale=gs)
    t64, pr64 = tgt.double(), pred.double()
    m64 = mask.double()[:, :, None] if mask is not None else torch.ones((B, L, 1), dtype=torch.float64, device=DEV)
    denom = (P * m64.sum()).item()
    total = B * L * P
    nb = max(1, min(1024, -(-total // (256 * 64))))
    h = -(-total // (256 * nb)) + 8 + nb + 6

    def lossof(t):
        return ((pr64 - t) ** 2 * m64).sum() / denom
    ref = lossof(t64)
    tol_l = h * U * ((pr64 - t64) ** 2 * m64).sum() / denom + 4 * U * ref.abs()
    last = torch.ones(total, dtype=torch.float64, device=DEV)
    last[torch.arange(total, device=DEV) % (256 * nb) >= 256 * (nb - 1)] = 0      # wrong: the last partial workgroup left out
    wrong_l = ((pr64 - t64) ** 2 * m64 * last.view(B, L, P)).sum() / denom
    _check(loss.view(1), ref.view(1), tol_l.view(1), [lossof(tgt_w.double()).view(1), wrong_l.view(1)], "loss")
    dref = 2 * gs * (pr64 - t64) * m64 / denom
    tol_d = 8 * U * dref.abs() + (UB * dref.abs() * (1 + 8 * U) if dtype == torch.bfloat16 else 0)
    _check(dpred, dref, tol_d, 2 * gs * (pr64 - tgt_w.double()) * m64 / denom, "dpred")


# ============================================================================================== cross-entropy
@pytest.mark.parametrize("dtype,B,C", [(torch.bfloat16, 257, 1), (torch.bfloat16, 300, 2), (torch.float32, 129, 63), (torch.bfloat16, 513, 64),
                                       (torch.bfloat16, 77, 65), (torch.float32, 37, 1000), (torch.bfloat16, 1330, 1000)])
def test_cross_entropy_vs_fp64(dtype, B, C):
    """logits uniform in [-80, 80], grad_scale = 0.75.  t = x - max is rounded (fp32 logits), which moves exp(t) by u |t| relative; exp is
    within 4 ulp; the normaliser is a positive sum of depth ceil(C/64) + 6; log within 2 ulp; two fp32 subtractions.  Loss: an ordered
    sum of depth ceil(B/256) + 8 times 1/B.  dlogits = gs/B (p - onehot); p below 2^-120 may come out as 0 (fp32 exp underflows).
    Wrong references: the label one class off; the loss without the last row.  C = 1: loss and dlogits are exactly 0."""
    ops = _ops()
    gs = 0.75
    x = (torch.rand((B, C), generator=_gen(B + C), device=DEV) * 160 - 80).to(dtype)
    lab = torch.randint(0, C, (B,), generator=_gen(B), device=DEV)
    loss, dl, rows = ops.cross_entropy(x, lab, grad_scale=gs)
    if C == 1:
        assert float(loss) == 0.0 and bool((dl.float() == 0).all())
        return
    x64 = x.double()
    mx = x64.max(1, keepdim=True).values
    s = torch.exp(x64 - mx).sum(1, keepdim=True)
    pr = torch.exp(x64 - mx) / s
    lse = mx + torch.log(s)
    row = (lse - x64.gather(1, lab[:, None]))[:, 0]
    lab_w = (lab + 1) % C
    h = -(-C // 64) + 6
    e_s = (h + 6) * U + U * (pr * (x64 - mx).abs()).sum(1, keepdim=True)        # relative error of the normaliser
    e_row = e_s[:, 0] + 2 * U * (torch.log(s).abs() + mx.abs() + lse.abs())[:, 0] + 2 * U * row.abs()
    row_w = (lse - x64.gather(1, lab_w[:, None]))[:, 0]
    _check(rows, row, e_row, row_w, "row loss")
    ref = row.sum() / B
    tol = (-(-B // 256) + 10) * U * row.abs().sum() / B + e_row.sum() / B
    _check(loss.view(1), ref.view(1), tol.view(1), [(row[:-1].sum() / B).view(1), (row_w.sum() / B).view(1)], "loss")
    y = torch.nn.functional.one_hot(lab, C).double()
    k = gs / B
    dref = k * (pr - y)
    t = k * (pr * (e_s + ((x64 - mx).abs() + 8) * U) + 2 * U * (pr - y).abs() + 2.0 ** -120)
    dw = k * (pr - torch.nn.functional.one_hot(lab_w, C).double())
    _check(dl, dref, t + _out_u(dtype) * (dref.abs() + t), dw, "dlogits")
