"""The two LayerScale kernels of csrc/layer_scale.hip per element against float64, in the manner of tests/test_drop_path_ops.py (whose
helpers' logic is copied here) with the mask of tests/dropout_ref.py.

    add : out[r][c] = res[r][c] + f_r m(r,c) (gamma[c] branch[r][c])              f_r = s[r // rows_per_sample] / keep, missing factors 1
    grad: g = f_r m dy;  dbranch = gamma g;  colsum[c] = sum_r gamma g;  gsum[c] = sum_r g branch

Exact tier: s is 0 or 2, p = 0.5 (1 / keep = 2 exactly), gamma is a signed power of two in {1/2, 1, 2}, the operands are multiples of 1/4
in [-2, 2] (1/4 in [-1, 1] for the large case).  Every product is then a multiple of 1/32 below 64 and every sum of such terms stays below
2^24 units, so products, sums and column sums are exact in fp32 whatever the order, and the results fit bf16's 8 significant bits.  The test
does not take that on trust: it asserts that the float64 reference survives a round trip through the output type (through fp32 for the
sums, together with the unit count) and then requires equality.  NaN in dropped samples and under the mask must leave no trace.

Real-valued tier: normal operands, gamma = 0.5 + 0.3 randn, keep = 0.9, p in {0, 0.1}; the reference sees the same rounded inputs, the same
fp32 gamma and the same fp32 f_r = fl(s * fl(1 / (1 - p))).  Arithmetic of the kernel: u = fl(gamma b), t = fl(f u), out = round(fl(res + t))
(the add possibly fused with the product before it, which only removes a rounding).  Bounds per element, U = 2^-24, u_out = 2^-8 (bf16) | U:
    add    : 2 U |f gamma b| + U |res + f gamma b| + u_out |out|      + 4 u_out U (|f gamma b| + |out|)     (second order)
    dbranch: 2 U |gamma g| + u_out |dbranch|                          + 4 u_out U |gamma g|
    sums   : h U sum|term| (1 + h U),  h = _colsum_depth (tests/test_drop_path_ops.py: its one product, the wave's chain, the 4 waves, the
             fold over the chunks) + 1 for the second product of either sum (f dy, then times gamma or times b)
Every bound is shown to reject plausibly wrong references: the gamma of the neighbouring column, a last 16-byte vector that was not
processed, dbranch without gamma, gamma sums taken from the scaled branch or including masked elements, the neighbouring sample's scale."""
import functools

import pytest
import torch

import dropout_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
UB = 2.0 ** -8
KEEP = 0.9


def _ops():
    from UCF_VIT._hip import ops
    return ops


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, seed, dtype):
    return torch.randn(shape, generator=_gen(seed), device=DEV, dtype=torch.float32).to(dtype)


def _quarters(shape, seed, dtype, k=8):
    return (torch.randint(-k, k + 1, shape, generator=_gen(seed), device=DEV).float() * 0.25).to(dtype)


def _pow2_gamma(D, seed):
    """signed powers of two in {1/2, 1, 2}"""
    e = torch.randint(-1, 2, (D,), generator=_gen(seed), device=DEV).float()
    sign = torch.randint(0, 2, (D,), generator=_gen(seed + 1), device=DEV).float() * 2 - 1
    return sign * torch.exp2(e)


def _out_u(dtype):
    return UB if dtype == torch.bfloat16 else U


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _within(got, ref, tol):
    return bool(((got.double() - ref).abs() <= tol).all())


def _check(got, ref, tol, wrong, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, "
                                 f"worst excess {float((err - tol)[bad].max()):.3e}")
    for name, w in wrong:
        assert not _within(got, w, tol), f"{what}: the bound does not reject the wrong reference '{name}'"


def _chunks(rows, D):
    """dp_chunks of csrc/row_pass.h"""
    cap = max(64, min(1024, 1024 // -(-D // 512)))
    return max(1, min(-(-rows // 16), cap))


def _colsum_depth(rows, D):
    R_ = _chunks(rows, D)
    n_w = -(-(-(-rows // R_)) // 4)
    return 1 + (n_w // 4 + 2 + n_w % 4) + 2 + (-(-R_ // 64) + 2 + 16 + 1)


def _scales(B, kept_value, pattern):
    """'mixed': sample i dropped when i % 3 == 1, except the last sample, which is kept; 'none': all kept; 'all': all dropped"""
    i = torch.arange(B, device=DEV)
    keep = {"mixed": (i % 3 != 1) | (i == B - 1), "none": i >= 0, "all": i < 0}[pattern]
    return keep.float() * torch.tensor(kept_value, dtype=torch.float32, device=DEV)


def _rows(s, rps):
    return s.double().repeat_interleave(rps)[:, None]


def _strided(make, rows, D, seed, dtype):
    """a [rows, D] view with row stride 3 D (the middle third of a [rows, 3 D] buffer)"""
    return make((rows, 3 * D), seed, dtype)[:, D:2 * D]


@functools.lru_cache(maxsize=None)
def _mask_cpu(seed, rows, D, p, row_step):
    return torch.from_numpy(R.keep_mask(seed, rows, D, p, row_step))


def _mask(seed, rows, D, p, row_step=1):
    """float64 [rows, D], 1 = kept (all ones for p == 0), computed once per shape on the host"""
    if p == 0.0:
        return torch.ones(rows, D, dtype=torch.float64, device=DEV)
    return _mask_cpu(seed, rows, D, p, row_step).to(DEV).double()


def _factor(s, p):
    """f per sample as the kernel forms it in fp32; s None: the quotient alone"""
    inv = torch.tensor(R.inv_keep(p) if p > 0.0 else 1.0, dtype=torch.float32, device=DEV)
    return s * inv if s is not None else inv


def _survives(t64, dtype):
    return torch.equal(t64.to(dtype).double(), t64)


def _sum_is_exact(terms64, unit):
    """all terms are multiples of `unit` and their absolute sum stays below 2^24 units: every partial sum is exact in fp32 in any order"""
    k = terms64 / unit
    return bool((k == k.round()).all()) and float(terms64.abs().sum(0).max()) / unit < 2.0 ** 24 and _survives(terms64.sum(0), torch.float32)


def _grad(ops, dy, br, gamma, **kw):
    D = dy.shape[1]
    cs, gs = torch.empty(D, device=DEV), torch.empty(D, device=DEV)
    out = ops.layer_scale_grad(dy, br, gamma, c_colsum=cs, c_gamma=gs, **kw)
    return out, cs, gs


SHAPES = [(B, rps, D) for B in (1, 3, 8) for rps in (1, 5, 197) for D in (64, 70, 100, 192, 1024)]
DTYPES = [torch.bfloat16, torch.float32]
IDS = [f"B{B}-rps{r}-D{D}" for B, r, D in SHAPES]


def _exact_case(ops, dtype, B, rps, D, p, seed, with_s, patterns, k=8, res_kinds=("dense", "strided", "none")):
    rows = B * rps
    gamma = _pow2_gamma(D, 5)
    g64 = gamma.double()[None, :]
    res, br, dy = (_quarters((rows, D), i, dtype, k) for i in (1, 2, 4))
    res_s = _strided(functools.partial(_quarters, k=k), rows, D, 3, dtype)
    m = _mask(seed, rows, D, p)
    nan = torch.full_like(br, float("nan"))
    kw = dict(rows_per_sample=rps, p=p, seed=seed)
    for pattern in patterns:
        s = _scales(B, 2.0, pattern) if with_s else None
        f = _rows(_factor(s, p).expand(B), rps)
        live = (f != 0) & (m != 0)                                    # where the kernel may read its operands
        dead = ~live.expand(rows, D)
        for kind in res_kinds:
            r = {"dense": res, "strided": res_s, "none": None}[kind]
            want = f * m * (g64 * br.double()) + (0.0 if r is None else r.double())
            assert _survives(want, dtype), "precondition: the reference is representable in the output type"
            out = ops.layer_scale_add(r, br, gamma, s=s, out=torch.empty_like(br), **kw)
            assert out.dtype == dtype and torch.equal(out.double(), want), (pattern, kind)
        # NaN in dropped samples and under the mask; in place over the branch
        brn = torch.where(dead, nan, br)
        want = res.double() + f * m * (g64 * br.double())
        out = ops.layer_scale_add(res, brn.clone(), gamma, s=s, **kw)
        assert torch.equal(out.double(), want)
        row_dead = (f == 0).expand(rows, D)
        assert torch.equal(_bits(out)[row_dead], _bits(res)[row_dead])          # a dropped row: the residual's own bits
        out = ops.layer_scale_add(None, brn.clone(), gamma, s=s, **kw)
        assert torch.equal(_bits(out)[row_dead], torch.zeros_like(_bits(out)[row_dead]))
        # backward
        g = f * m * dy.double()
        want_d, term_g = g64 * g, g * br.double()
        assert _survives(want_d, dtype) and _sum_is_exact(want_d, 2.0 ** -5) and _sum_is_exact(term_g, 2.0 ** -5), "precondition"
        dyn = torch.where(dead, nan, dy)
        out, cs, gs = _grad(ops, dyn, brn, gamma, s=s, **kw)
        assert out.dtype == dtype and torch.equal(out.double(), want_d) and not bool(torch.isnan(out).any())
        assert torch.equal(_bits(out)[row_dead], torch.zeros_like(_bits(out)[row_dead]))
        assert torch.equal(cs.double(), want_d.sum(0)) and torch.equal(gs.double(), term_g.sum(0))
        # accumulate flags, one sum at a time, no branch without the gamma sums
        acc0 = _quarters((D,), 7, torch.float32)
        cs2, gs2 = acc0.clone(), acc0.clone()
        ops.layer_scale_grad(dy, None, gamma, s=s, c_colsum=cs2, c_colsum_accumulate=True, **kw)
        ops.layer_scale_grad(dy, br, gamma, s=s, c_gamma=gs2, c_gamma_accumulate=True, **kw)
        assert torch.equal(cs2.double(), acc0.double() + want_d.sum(0)) and torch.equal(gs2.double(), acc0.double() + term_g.sum(0))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,rps,D", SHAPES, ids=IDS)
def test_exact_tier(B, rps, D, dtype):
    ops = _ops()
    assert R.inv_keep(0.5) == 2.0
    _exact_case(ops, dtype, B, rps, D, 0.5, 77 + D, True, ("mixed", "none", "all"))        # s in {0, 2}, mask, f in {0, 4}
    _exact_case(ops, dtype, B, rps, D, 0.0, 0, True, ("mixed",))                           # s alone
    _exact_case(ops, dtype, B, rps, D, 0.5, 78 + D, False, ("none",))                      # the mask alone, f = 2
    _exact_case(ops, dtype, B, rps, D, 0.0, 0, False, ("none",))                           # gamma alone: no row factor at all


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_class_row_tail_geometry(dtype):
    """ldr = N D, row_step = N, rows_per_sample = 1: the residual is the class rows of the stream read in place, and row b draws the mask of
    dense row b N"""
    ops = _ops()
    B, N, D, p, seed = 6, 7, 192, 0.5, 91
    gamma = _pow2_gamma(D, 5)
    stream = _quarters((B, N, D), 1, dtype)
    res = stream[:, 0]
    assert res.stride(0) == N * D
    br, dy = _quarters((B, D), 2, dtype), _quarters((B, D), 4, dtype)
    s = _scales(B, 2.0, "mixed")
    dense_mask = _mask(seed, B * N, D, p)
    m = _mask(seed, B, D, p, row_step=N)
    assert torch.equal(m, dense_mask.view(B, N, D)[:, 0]) and not torch.equal(m, dense_mask[:B])
    f = _rows(_factor(s, p), 1)
    g64 = gamma.double()[None, :]
    want = res.double() + f * m * (g64 * br.double())
    assert _survives(want, dtype)
    kw = dict(s=s, rows_per_sample=1, p=p, seed=seed, row_step=N)
    assert torch.equal(ops.layer_scale_add(res, br.clone(), gamma, **kw).double(), want)
    g = f * m * dy.double()
    out, cs, gs = _grad(ops, dy, br, gamma, **kw)
    assert torch.equal(out.double(), g64 * g)
    assert torch.equal(cs.double(), (g64 * g).sum(0)) and torch.equal(gs.double(), (g * br.double()).sum(0))


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["p0", "p0.1"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,rps,D", SHAPES, ids=IDS)
def test_real_valued_tier(B, rps, D, dtype, p):
    _real_case(B, rps, D, dtype, p, 0.5 + 0.3 * torch.randn(D, generator=_gen(20), device=DEV))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_default_init_gamma_meets_the_same_bounds(dtype):
    """gamma = 1e-5 everywhere (the default init_values): the gamma sums do not depend on gamma's size and must meet the same bound.  All
    columns share one gamma, so there is no neighbouring column to confuse, and next to a residual of order 1 the whole branch is below
    the rounding of the sum: the forward pass is judged without the residual, where the bound is relative to the branch itself"""
    _real_case(3, 5, 192, dtype, 0.1, torch.full((192,), 1e-5, device=DEV), tiny=True)


def _real_case(B, rps, D, dtype, p, gamma, tiny=False):
    neighbour_gamma = not tiny
    ops = _ops()
    rows = B * rps
    seed = 0xDEADBEEF00000000 + D
    epv = 8 if dtype == torch.bfloat16 else 4
    uo = _out_u(dtype)
    kept = (torch.ones(1) / KEEP).item()
    s = _scales(B, kept, "mixed")
    f = _rows(_factor(s, p), rps)
    f_next = _rows(_factor(s, p), rps).roll(-1, 0)
    m = _mask(seed, rows, D, p)
    g64 = gamma.double()[None, :]
    g64_next = g64.roll(1, 1)
    res, x, dy = _randn((rows, D), 11, dtype), _randn((rows, D), 12, dtype), _randn((rows, D), 14, dtype)
    res_s = _strided(_randn, rows, D, 13, dtype)
    x64, dy64 = x.double(), dy.double()
    last = slice(D - (D % epv or epv), D)                             # the last (partial) 16-byte vector of a row
    kw = dict(s=s, rows_per_sample=rps, p=p, seed=seed)
    what = f"{B}x{rps}x{D} p={p}"

    # forward
    for r in ((None,) if tiny else (res, res_s, None)):
        r64 = 0.0 if r is None else r.double()
        t = f * m * g64 * x64
        ref = r64 + t
        tol = 2 * U * t.abs() + U * ref.abs() + uo * ref.abs() + 4 * uo * U * (t.abs() + ref.abs())
        got = ops.layer_scale_add(r, x.clone(), gamma, **kw)           # in place over the branch
        unprocessed = ref.clone()
        unprocessed[:, last] = x64[:, last]                           # an unprocessed vector still holds the branch
        wrong = [("last vector not processed", unprocessed), ("no gamma", r64 + f * m * x64)]
        if neighbour_gamma:
            wrong.append(("gamma of the neighbouring column", r64 + f * m * g64_next * x64))
        if B > 1:
            wrong.append(("neighbour's scale", r64 + f_next * m * g64 * x64))
        if p > 0:
            wrong.append(("no mask", r64 + f * g64 * x64))
        _check(got, ref, tol, wrong, "add " + what)

    # backward
    g = f * m * dy64
    ref = g64 * g
    tol = 2 * U * ref.abs() + uo * ref.abs() + 4 * uo * U * ref.abs()
    got, cs, gs = _grad(ops, dy, x, gamma, **kw)
    unprocessed = ref.clone()
    unprocessed[:, last] = 0.0
    wrong = [("last vector not processed", unprocessed), ("dbranch without gamma", g)]
    if neighbour_gamma:
        wrong.append(("gamma of the neighbouring column", g64_next * g))
    if B > 1:
        wrong.append(("neighbour's scale", g64 * (f_next * m * dy64)))
    _check(got, ref, tol, wrong, "dbranch " + what)
    h = _colsum_depth(rows, D) + 1
    ctol = h * U * ref.abs().sum(0) * (1 + h * U)
    wrong = [("last row missing", ref[:-1].sum(0)), ("without gamma", g.sum(0))]
    if neighbour_gamma:
        wrong.append(("gamma of the neighbouring column", (g64_next * g).sum(0)))
    if B > 1:
        wrong.append(("neighbour's scale", (g64 * (f_next * m * dy64)).sum(0)))
    _check(cs, ref.sum(0), ctol, wrong, "colsum " + what)
    term = g * x64
    gtol = h * U * term.abs().sum(0) * (1 + h * U)
    wrong = [("from the scaled branch", (g * g64 * x64).sum(0)), ("last row missing", term[:-1].sum(0))]
    if p > 0:
        wrong.append(("including masked elements", (f * dy64 * x64).sum(0)))
    if B > 1:
        wrong.append(("neighbour's scale", (f_next * m * dy64 * x64).sum(0)))
    _check(gs, term.sum(0), gtol, wrong, "gamma sums " + what)

    # determinism: the same bits on a second call, both sums included; aliasing gives the bits of the out-of-place call
    got2, cs2, gs2 = _grad(ops, dy, x, gamma, **kw)
    assert torch.equal(_bits(got), _bits(got2)) and torch.equal(_bits(cs), _bits(cs2)) and torch.equal(_bits(gs), _bits(gs2))
    dyc = dy.clone()
    got3 = ops.layer_scale_grad(dyc, x, gamma, out=dyc, **kw)
    assert got3.data_ptr() == dyc.data_ptr() and torch.equal(_bits(got3), _bits(got))
    a1 = ops.layer_scale_add(res, x, gamma, out=torch.empty_like(x), **kw)
    a2 = ops.layer_scale_add(res, x, gamma, out=torch.empty_like(x), **kw)
    xc = x.clone()
    a3 = ops.layer_scale_add(res, xc, gamma, **kw)
    assert a3.data_ptr() == xc.data_ptr()
    assert torch.equal(_bits(a1), _bits(a2)) and torch.equal(_bits(a1), _bits(a3))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_element_path_and_vector_path_draw_the_same_mask(dtype):
    """D allows vectors, the pointers of the second run do not (operands one element into a flat buffer): the same logical matrix, the same
    mask, and with exact-tier operands the same bits"""
    ops = _ops()
    B, rps, D, p, seed = 3, 5, 192, 0.5, 1234567
    rows = B * rps
    off = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)
    gamma = _pow2_gamma(D, 5)
    s = _scales(B, 2.0, "mixed")
    res, br, dy = (_quarters((rows, D), i, dtype) for i in (1, 2, 4))
    res_o, br_o, dy_o = off(res), off(br), off(dy)
    assert br.data_ptr() % 16 == 0 and res_o.data_ptr() % 16 != 0 and br_o.data_ptr() % 16 != 0 and dy_o.data_ptr() % 16 != 0
    kw = dict(s=s, rows_per_sample=rps, p=p, seed=seed)
    f, m, g64 = _rows(_factor(s, p), rps), _mask(seed, rows, D, p), gamma.double()[None, :]
    want = res.double() + f * m * (g64 * br.double())
    a = ops.layer_scale_add(res, br, gamma, out=torch.empty_like(br), **kw)
    b = ops.layer_scale_add(res_o, br_o, gamma, out=off(torch.empty_like(br)), **kw)
    assert torch.equal(a.double(), want) and torch.equal(_bits(a), _bits(b))
    ga, csa, gsa = _grad(ops, dy, br, gamma, **kw)
    gb, csb, gsb = _grad(ops, dy_o, br_o, gamma, out=off(torch.empty_like(dy)), **kw)
    assert torch.equal(ga.double(), g64 * (f * m * dy.double())) and torch.equal(_bits(ga), _bits(gb))
    assert torch.equal(csa, csb) and torch.equal(gsa, gsb)


def test_vit_l_stream_the_grid_loops():
    """[665 x 197, 1024] bf16: 512 row chunks of 256 rows, every wave loops 64 times; exact tier (operands in [-1, 1], gamma in {1/2, 1, 2}),
    compared in fp32, which holds these values exactly.  The host restatement of the mask is too slow for 134 M elements: the mask is read
    off ops.dropout applied to ones (tests/test_dropout_ops.py pins that kernel's mask to the restatement bit for bit), and its first and
    last 8 rows are compared with the restatement here."""
    ops = _ops()
    B, rps, D, p, seed = 665, 197, 1024, 0.5, 0xABCDEF0123456789
    rows = B * rps
    assert _chunks(rows, D) == 512
    gamma = _pow2_gamma(D, 5)
    s = _scales(B, 2.0, "mixed")
    f = s.repeat_interleave(rps)[:, None] * 2.0
    m = ops.dropout(torch.ones(rows, D, device=DEV, dtype=torch.bfloat16), p, seed) != 0
    host = lambda r0, n: torch.from_numpy(R.keep_mask(seed, n, D, p, 1, shift=r0 * D)).to(DEV)
    assert torch.equal(m[:8], host(0, 8)) and torch.equal(m[-8:], host(rows - 8, 8))
    res, br = _quarters((rows, D), 1, torch.bfloat16, 4), _quarters((rows, D), 2, torch.bfloat16, 4)
    kw = dict(s=s, rows_per_sample=rps, p=p, seed=seed)
    want = torch.where(m, f * (gamma[None, :] * br.float()), torch.zeros((), device=DEV))
    assert float(want.abs().max()) <= 8.0
    # backward first (br is the branch output, res plays dy); the sums in float64 on the device
    g = torch.where(m, f * res.float(), torch.zeros((), device=DEV))
    out, cs, gs = _grad(ops, res, br, gamma, **kw)
    assert torch.equal(out.float(), gamma[None, :] * g)
    want_cs, want_gs = (gamma[None, :] * g).sum(0, dtype=torch.float64), (g * br.float()).sum(0, dtype=torch.float64)
    abs_gs = (g * br.float()).abs().sum(0, dtype=torch.float64)
    assert float(abs_gs.max()) * 32 < 2.0 ** 24 and float((gamma[None, :] * g).abs().sum(0, dtype=torch.float64).max()) * 32 < 2.0 ** 24
    assert torch.equal(cs.double(), want_cs) and torch.equal(gs.double(), want_gs)
    del out, g
    want += res.float()
    assert torch.equal(want.bfloat16().float(), want)
    out = ops.layer_scale_add(res, br, gamma, **kw)
    assert out.data_ptr() == br.data_ptr() and torch.equal(out.float(), want)


def test_cpu_tensors_and_bad_arguments_are_refused():
    ops = _ops()
    x = torch.zeros(10, 64)
    gamma = torch.ones(64)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ops.layer_scale_add(None, x, gamma)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ops.layer_scale_grad(x, x, gamma)
    xd, gd, sd = x.to(DEV), gamma.to(DEV), torch.ones(2, device=DEV)
    with pytest.raises(ValueError, match="not a multiple"):
        ops.layer_scale_add(None, xd, gd, s=sd, rows_per_sample=3)
    with pytest.raises(TypeError, match="rows / rows_per_sample"):
        ops.layer_scale_add(None, xd, gd, s=sd, rows_per_sample=2)
    with pytest.raises(TypeError, match="gamma must be"):
        ops.layer_scale_add(None, xd, gd.bfloat16())
    with pytest.raises(TypeError, match="gamma must be"):
        ops.layer_scale_grad(xd, xd, gd[:32])
    with pytest.raises(ValueError, match="branch is None"):
        ops.layer_scale_grad(xd, None, gd, c_gamma=torch.empty(64, device=DEV))
    for p in (1.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="0 <= p < 1"):
            ops.layer_scale_add(None, xd, gd, p=p)
    with pytest.raises(ValueError, match="row_step"):
        ops.layer_scale_grad(xd, xd, gd, p=0.5, row_step=0)
    with pytest.raises(TypeError, match="one dtype"):
        ops.layer_scale_add(xd.bfloat16(), xd, gd)
