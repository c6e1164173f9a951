"""The two stochastic-depth kernels of csrc/drop_path.hip per element against float64, in the manner of tests/test_rowwise_ops.py.

    add  : out[r] = res[r] + s[r // rows_per_sample] * branch[r]          scale: out[r] = s[r // rows_per_sample] * x[r]

Exact tier: keep = 0.5, so s is 0 or 2, and the operands are multiples of 1/4 in [-2, 2]: every product and sum is exact in fp32 and in
bf16, and the column sums (multiples of 1/2, below 2^22 in magnitude even at 131005 rows) are exact whatever the order.  A correct kernel
equals the float64 reference bit for bit.  A dropped sample is never read: add returns the residual's bits and scale returns zeros even
where the dropped rows hold NaN.

Real-valued tier: normal operands, keep = 0.9; the reference sees the same rounded inputs and the same fp32 s.  Arithmetic of the
kernel: t = fl(s * x) in fp32 (or fused into the addition), out = round_out(fl(res + t)).  Bounds, per element, U = 2^-24:
    add  : U |s x| + U |res + s x| + u_out |out|          scale: U |s x| + u_out |out|          (u_out = 2^-8 for bf16, U for fp32)
Column sums of scale: the terms t are summed in fp32 along a tree of depth h, so the error is at most h U sum|s x| with
    h = 1 (the product) + chain of one wave over its rows of a chunk (four rows folded pairwise per step: n_w // 4 + 2 + n_w % 4 with
        n_w = ceil(rows_per_chunk / 4)) + 2 (the 4 waves, pairwise) + ucfvit_reduce_rows over the R chunks (ceil(R / 64) + 2 + 16 + 1, as in
        tests/test_rowwise_ops.py).
Every bound is also shown to reject a plausibly wrong reference: the scale of the neighbouring sample (row r + 1), a last 16-byte vector
of every row that was not processed, and a scale without 1 / keep."""
import pytest
import torch

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
    """dp_chunks of csrc/drop_path.hip"""
    cap = max(64, min(1024, 1024 // -(-D // 512)))
    return max(1, min(-(-rows // 16), cap))


def _colsum_depth(rows, D):
    R = _chunks(rows, D)
    n_w = -(-(-(-rows // R)) // 4)
    return 1 + (n_w // 4 + 2 + n_w % 4) + 2 + (-(-R // 64) + 2 + 16 + 1)


def _scales(B, kept_value, pattern):
    """pattern 'mixed': sample i dropped when i % 3 == 1, except the last sample, which is kept (the wrong reference that misses the last
    row must differ); 'none': all kept; 'all': all dropped"""
    i = torch.arange(B, device=DEV)
    keep = {"mixed": (i % 3 != 1) | (i == B - 1), "none": i >= 0, "all": i < 0}[pattern]
    return keep.float() * torch.tensor(kept_value, dtype=torch.float32, device=DEV)


def _rows(s, rps):
    return s.double().repeat_interleave(rps)[:, None]


def _strided(make, rows, D, seed, dtype):
    """a [rows, D] view with row stride 3 D (the middle third of a [rows, 3 D] buffer)"""
    return make((rows, 3 * D), seed, dtype)[:, D:2 * D]


def _colsum_of_scale(ops, x, s, rps, **kw):
    cs = torch.empty(x.shape[1], device=DEV)
    out = ops.drop_path_scale(x, s, rps, c_colsum=cs, **kw)
    return out, cs


SHAPES = [(B, rps, D) for B in (1, 3, 8) for rps in (1, 5, 197) for D in (64, 100, 192, 1024)]
DTYPES = [torch.bfloat16, torch.float32]
IDS = [f"B{B}-rps{r}-D{D}" for B, r, D in SHAPES]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,rps,D", SHAPES, ids=IDS)
def test_exact_tier(B, rps, D, dtype):
    ops = _ops()
    rows = B * rps
    from UCF_VIT._hip import lib
    assert lib.load().ucfvit_drop_path_colsum_rows(rows, rps, D) == _chunks(rows, D)
    res, br = _quarters((rows, D), 1, dtype), _quarters((rows, D), 2, dtype)
    res_s = _strided(_quarters, rows, D, 3, dtype)
    for pattern in ("mixed", "none", "all"):
        s = _scales(B, 2.0, pattern)
        sr = _rows(s, rps)
        dropped = (sr == 0).expand(rows, D)
        # add: separate output, strided residual, and in place over the branch
        out = ops.drop_path_add(res, br, s, rps, out=torch.empty_like(br))
        assert out.dtype == dtype and torch.equal(out.double(), res.double() + sr * br.double())
        out = ops.drop_path_add(res_s, br.clone(), s, rps)
        assert torch.equal(out.double(), res_s.double() + sr * br.double())
        # dropped rows of the branch hold NaN: the residual comes through bit for bit, the kept rows are untouched by it
        brn = torch.where(dropped, torch.full_like(br, float("nan")), br)
        out = ops.drop_path_add(res, brn, s, rps)
        assert out.data_ptr() == brn.data_ptr()
        assert torch.equal(out.double(), res.double() + sr * br.double())
        assert torch.equal(_bits(out)[dropped], _bits(res)[dropped])
        # scale, with column sums
        out, cs = _colsum_of_scale(ops, torch.where(dropped, torch.full_like(br, float("nan")), br), s, rps)
        want = sr * br.double()
        assert torch.equal(out.double(), want) and not bool(torch.isnan(out).any())
        assert torch.equal(_bits(out)[dropped], torch.zeros_like(_bits(out)[dropped]))
        assert torch.equal(cs.double(), want.sum(0))
        acc0 = _quarters((D,), 7, torch.float32)
        cs2 = acc0.clone()
        ops.drop_path_scale(br, s, rps, c_colsum=cs2, c_colsum_accumulate=True)
        assert torch.equal(cs2.double(), acc0.double() + want.sum(0))
        assert torch.equal(ops.drop_path_scale(br.clone(), s, rps).double(), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,rps,D", SHAPES, ids=IDS)
def test_real_valued_tier(B, rps, D, dtype):
    ops = _ops()
    rows = B * rps
    epv = 8 if dtype == torch.bfloat16 else 4
    uo = _out_u(dtype)
    kept = (torch.ones(1) / KEEP).item()                               # 1 / keep as the module forms it: an fp32 division
    s = _scales(B, kept, "mixed")
    sr = _rows(s, rps)
    res, x = _randn((rows, D), 11, dtype), _randn((rows, D), 12, dtype)
    res_s = _strided(_randn, rows, D, 13, dtype)
    x64 = x.double()
    last = slice(D - (D % epv or epv), D)                             # the last (partial) 16-byte vector of a row

    def wrongs(f):
        """f(scale rows, processed mask) -> the reference under that scale; processed = False: the element was never written (0 here)"""
        w = [("no 1/keep", f((sr != 0).double()))]
        if B > 1:
            w.append(("neighbour's scale", f(_rows(s, rps).roll(-1, 0))))
        return w

    for r in (res, res_s):
        r64 = r.double()
        ref = r64 + sr * x64
        tol = U * (sr * x64).abs() + U * ref.abs() + uo * ref.abs()
        got = ops.drop_path_add(r, x.clone(), s, rps)
        unprocessed = ref.clone()
        unprocessed[:, last] = x64[:, last]                           # in place over the branch: an unprocessed vector still holds the branch
        _check(got, ref, tol, wrongs(lambda q: r64 + q * x64) + [("last vector not processed", unprocessed)], f"add {B}x{rps}x{D}")
    ref = sr * x64
    tol = U * ref.abs() + uo * ref.abs()
    got, cs = _colsum_of_scale(ops, x, s, rps)
    unprocessed = ref.clone()
    unprocessed[:, last] = 0.0
    _check(got, ref, tol, wrongs(lambda q: q * x64) + [("last vector not processed", unprocessed)], f"scale {B}x{rps}x{D}")
    ctol = _colsum_depth(rows, D) * U * ref.abs().sum(0)
    _check(cs, ref.sum(0), ctol, [("no 1/keep", ((sr != 0).double() * x64).sum(0)), ("last row missing", ref[:-1].sum(0))]
           + ([("neighbour's scale", (_rows(s, rps).roll(-1, 0) * x64).sum(0))] if B > 1 else []), f"scale colsum {B}x{rps}x{D}")
    # determinism: the same bits on a second call, column sums included
    got2, cs2 = _colsum_of_scale(ops, x, s, rps)
    assert torch.equal(_bits(got), _bits(got2)) and torch.equal(_bits(cs), _bits(cs2))
    a1 = ops.drop_path_add(res, x.clone(), s, rps)
    a2 = ops.drop_path_add(res, x.clone(), s, rps)
    assert torch.equal(_bits(a1), _bits(a2))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_pointers_off_16_byte_alignment_take_the_element_path(dtype):
    """D allows vectors, the pointers do not: operands one element into a flat buffer"""
    ops = _ops()
    B, rps, D = 3, 5, 192
    rows = B * rps
    off = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)
    s = _scales(B, 2.0, "mixed")
    sr = _rows(s, rps)
    res, br = off(_quarters((rows, D), 1, dtype)), off(_quarters((rows, D), 2, dtype))
    assert res.data_ptr() % 16 != 0 and br.data_ptr() % 16 != 0
    want = res.double() + sr * br.double()
    assert torch.equal(ops.drop_path_add(res, br, s, rps, out=torch.empty_like(res)).double(), want)
    out, cs = _colsum_of_scale(ops, br, s, rps, out=off(torch.empty_like(br)))
    assert torch.equal(out.double(), sr * br.double()) and torch.equal(cs.double(), (sr * br.double()).sum(0))


def test_vit_l_stream_the_grid_loops():
    """[665 x 197, 1024] bf16: 512 row chunks of 256 rows, every wave loops 64 times; exact tier, compared in fp32 (exact for these operands)"""
    ops = _ops()
    B, rps, D = 665, 197, 1024
    rows = B * rps
    assert _chunks(rows, D) == 512
    s = _scales(B, 2.0, "mixed")
    sr = s.repeat_interleave(rps)[:, None]
    res, br = _quarters((rows, D), 1, torch.bfloat16), _quarters((rows, D), 2, torch.bfloat16)
    want = sr * br.float()
    out, cs = _colsum_of_scale(ops, br, s, rps)
    assert torch.equal(out.float(), want)
    assert torch.equal(cs.double(), want.sum(0, dtype=torch.float64))
    want += res.float()
    out = ops.drop_path_add(res, br, s, rps)
    assert out.data_ptr() == br.data_ptr() and torch.equal(out.float(), want)


def test_cpu_tensors_and_bad_shapes_are_refused():
    ops = _ops()
    x = torch.zeros(10, 64)
    s = torch.ones(2)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ops.drop_path_scale(x, s, 5)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ops.drop_path_add(x, x.clone(), s, 5)
    xd, sd = x.to(DEV), s.to(DEV)
    with pytest.raises(ValueError, match="not a multiple"):
        ops.drop_path_scale(xd, sd, 3)
    with pytest.raises(TypeError, match="rows / rows_per_sample"):
        ops.drop_path_scale(xd, sd, 2)
    with pytest.raises(TypeError):
        ops.drop_path_scale(xd, sd.double(), 5)
