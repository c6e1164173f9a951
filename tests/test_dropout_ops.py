"""The two dropout kernels of csrc/dropout.hip per element against float64, in the manner of tests/test_drop_path_ops.py, with the mask
restated in numpy from include/ucfvit_hip.h (tests/dropout_ref.py):

    dropout: out[r] = f_r * m[r] * x[r]          dropout_add: out[r] = res[r] + f_r * m[r] * branch[r]
    f_r = fl32(s[r // rows_per_sample] * fl32(1 / (1 - p)))   (s = None: fl32(1 / (1 - p)))

Mask tier: x = 1 (and res = 0) gives out = m / keep bit for bit, over a table of shapes that a host model of the kernel's loops shows to
enter every one of them: the scalar and the 16-byte path, idle lanes, several column blocks, several row chunks, the four-row unrolled
loop (once and again) and the single-row loop behind it, an unaligned base pointer, row_step > 1.

Exact tier: p = 0.5 (1 / keep = 2), s in {0, 2}, operands multiples of 1/4 in [-2, 2]: f is 0 or 4, every product (a multiple of 1,
|.| <= 8) and sum (a multiple of 1/4, |.| <= 10: six significant bits) is exact in fp32 and in bf16, and the column sums (integers far
below 2^24) are exact whatever the order.  A correct kernel equals float64 bit for bit; rows with s == 0 are never read (NaN there).

Real-valued tier: normal operands, p = 0.1, row_step = 5; the reference sees the same rounded inputs and the same fp32 f.  Arithmetic of
the kernel: t = fl(f * x) in fp32 (or fused into the addition), out = round_out(fl(res + t)).  Bounds per element, U = 2^-24:
    add: U |f x| + U |res + f x| + u_out |out|        dropout: U |f x| + u_out |out|        (u_out = 2^-8 for bf16, U for fp32)
Column sums: depth h of the summation tree as in tests/test_drop_path_ops.py (the same geometry), error <= h U sum|f m x|.
Every bound is shown to reject three wrong references: the mask of element i + 1, a missing 1 / keep, and row_step ignored."""
import pytest
import torch

import dropout_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
UB = 2.0 ** -8
DTYPES = [torch.bfloat16, torch.float32]
DT_IDS = ["bf16", "fp32"]


def _ops():
    from UCF_VIT._hip import ops
    return ops


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, seed, dtype):
    return torch.randn(shape, generator=_gen(seed), device=DEV, dtype=torch.float32).to(dtype)


def _quarters(shape, seed, dtype, k=8):
    return (torch.randint(-k, k + 1, shape, generator=_gen(seed), device=DEV).float() * 0.25).to(dtype)


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _mask(seed, rows, D, p, row_step=1, shift=0):
    return torch.from_numpy(R.keep_mask(seed, rows, D, p, row_step, shift)).to(DEV).double()


def _off(t):
    """the same values one element into a flat buffer: no 16-byte alignment"""
    o = torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)
    assert o.data_ptr() % 16 != 0
    return o


def _chunks(rows, D):
    """dp_chunks of csrc/row_pass.h"""
    cap = max(64, min(1024, 1024 // -(-D // 512)))
    return max(1, min(-(-rows // 16), cap))


def _colsum_depth(rows, D):
    Rc = _chunks(rows, D)
    n_w = -(-(-(-rows // Rc)) // 4)
    return 1 + (n_w // 4 + 2 + n_w % 4) + 2 + (-(-Rc // 64) + 2 + 16 + 1)


def _loops_entered(rows, D, dtype, aligned):
    """host model of dropout_kernel's control flow (csrc/dropout.hip): which of its paths and loops a launch enters"""
    epv = 8 if dtype == torch.bfloat16 else 4
    W = epv if (D % epv == 0 and aligned) else 1
    chunks = _chunks(rows, D)
    rpc = -(-rows // chunks)
    seen = {"16-byte path" if W > 1 else "scalar path"}
    lanes = -(-D // W)
    if lanes % 64:
        seen.add("idle lanes")
    if lanes > 64:
        seen.add("column blocks")
    if chunks > 1:
        seen.add("row chunks")
    for chunk in range(chunks):
        r0, r1 = chunk * rpc, min(rows, chunk * rpc + rpc)
        for wave in range(4):
            r, n = r0 + wave, 0
            while r + 12 < r1:
                r, n = r + 16, n + 1
            if n >= 1:
                seen.add("unrolled loop")
            if n >= 2:
                seen.add("unrolled loop again")
            if r < r1:
                seen.add("single-row loop")
            if r + 4 < r1:
                seen.add("single-row loop again")
    return seen


EVERY_LOOP = {"16-byte path", "scalar path", "idle lanes", "column blocks", "row chunks", "unrolled loop", "unrolled loop again",
              "single-row loop", "single-row loop again"}
# rows, D, dtypes, row_step, aligned base
MASK_TABLE = [
    (1, 1, DTYPES, 1, True), (3, 5, DTYPES, 1, True),                       # scalar path
    (5, 8, [torch.bfloat16], 1, True), (7, 4, [torch.float32], 1, True),    # one vector per row
    (37, 200, DTYPES, 1, True),                                             # lanes idle
    (37, 201, DTYPES, 1, True),                                             # the scalar path over several column blocks and row chunks
    (130, 1032, DTYPES, 1, True),                                           # more than one column block
    (9, 64, DTYPES, 1, False),                                              # base pointer one element off
    (6, 24, DTYPES, 5, True),                                               # row_step
    (2565, 8200, DTYPES, 1, True),                                          # 64 chunks of 41 rows: the unrolled loop twice, then single rows
]
MASK_CASES = [(rows, D, dt, step, al) for rows, D, dts, step, al in MASK_TABLE for dt in dts]


def test_the_mask_table_enters_every_loop():
    seen = set()
    for rows, D, dt, _, aligned in MASK_CASES:
        seen |= _loops_entered(rows, D, dt, aligned)
    assert seen == EVERY_LOOP
    assert _loops_entered(2565, 8200, torch.bfloat16, True) >= {"unrolled loop again", "single-row loop again", "row chunks", "column blocks"}
    assert _loops_entered(9, 64, torch.float32, False) >= {"scalar path"} and _loops_entered(5, 8, torch.bfloat16, True) >= {"16-byte path"}


@pytest.mark.parametrize("rows,D,dtype,row_step,aligned", MASK_CASES,
                         ids=[f"{r}x{D}-{'bf16' if dt == torch.bfloat16 else 'fp32'}-step{st}{'' if al else '-off1'}" for r, D, dt, st, al in MASK_CASES])
def test_mask_tier(rows, D, dtype, row_step, aligned):
    ops = _ops()
    p, seed = 0.25, 0x0123456789ABCDEF + rows
    from UCF_VIT._hip import lib
    assert lib.load().ucfvit_drop_path_colsum_rows(rows, 1, D) == _chunks(rows, D)          # the geometry the partials are sized by
    m = _mask(seed, rows, D, p, row_step)
    want = (m.float() * torch.tensor(R.inv_keep(p), device=DEV)).to(dtype)
    assert 0 < int(m.sum()) < m.numel() or m.numel() < 4
    ones = torch.ones((rows, D), device=DEV, dtype=dtype)
    x = ones if aligned else _off(ones)
    out = ops.dropout(x, p, seed, row_step=row_step, out=None if aligned else _off(torch.empty_like(ones)))
    assert out.dtype == dtype and torch.equal(_bits(out), _bits(want))
    res = torch.zeros_like(ones)
    out = ops.dropout_add(res if aligned else _off(res), x.clone() if aligned else _off(ones.clone()), p, seed, row_step=row_step)
    assert torch.equal(_bits(out), _bits(want))
    cs = torch.empty(D, device=DEV)
    ops.dropout(x, p, seed, row_step=row_step, c_colsum=cs, out=None if aligned else _off(torch.empty_like(ones)))
    ref = m.sum(0) * R.inv_keep(p)                                   # equal terms fl32(4/3), one rounding per addition of the tree
    assert bool(((cs.double() - ref).abs() <= _colsum_depth(rows, D) * U * ref.abs()).all())


def _scales(B, kept_value, pattern):
    i = torch.arange(B, device=DEV)
    keep = {"mixed": (i % 3 != 1) | (i == B - 1), "none": i >= 0, "all": i < 0}[pattern]
    return keep.float() * torch.tensor(kept_value, dtype=torch.float32, device=DEV)


def _rows(s, rps):
    return s.double().repeat_interleave(rps)[:, None]


def _strided(make, rows, D, seed, dtype):
    return make((rows, 3 * D), seed, dtype)[:, D:2 * D]


SHAPES = [(B, rps, D) for B in (1, 3) for rps in (1, 5) for D in (64, 100, 1032)] + [(8, 197, 192)]
IDS = [f"B{B}-rps{r}-D{D}" for B, r, D in SHAPES]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,rps,D", SHAPES, ids=IDS)
def test_exact_tier(B, rps, D, dtype):
    ops = _ops()
    rows, p, seed = B * rps, 0.5, 77 + D
    assert R.inv_keep(p) == 2.0
    m = _mask(seed, rows, D, p)
    res, br = _quarters((rows, D), 1, dtype), _quarters((rows, D), 2, dtype)
    res_s = _strided(_quarters, rows, D, 3, dtype)
    nan = torch.full_like(br, float("nan"))
    for pattern in ("mixed", "none", "all", None):
        s = _scales(B, 2.0, pattern) if pattern is not None else None
        sr = _rows(s, rps) if s is not None else torch.ones((rows, 1), dtype=torch.float64, device=DEV)
        dropped = (sr == 0).expand(rows, D)
        t = 2.0 * sr * m * br.double()
        # add: separate output, strided residual, in place over the branch; rows with s == 0 hold NaN and return the residual's bits
        out = ops.dropout_add(res, br, p, seed, s=s, rows_per_sample=rps, out=torch.empty_like(br))
        assert out.dtype == dtype and torch.equal(out.double(), res.double() + t)
        out = ops.dropout_add(res_s, br.clone(), p, seed, s=s, rows_per_sample=rps)
        assert torch.equal(out.double(), res_s.double() + t)
        brn = torch.where(dropped, nan, br)
        out = ops.dropout_add(res, brn, p, seed, s=s, rows_per_sample=rps)
        assert out.data_ptr() == brn.data_ptr() and torch.equal(out.double(), res.double() + t)
        assert torch.equal(_bits(out)[dropped], _bits(res)[dropped])
        # dropout with column sums: separate output, accumulate, in place
        cs = torch.empty(D, device=DEV)
        out = ops.dropout(torch.where(dropped, nan, br), p, seed, s=s, rows_per_sample=rps, c_colsum=cs)
        assert torch.equal(out.double(), t) and not bool(torch.isnan(out).any())
        assert torch.equal(_bits(out)[dropped], torch.zeros_like(_bits(out)[dropped]))
        assert torch.equal(cs.double(), t.sum(0))
        acc0 = _quarters((D,), 7, torch.float32)
        cs2 = acc0.clone()
        ops.dropout(br, p, seed, s=s, rows_per_sample=rps, c_colsum=cs2, c_colsum_accumulate=True)
        assert torch.equal(cs2.double(), acc0.double() + t.sum(0))
        x = br.clone()
        assert ops.dropout(x, p, seed, s=s, rows_per_sample=rps, out=x).data_ptr() == x.data_ptr() and torch.equal(x.double(), t)
    # a NaN under the mask of a kept row does not pass: the dropped element is a select, not a product
    brm = torch.where(m == 0, nan, br)
    assert torch.equal(ops.dropout(brm, p, seed).double(), 2.0 * m * br.double())
    assert torch.equal(ops.dropout_add(res, brm, p, seed).double(), res.double() + 2.0 * m * br.double())


def _within(got, ref, tol):
    return bool(((got.double() - ref).abs() <= tol).all())


def _check(got, ref, tol, wrong, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, "
                                 f"worst excess {float((err - tol)[bad].max()):.3e}")
    for name, w in wrong:
        assert not _within(got, w, tol), f"{what}: the bound does not reject the wrong reference '{name}'"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("with_s", [False, True], ids=["no-s", "s"])
@pytest.mark.parametrize("B,rps,D", SHAPES, ids=IDS)
def test_real_valued_tier(B, rps, D, with_s, dtype):
    ops = _ops()
    rows, p, seed, step = B * rps, 0.1, 0xDEADBEEF00000000 + D, 5
    uo = UB if dtype == torch.bfloat16 else U
    inv = torch.tensor(R.inv_keep(p), dtype=torch.float32)
    s = _scales(B, (torch.ones(1) / 0.8).item(), "mixed") if with_s else None
    s_rows = s.cpu().repeat_interleave(rps)[:, None] if with_s else torch.ones((rows, 1))
    f = (s_rows * inv).double().to(DEV)                              # one fp32 product, as in the kernel
    f_nokeep = s_rows.double().to(DEV)
    m = _mask(seed, rows, D, p, step)
    wrong_masks = [("mask of element i + 1", _mask(seed, rows, D, p, step, shift=1))]
    if rows > 1:
        wrong_masks.append(("row_step ignored", _mask(seed, rows, D, p, 1)))
    res, x = _randn((rows, D), 11, dtype), _randn((rows, D), 12, dtype)
    res_s = _strided(_randn, rows, D, 13, dtype)
    x64 = x.double()

    def wrongs(make):
        return [(n, make(f, wm)) for n, wm in wrong_masks] + [("no 1/keep", make(f_nokeep, m))]

    for r in (res, res_s):
        r64 = r.double()
        t = f * m * x64
        ref = r64 + t
        tol = U * t.abs() + U * ref.abs() + uo * ref.abs()
        got = ops.dropout_add(r, x.clone(), p, seed, s=s, rows_per_sample=rps, row_step=step)
        _check(got, ref, tol, wrongs(lambda ff, mm: r64 + ff * mm * x64), f"add {B}x{rps}x{D}")
    ref = f * m * x64
    tol = U * ref.abs() + uo * ref.abs()
    cs = torch.empty(D, device=DEV)
    got = ops.dropout(x, p, seed, s=s, rows_per_sample=rps, row_step=step, c_colsum=cs)
    _check(got, ref, tol, wrongs(lambda ff, mm: ff * mm * x64), f"dropout {B}x{rps}x{D}")
    ctol = _colsum_depth(rows, D) * U * ref.abs().sum(0)
    _check(cs, ref.sum(0), ctol, [(n, w.sum(0)) for n, w in wrongs(lambda ff, mm: ff * mm * x64)], f"dropout colsum {B}x{rps}x{D}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_reproducible_and_seed_dependent(dtype):
    ops = _ops()
    x, res = _randn((37, 200), 1, dtype), _randn((37, 200), 2, dtype)
    cs1, cs2 = torch.empty(200, device=DEV), torch.empty(200, device=DEV)
    a, b = ops.dropout(x, 0.3, 99, c_colsum=cs1), ops.dropout(x, 0.3, 99, c_colsum=cs2)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(cs1), _bits(cs2))
    assert torch.equal(_bits(ops.dropout_add(res, x.clone(), 0.3, 99)), _bits(ops.dropout_add(res, x.clone(), 0.3, 99)))
    c = ops.dropout(x, 0.3, 100)
    assert not torch.equal(a == 0, c == 0)
    assert torch.equal((a == 0).cpu(), torch.from_numpy(~R.keep_mask(99, 37, 200, 0.3)) | (x == 0).cpu())
    # seeds that differ in the high word only are different keys
    assert not torch.equal(a == 0, ops.dropout(x, 0.3, 99 + (1 << 32)) == 0)


def test_bad_arguments_are_refused():
    ops = _ops()
    x = torch.zeros(10, 64, device=DEV)
    for p in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="0 < p < 1"):
            ops.dropout(x, p, 1)
    with pytest.raises(ValueError, match="row_step"):
        ops.dropout(x, 0.5, 1, row_step=0)
    with pytest.raises(ValueError, match="unsigned 64-bit"):
        ops.dropout(x, 0.5, -1)
    with pytest.raises(ValueError, match="not a multiple"):
        ops.dropout(x, 0.5, 1, rows_per_sample=3)
    with pytest.raises(TypeError, match="rows / rows_per_sample"):
        ops.dropout_add(x, x.clone(), 0.5, 1, s=torch.ones(3, device=DEV), rows_per_sample=5)
    with pytest.raises(TypeError):
        ops.dropout_add(x, x.clone().bfloat16(), 0.5, 1)
