"""ucfvit_seg_counts (csrc/seg_metric.hip: the argmax label map and the TP / PRED / LAB counts of a Dice accuracy in one pass) and the metric
arithmetic on top of it (UCF_VIT.utils.metrics.dice_from_counts / DiceMetric), bit for bit: every result of the kernels is an integer, so
there is no tolerance anywhere in this file.

GPU half.  Reference: torch.argmax(dim=1) of the SAME values on the CPU (bf16 logits are widened to fp32 first, which is exact and keeps
NaN, +-inf and every order relation) and integer counts taken with numpy.  test_seg_counts runs the table
    dtype {fp32, bf16} x layout {N C S contiguous, channels-last ld == n, channels-last padded ld = 8 and 16 (NaN in the padding columns)}
    x n {2, 3, 4, 5, 8} x B {1, 3},
and inside each case every S of S_LIST with every operand family of FAMILIES (the four sizes from a chunk upwards: three families each,
rotated over the table; measured on an MI355X: 86 GPU tests in 17.5 s, a case 0.34 s at the most, 0.8 s for whichever runs first).
S_LIST restates the kernels' constants (csrc/seg_metric.hip:
NT = 256 threads, SEG_CHUNK = 16384 voxels per workgroup, SEG_VPT = 8 voxels per lane and step of the N C S kernel, whose workgroup step is
NT x 8 = 2048, and 4 x NT = 1024 voxels per workgroup step of the channels-last kernel; test_route_names_the_constants reads them back from
ucfvit_seg_counts_route): 1, 3, 63, 64, 65, 255, one below / at / one above 8, 1024, 2048 and 16384, and 3 chunks + a step + 5.
Which kernel a case reaches follows from the route rules (restated in _expected_route and asserted against the library for every case):
the vector kernels need aligned bases and strides, so e.g. N C S with odd S or channels-last with ld = 3 runs the scalar kernel, and the
cases whose logits start one element into their allocation (test_offset_pointer_takes_the_scalar_kernel) must be refused by both.
Per call: pred equals argmax bit for bit, counts [B][3][8] equal the numpy counts including the zeros of the classes >= n, the call without
a prediction buffer gives the same counts, a second call repeats both.

Operand families: normal logits; logits from {-1, 0, 1} (most voxels tie: the first maximal class decides); all-equal logits (class 0
everywhere); rows with NaN, +inf, -inf in chosen classes (a NaN beats +inf, the first NaN wins, a row of -inf is a tie); labels uniform over
the classes, with class n - 1 absent (NaN Dice), all background, and with -1, n, 8 and 2^32 + 1 among them (no LAB / TP entry; the last
must not alias class 1).

Host half (no GPU): the argument checks through lib.load(), the workspace size, dice_from_counts / DiceMetric on CPU tensors against a plain
restatement of monai's ignore_empty Dice and MEAN reduction (monai is not installed: parity with it is unpinned), and dice_from_counts(group=)
over two gloo ranks."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT

DEV = "cuda"
NT, SEG_CHUNK, SEG_VPT = 256, 16384, 8          # csrc/seg_metric.hip
NCS_STEP, CL_STEP = NT * SEG_VPT, 4 * NT
S_LIST = [1, 3, 7, 8, 9, 63, 64, 65, 255, CL_STEP - 1, CL_STEP, CL_STEP + 1, NCS_STEP - 1, NCS_STEP, NCS_STEP + 1, SEG_CHUNK - 1, SEG_CHUNK,
          SEG_CHUNK + 1, 3 * SEG_CHUNK + NCS_STEP + 5]
FAMILIES = [("normal", "uniform"), ("ties", "absent"), ("equal", "uniform"), ("special", "outside"), ("normal", "background"),
            ("ties", "outside"), ("special", "absent")]
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------------------- operands and references
def make_logits(kind, B, n, S, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "normal":
        return torch.randn(B, n, S, generator=g)
    if kind == "ties":
        return torch.randint(-1, 2, (B, n, S), generator=g).float()
    if kind == "equal":
        return torch.full((B, n, S), 0.5)
    x = torch.randn(B, n, S, generator=g)                     # "special": voxel i takes pattern i % 7
    i = torch.arange(S)
    c1, c2 = (i // 7) % n, (i // 7 + 1) % n
    for b in range(B):
        xb = x[b]
        m = i % 7 == 0
        xb[c1[m], i[m]] = NAN                                 # one NaN
        m = i % 7 == 1
        xb[c1[m], i[m]] = NAN                                 # two NaN: the first wins
        xb[c2[m], i[m]] = NAN
        m = i % 7 == 2
        xb[c1[m], i[m]] = INF                                 # +inf, and a NaN that beats it
        xb[c2[m], i[m]] = NAN
        m = i % 7 == 3
        xb[:, i[m]] = -INF                                    # a row of -inf: a tie, class 0
        m = i % 7 == 4
        xb[:, i[m]] = -INF                                    # -inf everywhere but one class
        xb[c1[m], i[m]] = -3.0
        m = i % 7 == 5
        xb[c1[m], i[m]] = INF                                 # two +inf: the first wins
        xb[c2[m], i[m]] = INF
    return x


def make_labels(kind, B, n, S, seed):
    g = torch.Generator().manual_seed(seed + 1)
    if kind == "uniform":
        return torch.randint(0, n, (B, S), generator=g)
    if kind == "absent":
        return torch.randint(0, n - 1, (B, S), generator=g)
    if kind == "background":
        return torch.zeros(B, S, dtype=torch.int64)
    y = torch.randint(0, n, (B, S), generator=g)
    bad = torch.tensor([-1, n, 8, (1 << 32) + 1])
    pick = torch.randint(0, 8, (B, S), generator=g)
    return torch.where(pick < 4, bad[pick.clamp_max(3)], y)


def reference(logits, labels):
    """logits [B, n, S] (CPU, the values the kernel reads), labels [B, S] -> (pred uint8 [B, S], counts int64 [B, 3, 8])"""
    pred = torch.argmax(logits.float(), dim=1).numpy()
    lab = labels.numpy()
    counts = np.zeros((logits.shape[0], 3, 8), dtype=np.int64)
    for c in range(logits.shape[1]):                        # a label in [n, 8) is outside the classes: it counts nowhere, like -1
        counts[:, 0, c] = ((pred == c) & (lab == c)).sum(axis=1)
        counts[:, 1, c] = (pred == c).sum(axis=1)
        counts[:, 2, c] = (lab == c).sum(axis=1)
    return pred.astype(np.uint8), counts


def dice_restated(counts, include_background):
    """monai DiceHelper(ignore_empty=True) on one-hot maps: 2 |pred & y| / (|pred| + |y|) where |y| > 0, else NaN; float64, rounded once"""
    c = counts.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(c[:, 2] > 0, 2.0 * c[:, 0] / (c[:, 1] + c[:, 2]), np.nan)
    return (d if include_background else d[:, 1:]).astype(np.float32)


def mean_restated(per_item_batches):
    """monai do_metric_reduction(MEAN) over the concatenated per-item values: nanmean over the classes of an item, then the mean over the
    items with at least one non-NaN class; (0, 0) when there is none"""
    f = np.concatenate(per_item_batches, axis=0).astype(np.float64)
    ok = ~np.isnan(f)
    k = ok.sum(axis=1)
    item = np.where(k > 0, np.where(ok, f, 0.0).sum(axis=1) / np.maximum(k, 1), 0.0)
    m = int((k > 0).sum())
    return (item.sum() / m if m else 0.0), m


def same_bits(got, want):
    """fp32 arrays equal bit for bit, every NaN standing for every other"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(np.isnan(got), np.isnan(want)) and \
        np.array_equal(got[~np.isnan(got)].view(np.int32), want[~np.isnan(want)].view(np.int32))


def lay_out(x, layout, dtype):
    """x [B, n, S] CPU values -> the device tensor [B, n, S] in the layout under test"""
    B, n, S = x.shape
    if layout == "ncs":
        return x.to(dtype).to(DEV)
    ld = n if layout == "cl" else int(layout[2:])
    buf = torch.full((B, S, ld), NAN, dtype=dtype)
    buf[:, :, :n] = x.permute(0, 2, 1).to(dtype)
    return buf.to(DEV)[:, :, :n].permute(0, 2, 1)


def _expected_route(t, B, n, S, want_pred=True):
    """the rules of seg_route (csrc/seg_metric.hip) for a tensor torch allocated (bases aligned to at least 64 bytes)"""
    from UCF_VIT._hip import ops
    sb, sc, ss = ops.dice_strides(t)
    es = t.element_size()
    if sc == 1 and ss >= n:
        nv = 2 if n <= 2 else 4 if n <= 4 else 8
        vb = min(nv * es, 16)
        if (ss * es) % vb == 0 and (sb * es) % vb == 0 and (not want_pred or B == 1 or S % 4 == 0):
            return f"cl nv{nv}"
    if ss == 1 and (sc * es) % 16 == 0 and (sb * es) % 16 == 0 and (B == 1 or S % SEG_VPT == 0):
        return "ncs"
    return "scalar"


# ------------------------------------------------------------------------------------------------------------------------------ GPU half
CASES = [(dt, lay, n, B) for dt in ("fp32", "bf16") for lay in ("ncs", "cl", "cl8", "cl16") for n in (2, 3, 4, 5, 8) for B in (1, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,layout,n,B", CASES, ids=[f"{a}-{b}-n{c}-B{d}" for a, b, c, d in CASES])
def test_seg_counts(dt, layout, n, B):
    from UCF_VIT._hip import ops
    from UCF_VIT.utils.metrics import dice_from_counts
    dtype = torch.float32 if dt == "fp32" else torch.bfloat16
    routes = set()
    for si, S in enumerate(S_LIST):
        # every family at every S up to NCS_STEP + 1; the four multi-thousand-voxel sizes take three families each, rotated over the table so
        # that every family meets every one of them in some case (the kernel's path depends on S and the layout, not on the values)
        fams = range(len(FAMILIES)) if S <= NCS_STEP + 1 else [(si + n + B + 2 * k) % len(FAMILIES) for k in range(3)]
        for f in fams:
            lk, yk = FAMILIES[f]
            x = make_logits(lk, B, n, S, 1000 * n + 10 * B + f).to(dtype)            # the rounded values are the operands
            y = make_labels(yk, B, n, S, 77 * n + B + f)
            want_pred, want_counts = reference(x, y)
            t, yd = lay_out(x.float(), layout, dtype), y.to(DEV)
            if layout != "ncs" and S > 1:
                assert not t.is_contiguous() and t.storage_offset() == 0
            route = ops.seg_counts_route(t, yd)
            assert route.split(" chunk")[0].replace(" vpt8", "") == _expected_route(t, B, n, S), (S, route)
            routes.add(route.split()[0])
            pred, counts = ops.seg_counts(t, yd if f % 2 == 0 else yd.view(B, 1, S))
            full = counts._base if counts._base is not None else counts
            assert pred.dtype == torch.uint8 and tuple(pred.shape) == (B, S) and tuple(full.shape) == (B, 3, 8) and full.dtype == torch.int64
            assert np.array_equal(pred.cpu().numpy(), want_pred), (S, lk, yk)
            assert np.array_equal(full.cpu().numpy(), want_counts), (S, lk, yk)
            if lk == "equal":
                assert int(pred.max()) == 0
            none, counts0 = ops.seg_counts(t, yd, want_pred=False)
            assert none is None and np.array_equal(counts0._base.cpu().numpy(), want_counts), (S, lk, yk)
            pred2, counts2 = ops.seg_counts(t, yd)
            assert torch.equal(pred2, pred) and torch.equal(counts2._base, full)
            for bg in (False, True):
                d = dice_from_counts(counts, include_background=bg)
                assert d.is_cuda and d.dtype == torch.float32
                assert same_bits(d.cpu().numpy(), dice_restated(want_counts[:, :, :n], bg)), (S, lk, yk)
    # the table reaches the kernels it is meant to reach
    if layout == "ncs":
        assert routes == {"ncs", "scalar"}
    elif layout == "cl" and n in (3, 5):
        assert routes == {"scalar"}
    else:
        assert "cl" in routes and (B == 1 or "scalar" in routes)


def _raw(L, logits, labels, B, n, S, strides, want_pred):
    """ucfvit_seg_counts as ops calls it, on a logits tensor of any storage offset"""
    from UCF_VIT._hip import ops
    pred = torch.full((B, S), 255, dtype=torch.uint8, device=DEV) if want_pred else None
    counts = torch.full((B, 3, 8), -1, dtype=torch.int64, device=DEV)
    ws = ops.workspace(L.ucfvit_seg_counts_workspace(B, S), labels.device)
    buf = ctypes.create_string_buffer(96)
    args = (logits.data_ptr(), labels.data_ptr(), pred.data_ptr() if want_pred else None)
    assert L.ucfvit_seg_counts_route(*args, B, n, S, *strides, ops.dt(logits), buf, len(buf)) > 0
    rc = L.ucfvit_seg_counts(*args, counts.data_ptr(), B, n, S, *strides, ws.data_ptr(), ops.dt(logits), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.ucfvit_last_error()
    return pred, counts, buf.value.decode()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("layout", ["ncs", "cl8"])
def test_offset_pointer_takes_the_scalar_kernel(dt, layout):
    """the same operands at an aligned base (a vector kernel) and one element further into the allocation (both vector kernels must refuse:
    the route says scalar) give the same bits"""
    from UCF_VIT._hip import lib
    L = lib.load()
    dtype = torch.float32 if dt == "fp32" else torch.bfloat16
    B, n, S = 3, 4, SEG_CHUNK + NCS_STEP
    x = make_logits("special", B, n, S, 5).to(dtype)
    y = make_labels("outside", B, n, S, 6)
    want_pred, want_counts = reference(x, y)
    yd = y.to(DEV)
    if layout == "ncs":
        flat, strides = x.reshape(-1), (n * S, S, 1)
    else:
        buf = torch.full((B, S, 8), NAN, dtype=dtype)
        buf[:, :, :n] = x.permute(0, 2, 1)
        flat, strides = buf.reshape(-1), (S * 8, 1, 8)
    for off, name in ((0, "ncs" if layout == "ncs" else "cl nv4"), (1, "scalar")):
        store = torch.full((flat.numel() + 8,), NAN, dtype=dtype, device=DEV)
        store[off:off + flat.numel()] = flat.to(DEV)
        t = store[off:]
        assert t.data_ptr() % 16 == off * t.element_size()
        for want in (True, False):
            pred, counts, route = _raw(L, t, yd, B, n, S, strides, want)
            assert route.startswith(name), route
            assert np.array_equal(counts.cpu().numpy(), want_counts)
            assert pred is None or np.array_equal(pred.cpu().numpy(), want_pred)


@pytest.mark.gpu
def test_route_names_the_constants():
    from UCF_VIT._hip import ops
    y = torch.zeros(1, 4096, dtype=torch.int64, device=DEV)
    assert ops.seg_counts_route(torch.zeros(1, 4, 4096, device=DEV), y) == f"ncs vpt{SEG_VPT} chunk{SEG_CHUNK} step{NCS_STEP}"
    assert ops.seg_counts_route(torch.zeros(1, 4096, 4, device=DEV).permute(0, 2, 1), y) == f"cl nv4 chunk{SEG_CHUNK} step{CL_STEP}"
    assert ops.seg_counts_route(torch.zeros(1, 4096, 3, device=DEV).permute(0, 2, 1), y) == f"scalar chunk{SEG_CHUNK}"


@pytest.mark.gpu
def test_seg_counts_refuses_what_it_cannot_read():
    from UCF_VIT._hip import ops
    x = torch.zeros(2, 3, 16, device=DEV)
    with pytest.raises(TypeError):
        ops.seg_counts(x, torch.zeros(2, 16, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.seg_counts(x, torch.zeros(2, 15, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        ops.seg_counts(torch.zeros(2, 9, 16, device=DEV), torch.zeros(2, 16, dtype=torch.int64, device=DEV))
    with pytest.raises(TypeError):
        ops.seg_counts(x.half(), torch.zeros(2, 16, dtype=torch.int64, device=DEV))


# ----------------------------------------------------------------------------------------------------------------------------- host half
def test_argument_checks_without_gpu():
    """the checks come before any HIP call: each refusal returns -1 with a message that names the entry point"""
    from UCF_VIT._hip import lib
    L = lib.load()
    p = 4096                                   # a non-null address that is never dereferenced: every call below is refused first
    ok = dict(logits=p, labels=p, pred=None, counts=p, B=2, n=4, S=64, sb=256, sc=64, ss=1, ws=p, dtype=lib.F32)

    def call(**kw):
        a = dict(ok, **kw)
        rc = L.ucfvit_seg_counts(a["logits"], a["labels"], a["pred"], a["counts"], a["B"], a["n"], a["S"], a["sb"], a["sc"], a["ss"], a["ws"],
                                 a["dtype"], None)
        return rc, L.ucfvit_last_error()

    for kw, word in ((dict(logits=None), b"null pointer"), (dict(labels=None), b"null pointer"), (dict(counts=None), b"null pointer"),
                     (dict(ws=None), b"null pointer"), (dict(n=1), b"classes"), (dict(n=9), b"classes"), (dict(sc=0), b"strides"),
                     (dict(ss=0), b"strides"), (dict(sb=0), b"strides"), (dict(dtype=7), b"dtype"), (dict(B=0), b"B in"), (dict(B=65536), b"B in"),
                     (dict(S=0), b"B in")):
        rc, msg = call(**kw)
        assert rc == -1 and b"ucfvit_seg_counts" in msg and word in msg, (kw, rc, msg)
    buf = ctypes.create_string_buffer(64)
    assert L.ucfvit_seg_counts_route(p, p, None, 2, 9, 64, 576, 64, 1, lib.F32, buf, 64) == -1 and b"ucfvit_seg_counts_route" in L.ucfvit_last_error()
    assert L.ucfvit_seg_counts_route(p, p, None, 2, 4, 64, 256, 64, 1, lib.F32, None, 64) == -1
    # the route itself is host arithmetic on addresses and strides
    assert L.ucfvit_seg_counts_route(p, p, p, 2, 4, 64, 256, 64, 1, lib.F32, buf, 64) > 0 and buf.value.startswith(b"ncs")
    assert L.ucfvit_seg_counts_route(p + 4, p, p, 2, 4, 64, 256, 64, 1, lib.F32, buf, 64) > 0 and buf.value.startswith(b"scalar")
    assert L.ucfvit_seg_counts_route(p, p, p, 2, 4, 64, 512, 1, 8, lib.BF16, buf, 64) > 0 and buf.value.startswith(b"cl nv4")
    assert L.ucfvit_seg_counts_route(p + 2, p, p, 2, 4, 64, 512, 1, 8, lib.BF16, buf, 64) > 0 and buf.value.startswith(b"scalar")
    assert L.ucfvit_seg_counts_route(p, p, p, 2, 4, 63, 63 * 8, 1, 8, lib.BF16, buf, 64) > 0 and buf.value.startswith(b"scalar")     # pred rows unaligned
    assert L.ucfvit_seg_counts_route(p, p, None, 2, 4, 63, 63 * 8, 1, 8, lib.BF16, buf, 64) > 0 and buf.value.startswith(b"cl nv4")  # no pred: fine
    assert L.ucfvit_seg_counts_route(p, p, p, 1, 4, 63, 63 * 8, 1, 8, lib.BF16, buf, 4) > 4 and buf.value == b"cl "                  # truncated to cap


def test_workspace_is_positive_and_monotone():
    from UCF_VIT._hip import lib
    L = lib.load()
    prev_s = 0
    for S in (1, SEG_CHUNK - 1, SEG_CHUNK, SEG_CHUNK + 1, 1 << 20, 512 * 512 * 128):
        w = L.ucfvit_seg_counts_workspace(1, S)
        assert w > 0 and w >= prev_s
        prev_s = w
        prev_b = 0
        for B in (1, 2, 3, 65535):
            wb = L.ucfvit_seg_counts_workspace(B, S)
            assert wb > prev_b
            prev_b = wb
    assert L.ucfvit_seg_counts_workspace(1, SEG_CHUNK + 1) > L.ucfvit_seg_counts_workspace(1, SEG_CHUNK)
    assert L.ucfvit_seg_counts_workspace(2, 512 * 512 * 128) == 2 * 2048 * 24 * 4


def _counts(rows):
    """rows: per item a list of (TP, PRED, LAB) per class -> int64 [B, 3, n]"""
    return torch.tensor(rows, dtype=torch.int64).permute(0, 2, 1).contiguous()


COUNTS_A = _counts([[(50, 60, 55), (7, 9, 11), (0, 3, 0), (0, 0, 4)],          # class 2 absent (NaN), class 3 never predicted (0)
                    [(64, 64, 64), (0, 0, 0), (0, 0, 0), (0, 0, 0)],           # every non-background class absent
                    [(1, 2, 3), (33333, 44444, 55555), (1, 1, 1), (0, 5, 7)]])
COUNTS_B = _counts([[(9, 9, 9), (0, 2, 0), (0, 1, 0), (0, 0, 0)]])             # a batch with no non-NaN item (background excluded)


def test_dice_from_counts_on_cpu_tensors():
    from UCF_VIT.utils.metrics import dice_from_counts
    for counts in (COUNTS_A, COUNTS_B):
        for bg in (False, True):
            d = dice_from_counts(counts, include_background=bg)
            assert d.dtype == torch.float32 and tuple(d.shape) == (counts.shape[0], 4 if bg else 3)
            assert same_bits(d.numpy(), dice_restated(counts.numpy(), bg))
    d = dice_from_counts(COUNTS_A).numpy()
    assert d[0, 0] == np.float32(14.0 / 20.0) and np.isnan(d[0, 1]) and d[0, 2] == 0.0 and np.isnan(d[1]).all() and d[2, 1] == 1.0
    with pytest.raises(ValueError):
        dice_from_counts(COUNTS_A.float())
    with pytest.raises(ValueError):
        dice_from_counts(COUNTS_A[:, :2])


def test_dice_metric_aggregate_is_the_restated_mean_reduction():
    from UCF_VIT.utils.metrics import DiceMetric
    m = DiceMetric(include_background=False)
    with pytest.raises(RuntimeError):
        m.aggregate()
    # not_nans == 0: the mean is 0, as monai's reduction leaves it
    d = m.update(COUNTS_B)
    assert np.isnan(d.numpy()).all()
    mean, nn = m.aggregate()
    assert mean.item() == 0.0 and nn.item() == 0.0
    # a running state over two calls; the all-absent item of COUNTS_A does not count
    per = [d.numpy(), m.update(COUNTS_A).numpy()]
    mean, nn = m.aggregate()
    want, want_n = mean_restated(per)
    assert nn.item() == want_n == 2 and mean.dtype == torch.float32 and mean.item() == np.float32(want)
    m.reset()
    per = [m.update(COUNTS_A[2:]).numpy()]
    mean, nn = m.aggregate()
    assert nn.item() == 1 and mean.item() == np.float32(mean_restated(per)[0])
    mb = DiceMetric(include_background=True)
    per = [mb.update(COUNTS_A).numpy(), mb.update(COUNTS_B).numpy()]
    mean, nn = mb.aggregate()
    want, want_n = mean_restated(per)
    assert nn.item() == want_n == 4 and mean.item() == np.float32(want)


def _gloo_worker(rank, world, port, q):
    for p in (os.path.join(ROOT, "ucf-vit_amd"), ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from UCF_VIT.utils.metrics import DiceMetric, dice_from_counts
        mine = SLABS[rank].clone()
        keep = mine.clone()
        d = dice_from_counts(mine, include_background=True, group=dist.group.WORLD)
        m = DiceMetric(include_background=False, group=dist.group.WORLD)
        m.update(mine)
        q.put((rank, d.numpy(), dice_from_counts(mine, include_background=True).numpy(), bool(torch.equal(mine, keep)), m.aggregate()[0].item()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


# two X-slabs of one volume: neither slab's own Dice is the whole volume's
SLABS = [_counts([[(10, 30, 12), (5, 6, 20), (0, 0, 0)]]), _counts([[(20, 22, 40), (1, 9, 2), (0, 4, 3)]])]


def test_dice_from_counts_sums_the_slabs_of_a_group():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, 29587, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    whole = (SLABS[0] + SLABS[1]).numpy()
    want = dice_restated(whole, True)
    for rank, d, own, untouched, agg in res:
        assert same_bits(d, want), rank
        assert not same_bits(own, want) and same_bits(own, dice_restated(SLABS[rank].numpy(), True))
        assert untouched                                  # the caller's counts are not summed in place
        assert agg == np.float32(mean_restated([dice_restated(whole, False)])[0])
