"""Dynamic loss scaling on the device (csrc/grad_scaler.hip, _hip/grad_scaler.py, HipAdamW.step_scaled).

Exact tier: the non-finite check is a predicate; a skipped step must leave p, m, v and the bf16 shadow bit-identical; deleting the skipped
iterations of a run must not change its result (a skip does not advance the bias correction); a constant power-of-two scale must not change
any bit (multiplying and dividing by 2^k is exact while every value stays normal); scale, growth tracker and step counts must EQUAL those of
torch.amp.GradScaler (small integers and powers of two).
Real-valued tier: ucfvit_adamw_scaled against an fp64 AdamW step from the same fp32 state with the per-element bounds of
tests/test_rowwise_ops.py::test_adamw_vs_fp64 (restated here), and a 45-step trajectory against torch.optim.AdamW on the CPU."""
import math

import pytest
import torch

from conftest import load_golden
from det_weights import det_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24          # fp32 unit roundoff
VARS = ["red", "green", "blue"]
BIG_N = 3 * 2 ** 20 + 3
MAE_KW = dict(img_size=[32, 32], patch_size=8, in_chans=3, embed_dim=64, depth=2, num_heads=2, class_token=False, weight_init='skip',
              mask_ratio=0.75, linear_decoder=False, decoder_depth=1, decoder_embed_dim=32, decoder_num_heads=1, mlp_ratio_decoder=4.0)


def _ops():
    from UCF_VIT._hip import ops
    return ops


def _lib():
    from UCF_VIT._hip import lib
    return lib


def _scaler(**kw):
    from UCF_VIT._hip.grad_scaler import HipGradScaler
    return HipGradScaler(**kw)


def _const_scaler(scale=1.0):
    """a scale that never moves: no growth inside the run, backoff 1.0"""
    return _scaler(init_scale=scale, backoff_factor=1.0, growth_interval=10 ** 6)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, seed, dtype=torch.float32, scale=1.0):
    return (torch.randn(shape, generator=_gen(seed), device=DEV, dtype=torch.float32) * scale).to(dtype)


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


# ============================================================================================== 1. the check kernel
def _nf_stride(n, dtype):
    """elements one grid-stride pass of grad_nonfinite_kernel covers: 16-byte vectors, 256 threads, at most 1024 workgroups"""
    epv = 16 // torch.tensor([], dtype=dtype).element_size()
    nvec = (n + epv - 1) // epv
    return epv, min((nvec + 255) // 256, 1024) * 256 * epv


def _flag(ops, g, mult=1.0, scale=1.0, st=None):
    lib = _lib()
    if st is None:
        st = _const_scaler(scale).device_state()
    ops.grad_nonfinite(g, st, mult)
    f = st[lib.GS_FOUND_INF].item()
    assert f in (0.0, 1.0)
    return f == 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_nonfinite_check(dtype):
    """finite buffers leave the flag 0; one +Inf / -Inf / NaN at the first element, the last element (the scalar tail when n is not a
    multiple of the vector width) and inside the second grid-stride pass sets it; so does a finite value whose product with
    mult * inv_scale overflows fp32; the largest finite value with multiplier 1 does not; the flag is sticky.  The two sizes beyond
    3*2^20+3 reach the 4-fold unrolled part of the loop (4 strides of 1024 * 256 vectors), with a plant under each of its four loads."""
    ops, lib = _ops(), _lib()
    epv = _nf_stride(1, dtype)[0]
    for n in [1, 2, 3, 4, 5, 1003, BIG_N, (5 * 2 ** 20 + 3) * epv // 4]:
        g = _randn(n, n, dtype)
        assert not _flag(ops, g), f"finite buffer n={n}"
        _, stride = _nf_stride(n, dtype)
        spots = {0, n - 1}
        if n > stride:
            spots.add(stride + 5 * epv + 1)                            # second grid-stride pass
            assert n >= BIG_N
        if n > 4 * stride:
            spots.update(u * stride + 7 * epv + u for u in range(5))   # each load of the unrolled iteration, and the remainder loop
        assert max(spots) < n
        for bad in (float("inf"), float("-inf"), float("nan")):
            for i in sorted(spots):
                keep = g[i].clone()
                g[i] = bad
                assert _flag(ops, g), f"{bad} at {i} of n={n} not seen"
                g[i] = keep
        assert not _flag(ops, g), f"buffer restored n={n}"
        # overflow of the product, through mult and through inv_scale
        i = n // 2
        keep = g[i].clone()
        g[i] = 1e30
        assert not _flag(ops, g), "1e30 itself is finite"
        assert _flag(ops, g, mult=1e10), f"1e30 * 1e10 overflows, n={n}"
        assert _flag(ops, g, scale=2.0 ** -40), f"1e30 * 2^40 overflows, n={n}"
        assert not _flag(ops, g, mult=1e-10, scale=2.0 ** -40), "1e30 * 1e-10 * 2^40 is finite"
        g[i] = torch.finfo(dtype).max
        g[0] = -torch.finfo(dtype).max
        assert not _flag(ops, g), f"largest finite value, multiplier 1, n={n}"
        g[i] = keep
        # sticky
        st = _const_scaler().device_state()
        g[n - 1] = float("inf")
        assert _flag(ops, g, st=st)
        g[n - 1] = 0.0
        assert _flag(ops, g, st=st), "a clean second segment cleared the flag"
        ops.grad_scaler_update(st)
        assert st[lib.GS_FOUND_INF].item() == 0.0 and st[lib.GS_SKIPPED_STEPS].item() == 1.0
        assert not _flag(ops, g, st=st)


# ============================================================================================== 2. a skipped step moves nothing
def _mae_bf16(seed=26):
    from UCF_VIT.simple.arch import MAE
    m = MAE(**MAE_KW)
    m.load_state_dict(det_state_dict(m, seed))
    m = m.to(DEV)
    m.set_compute_dtype(torch.bfloat16)
    return m


def _fill_grads(st, seed):
    st.flat_g.copy_(_randn(st.total, seed, scale=1e-2))
    for p, o in zip(st.params, st.offsets):
        p.grad = st.grad_view(p, o, p.numel())


@pytest.mark.parametrize("path", ["flat", "per_parameter"])
def test_skipped_step_moves_nothing(path):
    from UCF_VIT._hip.optim import HipAdamW
    from UCF_VIT._hip.params import ensure_store
    from UCF_VIT.utils.misc import configure_optimizer
    m = _mae_bf16()
    st = ensure_store(m)
    st.refresh_shadow()
    if path == "flat":
        opt = configure_optimizer(m, 1e-3, 0.9, 0.95, 1e-2)
    else:
        ps = list(st.params)
        del ps[3]                                       # not a contiguous run of the store any more: one launch per parameter
        opt = HipAdamW(ps, lr=1e-3, betas=(0.9, 0.95), weight_decay=1e-2)
    sc = _scaler(init_scale=4.0, growth_interval=100)
    _fill_grads(st, 1)
    sc.step(opt)
    sc.update()
    assert bool(opt._flat) == (path == "flat")
    st.refresh_shadow()
    moments = lambda: [t.clone() for s in opt.state.values() for t in (s["exp_avg"], s["exp_avg_sq"])]    # noqa: E731
    p0, s0, mom0 = st.flat_p.clone(), st.flat_s.clone(), moments()
    assert any(bool(t.any()) for t in mom0)

    _fill_grads(st, 2)
    victim = st.params[-1] if path == "flat" else st.params[5]
    victim.grad.view(-1)[victim.numel() // 2] = float("inf")
    sc.step(opt)
    sc.update()
    st.refresh_shadow()
    assert _same(st.flat_p, p0) and _same(st.flat_s, s0)
    assert all(_same(a, b) for a, b in zip(moments(), mom0))
    assert sc.get_scale() == 2.0 and sc.counters() == (1, 1)

    _fill_grads(st, 3)                                   # and the next clean step moves everything again
    sc.step(opt)
    sc.update()
    st.refresh_shadow()
    assert not _same(st.flat_p, p0) and not _same(st.flat_s, s0)
    assert sc.counters() == (2, 1)
    assert {int(s["step"]) for s in opt.state_dict()["state"].values()} == {2}


# ============================================================================================== 3. skips do not advance the bias correction
def _two_group_params(seed):
    ps = [torch.nn.Parameter(_randn(1003, seed)), torch.nn.Parameter(_randn(4099, seed + 1))]
    return ps


def _opt_two_groups(ps):
    from UCF_VIT._hip.optim import HipAdamW
    return HipAdamW([dict(params=[ps[0]], weight_decay=0.05), dict(params=[ps[1]], weight_decay=0.0)], lr=1e-3, betas=(0.9, 0.95))


def _run_script(iters, skip, ps, opt, sc):
    for i in iters:
        for k, p in enumerate(ps):
            p.grad = _randn(p.numel(), 100 * i + k, scale=1e-2 * (1 + i % 3))
        if i in skip:
            ps[i % 2].grad[i] = float("nan") if i % 2 else float("inf")
        sc.step(opt)
        sc.update()
        opt.zero_grad()


def test_skips_do_not_advance_bias_correction():
    """12 iterations with non-finite gradients at 2, 3 and 7 end exactly where the 9 clean iterations alone end"""
    skip = {2, 3, 7}
    pa, pb = _two_group_params(5), _two_group_params(5)
    oa, ob = _opt_two_groups(pa), _opt_two_groups(pb)
    sa, sb = _const_scaler(), _const_scaler()
    _run_script(range(12), skip, pa, oa, sa)
    _run_script([i for i in range(12) if i not in skip], set(), pb, ob, sb)
    for a, b in zip(pa, pb):
        assert _same(a.data, b.data)
        assert _same(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) and _same(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])
    assert sa.counters() == (9, 3) and sb.counters() == (9, 0)
    for o in (oa, ob):
        assert [int(s["step"]) for s in o.state_dict()["state"].values()] == [9, 9]
    assert [int(oa.state[p]["step"]) for p in pa] == [12, 12]        # the host side counts calls


def test_resume_under_a_scaler_continues_bit_exactly():
    """state_dict() after 4 calls with one skip reports step 3; a fresh optimizer + scaler loaded from the dicts continue with t = 4"""
    pa = _two_group_params(9)
    oa, sa = _opt_two_groups(pa), _scaler(init_scale=64.0, growth_interval=2, min_scale=16.0)
    _run_script(range(6), {2}, pa, oa, sa)
    pb = _two_group_params(9)
    ob, sb = _opt_two_groups(pb), _scaler(init_scale=64.0, growth_interval=2, min_scale=16.0)
    _run_script(range(4), {2}, pb, ob, sb)
    osd, ssd = ob.state_dict(), sb.state_dict()
    assert [int(s["step"]) for s in osd["state"].values()] == [3, 3]
    assert ssd == dict(scale=64.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2, _growth_tracker=1, min_scale=16.0)
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pb]
    oc, sc = _opt_two_groups(pc), _scaler()
    oc.load_state_dict(osd)
    sc.load_state_dict(ssd)
    _run_script(range(4, 6), set(), pc, oc, sc)
    for a, c in zip(pa, pc):
        assert _same(a.data, c.data) and _same(oa.state[a]["exp_avg_sq"], oc.state[c]["exp_avg_sq"])
    assert sc.state_dict() == sa.state_dict()
    assert [int(s["step"]) for s in oc.state_dict()["state"].values()] == [5, 5]


# ============================================================================================== 4. power-of-two invariance
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_power_of_two_scale_changes_no_bit(gdt):
    """|g| in [2^-20, 2^6]: g * 2^16 <= 2^22 and g >= 2^-20 are normal in fp32 and bf16, so (g * 2^k) * 2^-k == g exactly"""
    ops = _ops()
    n, steps = 4099, 5
    mag = torch.exp2(torch.rand(steps, n, generator=_gen(3), device=DEV) * 26.0 - 20.0)
    sign = torch.where(torch.rand(steps, n, generator=_gen(4), device=DEV) < 0.5, -1.0, 1.0)
    gs = (mag * sign).to(gdt)
    assert float(gs.float().abs().min()) >= 2.0 ** -20 and float(gs.float().abs().max()) <= 2.0 ** 6
    out = {}
    for k in (0, 7, 13, 16):
        st = _const_scaler(2.0 ** k).device_state()
        p = _randn(n, 11)
        m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        sh = torch.empty(n, dtype=torch.bfloat16, device=DEV)
        for s in range(steps):
            g = (gs[s].float() * 2.0 ** k).to(gdt)
            assert torch.equal(g.float() * 2.0 ** -k, gs[s].float())
            ops.grad_nonfinite(g, st)
            ops.adamw_scaled(p, g, m, v, sh, 1e-3, 0.9, 0.95, 1e-8, 0.05, st)
            ops.grad_scaler_update(st)
        assert st.tolist()[:6] == [2.0 ** k, 2.0 ** -k, 0.0, float(steps), float(steps), 0.0]
        out[k] = (p, m, v, sh)
    assert bool(out[0][2].any())
    for k in (7, 13, 16):
        for a, b, what in zip(out[k], out[0], "pmvs"):
            assert _same(a, b), f"{what} differs at scale 2^{k}"


# ============================================================================================== 5. against plain AdamW in fp64
def _adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, gs):
    """tests/test_rowwise_ops.py::_adamw_ref restated: the fp64 torch.optim.AdamW update from the kernel's fp32 state (hyper-parameters as the
    fp32 values the kernel uses; bias corrections formed in double and rounded once to fp32), its per-element bounds and wrong references:
    p without the v bias correction, p moved along the previous first moment"""
    f = lambda a: float(torch.tensor(a, dtype=torch.float32))          # noqa: E731
    bc1, bc2 = f(1.0 - b1 ** step), f(1.0 - b2 ** step)
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


def _within(got, ref, tol):
    return bool(((got.double() - ref).abs() <= tol).all())


def _check(got, ref, tol, wrong, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, "
                                 f"worst excess {float((err - tol)[bad].max()):.3e}")
    for w in wrong:
        assert not _within(got, w, tol), f"{what}: the bound does not reject a wrong reference"


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("gs,wd,with_shadow", [(1.0, 0.0, True), (0.125, 0.05, False)])
def test_adamw_scaled_vs_fp64(gdt, gs, wd, with_shadow):
    """no skips, scale 1: steps 1 .. 5 and 1000 (the applied-step count is written into the state block), each compared per element with an
    fp64 step from the same fp32 state, at the sizes of test_adamw_vs_fp64 (n % 4 tails, vector body, a second grid-stride pass)"""
    ops, lib = _ops(), _lib()
    lr, b1, b2, eps = 1e-3, 0.9, 0.95, 1e-8
    st = _const_scaler().device_state()
    for n in [1, 2, 3, 4, 5, 1003, BIG_N]:
        p = _randn(n, n)
        m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        sh = torch.empty(n, dtype=torch.bfloat16, device=DEV) if with_shadow else None
        for step in [1, 2, 3, 4, 5, 1000]:
            g = _randn(n, n * 7 + step, gdt, scale=1e-2 * step if step < 10 else 1e-2)
            p1, m1, v1, e_p, e_m, e_v, w = _adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, gs)
            st[lib.GS_APPLIED_STEPS] = step - 1
            ops.grad_nonfinite(g, st, gs)
            ops.adamw_scaled(p, g, m, v, sh, lr, b1, b2, eps, wd, st, grad_scale=gs)
            _check(m, m1, e_m + U * m1.abs(), [w["m"]], f"m n={n} step={step}")
            _check(v, v1, e_v + U * v1, [w["v"]], f"v n={n} step={step}")
            _check(p, p1, e_p, [w["p_oldm"]] + ([w["p_nobc2"]] if step <= 5 else []), f"p n={n} step={step}")
            if with_shadow:
                assert _same(sh, p.to(torch.bfloat16)), f"shadow n={n} step={step}"
    assert st[lib.GS_FOUND_INF].item() == 0.0


# ============================================================================================== 6. schedule and trajectory against torch
FLOOR = 128.0
INF_STEPS = {3, 4, 6, 7, 8, 9, 10, 11, 20, 30, 31}


def test_schedule_and_trajectory_match_torch_on_the_cpu():
    """torch.amp.GradScaler("cpu", init_scale=8192, growth_interval=3) + torch.optim.AdamW with the reference's floor of 128 applied after
    each update(), two parameter groups, 45 steps; the loss factor is Inf at INF_STEPS (two consecutive, then six in a row: 2048 -> 32
    would pass the floor, so the scale stops at 128).  loss = sum(0.5 a w^2) c_t has the elementwise gradient a w c_t, the same IEEE
    operations on both devices.  After every step scale, growth tracker and step counts are EQUAL.  p: test_adamw_matches_torch holds
    this pairing to rel_err < 1e-6 after 3 steps; allowed here 1e-6 * applied / 3 = 1.13e-5 (34 applied steps).
    Measured on MI355X: 7.56e-7 and 6.88e-8 for the two groups."""
    from conftest import rel_err
    from UCF_VIT._hip.optim import HipAdamW
    g = torch.Generator().manual_seed(17)
    w0 = [torch.randn(257, generator=g), torch.randn(64, generator=g)]
    a = [torch.rand(257, generator=g) + 0.5, torch.rand(64, generator=g) + 0.5]
    kw = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8)

    def groups(ws):
        return [dict(params=[ws[0]], weight_decay=0.05), dict(params=[ws[1]], weight_decay=0.0)]

    wr = [torch.nn.Parameter(w.clone()) for w in w0]
    opt_r = torch.optim.AdamW(groups(wr), **kw)
    ref = torch.amp.GradScaler("cpu", init_scale=8192.0, growth_interval=3)
    wh = [torch.nn.Parameter(w.clone().to(DEV)) for w in w0]
    ah = [t.to(DEV) for t in a]
    opt_h = HipAdamW(groups(wh), **kw)
    sc = _scaler(init_scale=8192.0, growth_interval=3, min_scale=FLOOR)
    scales = []
    for t in range(45):
        c = float("inf") if t in INF_STEPS else 1.0 + 0.25 * (t % 4)
        loss_r = sum((0.5 * x * w * w).sum() for x, w in zip(a, wr)) * c
        ref.scale(loss_r).backward()
        ref.step(opt_r)
        ref.update()
        if ref._scale < FLOOR:
            ref._scale.fill_(FLOOR)
        opt_r.zero_grad()
        loss_h = sum((0.5 * x * w * w).sum() for x, w in zip(ah, wh)) * c
        sc.scale(loss_h).backward()
        sc.step(opt_h)
        sc.update()
        opt_h.zero_grad()
        assert sc.get_scale() == ref.get_scale(), t
        assert sc.state_dict()["_growth_tracker"] == ref.state_dict()["_growth_tracker"], t
        steps_r = [int(opt_r.state[w]["step"]) for w in wr if w in opt_r.state]
        steps_h = [int(s["step"]) for s in opt_h.state_dict()["state"].values()]
        assert steps_h == (steps_r or [0, 0]), t
        scales.append(sc.get_scale())
    applied = 45 - len(INF_STEPS)
    assert sc.counters() == (applied, len(INF_STEPS))
    assert scales[2] == 16384.0 and scales[4] == 4096.0 and min(scales) == FLOOR and scales.count(FLOOR) >= 2
    errs = [rel_err(h, r) for h, r in zip(wh, wr)]
    print(f"trajectory rel_err vs torch CPU after {applied} applied steps: {errs[0]:.3e} {errs[1]:.3e} (bound {1e-6 * applied / 3:.3e})")
    assert max(errs) < 1e-6 * applied / 3


# ============================================================================================== 7. end to end on a model
def test_mae_bf16_survives_an_inf_batch():
    """ten bf16 MAE steps under configure_grad_scaler(True); at step 4 one input image is Inf: that step leaves the master weights and the
    shadows bit-identical and halves the scale; afterwards everything is finite.  Losses of steps 1-3 against a run without the scaler:
    bound 6e-2 (the bf16 model tolerance of test_mae_small_vs_reference); the runs differ only by an exact power-of-two scaling of the bf16
    gradients.  Measured on MI355X: relative difference 0 (the three losses are equal to the last bit)."""
    from UCF_VIT.utils.metrics import patch_mse_loss
    from UCF_VIT.utils.misc import configure_grad_scaler, configure_optimizer
    g = load_golden("model_mae_small.npz")
    x0, noise = g["x"].to(DEV), g["noise"].to(DEV)

    def run(with_scaler, steps):
        m = _mae_bf16()
        opt = configure_optimizer(m, 1e-3, 0.9, 0.95, 1e-2)
        sc = configure_grad_scaler(with_scaler)
        losses = []
        for i in range(1, steps + 1):
            x = x0.clone()
            if with_scaler and i == 4:
                x[0] = float("inf")
            pred, _ = m(x, VARS, noise=noise)
            loss = patch_mse_loss(pred, x, 8)
            st = m._ucf_store
            before = (st.flat_p.clone(), st.flat_s.clone(), sc.get_scale())
            sc.scale(loss).backward()
            sc.step(opt)
            sc.update()
            opt.zero_grad()
            losses.append(loss.item())
            if with_scaler:
                assert bool(opt._flat), "fused flat-segment AdamW path was not taken"
                moved = not _same(st.flat_p, before[0])
                if i == 4:
                    assert not moved and _same(st.flat_s, before[1]) and sc.get_scale() == before[2] / 2 == 4096.0
                else:
                    assert moved and sc.get_scale() == before[2]
        return m, sc, losses

    m, sc, ls = run(True, 10)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert bool(torch.isfinite(m._ucf_store.flat_s.float()).all())
    assert not math.isfinite(ls[3]) and all(math.isfinite(v) for v in ls[:3] + ls[4:])
    assert sc.counters() == (9, 1)
    _, _, lp = run(False, 3)
    d = [abs(a - b) / abs(b) for a, b in zip(ls[:3], lp)]
    print(f"MAE bf16 losses, scaler vs none, steps 1-3: {ls[:3]} vs {lp}: rel diff {max(d):.3e} (bound 6e-2)")
    assert max(d) < 6e-2


# ============================================================================================== 8. no host synchronisation
def test_step_path_does_not_synchronise():
    """scale(), step() and update() under torch.cuda.set_sync_debug_mode("error"), flat path (with a skipped step) and per-parameter path;
    the mode is first shown to raise on a deliberate .item() (it does on ROCm, torch 2.10)"""
    from UCF_VIT._hip.params import ensure_store
    from UCF_VIT.utils.misc import configure_optimizer
    m = _mae_bf16()
    st = ensure_store(m)
    st.refresh_shadow()
    opt = configure_optimizer(m, 1e-3, 0.9, 0.95, 1e-2)
    sc = _scaler(init_scale=8.0)
    ps = _two_group_params(3)
    opt2, sc2 = _opt_two_groups(ps), _scaler(init_scale=8.0)
    sc.device_state(), sc2.device_state()          # the state block is created on first use: one host-to-device copy per scaler
    one = torch.ones((), device=DEV)

    class no_sync:
        def __enter__(self):
            torch.cuda.synchronize()
            self.prev = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")

        def __exit__(self, *exc):
            torch.cuda.set_sync_debug_mode(self.prev)

    with no_sync():
        with pytest.raises(RuntimeError):
            one.item()
    for i in range(3):
        _fill_grads(st, 40 + i)
        if i == 1:
            st.flat_g[7] = float("inf")
        for k, p in enumerate(ps):
            p.grad = _randn(p.numel(), 50 + 2 * i + k)
        with no_sync():
            loss = sc.scale(one)
            sc.step(opt)
            sc.update()
            sc2.scale(one)
            sc2.step(opt2)
            sc2.update()
    assert loss.item() == 4.0 and sc.counters() == (2, 1) and sc2.counters() == (3, 0)


# ============================================================================================== 9. entry point
def test_train_masked_simple_runs_and_resumes_with_the_grad_scaler(tmp_path):
    """train_masked_simple.py on the config of test_train_masked_simple_entry_point_runs (rebuilt here) with `use_grad_scaler: True` under
    `model:`: 2 epochs, the checkpoint holds scaler_state_dict with the reference's constants, and a third epoch resumes from it"""
    import os
    import subprocess
    import sys
    import yaml
    from conftest import ROOT
    cfg = yaml.safe_load(open(os.path.join(ROOT, "ucf-vit_amd", "configs", "catsdogs_vit_tiny_smoke.yaml")))
    cfg["trainer"].update(data_type="bfloat16", loss_fn="maskMSE", checkpoint_path=str(tmp_path))
    cfg["model"]["net"]["init_args"].update(tile_size=[64, 64], patch_size=8, embed_dim=128, depth=3, num_heads=2, mask_ratio=0.75,
                                            linear_decoder=False, decoder_depth=2, decoder_embed_dim=64, decoder_num_heads=2,
                                            mlp_ratio_decoder=4.0)
    cfg["model"].update(lr=1e-3, warmup_steps=2, use_grad_scaler=True)
    cfg["load_balancing"]["batches_per_rank_epoch"]["catsdogs"] = 8

    def run(cfg):
        p = tmp_path / "cfg.yaml"
        p.write_text(yaml.safe_dump(cfg))
        env = dict(os.environ, MASTER_PORT="29583")
        out = subprocess.run([sys.executable, os.path.join(ROOT, "ucf-vit_amd", "training_scripts", "train_masked_simple.py"), str(p)],
                             capture_output=True, text=True, timeout=280, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        return [float(l.split("epoch_loss")[1].split()[0]) for l in out.stdout.splitlines() if "epoch_loss" in l], out.stdout

    losses, text = run(cfg)
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses) and losses[1] < losses[0], text
    ck = torch.load(tmp_path / "multi_last_odd.ckpt", map_location="cpu", weights_only=True)
    ssd = ck["scaler_state_dict"]
    assert ssd == dict(scale=8192.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=100, _growth_tracker=16, min_scale=128.0)
    assert {int(s["step"]) for s in ck["optimizer_state_dict"]["state"].values()} == {16}
    cfg["trainer"].update(resume_from_checkpoint=True, checkpoint_filename_for_loading="multi_last_odd", max_epochs=3)
    losses3, text = run(cfg)
    assert "epoch: 2" in text and len(losses3) == 1 and math.isfinite(losses3[0]) and losses3[0] < losses[0], text
    ck = torch.load(tmp_path / "multi_last_even.ckpt", map_location="cpu", weights_only=True)
    assert ck["epoch"] == 2 and ck["scaler_state_dict"]["_growth_tracker"] == 24
    assert {int(s["step"]) for s in ck["optimizer_state_dict"]["state"].values()} == {24}
