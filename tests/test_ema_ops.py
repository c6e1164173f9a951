"""ucfvit_adamw_ema / ucfvit_adamw_scaled_ema on the MI355X.

Exact tier: p, m, v and the bf16 shadow have the bits ucfvit_adamw / ucfvit_adamw_scaled give on copies of the same inputs (the average is a
template parameter of one body: the instantiation without it is the one those entry points launch).
Per element: ema against e + r (p_new - e) in float64 (tests/ddim_ref.py), p_new being the fp32 value the kernel stored.  The bound
u (2 r |p_new - e| + |e'|) (1 + 2u), u = 2^-24, comes from the three roundings (difference, product, sum; a fused multiply-add skips the
second) and is derived in ddim_ref.ema_bound, not measured; tests/test_ema_ddim_cpu.py checks it on the host for both evaluations.
Where p_new == e the result is e exactly.  With ema_rate = 1 the result is p_new exactly wherever p_new - e is exact, which Sterbenz's lemma
gives for e / 2 <= p_new <= 2 e: the inputs of that case are drawn there (e = k p_new, k in [0.6, 1.9]).

Sizes: tail only (1, 3), one vector (4), vector + tail (5, 7, 1027), and 2^21 + 1027: beyond the 2048 x 256 x 4 elements one pass of the grid
covers, so the grid-stride loop runs twice for some lanes and the tail sits past it."""
import numpy as np
import pytest
import torch

import ddim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 3, 4, 5, 7, 1027, 2 ** 21 + 1027]
HP = (1e-3, 0.9, 0.95, 1e-8, 0.01)            # lr, beta1, beta2, eps, weight decay
STEP = 3
GSCALE = 0.5


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def inputs(n, gdtype, shadow, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    f = lambda a: torch.from_numpy(a.astype(np.float32)).to(DEV)
    d = dict(p=f(g.standard_normal(n)), g=f(g.standard_normal(n) * 0.1).to(gdtype), m=f(g.standard_normal(n) * 0.01),
             v=f(g.uniform(0.0, 0.01, n)), sh=torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV) if shadow else None)
    d["p"][::11] = 0.0
    return d, f(g.standard_normal(n))


def clone(d):
    return {k: None if v is None else v.clone() for k, v in d.items()}


def gs_state(found_inf):
    s = torch.zeros(16, dtype=torch.float32)
    s[0], s[1], s[2], s[4] = 4.0, 0.25, found_inf, float(STEP - 1)       # scale, 1 / scale, FOUND_INF, applied steps
    return s.to(DEV)


def run_plain(d, ema, rate):
    from UCF_VIT._hip import ops
    if ema is None:
        ops.adamw(d["p"], d["g"], d["m"], d["v"], d["sh"], *HP, STEP, GSCALE)
    else:
        ops.adamw_ema(d["p"], d["g"], d["m"], d["v"], d["sh"], ema, *HP, STEP, rate, GSCALE)


def run_scaled(d, ema, rate, state):
    from UCF_VIT._hip import ops
    if ema is None:
        ops.adamw_scaled(d["p"], d["g"], d["m"], d["v"], d["sh"], *HP, state, GSCALE)
    else:
        ops.adamw_scaled_ema(d["p"], d["g"], d["m"], d["v"], d["sh"], ema, *HP, state, rate, GSCALE)


def check_against(base, got, ema0, ema, rate, what):
    for k in ("p", "m", "v", "sh"):
        if base[k] is not None:
            assert same_bits(base[k], got[k]), (what, k)
    p_new = got["p"].cpu().numpy()
    e0, e1 = ema0.cpu().numpy(), ema.cpu().numpy()
    err = np.abs(e1.astype(np.float64) - R.ema64(e0, p_new, rate))
    bound = R.ema_bound(e0, p_new, rate)
    print(f"{what}: worst ema err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all(), what
    same = p_new == e0
    assert np.array_equal(e1[same], e0[same]), what
    return int(same.sum())


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", SIZES)
def test_adamw_ema(n, gdtype, shadow):
    from UCF_VIT._hip import ops
    d0, ema0 = inputs(n, gdtype, shadow, 100 + n % 97)
    rate = ops.ema_rate(0.9)
    base = clone(d0)
    run_plain(base, None, None)
    assert not same_bits(base["p"], d0["p"])                                # the step moved the weights
    ema0[::5] = base["p"][::5]                                              # p_new == e on every fifth element
    got, ema = clone(d0), ema0.clone()
    run_plain(got, ema, rate)
    assert check_against(base, got, ema0, ema, rate, f"adamw_ema n={n}") >= (n + 4) // 5
    assert not same_bits(ema, ema0) or n == 1
    # rate 1: p_new itself where the difference is exact
    k = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).uniform(0.6, 1.9, n).astype(np.float32)).to(DEV)
    e_near = base["p"] * k
    got, ema = clone(d0), e_near.clone()
    run_plain(got, ema, 1.0)
    assert same_bits(ema, base["p"]) and same_bits(got["p"], base["p"])


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", SIZES)
def test_adamw_scaled_ema(n, gdtype, shadow):
    from UCF_VIT._hip import ops
    d0, ema0 = inputs(n, gdtype, shadow, 300 + n % 97)
    rate = ops.ema_rate(0.99)
    base = clone(d0)
    run_scaled(base, None, None, gs_state(0.0))
    assert not same_bits(base["p"], d0["p"])
    ema0[::5] = base["p"][::5]
    got, ema = clone(d0), ema0.clone()
    run_scaled(got, ema, rate, gs_state(0.0))
    check_against(base, got, ema0, ema, rate, f"adamw_scaled_ema n={n}")
    # the check fired: nothing moves, the average included
    got, ema = clone(d0), ema0.clone()
    run_scaled(got, ema, rate, gs_state(1.0))
    for key in ("p", "m", "v", "sh"):
        if d0[key] is not None:
            assert same_bits(got[key], d0[key]), key
    assert same_bits(ema, ema0)


def test_refusals_return_before_any_launch():
    from UCF_VIT._hip import ops
    from UCF_VIT._hip.lib import HipLibraryError
    d0, ema0 = inputs(64, torch.float32, True, 7)
    got, ema = clone(d0), ema0.clone()
    pad = torch.zeros(65, device=DEV)
    cases = [(lambda: run_plain(got, ema, 0.0), "ema_rate"), (lambda: run_plain(got, ema, 1.5), "ema_rate"),
             (lambda: run_plain(got, ema, float("nan")), "ema_rate"), (lambda: run_scaled(got, ema, -1.0, gs_state(0.0)), "ema_rate"),
             (lambda: run_scaled(got, ema, float("nan"), gs_state(0.0)), "ema_rate"),
             (lambda: run_plain(got, pad[1:], 0.1), "16-byte aligned"), (lambda: run_scaled(got, pad[1:], 0.1, gs_state(0.0)), "16-byte aligned")]
    for fn, msg in cases:
        with pytest.raises(HipLibraryError, match=msg):
            fn()
    with pytest.raises(ValueError, match="p's size"):
        run_plain(got, torch.zeros(63, device=DEV), 0.1)
    with pytest.raises(ValueError, match="p's size"):
        run_plain(got, torch.zeros(64, device=DEV, dtype=torch.float64), 0.1)
    torch.cuda.synchronize()
    for key in ("p", "m", "v", "sh"):
        assert same_bits(got[key], d0[key]), key
    assert same_bits(ema, ema0) and not pad.any()
