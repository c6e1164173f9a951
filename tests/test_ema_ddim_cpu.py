"""The weights' moving average and the DDIM sampler without a GPU: binding of ucfvit_adamw_ema / ucfvit_adamw_scaled_ema / ucfvit_ddim_step,
their argument validation (before any HIP call), the strided schedule and its coefficients against float64, what the Python layers refuse,
the sampler's point-mass identity on the fp32 restatement of the step (tests/ddim_ref.py), and the host half of the moving average's bound."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ddim_ref as R
from conftest import ROOT

NEW = ("ucfvit_adamw_ema", "ucfvit_adamw_scaled_ema", "ucfvit_ddim_step")
F = np.float32


def _lib():
    from UCF_VIT._hip import lib
    return lib, lib.load()


def _sched(T=1000):
    from UCF_VIT.ddpm.ddpm import DDPM_Scheduler
    s = DDPM_Scheduler(T)
    return s, s.alpha.double().numpy()


def test_binding_arity_and_abi_version():
    lib, L = _lib()
    header = open(os.path.join(ROOT, "include", "ucfvit_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert name in lib.SIGNATURES
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(lib.SIGNATURES[name][1]), name
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NEW) <= set(re.findall(r"\bT (ucfvit_[a-z0-9_]+)", out))
    assert lib.ABI_VERSION == L.ucfvit_abi_version() == 24          # symbols were only added


@pytest.mark.parametrize("T,Ss", [(1000, (1, 2, 3, 7, 50, 999, 1000)), (5, (1, 2, 3, 4, 5))])
def test_ddim_timesteps(T, Ss):
    s, _ = _sched(T)
    for S in Ss:
        tau = s.ddim_timesteps(S)
        assert tau == R.ddim_timesteps(T, S)
        assert len(tau) == S and tau[-1] == T - 1 and tau[0] >= 0
        assert all(b > a for a, b in zip(tau, tau[1:]))
        if S > 1:
            assert tau[0] == 0
            # k (T-1) / (S-1) rounded to the nearest step
            assert all(abs(t - k * (T - 1) / (S - 1)) <= 0.5 for k, t in enumerate(tau))
        if S == T:
            assert tau == list(range(T))


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_ddim_coefficients_against_float64(eta):
    s, alpha = _sched(1000)
    for i, ip in R.pairs(1000, 7):
        got = s.ddim_coefficients(i, ip, eta)
        c = R.ddim_coefficients64(alpha, i, ip, eta)
        assert len(got) == 7
        for k, g in zip(R.ORDER, got):
            assert isinstance(g, float) and g == float(F(c[k])), (i, ip, k)                    # float64, rounded once
        assert abs(c["c_eps"] ** 2 + c["sigma"] ** 2 - (1.0 - c["ab_prev"])) <= 1e-12
        assert abs(c["s_ab"] * c["r_ab"] - 1.0) <= 1e-15 and abs(c["s_1mab"] * c["r_1mab"] - 1.0) <= 1e-15
        if eta == 0.0:
            assert got[6] == 0.0
        elif ip >= 0:
            assert got[6] > 0.0
        if ip < 0:
            assert got[4] == 1.0 and got[5] == 0.0 and got[6] == 0.0                           # the last step returns x0_hat itself
    # eta = 1 over every step is the ancestral sampler's variance: sigma_i^2 = beta_i (1 - abar_{i-1}) / (1 - abar_i)
    if eta == 1.0:
        beta = s.beta.double().numpy()
        for i in (1, 2, 500, 999):
            c = R.ddim_coefficients64(alpha, i, i - 1, 1.0)
            # the table is fp32: abar_i = fl(abar_{i-1} fl(1 - beta_i)), two roundings of 2^-24 relative, so 1 - abar_i / abar_{i-1} is beta_i
            # to 2^-23 absolute
            ratio = (1 - alpha[i - 1]) / (1 - alpha[i])
            assert abs(c["sigma"] ** 2 - beta[i] * ratio) <= 2.0 ** -23 * ratio


def test_python_layers_refuse():
    from UCF_VIT._hip import functional as HF
    from UCF_VIT._hip import ops
    from UCF_VIT._hip.optim import HipAdamW
    from UCF_VIT.utils.misc import configure_optimizer
    s, _ = _sched(10)
    for S in (0, -1, 11):
        with pytest.raises(ValueError, match="num_steps"):
            s.ddim_timesteps(S)
    for eta in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="eta"):
            s.ddim_coefficients(5, 2, eta)
    for i, ip in ((5, 5), (5, 7), (10, 2), (3, -2)):
        with pytest.raises(ValueError, match="steps"):
            s.ddim_coefficients(i, ip, 0.0)
    w = torch.nn.Parameter(torch.zeros(8))
    for d in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            HipAdamW([w], ema_decay=d)
        with pytest.raises(ValueError, match="ema_decay"):
            configure_optimizer(torch.nn.Linear(2, 2), 1e-3, 0.9, 0.95, 0.0, ema_decay=d)
    assert HipAdamW([w], ema_decay=0.0)._ema_rate == 1.0
    opt = HipAdamW([w], ema_decay=0.9999)
    assert opt._ema_rate == 1.0 - 0.9999 and opt.ema_decay == 0.9999                           # the double, not a float's 1 - decay
    assert HipAdamW([w])._ema_rate is None
    with pytest.raises(RuntimeError, match="keeps no average"):
        HipAdamW([w]).load_ema_state_dict(torch.nn.Linear(2, 2), {})
    assert "ema" not in "".join(map(str, opt.state_dict().keys())) and opt.state_dict()["state"] == {}
    x = torch.zeros(2, 3, 8, 8)
    pred = torch.zeros(2, 4, 48)
    coef = (0.8, 0.6, 1.25, 1 / 0.6, 0.9, 0.4, 0.0)
    no_cpu = dict(match="there is no CPU path")
    with pytest.raises(RuntimeError, **no_cpu):
        ops.ddim_step(x, pred, None, 4, *coef)
    with pytest.raises(RuntimeError, **no_cpu):
        HF.ddim_step(x, pred, None, 4, coef)
    with pytest.raises(RuntimeError, **no_cpu):
        s.ddim_step(x, pred, 5, 2, None, 4)
    for clip in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="clip"):
            ops.ddim_step(x, pred, None, 4, *coef, clip=clip)
        with pytest.raises(ValueError, match="clip"):
            s.ddim_step(x, pred, 5, 2, None, 4, clip=clip)
        with pytest.raises(ValueError, match="clip"):
            s.sample_ddim(None, (1, 3, 8, 8), None, num_steps=2, clip_denoised=clip)
    with pytest.raises(ValueError, match="needs noise"):
        s.ddim_step(x, pred, 5, 2, None, 4, eta=1.0)
    t8 = torch.zeros(8)
    with pytest.raises(RuntimeError, **no_cpu):
        ops.adamw_ema(t8, t8, t8, t8, None, t8, 1e-3, 0.9, 0.95, 1e-8, 0.0, 1, 0.1)
    with pytest.raises(RuntimeError, **no_cpu):
        ops.adamw_scaled_ema(t8, t8, t8, t8, None, t8, 1e-3, 0.9, 0.95, 1e-8, 0.0, torch.zeros(16), 0.1)


def test_argument_validation_needs_no_gpu():
    lib, L = _lib()
    buf = (ctypes.c_float * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15
    err = lambda: L.ucfvit_last_error().decode()

    def ae(pp=p, g=p, m=p, v=p, sh=p, ema=p, n=8, rate=0.1, dtype=lib.F32):
        return L.ucfvit_adamw_ema(pp, g, m, v, sh, ema, n, 1e-3, 0.9, 0.95, 1e-8, 0.0, 0.1, 0.05, 1.0, rate, dtype, None)

    def se(pp=p, g=p, m=p, v=p, sh=p, ema=p, n=8, rate=0.1, dtype=lib.F32, state=p):
        return L.ucfvit_adamw_scaled_ema(pp, g, m, v, sh, ema, n, 1e-3, 0.9, 0.95, 1e-8, 0.0, 1.0, rate, dtype, state, None)

    for fn, name in ((ae, "ucfvit_adamw_ema:"), (se, "ucfvit_adamw_scaled_ema:")):
        assert fn(ema=None) == -1 and name in err() and "null pointer" in err()
        assert fn(pp=None) == -1 and "null pointer" in err()
        assert fn(ema=p + 4) == -1 and "16-byte aligned" in err()
        assert fn(ema=p + 8) == -1 and "16-byte aligned" in err()
        for r in (0.0, -0.5, 1.5, float("nan"), float("inf")):
            assert fn(rate=r) == -1 and "ema_rate" in err() and "(0, 1]" in err(), r
        assert fn(n=-1) == -1 and "negative size" in err()
        assert fn(dtype=7) == -1 and "dtype" in err()
        assert fn(n=0) == 0 and fn(n=0, rate=1.0) == 0                                          # nothing to do, no launch
    assert se(state=None) == -1 and "null state" in err()

    dims = (ctypes.c_int64 * 3)(8, 8, 1)

    def st(x=p, pred=p, z=p, out=p, B=1, C=1, dm=dims, nd=2, ps=4, sigma=0.5, clip=0.0, dtype=lib.F32):
        return L.ucfvit_ddim_step(x, pred, z, out, B, C, dm, nd, ps, 0.8, 0.6, 1.25, 1.0 / 0.6, 0.9, 0.4, sigma, clip, dtype, None)

    assert st(x=None) == -1 and "ucfvit_ddim_step" in err() and "null pointer" in err()
    assert st(pred=None) == -1 and st(out=None) == -1 and st(dm=None) == -1
    assert st(nd=1) == -1 and "nd must be 2 or 3" in err()
    assert st(dtype=3) == -1 and "dtype" in err()
    assert st(ps=3) == -1 and "not a multiple of p=3" in err()
    assert st(ps=0) == -1 and "bad sizes" in err()
    assert st(z=None, sigma=0.5) == -1 and "without noise" in err()
    assert st(x=p + 2) == -1 and "misaligned" in err()
    assert st(clip=-1.0) == -1 and "clip" in err()
    assert st(clip=float("nan")) == -1 and "clip" in err()
    big = (ctypes.c_int64 * 3)(1 << 16, 1 << 16, 1)
    assert st(dm=big) == -1 and "2^31" in err()
    assert st(B=0) == 0 and st(B=0, clip=1.0, z=None, sigma=0.0) == 0


@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("S", [1, 2, 3, 7, 50, 1000])
def test_point_mass_identity_on_the_fp32_restatement(S, eta, clip):
    """With the data distribution a point mass at c the exact noise prediction is eps_hat = (x - sqrt(abar) c) / sqrt(1 - abar), and every
    sampler of the family returns c from any x_T: x0_hat = c at every step, and the last step returns x0_hat.  In fp32 the last step computes
    x0_hat = (x - s_1mab e) r_ab at abar of tau_0: step 0 for S >= 2 (abar = 0.9999: the error is a rounding of c), step T-1 for S = 1
    (abar = 4e-5: the roundings of x and e, of size u |x_T|, are amplified by 1 / sqrt(abar) = 157).  Measured on this restatement with these
    inputs: 5.96e-8 for every S >= 2 and 5.6e-5 for S = 1; the bounds are 2^-22 and 2^-12, 4x over those."""
    _, alpha = _sched(1000)
    g = np.random.Generator(np.random.PCG64(17))
    c = g.uniform(-1.0, 1.0, 4096).astype(F)
    x_T = g.standard_normal(4096).astype(F)
    ng = np.random.Generator(np.random.PCG64(18))
    out = R.point_mass_sampler32(alpha, c, x_T, S, eta, clip, lambda k: ng.standard_normal(4096).astype(F))
    err = float(np.abs(out.astype(np.float64) - c.astype(np.float64)).max())
    print(f"S={S} eta={eta} clip={clip}: max |x_0 - c| = {err:.3e}")
    assert err <= (2.0 ** -12 if S == 1 else 2.0 ** -22)


def test_ema_bound_holds_for_both_fp32_evaluations():
    """the host half of tests/test_ema_ops.py's bound: e + r (p - e) in fp32 with the product and the sum rounded separately, and with a
    fused multiply-add (the product exact, one rounding of the sum: evaluated in float64, where the product of two fp32 values and its sum with
    a third of comparable size are exact enough that the one rounding to fp32 is the only one that matters), both inside R.ema_bound"""
    g = np.random.Generator(np.random.PCG64(23))
    n = 100_000
    rate = np.concatenate([np.full(n // 4, v) for v in (1e-4, 1e-2, 1.0)] + [g.uniform(1e-5, 1.0, n - 3 * (n // 4))]).astype(F)
    e = (g.standard_normal(n) * 10.0 ** g.uniform(-3, 2, n)).astype(F)
    gap = (10.0 ** g.uniform(-8, 3, n) * g.choice([-1.0, 1.0], n))
    gap[::7] = 0.0                                                                              # p == e
    gap[1::7] = 1e3
    p = (e.astype(np.float64) + gap).astype(F)
    p[::7] = e[::7]
    d = p - e                                                                                   # fp32
    separate = e + rate * d
    fused = (e.astype(np.float64) + rate.astype(np.float64) * d.astype(np.float64)).astype(F)
    assert separate.dtype == F and d.dtype == F
    want = e.astype(np.float64) + rate.astype(np.float64) * (p.astype(np.float64) - e.astype(np.float64))
    bound = R.U * (2 * rate.astype(np.float64) * np.abs(p.astype(np.float64) - e.astype(np.float64)) + np.abs(want)) * (1 + 2 * R.U)
    # R.ema_bound is the same expression for one rate: check it on the three fixed rates
    for r in (1e-4, 1e-2, 1.0):
        sel = rate == F(r)
        assert sel.sum() >= n // 4
        assert np.array_equal(R.ema_bound(e[sel], p[sel], r), bound[sel]) and np.array_equal(R.ema64(e[sel], p[sel], r), want[sel])
    for name, got in (("separate", separate), ("fused", fused)):
        err = np.abs(got.astype(np.float64) - want)
        worst = float(np.max(err / np.maximum(bound, 1e-300)))
        print(f"{name}: worst err / bound = {worst:.3f}")
        assert (err <= bound).all()
        assert np.array_equal(got[::7], e[::7])                                                 # exact where p == e
    # rate 1 returns p itself wherever p - e is exact, which Sterbenz's lemma gives for e / 2 <= p <= 2 e (tests/test_ema_ops.py relies on it)
    sel = (rate == F(1.0)) & (np.abs(gap) <= 0.5 * np.abs(e))
    assert sel.sum() > 1000 and np.array_equal(separate[sel], p[sel]) and np.array_equal(fused[sel], p[sel])
