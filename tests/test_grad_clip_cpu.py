"""Gradient clipping by global norm without a GPU: the float64 helper against torch.nn.utils.clip_grad_norm_, the constructor and
sharded-parameter refusals of HipAdamW, the library's argument checks (made before any HIP call), the host-only partial count, and that an
optimizer without max_grad_norm binds nothing."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import grad_clip_ref as R
from UCF_VIT._hip.lib import GC_COEF, GC_MAX_NORM, GC_NORM, GC_STATE_FLOATS          # the state block all of this is about


def _f(x):
    return ctypes.c_float(x)


# ============================================================================================== the helper against torch in float64
def _torch_clip(tensors, max_norm):
    ps = [torch.nn.Parameter(torch.zeros(t.shape, dtype=torch.float64)) for t in tensors]
    for p, t in zip(ps, tensors):
        p.grad = t.double().clone()
    norm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    return norm, [p.grad for p in ps]


@pytest.mark.parametrize("case", ["below", "above", "zero", "scaled"])
def test_helper_matches_torch_clip_grad_norm_in_float64(case):
    g = torch.Generator().manual_seed(11)
    ts = [torch.randn(257, generator=g), torch.randn(3, 64, generator=g) * 3.0, torch.randn(1, generator=g)]
    mult, inv = 1.0, None
    if case == "zero":
        ts = [torch.zeros_like(t) for t in ts]
    if case == "scaled":
        mult, inv = 0.5, 0.25                                       # powers of two: fl32(g * k) is g * k exactly
    k = mult * (1.0 if inv is None else inv)
    norm_t = float(torch.sqrt(sum((t.double() * k).pow(2).sum() for t in ts)))
    max_norm = {"below": 2.0 * norm_t, "above": 0.25 * norm_t, "zero": 1.0, "scaled": 0.5 * norm_t}[case]
    norm_ref, clipped = _torch_clip([t.double() * k for t in ts], max_norm)
    norm = R.norm64([t.numpy() for t in ts], mult, inv)
    assert abs(norm - norm_ref) <= 4 * R.U64 * norm_ref
    coef = R.coef64(norm, max_norm)
    assert (coef == 1.0) == (case in ("below", "zero"))
    for t, c in zip(ts, clipped):
        want = t.double() * k * coef
        assert torch.allclose(c, want, rtol=1e-7, atol=0.0)      # float(np.float32(max_norm)) against torch's double max_norm: 6e-8
    assert R.coef64(float("inf"), 1.0) == 0.0 and math.isnan(R.coef64(float("nan"), 1.0))


def test_products_are_rounded_to_fp32_before_squaring():
    g = np.array([1.0 + 2.0 ** -23, 3.0], dtype=np.float32)
    x = R.products(g, mult=1.0 / 3.0)
    assert x.dtype == np.float64 and np.array_equal(x, (g * np.float32(1.0 / 3.0)).astype(np.float64))
    assert R.products(g, 0.5, 0.1)[1] == float(np.float32(3.0) * np.float32(np.float32(0.5) * np.float32(0.1)))
    assert R.U32 < R.norm_rel_bound(2 ** 22, 2048) < 1.01 * R.U32          # the double accumulation costs 2^-32 of the 2^-24


# ============================================================================================== HipAdamW's host side
@pytest.mark.parametrize("bad", [0.0, -1.0, float("inf"), float("nan"), 1, True, "1.0", torch.tensor(1.0)])
def test_constructor_refuses_bad_thresholds(bad):
    from UCF_VIT._hip.optim import HipAdamW
    from UCF_VIT.utils.misc import configure_optimizer
    w = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="max_grad_norm"):
        HipAdamW([w], max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        configure_optimizer(torch.nn.Linear(2, 2), 1e-3, 0.9, 0.95, 0.0, max_grad_norm=bad)
    opt = HipAdamW([w], max_grad_norm=1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.max_grad_norm = bad
    assert opt.max_grad_norm == 1.0


def test_threshold_is_kept_settable_and_out_of_state_dict():
    from UCF_VIT._hip.optim import HipAdamW
    from UCF_VIT.utils.misc import configure_optimizer
    w = torch.nn.Parameter(torch.zeros(4))
    plain, opt = HipAdamW([w]), HipAdamW([w], max_grad_norm=0.5)
    assert plain.max_grad_norm is None and opt.max_grad_norm == 0.5
    opt.max_grad_norm = 2.0
    assert opt.max_grad_norm == 2.0
    assert opt._gc is None and opt._gc_ws is None                      # nothing is allocated before the first clipped step
    assert opt.state_dict().keys() == plain.state_dict().keys()
    assert opt.state_dict()["param_groups"][0].keys() == plain.state_dict()["param_groups"][0].keys()
    assert configure_optimizer(torch.nn.Linear(2, 2), 1e-3, 0.9, 0.95, 0.0, max_grad_norm=3.0).max_grad_norm == 3.0
    assert configure_optimizer(torch.nn.Linear(2, 2), 1e-3, 0.9, 0.95, 0.0).max_grad_norm is None
    with pytest.raises(RuntimeError, match="does not clip"):
        plain.grad_norm()


def test_clipping_refuses_sharded_parameters():
    from UCF_VIT._hip.grad_scaler import HipGradScaler
    from UCF_VIT._hip.optim import HipAdamW
    w = torch.nn.Parameter(torch.zeros(4))
    w.grad = torch.zeros(4)
    w._ucf_sharded = "sequence"
    opt = HipAdamW([w], max_grad_norm=1.0)
    with pytest.raises(NotImplementedError, match="sequence-parallel.*sum over the group"):
        opt.step()
    with pytest.raises(NotImplementedError, match="sequence-parallel"):
        HipGradScaler().step(opt)
    assert opt._gc is None


def test_without_max_grad_norm_nothing_is_bound(monkeypatch):
    """max_grad_norm=None: no clip state, no workspace, and step() reaches none of the new ops (replaced by a tripwire) but ops.adamw
    (replaced by a recorder: the tensors are on the host); with a threshold the same step asks for the partial count first"""
    from UCF_VIT._hip import ops
    from UCF_VIT._hip.optim import HipAdamW
    calls = []

    def tripwire(*a, **k):
        raise AssertionError("a clipping op was called")

    for name in ("grad_sqnorm_partials", "grad_sqnorm", "grad_clip_coef", "clipped_adamw"):
        monkeypatch.setattr(ops, name, tripwire)
    monkeypatch.setattr(ops, "adamw", lambda *a, **k: calls.append("adamw"))
    w = torch.nn.Parameter(torch.zeros(4))
    w.grad = torch.zeros(4)
    opt = HipAdamW([w])
    opt.step()
    assert calls == ["adamw"] and opt._gc is None and opt._gc_ws is None
    with pytest.raises(AssertionError, match="a clipping op was called"):
        HipAdamW([w], max_grad_norm=1.0).step()
    assert calls == ["adamw"]


# ============================================================================================== the library without a device
def test_state_layout_constants_match_the_header():
    from conftest import ROOT
    from UCF_VIT._hip import lib
    txt = open(os.path.join(ROOT, "include", "ucfvit_hip.h")).read()
    defs = dict(re.findall(r"#define UCFVIT_GC_([A-Z_]+) (\d+)", txt))
    assert set(defs) == {"MAX_NORM", "NORM", "COEF", "STATE_FLOATS"}
    for name, value in defs.items():
        assert getattr(lib, "GC_" + name) == int(value), name
    assert sorted((GC_MAX_NORM, GC_NORM, GC_COEF)) == [0, 1, 2] and GC_STATE_FLOATS >= 4 and GC_STATE_FLOATS % 4 == 0
    assert lib.ABI_VERSION == 24


def test_partial_counts():
    from UCF_VIT._hip import lib
    L = lib.load()
    P = L.ucfvit_grad_sqnorm_partials
    assert P(0, lib.F32) == 0 and P(0, lib.BF16) == 0
    assert P(1, lib.F32) == 1 and P(1, lib.BF16) == 1
    assert P(1024, lib.F32) == 1 and P(1025, lib.F32) == 2              # 256 threads x 4 floats per workgroup
    assert P(2048, lib.BF16) == 1 and P(2049, lib.BF16) == 2            # 256 threads x 8 bf16
    assert P(1024 * 1024, lib.F32) == 1024 and P(1024 * 1024 + 1, lib.F32) == 1024      # the grid is capped
    assert P(2 ** 40, lib.F32) == 1024 and P(2 ** 40, lib.BF16) == 1024
    assert P(-1, lib.F32) == -1 and b"ucfvit_grad_sqnorm_partials" in L.ucfvit_last_error()
    assert P(8, 5) == -1 and b"bad dtype" in L.ucfvit_last_error()


def test_entry_points_reject_bad_arguments_without_gpu():
    from UCF_VIT._hip import lib
    L = lib.load()
    buf = (ctypes.c_float * 96)()                      # host memory: only its (16-byte aligned) address is looked at
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    st, ws = a + 64, a + 128

    def rejected(rc, word):
        msg = L.ucfvit_last_error()
        assert rc == -1 and word in msg, (rc, msg)

    sq = L.ucfvit_grad_sqnorm
    rejected(sq(None, 8, lib.F32, _f(1.0), None, ws, None), b"null pointer")
    rejected(sq(a, 8, lib.F32, _f(1.0), st, None, None), b"null partials")
    rejected(sq(a, -1, lib.F32, _f(1.0), None, ws, None), b"negative size")
    rejected(sq(a, 8, 7, _f(1.0), None, ws, None), b"bad dtype")
    rejected(sq(a + 4, 8, lib.BF16, _f(1.0), None, ws, None), b"16-byte aligned")
    rejected(sq(a, 8, lib.F32, _f(1.0), None, ws + 4, None), b"8-byte aligned")
    rejected(sq(a, 8, lib.F32, _f(1.0), st + 2, ws, None), b"misaligned state")
    assert sq(None, 0, lib.F32, _f(1.0), None, None, None) == 0          # an empty segment is accepted with null pointers and launches nothing

    cc = L.ucfvit_grad_clip_coef
    rejected(cc(ws, -1, st, None), b"negative count")
    rejected(cc(ws, 4, None, None), b"null state")
    rejected(cc(None, 4, st, None), b"null partials")
    rejected(cc(ws + 4, 4, st, None), b"8-byte aligned")
    rejected(cc(ws, 4, st + 2, None), b"misaligned state")

    def adamw(p=a, g=a, m=a, v=a, ema=None, n=8, dtype=lib.F32, rate=0.0, gs=None, gc=st):
        return L.ucfvit_adamw_clipped(p, g, m, v, None, ema, n, _f(1e-3), 0.9, 0.95, _f(1e-8), _f(0.0), _f(0.1), _f(0.05), _f(1.0), _f(rate),
                                      dtype, gs, gc, None)

    rejected(adamw(p=None), b"null pointer")
    rejected(adamw(g=None), b"null pointer")
    rejected(adamw(v=None), b"null pointer")
    rejected(adamw(gc=None), b"null clip state")
    rejected(adamw(n=-3), b"negative size")
    rejected(adamw(dtype=2), b"bad grad dtype")
    rejected(adamw(m=a + 4), b"aligned")
    rejected(adamw(ema=a + 4, rate=0.1), b"aligned")
    rejected(adamw(gs=st + 34), b"aligned")
    rejected(adamw(gc=st + 2), b"aligned")
    rejected(adamw(g=a + 8), b"fp32 grads must be 16-byte aligned")
    for rate in (0.0, 1.5, float("nan")):
        rejected(adamw(ema=a, rate=rate), b"ema_rate")
    assert adamw(n=0) == 0                                               # nothing to do, nothing launched
