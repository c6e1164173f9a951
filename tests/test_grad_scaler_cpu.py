"""The loss scaler's host side without a GPU: argument validation of its three entry points (before any HIP call), the disabled
pass-through, and state_dict compatibility with torch.amp.GradScaler."""
import ctypes

import pytest
import torch


def _f(x):
    return ctypes.c_float(x)


def test_scaler_entry_points_reject_bad_arguments_without_gpu():
    from UCF_VIT._hip import lib
    L = lib.load()
    buf = (ctypes.c_float * 64)()                      # host memory: only its (16-byte aligned) address is looked at
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    st = a + 64

    def rejected(rc, word):
        msg = L.ucfvit_last_error()
        assert rc == -1 and word in msg, (rc, msg)

    rejected(L.ucfvit_grad_nonfinite(None, 8, lib.F32, _f(1.0), st, None), b"null pointer")
    rejected(L.ucfvit_grad_nonfinite(a, 8, lib.F32, _f(1.0), None, None), b"null state")
    rejected(L.ucfvit_grad_nonfinite(a, -1, lib.F32, _f(1.0), st, None), b"negative size")
    rejected(L.ucfvit_grad_nonfinite(a, 8, 7, _f(1.0), st, None), b"bad dtype")
    rejected(L.ucfvit_grad_nonfinite(a + 4, 8, lib.BF16, _f(1.0), st, None), b"16-byte aligned")

    def adamw(p=a, g=a, m=a, v=a, n=8, dtype=lib.F32, state=st):
        return L.ucfvit_adamw_scaled(p, g, m, v, None, n, _f(1e-3), 0.9, 0.95, _f(1e-8), _f(0.0), _f(1.0), dtype, state, None)

    rejected(adamw(p=None), b"null pointer")
    rejected(adamw(g=None), b"null pointer")
    rejected(adamw(v=None), b"null pointer")
    rejected(adamw(state=None), b"null state")
    rejected(adamw(n=-3), b"negative size")
    rejected(adamw(dtype=2), b"bad grad dtype")
    rejected(adamw(m=a + 4), b"aligned")

    rejected(L.ucfvit_grad_scaler_update(None, None), b"null state")
    rejected(L.ucfvit_grad_scaler_update(st + 2, None), b"misaligned")


def test_state_layout_constants_match_the_header():
    import os
    import re
    from conftest import ROOT
    from UCF_VIT._hip import lib
    txt = open(os.path.join(ROOT, "include", "ucfvit_hip.h")).read()
    defs = dict(re.findall(r"#define UCFVIT_GS_([A-Z_]+) (\d+)", txt))
    assert len(defs) == 11
    for name, value in defs.items():
        assert getattr(lib, "GS_" + name) == int(value), name


def test_disabled_scaler_passes_through_to_a_plain_optimizer():
    from UCF_VIT._hip.grad_scaler import HipGradScaler
    torch.manual_seed(0)
    w = torch.nn.Parameter(torch.randn(5))
    w_ref = w.detach().clone()
    opt = torch.optim.SGD([w], lr=0.5)
    sc = HipGradScaler(enabled=False)
    assert not sc.is_enabled()
    loss = (w * w).sum()
    assert sc.scale(loss) is loss
    sc.scale(loss).backward()
    sc.step(opt)
    sc.update()
    assert torch.equal(w.detach(), w_ref - 0.5 * 2 * w_ref)
    assert sc.get_scale() == 1.0 and sc.state_dict() == {}
    sc.load_state_dict({"scale": 4.0})                              # ignored, as torch does when disabled
    assert sc._state is None                                        # never touched a device


def test_unscale_is_refused_with_the_reason():
    from UCF_VIT._hip.grad_scaler import HipGradScaler
    with pytest.raises(NotImplementedError, match="unscaling is folded into AdamW's read, and nothing here clips gradients"):
        HipGradScaler(enabled=False).unscale_(None)


def test_load_state_dict_accepts_a_torch_grad_scaler_dict():
    from UCF_VIT._hip.grad_scaler import HipGradScaler
    ref = torch.amp.GradScaler("cpu", init_scale=512.0, growth_factor=4.0, backoff_factor=0.25, growth_interval=7)
    sd = ref.state_dict()
    assert set(sd) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    sc = HipGradScaler(min_scale=128.0)
    sc.load_state_dict(sd)
    assert sc._state is None                                        # held on the host until a device is needed
    assert sc._init == dict(scale=512.0, growth_factor=4.0, backoff_factor=0.25, growth_interval=7, _growth_tracker=0, min_scale=128.0)
    sc.load_state_dict(dict(sd, min_scale=2.0, _growth_tracker=3))
    assert sc._init["min_scale"] == 2.0 and sc._init["_growth_tracker"] == 3
    with pytest.raises(RuntimeError, match="empty"):
        sc.load_state_dict({})


def test_configure_grad_scaler_uses_the_reference_constants():
    from UCF_VIT.utils.misc import configure_grad_scaler
    sc = configure_grad_scaler(True)
    assert sc.is_enabled() and sc._init == dict(scale=8192.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=100,
                                                min_scale=128.0, _growth_tracker=0)
    assert not configure_grad_scaler(False).is_enabled()


def test_scaler_refuses_sharded_parameters_and_foreign_optimizers():
    from UCF_VIT._hip.grad_scaler import HipGradScaler
    from UCF_VIT._hip.optim import HipAdamW
    w = torch.nn.Parameter(torch.zeros(4))
    sc = HipGradScaler()
    with pytest.raises(TypeError, match="HipAdamW"):
        sc.step(torch.optim.SGD([w], lr=0.1))
    w._ucf_sharded = "tensor"
    with pytest.raises(NotImplementedError, match="tensor-parallel"):
        sc.step(HipAdamW([w]))
