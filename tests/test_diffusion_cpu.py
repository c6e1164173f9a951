"""DDPM training and sampling without a GPU: the binding of the entry points of csrc/diffusion.hip and of the time-token kernels, their
argument validation (before any HIP call), the scheduler tables against the reference's (ddpm_schedule.npz), the reverse-step coefficients,
the float64 restatement of the model (tests/diffusion_ref.py) against both reference fixtures, and what the modules do off the device."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import diffusion_ref as DRF
from conftest import GOLDEN, ROOT, load_golden, rel_err

NEW = ("ucfvit_ddpm_q_sample", "ucfvit_time_tokens_fwd", "ucfvit_time_tokens_bwd_workspace", "ucfvit_time_tokens_bwd", "ucfvit_relu_dropout",
       "ucfvit_relu_dropout_bwd", "ucfvit_ddpm_step")


def _lib():
    from UCF_VIT._hip import lib
    return lib, lib.load()


def _golden(name):
    """load_golden for a fixture that also holds the state_dict's key list (a string array)"""
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
        keys = [str(k) for k in z["sd_keys"]]
        return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files if k != "sd_keys"}, keys


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


def test_argument_validation_needs_no_gpu():
    lib, L = _lib()
    buf = (ctypes.c_float * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15                          # 16-byte aligned, far from the buffer's end
    dims = (ctypes.c_int64 * 3)(8, 8, 1)
    err = lambda: L.ucfvit_last_error().decode()

    def qs(x0=p, eps=p, t=p, a=p, b=p, out=p, B=2, n=12, T=10):
        return L.ucfvit_ddpm_q_sample(x0, eps, t, a, b, out, B, n, T, None)

    for k in ("x0", "eps", "t", "a", "b", "out"):
        assert qs(**{k: None}) == -1 and "ucfvit_ddpm_q_sample" in err() and "null pointer" in err(), k
    assert qs(B=-1) == -1 and "bad sizes" in err()
    assert qs(n=0) == -1 and "bad sizes" in err()
    assert qs(T=0) == -1 and "T=0" in err()
    assert qs(x0=p + 2) == -1 and "misaligned" in err()
    assert qs(t=p + 4) == -1 and "misaligned" in err()
    assert qs(B=0) == 0                                             # nothing to do, no launch

    def tf(patches=p, cls=p, pos=p, temb=p, out=p, B=2, Lp=3, D=8, has_cls=1, dtype=lib.F32):
        return L.ucfvit_time_tokens_fwd(patches, cls, pos, temb, out, B, Lp, D, has_cls, dtype, None)

    assert tf(patches=None) == -1 and "ucfvit_time_tokens_fwd" in err() and "null pointer" in err()
    assert tf(temb=None) == -1 and "null pointer" in err()
    assert tf(out=None) == -1 and "null pointer" in err()
    assert tf(cls=None) == -1 and "has_cls without cls" in err()
    assert tf(D=6) == -1 and "multiple of 4" in err()
    assert tf(D=12, dtype=lib.BF16) == -1 and "multiple of 8" in err()
    assert tf(dtype=9) == -1 and "dtype" in err()
    assert tf(temb=p + 4) == -1 and "16-byte aligned" in err()
    assert tf(D=0) == -1 and "bad sizes" in err()
    assert tf(B=0) == 0

    def tb(dout=p, dpatches=p, dpos=p, dcls=p, dtemb=p, B=2, Lp=3, D=8, has_cls=1, acc=0, ws=p, dtype=lib.F32):
        return L.ucfvit_time_tokens_bwd(dout, dpatches, dpos, dcls, dtemb, B, Lp, D, has_cls, acc, ws, dtype, None)

    assert tb(dout=None) == -1 and "ucfvit_time_tokens_bwd" in err() and "null pointer" in err()
    assert tb(dtemb=None) == -1 and "null pointer" in err()
    assert tb(ws=None) == -1 and "null pointer" in err()
    assert tb(D=6) == -1 and "multiple of 4" in err()
    assert tb(dtype=-1) == -1 and "dtype" in err()
    assert tb(dout=p + 4) == -1 and "16-byte aligned" in err()
    assert tb(Lp=0, has_cls=0) == -1 and "no token rows" in err()
    assert tb(B=0) == 0
    assert L.ucfvit_time_tokens_bwd_workspace(2, 3, 8, 1) == 1 * 2 * 8 * 4            # 4 rows: one chunk of 8
    assert L.ucfvit_time_tokens_bwd_workspace(2, 197, 1024, 0) == 25 * 2 * 1024 * 4   # 197 rows: 25 chunks
    assert L.ucfvit_time_tokens_bwd_workspace(0, 3, 8, 1) == 0 and L.ucfvit_time_tokens_bwd_workspace(2, 3, 0, 1) == 0

    def rd(x=p, out=p, rows=4, D=8, prob=0.5, dtype=lib.F32):
        return L.ucfvit_relu_dropout(x, out, rows, D, prob, 7, dtype, None)

    def rb(x=p, dy=p, dx=p, rows=4, D=8, prob=0.5, dtype=lib.F32):
        return L.ucfvit_relu_dropout_bwd(x, dy, dx, rows, D, prob, 7, dtype, None)

    assert rd(x=None) == -1 and "ucfvit_relu_dropout:" in err() and "null pointer" in err()
    assert rd(out=None) == -1 and "null pointer" in err()
    assert rd(D=0) == -1 and "D=0" in err()
    assert rd(rows=-1) == -1 and "row count -1" in err()
    assert rd(prob=1.0) == -1 and "[0, 1)" in err()
    assert rd(prob=-0.1) == -1 and "[0, 1)" in err()
    assert rd(prob=float("nan")) == -1 and "[0, 1)" in err()
    assert rd(dtype=5) == -1 and "dtype" in err()
    assert rd(rows=0) == 0
    assert rb(x=None) == -1 and "ucfvit_relu_dropout_bwd" in err() and "null pointer" in err()
    assert rb(dy=None) == -1 and rb(dx=None) == -1
    assert rb(prob=1.5) == -1 and "[0, 1)" in err()
    assert rb(D=-2) == -1 and rb(dtype=5) == -1 and rb(rows=0) == 0

    def st(x=p, pred=p, z=p, out=p, B=1, C=1, dm=dims, nd=2, ps=4, c1=1.0, c2=1.0, sigma=0.5, dtype=lib.F32):
        return L.ucfvit_ddpm_step(x, pred, z, out, B, C, dm, nd, ps, c1, c2, sigma, dtype, None)

    assert st(x=None) == -1 and "ucfvit_ddpm_step" in err() and "null pointer" in err()
    assert st(pred=None) == -1 and st(out=None) == -1 and st(dm=None) == -1
    assert st(nd=1) == -1 and "nd must be 2 or 3" in err()
    assert st(nd=4) == -1 and "nd must be 2 or 3" in err()
    assert st(dtype=3) == -1 and "dtype" in err()
    assert st(ps=3) == -1 and "not a multiple of p=3" in err()
    assert st(ps=0) == -1 and "bad sizes" in err()
    assert st(C=0) == -1 and "bad sizes" in err()
    assert st(z=None, sigma=0.5) == -1 and "without noise" in err()
    assert st(x=p + 2) == -1 and "misaligned" in err()
    big = (ctypes.c_int64 * 3)(1 << 16, 1 << 16, 1)
    assert st(dm=big) == -1 and "2^31" in err()
    assert st(B=0) == 0


def test_ops_and_modules_refuse_cpu_tensors():
    from UCF_VIT._hip import functional as HF
    from UCF_VIT._hip import ops
    from UCF_VIT.ddpm.ddpm import DDPM_Scheduler
    from UCF_VIT.simple.arch import DiffusionVIT
    x = torch.zeros(2, 3, 8, 8)
    t = torch.tensor([0, 1])
    tab = torch.ones(10)
    no_cpu = dict(match="there is no CPU path")
    with pytest.raises(RuntimeError, **no_cpu):
        ops.ddpm_q_sample(x, x, t, tab, tab)
    with pytest.raises(RuntimeError, **no_cpu):
        ops.time_tokens_fwd(torch.zeros(6, 8), None, None, torch.zeros(2, 8), 2, 3, 8)
    with pytest.raises(RuntimeError, **no_cpu):
        ops.time_tokens_bwd(torch.zeros(2, 3, 8), 2, 3, 8, False, False)
    with pytest.raises(RuntimeError, **no_cpu):
        ops.relu_dropout(torch.zeros(4, 8), 0.5, 1)
    with pytest.raises(RuntimeError, **no_cpu):
        ops.relu_dropout_bwd(torch.zeros(4, 8), torch.zeros(4, 8), 0.5, 1)
    with pytest.raises(RuntimeError, **no_cpu):
        ops.ddpm_step(x, torch.zeros(2, 4, 48), None, 4, 1.0, 1.0, 0.0)
    with pytest.raises(RuntimeError, **no_cpu):
        HF.q_sample(x, t, x, tab, tab)
    s = DDPM_Scheduler(10)
    with pytest.raises(RuntimeError, **no_cpu):
        s.q_sample(x, t, x)
    with pytest.raises(RuntimeError, **no_cpu):
        s.step(x, torch.zeros(2, 4, 48), 0, None, 4)
    m = DiffusionVIT(**DRF.SMALL_KW).eval()
    with pytest.raises(RuntimeError, **no_cpu):
        m.temporalEmbeddings(x, t)
    with pytest.raises(RuntimeError, **no_cpu):
        m.timeEmbeddingMap(torch.zeros(2, 64))
    with pytest.raises(RuntimeError, match="is on cpu"):            # the whole model: its parameter store refuses first
        m(torch.zeros(2, 3, 32, 32), t, None)
    with pytest.raises(TypeError, match="integer tensor"):
        m.temporalEmbeddings(x, [0, 1])
    with pytest.raises(IndexError, match=r"outside \[0, 10\)"):
        m.temporalEmbeddings(x, torch.tensor([0, 10]))
    # wrapper checks that come before the library
    with pytest.raises(ValueError, match="0 <= p < 1"):
        ops._chk_relu_dropout(1.0, 0, "relu_dropout")
    with pytest.raises(ValueError, match="needs noise"):
        s.step(x, torch.zeros(2, 4, 48), 3, None, 4)


def test_scheduler_tables_equal_the_reference_bit_for_bit():
    from UCF_VIT.ddpm.ddpm import DDPM_Scheduler
    g = load_golden("ddpm_schedule.npz")
    s = DDPM_Scheduler(1000)
    assert s.beta.dtype == s.alpha.dtype == torch.float32
    assert torch.equal(s.beta, g["beta"]) and torch.equal(s.alpha, g["alpha"])
    assert s.state_dict() == {} and {"beta", "alpha", "sqrt_ab", "sqrt_1mab"} <= dict(s.named_buffers()).keys()
    t = torch.tensor([0, 17, 999])
    b, a = s(t)
    assert torch.equal(b, g["beta"][t]) and torch.equal(a, g["alpha"][t])
    a64 = g["alpha"].double()
    assert torch.equal(s.sqrt_ab, a64.sqrt().float()) and torch.equal(s.sqrt_1mab, (1 - a64).sqrt().float())
    assert DDPM_Scheduler().num_time_steps == 1000


def test_step_coefficients_are_the_float64_formula_rounded_once():
    from UCF_VIT.ddpm.ddpm import DDPM_Scheduler
    g = load_golden("ddpm_schedule.npz")
    s = DDPM_Scheduler(1000)
    beta, abar = g["beta"].double().numpy(), g["alpha"].double().numpy()
    for i in (0, 1, 2, 500, 998, 999):
        c1, c2, sigma = s.coefficients(i)
        assert c1 == float(np.float32(1.0 / math.sqrt(1.0 - beta[i])))
        assert c2 == float(np.float32(beta[i] / math.sqrt(1.0 - abar[i])))
        assert sigma == (float(np.float32(math.sqrt(beta[i]))) if i else 0.0)
    for bad in (-1, 1000):
        with pytest.raises(ValueError, match="outside"):
            s.coefficients(bad)


@pytest.mark.parametrize("name", list(DRF.FIXTURES))
def test_fp64_restatement_reproduces_the_reference_model(name):
    """Yardstick validation: diffusion_ref.model64 in float64 against the reference DiffusionVIT of the fixture: output, input gradient and
    every parameter gradient, conftest.rel_err < 1e-5 (the bound of test_qk_norm_cpu's restatement test)."""
    from UCF_VIT.simple.arch import DiffusionVIT
    g, keys = _golden(name)
    kw = DRF.FIXTURES[name]
    sd = DRF.fixture_state_dict(DiffusionVIT(**kw), g)
    P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x = g["x"].double().requires_grad_(True)
    y = DRF.model64(P, kw, x, g["t"], None)
    y.backward(g["gy"].double())
    assert rel_err(y, g["y"]) < 1e-5 and rel_err(x.grad, g["gx"]) < 1e-5
    worst = 0.0
    for k in (k[2:] for k in g if k.startswith("g.")):
        e = rel_err(P[k].grad, g["g." + k])
        worst = max(worst, e)
        assert e < 1e-5, (k, e)
    print(f"{name}: worst gradient rel_err {worst:.2e}")


@pytest.mark.parametrize("name", list(DRF.FIXTURES))
def test_state_dict_keys_match_the_fixture(name):
    from UCF_VIT.simple.arch import DiffusionVIT
    g, keys = _golden(name)
    m = DiffusionVIT(**DRF.FIXTURES[name])
    assert list(m.state_dict()) == keys
    assert {k[2:] for k in g if k.startswith("g.")} == {k for k, _ in m.named_parameters()}
    assert {k[2:]: tuple(v.shape) for k, v in g.items() if k.startswith("w.")} == \
        {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("timeEmbeddingMap.") or k == "decoder_pos_embed"}
    from UCF_VIT.simple import building_blocks as S
    assert type(m.timeEmbeddingMap.linear1) is S.Linear and type(m.timeEmbeddingMap.linear2) is S.Linear
    assert type(m.timeEmbeddingMap.dropout) is S.HipDropout and m.timeEmbeddingMap.dropout.p == 0.5
    assert not m.eval().timeEmbeddingMap.dropout.active() and m.train().timeEmbeddingMap.dropout.active()
    assert "temporalEmbeddings.embeddings" in dict(m.named_buffers()) and not any("temporalEmbeddings" in k for k in keys)
    assert torch.equal(m.temporalEmbeddings.embeddings.double(), DRF.time_table(10, m.embed_dim))


def test_unsupported_configurations_raise():
    from UCF_VIT.simple.arch import DiffusionVIT
    x, t = torch.zeros(2, 3, 32, 32), torch.tensor([1, 7])
    m = DiffusionVIT(**DRF.SMALL_KW)
    m.use_adaptive_pos_emb = True
    with pytest.raises(NotImplementedError, match="use_adaptive_pos_emb"):
        m(x, t, None)
    m = DiffusionVIT(**DRF.SMALL_KW)
    m.tensor_par_size, m.tensor_par_group = 2, "my_tp_group"
    with pytest.raises(NotImplementedError, match="dropout p=0.5 under a tensor-parallel group.*my_tp_group.*same seed"):
        m.train()(x, t, None)
    m = DiffusionVIT(**DRF.SMALL_KW)
    m.seq_par_size = 2
    with pytest.raises(NotImplementedError, match="dropout p=0.5 under a sequence-parallel group.*2 ranks.*same seed"):
        m.train()(x, t, None)
    with pytest.raises(RuntimeError, match="is on cpu"):            # eval: no active dropout, the group is not refused; the CPU model is
        m.eval()(x, t, None)
    import UCF_VIT.fsdp.arch as FA
    assert not hasattr(FA, "DiffusionVIT")


def test_config_keys_reach_the_model_arguments():
    import yaml
    sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd", "training_scripts"))
    try:
        import train_diffusion_simple as T
    finally:
        sys.path.pop(0)
    conf = yaml.safe_load(open(os.path.join(ROOT, "ucf-vit_amd", "configs", "diffusion_smoke.yaml")))
    margs, a, d = T.diffusion_args(conf)
    assert margs["time_steps"] == 10 and margs["class_token"] is False and margs["img_size"] == [32, 32] and margs["patch_size"] == 8
    assert margs["decoder_embed_dim"] == 32 and margs["decoder_depth"] == 1 and margs["linear_decoder"] is False
    assert conf["model"]["loss_fn"] == "MSE" and conf["model"]["use_grad_scaler"] is False
    conf["model"]["net"]["init_args"]["num_time_steps"] = 1000
    assert T.diffusion_args(conf)[0]["time_steps"] == 1000
    from UCF_VIT.simple.arch import DiffusionVIT
    m = DiffusionVIT(weight_init='skip', **T.diffusion_args(conf)[0])
    assert m.temporalEmbeddings.embeddings.shape == (1000, 64)
    import _common
    assert _common.seed_dropout(m, "cpu", 0) == 1 and m.timeEmbeddingMap.dropout.generator is not None
