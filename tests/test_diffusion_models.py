"""DiffusionVIT, the DDPM scheduler and the two entry scripts on the MI355X: both reference fixtures in eval(), train() against the float64
restatement with the recorded dropout seed, t on the device, one training iteration, the sampler, and the scripts on the smoke config.
Tolerances: conftest.rel_err below 1e-3 in fp32 and 6e-2 in bf16, the two numbers tests/test_hip_models.py uses for model fixtures."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import diffusion_ref as DRF
from conftest import GOLDEN, ROOT, load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOLS = [(torch.float32, 1e-3), (torch.bfloat16, 6e-2)]
U = 2.0 ** -24
_CACHE = {}


def golden(name):
    if name not in _CACHE:
        with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
            _CACHE[name] = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files if k != "sd_keys"}
    return _CACHE[name]


def build(name, dtype):
    from UCF_VIT.simple.arch import DiffusionVIT
    g = golden(name)
    m = DiffusionVIT(**DRF.FIXTURES[name])
    sd = DRF.fixture_state_dict(m, g)
    m.load_state_dict(sd)
    m.set_compute_dtype(dtype)
    return m.to(DEV), g, sd


def ref64(name, sd, x, t, gy, dropout):
    """float64 output and gradients of the restatement, computed once per (fixture, dropout site)"""
    key = (name, dropout)
    if key not in _CACHE:
        P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        y = DRF.model64(P, DRF.FIXTURES[name], x.double(), t, dropout)
        y.backward(gy.double())
        _CACHE[key] = (y.detach(), {k: v.grad for k, v in P.items() if v.grad is not None})
    return _CACHE[key]


def run(m, x, t, gy):
    m.zero_grad(set_to_none=True)
    y = m(x.to(DEV), t, None)
    y.float().backward(gy.to(DEV))
    torch.cuda.synchronize()
    return y.detach().float().cpu(), {k: p.grad.detach().float().cpu() for k, p in m.named_parameters()}


@pytest.mark.parametrize("dtype,tol", TOLS)
@pytest.mark.parametrize("name", list(DRF.FIXTURES))
def test_eval_reproduces_the_reference_fixture(name, dtype, tol):
    m, g, _ = build(name, dtype)
    y, grads = run(m.eval(), g["x"], g["t"], g["gy"])
    assert rel_err(y, g["y"]) < tol
    for k, gr in grads.items():
        assert rel_err(gr, g["g." + k]) < tol, k


@pytest.mark.parametrize("dtype,tol", TOLS)
@pytest.mark.parametrize("name", list(DRF.FIXTURES))
def test_train_matches_the_float64_restatement(name, dtype, tol):
    m, g, sd = build(name, dtype)
    drop = m.train().timeEmbeddingMap.dropout

    def seeded(s):
        drop.generator = torch.Generator().manual_seed(s)
        return run(m, g["x"], g["t"], g["gy"])

    y, grads = seeded(5)
    seed = drop.last_seed
    y64, g64 = ref64(name, sd, g["x"], g["t"], g["gy"], (0.5, seed))
    assert rel_err(y, y64) < tol
    for k, gr in grads.items():
        assert rel_err(gr, g64[k]) < tol, k
    assert rel_err(y64, g["y"]) > 1e-2                                  # the mask matters: the eval() output is another one
    y2, grads2 = seeded(5)                                              # the same seeds: the same bits
    assert drop.last_seed == seed and torch.equal(y, y2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    y3, _ = seeded(6)
    assert drop.last_seed != seed and not torch.equal(y, y3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_t_on_the_device_and_on_the_cpu_give_the_same_bits(dtype):
    m, g, _ = build("model_diffusion_small.npz", dtype)
    y_cpu, gr_cpu = run(m.eval(), g["x"], g["t"], g["gy"])
    y_dev, gr_dev = run(m, g["x"], g["t"].to(DEV), g["gy"])
    assert torch.equal(y_cpu, y_dev) and all(torch.equal(gr_cpu[k], gr_dev[k]) for k in gr_cpu)
    y_i32, _ = run(m, g["x"], g["t"].to(DEV, torch.int32), g["gy"])
    assert torch.equal(y_cpu, y_i32)


@pytest.mark.parametrize("dtype,tol", TOLS)
def test_one_training_iteration_equals_its_float64_statement(dtype, tol):
    """x_t from the reference schedule's alpha (ddpm_schedule.npz), the model in train() with a recorded dropout seed, loss =
    MSE(unpatchify(pred), e): loss and every parameter gradient against float64"""
    from UCF_VIT._hip import functional as HF
    from UCF_VIT.ddpm.ddpm import DDPM_Scheduler
    name = "model_diffusion_small.npz"
    kw = DRF.FIXTURES[name]
    m, g, sd = build(name, dtype)
    sched = DDPM_Scheduler(1000).to(DEV)
    x0, t = g["x"], torch.tensor([3, 9])
    e = torch.from_numpy(np.random.Generator(np.random.PCG64(77)).standard_normal(tuple(x0.shape)).astype(np.float32))
    drop = m.train().timeEmbeddingMap.dropout
    drop.generator = torch.Generator().manual_seed(11)
    m.zero_grad(set_to_none=True)
    x_t = sched.q_sample(x0.to(DEV), t.to(DEV), e.to(DEV))
    loss = HF.patch_mse(m(x_t, t.to(DEV), None), e.to(DEV), kw["patch_size"])
    loss.backward()
    torch.cuda.synchronize()
    a64 = load_golden("ddpm_schedule.npz")["alpha"].double()[t].view(-1, 1, 1, 1)
    xt64 = a64.sqrt() * x0.double() + (1 - a64).sqrt() * e.double()
    assert rel_err(x_t, xt64) < 1e-6
    P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    pred = DRF.model64(P, kw, xt64, t, (0.5, drop.last_seed))
    eps_hat = torch.einsum("nhwpqc->nchpwq", pred.reshape(2, 4, 4, 8, 8, 3)).reshape(2, 3, 32, 32)     # the reference's unpatchify
    loss64 = ((eps_hat - e.double()) ** 2).mean()
    loss64.backward()
    print(f"loss hip {loss.item():.6f} float64 {loss64.item():.6f}")
    assert abs(loss.item() - loss64.item()) < tol * max(1.0, abs(loss64.item()))
    for k, p in m.named_parameters():
        assert rel_err(p.grad, P[k].grad) < tol, k


def _smoke_model(dtype=torch.float32):
    from UCF_VIT.simple.arch import DiffusionVIT
    torch.manual_seed(0)
    m = DiffusionVIT(**DRF.SMALL_KW)
    m.set_compute_dtype(dtype)
    return m.to(DEV)


def test_sampler_is_finite_and_repeatable():
    from UCF_VIT.ddpm.ddpm import DDPM_Scheduler
    m = _smoke_model().train()
    sched = DDPM_Scheduler(10).to(DEV)
    shape = (2, 3, 32, 32)
    gen = torch.Generator(device=DEV)
    a = sched.sample(m, shape, None, generator=gen.manual_seed(3))
    assert m.training                                                    # sample() ran it in eval() and put the mode back
    b = sched.sample(m, shape, None, generator=gen.manual_seed(3))
    c = sched.sample(m, shape, None, generator=gen.manual_seed(4))
    assert a.shape == shape and a.dtype == torch.float32 and torch.isfinite(a).all()
    assert torch.equal(a, b) and not torch.equal(a, c)


@pytest.mark.parametrize("i", [0, 5, 999])
def test_step_inverts_q_sample_when_the_noise_is_known(i):
    """Coefficients and kernel agree.  With the true eps for the model's prediction, q_sample at step i followed by step(i):
    (1) the step's output against float64 ddpm_step of the x_t the device holds, with the fp32 coefficients of sched.coefficients(i), within
        the ddpm_step bound 4u (|c1| (|x_t| + |c2 eps|) + |sigma z|) of tests/test_diffusion_ops.py;
    (2) x0-consistency: in exact arithmetic the result is (sqrt(abar_i) x0 + (sqrt(1 - abar_i) - beta_i / sqrt(1 - abar_i)) eps) / sqrt(1 - beta_i)
        + sigma_i z, which at i = 0 is x0 itself.  Against that float64 formula the chain has more roundings than the step alone: q_sample 3u,
        the two tables' own rounding 1u, the step 4u, c1 and c2 rounded to fp32 2u: 10u on the sum of the terms' magnitudes."""
    from UCF_VIT.ddpm.ddpm import DDPM_Scheduler
    sched = DDPM_Scheduler(1000).to(DEV)
    shape, p = (2, 3, 16, 24), 8
    r = np.random.Generator(np.random.PCG64(91))
    x0, eps, z = (torch.from_numpy(r.standard_normal(shape).astype(np.float32)) for _ in range(3))
    pred = torch.einsum("nchpwq->nhwpqc", eps.reshape(2, 3, 2, p, 3, p)).reshape(2, 6, p * p * 3).contiguous()            # patchify(eps)
    x_t = sched.q_sample(x0.to(DEV), torch.full((2,), i, device=DEV), eps.to(DEV))
    out = sched.step(x_t, pred.to(DEV), i, z.to(DEV) if i else None, p).double().cpu().numpy()
    # (1) the ddpm_step bound
    want, terms = DRF.ddpm_step(x_t.cpu().numpy(), pred.numpy(), z.numpy() if i else None, p, *sched.coefficients(i))
    err = np.abs(out - want)
    print(f"step {i}: worst err / (4 u terms) = {np.max(err / (4 * U * terms)):.3f}")
    assert (err <= 4 * U * terms).all()
    # (2) x0-consistency
    g = load_golden("ddpm_schedule.npz")
    beta, abar = g["beta"].double()[i].item(), g["alpha"].double()[i].item()
    c1, c2, sigma = 1 / np.sqrt(1 - beta), beta / np.sqrt(1 - abar), np.sqrt(beta) if i else 0.0
    x64, e64, z64 = (v.double().numpy() for v in (x0, eps, z))
    a, b = np.sqrt(abar), np.sqrt(1 - abar)
    want = c1 * (a * x64 + b * e64 - c2 * e64) + sigma * z64
    terms = c1 * (np.abs(a * x64) + np.abs(b * e64) + np.abs(c2 * e64)) + np.abs(sigma * z64)
    err = np.abs(out - want)
    print(f"step {i}: worst chain err / (10 u terms) = {np.max(err / (10 * U * terms)):.3f}")
    assert (err <= 10 * U * terms).all()
    if i == 0:      # x0 again, up to what the fp32 table loses: abar_0 is fl(1 - beta_0), so sqrt(1 - abar_0) and c2 cancel only to |b - c2|
        assert (np.abs(out - x64) <= 10 * U * terms + c1 * abs(b - c2) * np.abs(e64)).all()
        assert c1 * abs(b - c2) < 1e-5


def test_scripts_run_the_smoke_config(tmp_path):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "ucf-vit_amd", "configs", "diffusion_smoke.yaml")))
    cfg["trainer"]["checkpoint_path"] = str(tmp_path)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))

    def entry(script, port):
        env = dict(os.environ, MASTER_PORT=str(port))
        out = subprocess.run([sys.executable, os.path.join(ROOT, "ucf-vit_amd", "training_scripts", script), str(p)],
                             capture_output=True, text=True, timeout=280, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stdout

    out = entry("train_diffusion_simple.py", 29641)
    losses = [float(v) for v in re.findall(r"epoch: \d+ epoch_loss ([-+.\deinfa]+) images/s", out)]
    print(out)
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[1] <= losses[0]
    ck = torch.load(tmp_path / "multi_last_odd.ckpt", map_location="cpu", weights_only=True)
    assert ck["epoch"] == 1 and "module.timeEmbeddingMap.linear2.weight" in ck["model_state_dict"]
    out = entry("inference_diffusion_simple.py", 29642)
    s = np.load(tmp_path / "samples.npy")
    assert s.shape == (2, 3, 32, 32) and s.dtype == np.float32 and np.isfinite(s).all()
