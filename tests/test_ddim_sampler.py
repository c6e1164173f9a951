"""DDPM_Scheduler.sample_ddim on the MI355X: the point-mass identity through the whole loop (tolerances of tests/test_ema_ddim_cpu.py), no noise
at eta = 0, repeatability, the training flag, every step of S = T, eta = 1 against the float64 posterior-variance sampler, and both scripts on
configs/diffusion_ema_ddim_smoke.yaml."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ddim_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def patchify(img, p):
    B, C, H, W = img.shape
    return torch.einsum("nchpwq->nhwpqc", img.reshape(B, C, H // p, p, W // p, p)).reshape(B, (H // p) * (W // p), p * p * C).contiguous()


class PointMass(torch.nn.Module):
    """the exact noise prediction of a data distribution that is a point mass at c: eps_hat = (x - sqrt(abar_t) c) / sqrt(1 - abar_t), formed
    in float64 from the fp32 x and rounded once, returned in pred's patch layout (fp32)"""
    patch_size = 8

    def __init__(self, c, alpha):
        super().__init__()
        self.c, self.alpha = c.double(), alpha.double()

    def forward(self, x, t, variables):
        ab = self.alpha[t].view(-1, 1, 1, 1)
        return patchify(((x.double() - ab.sqrt() * self.c) / (1.0 - ab).sqrt()).float(), self.patch_size)


class Recorder(torch.nn.Module):
    """a smooth stand-in for a model that keeps what it saw and what it answered"""
    patch_size = 4

    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, x, t, variables):
        e = torch.tanh(0.5 * x + 0.1 * t.view(-1, 1, 1, 1).float())
        self.seen.append((x.clone(), t.clone(), e.clone()))
        return patchify(e, self.patch_size)


class Raises(torch.nn.Module):
    patch_size = 4

    def forward(self, x, t, variables):
        raise RuntimeError("model failed")


def sched(T):
    from UCF_VIT.ddpm.ddpm import DDPM_Scheduler
    return DDPM_Scheduler(T).to(DEV)


@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("S", [1, 2, 7, 50])
def test_point_mass_identity(S, eta, clip):
    s = sched(1000)
    shape = (2, 3, 16, 16)
    c = torch.from_numpy(np.random.Generator(np.random.PCG64(17)).uniform(-1.0, 1.0, shape).astype(np.float32)).to(DEV)
    m = PointMass(c, s.alpha)
    out = s.sample_ddim(m, shape, None, num_steps=S, eta=eta, clip_denoised=clip, generator=torch.Generator(device=DEV).manual_seed(3))
    err = float((out.double() - c.double()).abs().max())
    print(f"S={S} eta={eta} clip={clip}: max |x_0 - c| = {err:.3e}")
    assert out.shape == shape and out.dtype == torch.float32
    assert err <= (2.0 ** -12 if S == 1 else 2.0 ** -22)


def test_eta_zero_draws_no_noise_and_runs_repeat():
    s = sched(1000)
    shape = (2, 3, 16, 16)
    c = torch.zeros(shape, device=DEV)
    m = PointMass(c, s.alpha)
    gen = torch.Generator(device=DEV)
    s.sample_ddim(m, shape, None, num_steps=7, eta=0.0, generator=gen.manual_seed(3))
    after = gen.get_state()
    ref = torch.Generator(device=DEV).manual_seed(3)
    torch.randn(shape, dtype=torch.float32, device=DEV, generator=ref)                     # x_T alone
    assert torch.equal(after, ref.get_state())
    s.sample_ddim(m, shape, None, num_steps=7, eta=1.0, generator=gen.manual_seed(3))
    assert not torch.equal(gen.get_state(), ref.get_state())                               # eta = 1 does draw
    rec = Recorder()
    shape = (2, 3, 8, 8)
    a = s.sample_ddim(rec, shape, None, num_steps=5, eta=1.0, clip_denoised=1.0, generator=gen.manual_seed(4))
    b = s.sample_ddim(rec, shape, None, num_steps=5, eta=1.0, clip_denoised=1.0, generator=gen.manual_seed(4))
    d = s.sample_ddim(rec, shape, None, num_steps=5, eta=1.0, clip_denoised=1.0, generator=gen.manual_seed(5))
    assert torch.equal(a, b) and not torch.equal(a, d) and torch.isfinite(a).all()
    assert [int(t[1][0]) for t in rec.seen[:5]] == s.ddim_timesteps(5)[::-1]               # the model sees the strided steps, descending


def test_training_flag_is_restored():
    s = sched(10)
    for m in (Recorder(), Raises()):
        for mode in (True, False):
            m.train(mode)
            if isinstance(m, Raises):
                with pytest.raises(RuntimeError, match="model failed"):
                    s.sample_ddim(m, (1, 3, 8, 8), None, num_steps=3)
            else:
                s.sample_ddim(m, (1, 3, 8, 8), None, num_steps=3)
            assert m.training == mode
    rec = Recorder().train()
    flags = []
    rec.register_forward_pre_hook(lambda mod, args: flags.append(mod.training))
    s.sample_ddim(rec, (1, 3, 8, 8), None, num_steps=3)
    assert flags == [False] * 3                                                             # eval() inside the loop


def test_every_step_with_eta_one_is_the_posterior_variance_sampler():
    """S = T = 5, eta = 1, no clamp.  Every step of the loop against the float64 ancestral step with the posterior variance,
    x_{i-1} = (x_i - b_i / sqrt(1 - abar_i) e) / sqrt(1 - b_i) + sqrt(b_i (1 - abar_{i-1}) / (1 - abar_i)) z,  b_i = 1 - abar_i / abar_{i-1}
    (abar_{-1} = 1), fed the x_i, e and z the device used.  Bound per element: the fp32 evaluation against its own float64 statement
    (ddim_ref.ddim_step64), the seven coefficients' rounding to fp32 (u on each factor: three on the x0 term, one on the eps term, one on the
    noise), and 1e-12 of the terms for the float64 evaluation of two algebraically equal forms."""
    T = 5
    s = sched(T)
    alpha = s.alpha.double().cpu().numpy()
    shape = (2, 3, 8, 8)
    rec = Recorder()
    out = s.sample_ddim(rec, shape, None, num_steps=T, eta=1.0, generator=torch.Generator(device=DEV).manual_seed(9))
    gen = torch.Generator(device=DEV).manual_seed(9)
    x_T = torch.randn(shape, dtype=torch.float32, device=DEV, generator=gen)
    assert torch.equal(rec.seen[0][0], x_T) and len(rec.seen) == T
    xs = [t[0].cpu().numpy() for t in rec.seen] + [out.cpu().numpy()]
    for k, (i, ip) in enumerate(R.pairs(T, T)):
        assert (i, ip) == (T - 1 - k, T - 2 - k) and int(rec.seen[k][1][0]) == i
        z = torch.randn(shape, dtype=torch.float32, device=DEV, generator=gen).cpu().numpy() if ip >= 0 else None
        x, e = xs[k].astype(np.float64), rec.seen[k][2].cpu().numpy().astype(np.float64)
        ab, abp = alpha[i], alpha[ip] if ip >= 0 else 1.0
        b = 1.0 - ab / abp
        want = (x - b / np.sqrt(1.0 - ab) * e) / np.sqrt(1.0 - b)
        sig = np.sqrt(b * (1.0 - abp) / (1.0 - ab))
        if z is not None:
            want = want + sig * z.astype(np.float64)
        coef = R.coef32(alpha, i, ip, 1.0)
        _, bound = R.ddim_step64(xs[k], rec.seen[k][2].cpu().numpy(), z, coef, None)
        c = R.ddim_coefficients64(alpha, i, ip, 1.0)
        x0_terms = c["c_x0"] * c["r_ab"] * (np.abs(x) + c["s_1mab"] * np.abs(e))
        terms = x0_terms + c["c_eps"] * np.abs(e) + (sig * np.abs(z) if z is not None else 0.0)
        bound = bound + U * (3 * x0_terms + c["c_eps"] * np.abs(e) + (sig * np.abs(z) if z is not None else 0.0)) * (1 + 8 * U) + 1e-12 * terms
        err = np.abs(xs[k + 1].astype(np.float64) - want)
        print(f"step {i} -> {ip}: worst err / bound {np.max(err / bound):.3f}")
        assert (err <= bound).all(), (i, ip)


class _Wrapped(torch.nn.Module):
    """the 'module.' prefix of the scripts' data-parallel wrapper, without a process group"""

    def __init__(self, module):
        super().__init__()
        self.module = module


def test_scripts_run_the_ema_ddim_config(tmp_path):
    """two epochs of training, the script's own resume() on that checkpoint in this process (weights and average come back bit for bit), a
    third epoch resumed by the script, inference from the averaged weights.  Two runs of the script do not repeat each other (every process
    draws its own initial weights and noise), so the resumed epoch is checked for what it must do, not against a second run."""
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "ucf-vit_amd", "configs", "diffusion_ema_ddim_smoke.yaml")))
    assert cfg["model"]["ema_decay"] and cfg["trainer"]["sampler"] == "ddim" and cfg["trainer"]["max_epochs"] == 2
    cfg["trainer"]["checkpoint_path"] = str(tmp_path)
    p = tmp_path / "cfg.yaml"

    def entry(script, port, **trainer):
        cfg["trainer"].update(trainer)
        p.write_text(yaml.safe_dump(cfg))
        env = dict(os.environ, MASTER_PORT=str(port))
        out = subprocess.run([sys.executable, os.path.join(ROOT, "ucf-vit_amd", "training_scripts", script), str(p)],
                             capture_output=True, text=True, timeout=280, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stdout

    load = lambda name: torch.load(tmp_path / name, map_location="cpu", weights_only=True)
    bits = lambda a, b: a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))
    probe = "module.blocks.0.mlp.fc1.weight"
    out = entry("train_diffusion_simple.py", 29651)
    assert len(re.findall(r"epoch: \d+ epoch_loss", out)) == 2
    odd = load("multi_last_odd.ckpt")
    ema, raw = odd["model_ema_state_dict"], odd["model_state_dict"]
    assert odd["epoch"] == 1 and list(ema.keys()) == list(raw.keys()) and "module.timeEmbeddingMap.linear2.weight" in ema
    assert all(torch.isfinite(v).all() for v in ema.values()) and not bits(ema[probe], raw[probe])
    assert all(set(e.keys()) == {"step", "exp_avg", "exp_avg_sq"} for e in odd["optimizer_state_dict"]["state"].values())
    # the script's resume() in this process
    sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd", "training_scripts"))
    import train_diffusion_simple as T
    from UCF_VIT.utils.misc import configure_grad_scaler, configure_optimizer, configure_scheduler
    conf = dict(cfg, trainer=dict(cfg["trainer"], resume_from_checkpoint=True))
    model = T.build_model(conf, DEV)[0]
    net, m = _Wrapped(model), conf["model"]
    opt = configure_optimizer(model, float(m["lr"]), float(m["beta_1"]), float(m["beta_2"]), float(m["weight_decay"]), ema_decay=float(m["ema_decay"]))
    sch = configure_scheduler(opt, int(m["warmup_steps"]), int(m["max_steps"]), float(m["warmup_start_lr"]), float(m["eta_min"]))
    assert T.resume(conf, net, opt, sch, configure_grad_scaler(False))[0] == 2
    back, now = opt.ema_state_dict(net), net.state_dict()
    assert all(bits(back[k], ema[k]) for k in ema) and all(bits(now[k], raw[k]) for k in raw)
    # a third epoch resumed by the script: it goes on from the restored average, which moves on with the weights
    out = entry("train_diffusion_simple.py", 29652, resume_from_checkpoint=True, max_epochs=3)
    assert re.findall(r"epoch: (\d+) epoch_loss", out) == ["2"]
    even = load("multi_last_even.ckpt")
    assert even["epoch"] == 2 and len(even["loss_list"]) == 3
    e2, r2 = even["model_ema_state_dict"], even["model_state_dict"]
    assert all(torch.isfinite(v).all() for v in e2.values()) and not bits(e2[probe], ema[probe]) and not bits(e2[probe], r2[probe])
    # two steps at decay 0.9 from the restored average e and weights p: e2 = 0.81 e + 0.09 p1 + 0.1 p2.  An AdamW step moves a weight by at
    # most lr |m_hat| / sqrt(v_hat) < 2 lr (beta 0.9 / 0.95: the ratio stays below 1.2 with its bias corrections), so |p_k - p| < 2 k lr and
    # |e2 - (0.81 e + 0.19 p)| < 0.09 * 2 lr + 0.1 * 4 lr (+ 1e-5 for weight decay and roundoff).  An average restarted from the loaded
    # weights would give 0.81 p + 0.09 p1 + 0.1 p2, which is 0.81 |e - p| from `want`: the last line shows that to be outside the bound
    lr = float(m["lr"])
    tol = 0.09 * 2 * lr + 0.1 * 4 * lr + 1e-5
    for k in (probe, "module.pos_embed"):
        want = 0.81 * ema[k].double() + 0.19 * raw[k].double()
        assert float((e2[k].double() - want).abs().max()) <= tol, k
    assert 0.81 * float((ema[probe].double() - raw[probe].double()).abs().max()) > tol
    out = entry("inference_diffusion_simple.py", 29653, resume_from_checkpoint=False)
    print(out)
    assert re.search(r"sampler ddim steps 4 weights ema ", out)
    smp = np.load(tmp_path / "samples.npy")
    assert smp.shape == (2, 3, 32, 32) and smp.dtype == np.float32 and np.isfinite(smp).all()
    assert np.abs(smp).max() <= 1.0                                                          # clip_denoised 1.0: the last step returns the clamped x0
