"""HipAdamW(max_grad_norm=...) on the MI355X: both update paths (one flat run per group of a HipParamStore, and loose nn.Parameters updated
one by one), with and without the loss scaler, with and without the weights' moving average, the call sequence, a small model through
configure_optimizer, and the diffusion scripts on configs/grad_clip_smoke.yaml.

References.  grad_norm() of every step against the float64 norm of that step's own gradients (as fp32 products with the scaler's 1 / scale)
within grad_clip_ref.norm_bound, which is derived for the double accumulation, not measured.  The weights: (a) exact, against a twin
optimizer without clipping whose grad_scale is the coefficient the clipped one read back: ucfvit_adamw_clipped multiplies the same two fp32
factors; (b) a 30-step trajectory against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW on the CPU with the bound of
test_grad_scaler.py::test_schedule_and_trajectory_match_torch_on_the_cpu, 1e-6 * applied / 3."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import grad_clip_ref as R
from conftest import ROOT, load_golden, rel_err
from det_weights import det_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
VARS = ["red", "green", "blue"]
VIT_KW = dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=64, depth=2, num_heads=2)
CLIP_OPS = ("grad_sqnorm", "grad_clip_coef", "clipped_adamw")
OLD_OPS = ("adamw", "adamw_ema", "adamw_scaled", "adamw_scaled_ema", "grad_nonfinite")


def _scaler(**kw):
    from UCF_VIT._hip.grad_scaler import HipGradScaler
    return HipGradScaler(**kw)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class _spy:
    """records the names of the optimizer / scaler ops that HipAdamW calls"""

    def __enter__(self):
        from UCF_VIT._hip import ops
        self.ops, self.calls = ops, []
        self.real = {n: getattr(ops, n) for n in CLIP_OPS + OLD_OPS}
        for n in self.real:
            setattr(ops, n, self._wrap(n))
        return self.calls

    def _wrap(self, n):
        def f(*a, **k):
            self.calls.append(n)
            return self.real[n](*a, **k)
        return f

    def __exit__(self, *exc):
        for n, f in self.real.items():
            setattr(self.ops, n, f)


def _grad_norm64(params, inv_scale=None):
    return R.norm64([p.grad.detach().float().cpu().numpy() for p in params if p.grad is not None], 1.0, inv_scale), \
        sum(p.grad.numel() for p in params if p.grad is not None)


# ============================================================================================== 1. trajectory against torch on the CPU
MAX_NORM = 1.0
FACTORS = (0.02, 1.0, 0.03, 0.5)          # loss factors: gradient norms of about 0.4, 18, 0.5 and 9 around the threshold 1
INF_STEPS = {3, 4, 10, 11, 12, 20}
FLOOR = 128.0


def _trajectory(with_scaler, max_grad_norm=MAX_NORM, steps=30):
    """test_schedule_and_trajectory_match_torch_on_the_cpu with clipping: loss = sum(0.5 a w^2) c_t has the elementwise gradient a w c_t, the
    same IEEE operations on both devices; two groups of loose parameters.  Returns per-step records and the final weights of both sides."""
    from UCF_VIT._hip import lib
    from UCF_VIT._hip.optim import HipAdamW
    g = torch.Generator().manual_seed(17)
    w0 = [torch.randn(257, generator=g), torch.randn(64, generator=g)]
    a = [torch.rand(257, generator=g) + 0.5, torch.rand(64, generator=g) + 0.5]
    kw = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8)

    def groups(ws):
        return [dict(params=[ws[0]], weight_decay=0.05), dict(params=[ws[1]], weight_decay=0.0)]

    wr = [torch.nn.Parameter(w.clone()) for w in w0]
    opt_r = torch.optim.AdamW(groups(wr), **kw)
    wh = [torch.nn.Parameter(w.clone().to(DEV)) for w in w0]
    ah = [t.to(DEV) for t in a]
    opt_h = HipAdamW(groups(wh), max_grad_norm=max_grad_norm, **kw)
    ref = torch.amp.GradScaler("cpu", init_scale=8192.0, growth_interval=3) if with_scaler else None
    sc = _scaler(init_scale=8192.0, growth_interval=3, min_scale=FLOOR) if with_scaler else None
    rec = []
    for t in range(steps):
        c = float("inf") if with_scaler and t in INF_STEPS else FACTORS[t % 4]
        loss_r = sum((0.5 * x * w * w).sum() for x, w in zip(a, wr)) * c
        loss_h = sum((0.5 * x * w * w).sum() for x, w in zip(ah, wh)) * c
        before = [w.detach().clone() for w in wh]
        if with_scaler:
            ref.scale(loss_r).backward()
            ref.unscale_(opt_r)
            norm_r = float(torch.nn.utils.clip_grad_norm_(wr, max_grad_norm if max_grad_norm is not None else 1e30))
            gmax_r = max(float(w.grad.abs().max()) for w in wr)
            ref.step(opt_r)
            ref.update()
            if ref._scale < FLOOR:
                ref._scale.fill_(FLOOR)
            inv = sc.device_state()[lib.GS_INV_SCALE].item()
            sc.scale(loss_h).backward()
            norm64, n = _grad_norm64(wh, inv)
            sc.step(opt_h)
            sc.update()
            assert sc.get_scale() == ref.get_scale(), t
        else:
            loss_r.backward()
            gmax_r = max(float(w.grad.abs().max()) for w in wr)
            norm_r = float(torch.nn.utils.clip_grad_norm_(wr, max_grad_norm if max_grad_norm is not None else 1e30))
            opt_r.step()
            loss_h.backward()
            norm64, n = _grad_norm64(wh)
            opt_h.step()
        skipped = math.isinf(c)
        if max_grad_norm is not None:
            rec.append(dict(t=t, skipped=skipped, norm=opt_h.grad_norm().item(), coef=opt_h.clip_coef().item(), norm64=norm64, n=n,
                            norm_r=norm_r, gmax_r=gmax_r))
        if skipped:
            assert all(_same(x, y) for x, y in zip(before, wh)), f"step {t} was skipped but moved the weights"
        else:
            assert not any(_same(x, y) for x, y in zip(before, wh)), t
        opt_r.zero_grad()
        opt_h.zero_grad()
    return rec, wh, wr, sc


@pytest.mark.parametrize("with_scaler", [False, True])
def test_trajectory_matches_torch_clip_grad_norm_on_the_cpu(with_scaler):
    """30 steps, two groups, some steps clip and some do not (and under the scaler six are skipped).  Weights: rel_err < 1e-6 * applied / 3.
    grad_norm() per step: against the float64 norm of the step's own gradients within the derived bound; against the norm torch returned,
    which is an fp32 sum over gradients of slightly different weights, within the sum of (i) the derived bound, (ii) n u32 for torch's fp32
    accumulation, (iii) the divergence the weight bound allows: |norm_h - norm_r| <= ||g_h - g_r|| <= sqrt(n) max|dg|, and with g = a w c,
    a in [0.5, 1.5], max|dg| <= 3 E max|g| for a weight divergence E = 1e-6 * (applied so far) / 3 in rel_err's metric (plus u32 max|g| for
    the roundings of g itself).  The same run without max_grad_norm must miss the weight bound, or the test would not see clipping."""
    rec, wh, wr, sc = _trajectory(with_scaler)
    applied, worst, worst_r = 0, 0.0, 0.0
    for r in rec:
        if r["skipped"]:
            assert not math.isfinite(r["norm"]) and not r["coef"] > 0.0, r        # Inf norm: coefficient 0; NaN norm: NaN
            assert not math.isfinite(r["norm_r"])
            continue
        bound = R.norm_bound(r["norm64"], r["n"], 2)
        worst = max(worst, abs(r["norm"] - r["norm64"]) / bound)
        assert abs(r["norm"] - r["norm64"]) <= bound, r
        e_w = 1e-6 * applied / 3
        allowed = bound + r["n"] * R.U32 * r["norm_r"] + math.sqrt(r["n"]) * (3 * e_w + R.U32) * r["gmax_r"]
        worst_r = max(worst_r, abs(r["norm"] - r["norm_r"]) / allowed)
        assert abs(r["norm"] - r["norm_r"]) <= allowed, r
        cref = R.coef64(r["norm64"], MAX_NORM)
        assert (r["coef"] == 1.0) if r["norm"] + 1e-6 <= MAX_NORM else abs(r["coef"] - cref) <= R.coef_bound(cref, r["n"], 2), r
        applied += 1
    clipped = [r["coef"] < 1.0 for r in rec if not r["skipped"]]
    assert any(clipped) and not all(clipped), "the factors were chosen so that some steps clip and some do not"
    assert applied == 30 - (len(INF_STEPS) if with_scaler else 0)
    if with_scaler:
        assert sc.counters() == (applied, len(INF_STEPS))
    errs = [rel_err(h, r) for h, r in zip(wh, wr)]
    print(f"scaler={with_scaler}: worst grad_norm err / bound {worst:.3f} (own gradients) {worst_r:.3f} (torch's norm); trajectory rel_err after "
          f"{applied} applied steps {errs[0]:.3e} {errs[1]:.3e} (bound {1e-6 * applied / 3:.3e})")
    assert max(errs) < 1e-6 * applied / 3
    _, wn, _, _ = _trajectory(with_scaler, max_grad_norm=None)
    assert max(rel_err(h, r) for h, r in zip(wn, wr)) > 100 * 1e-6 * applied / 3, "a run without clipping passes too: the test sees nothing"


# ============================================================================================== 2. exact: the twin with grad_scale = COEF
def _build(dtype, seed=21):
    from UCF_VIT.simple.arch import VIT
    m = VIT(**VIT_KW)
    m.load_state_dict(det_state_dict(m, seed))
    m = m.to(DEV)
    m.set_compute_dtype(dtype)
    return m


def _backward(m, scale=None):
    from UCF_VIT.utils.metrics import cross_entropy_loss
    g = load_golden("model_vit_small.npz")
    loss = cross_entropy_loss(m(g["x"].to(DEV), VARS), g["labels"].to(DEV))
    (loss if scale is None else scale.scale(loss)).backward()
    return loss


@pytest.mark.parametrize("ema_decay", [None, 0.9])
@pytest.mark.parametrize("path", ["flat", "per_parameter"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_clipped_step_equals_a_twin_scaled_by_the_coefficient(dtype, path, ema_decay):
    """two models with equal weights take two steps on equal gradients.  The first clips at a third of its gradient norm; the second does
    not clip and gets grad_scale = the first one's clip_coef() of that step: weights, shadows and averages end with the same bits.  `flat`:
    one launch per group over the store; `per_parameter`: one gradient is taken away, so its group is updated parameter by parameter (and
    the norm is summed over one segment per parameter)."""
    from UCF_VIT.utils.misc import configure_optimizer
    ma, mb = _build(dtype), _build(dtype)
    oa = configure_optimizer(ma, 1e-3, 0.9, 0.95, 1e-2, ema_decay=ema_decay, max_grad_norm=1.0)
    ob = configure_optimizer(mb, 1e-3, 0.9, 0.95, 1e-2, ema_decay=ema_decay)
    for step in range(2):
        _backward(ma), _backward(mb)
        if path == "per_parameter":
            for m in (ma, mb):
                dict(m.named_parameters())["head.bias"].grad = None
        pa = [p for p in ma.parameters()]
        norm64, n = _grad_norm64(pa)
        oa.max_grad_norm = norm64 / 3.0                                   # a device-side write once the state exists
        with _spy() as calls:
            oa.step()
        assert bool(oa._flat) and len(oa._flat) == (2 if path == "flat" else 1)
        n_seg = calls.count("grad_sqnorm")
        assert calls[:n_seg + 1] == ["grad_sqnorm"] * n_seg + ["grad_clip_coef"], "an update was launched before the coefficient was final"
        assert set(calls[n_seg + 1:]) == {"clipped_adamw"} and (n_seg == 2 if path == "flat" else n_seg > 2)
        norm, c = oa.grad_norm().item(), oa.clip_coef().item()
        assert abs(norm - norm64) <= R.norm_bound(norm64, n, 1024 * n_seg), (norm, norm64)
        assert abs(c - 1.0 / 3.0) < 1e-4
        ob.grad_scale = c
        ob.step()
        oa.zero_grad(), ob.zero_grad()
        for (k, x), y in zip(ma.named_parameters(), mb.parameters()):
            assert _same(x, y), (step, k)
        if dtype == torch.bfloat16 and path == "flat":
            assert _same(ma._ucf_store.flat_s, mb._ucf_store.flat_s)
        if ema_decay is not None:
            ea, eb = oa.ema_state_dict(ma), ob.ema_state_dict(mb)
            assert all(_same(ea[k], eb[k]) for k in ea)
            assert not all(_same(ea[k], v) for k, v in ma.state_dict().items())
    assert set(oa.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}


def test_scaler_ema_and_clipping_together_on_loose_parameters():
    """loose parameters under a loss scaler at the power-of-two scale 4 with a moving average: (1 * 0.25) * c and (c * 0.25) round alike,
    so the twin without clipping at grad_scale = c ends with the same bits; a step with an Inf gradient moves nothing on either side"""
    from UCF_VIT._hip.optim import HipAdamW

    def make():
        g = torch.Generator().manual_seed(3)
        ps = [torch.nn.Parameter(torch.randn(1003, generator=g).to(DEV)), torch.nn.Parameter(torch.randn(4099, generator=g).to(DEV))]
        return ps, _scaler(init_scale=4.0, backoff_factor=1.0, growth_interval=10 ** 6)

    (pa, sa), (pb, sb) = make(), make()
    kw = dict(lr=1e-3, betas=(0.9, 0.95), ema_decay=0.9)
    oa = HipAdamW([dict(params=[pa[0]], weight_decay=0.05), dict(params=[pa[1]], weight_decay=0.0)], max_grad_norm=0.5, **kw)
    ob = HipAdamW([dict(params=[pb[0]], weight_decay=0.05), dict(params=[pb[1]], weight_decay=0.0)], **kw)
    g = torch.Generator().manual_seed(4)
    for step in range(4):
        grads = [torch.randn(p.numel(), generator=g).to(DEV) * (0.5 if step % 2 else 0.001) for p in pa]
        if step == 2:
            grads[1][4098] = float("inf")
        for ps in (pa, pb):
            for p, gr in zip(ps, grads):
                p.grad = gr.clone()
        before = [p.detach().clone() for p in pa]
        with _spy() as calls:
            sa.step(oa)
        sa.update()
        assert calls == ["grad_sqnorm", "grad_sqnorm", "grad_clip_coef", "clipped_adamw", "clipped_adamw"]
        c = oa.clip_coef().item()
        if step == 2:
            assert c == 0.0 and math.isinf(oa.grad_norm().item()) and all(_same(x, y) for x, y in zip(before, pa))
        else:
            assert (c < 1.0) == bool(step % 2), (step, c)
        ob.grad_scale = c if step != 2 else 1.0
        sb.step(ob)
        sb.update()
        for x, y in zip(pa, pb):
            assert _same(x, y), step
            assert _same(oa._ema[x], ob._ema[y]), step
    assert sa.counters() == (3, 1) and sb.counters() == (3, 1)


# ============================================================================================== 3. the call sequence
def test_call_sequences_with_and_without_clipping():
    """clipping and scaling together issue no ucfvit_grad_nonfinite (the fused pass sets the flag); with max_grad_norm=None the sequence of
    ops calls is the one the optimizer has always issued"""
    from UCF_VIT._hip.optim import HipAdamW

    def make(**kw):
        ps = [torch.nn.Parameter(torch.ones(1003, device=DEV)), torch.nn.Parameter(torch.ones(64, device=DEV))]
        return ps, HipAdamW([dict(params=[ps[0]], weight_decay=0.05), dict(params=[ps[1]], weight_decay=0.0)], lr=1e-3, **kw)

    def step(ps, opt, sc=None):
        for p in ps:
            p.grad = torch.full_like(p, 0.25)
        with _spy() as calls:
            sc.step(opt) if sc is not None else opt.step()
        return calls

    assert step(*make()) == ["adamw", "adamw"]
    assert step(*make(ema_decay=0.5)) == ["adamw_ema", "adamw_ema"]
    assert step(*make(), _scaler()) == ["grad_nonfinite", "grad_nonfinite", "adamw_scaled", "adamw_scaled"]
    assert step(*make(ema_decay=0.5), _scaler()) == ["grad_nonfinite", "grad_nonfinite", "adamw_scaled_ema", "adamw_scaled_ema"]
    clipped = ["grad_sqnorm", "grad_sqnorm", "grad_clip_coef", "clipped_adamw", "clipped_adamw"]
    assert step(*make(max_grad_norm=1.0)) == clipped
    ps, opt = make(max_grad_norm=1.0)
    sc = _scaler(init_scale=2.0)
    assert step(ps, opt, sc) == clipped
    assert opt.grad_norm().item() == pytest.approx(0.25 / 2.0 * math.sqrt(1067), rel=1e-6) and sc.device_state()[2].item() == 0.0
    # a parameter without a gradient is left out of the norm and of the update
    ps[1].grad = None
    with _spy() as calls:
        opt.step()
    assert calls == ["grad_sqnorm", "grad_clip_coef", "clipped_adamw"]
    # switched off again: the old sequence, and the state keeps the last values
    opt.max_grad_norm = None
    assert step(ps, opt) == ["adamw", "adamw"]


def test_clipped_step_path_does_not_synchronise():
    """step() with clipping, with and without the scaler, and the threshold's setter under torch.cuda.set_sync_debug_mode("error"); the
    first step (which allocates the state block and the workspace by device-side writes) included"""
    from UCF_VIT._hip.optim import HipAdamW
    ps = [torch.nn.Parameter(torch.ones(1003, device=DEV)), torch.nn.Parameter(torch.ones(4099, device=DEV))]
    o1, o2 = HipAdamW([ps[0]], max_grad_norm=1.0), HipAdamW([ps[1]], max_grad_norm=1.0)
    sc = _scaler(init_scale=8.0)
    sc.device_state()
    for p in ps:
        p.grad = torch.full_like(p, 0.5)
    one = torch.ones((), device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            one.item()
        for _ in range(2):
            o1.step()
            sc.step(o2)
            sc.update()
            o1.max_grad_norm = 2.0
            n, c = o1.grad_norm(), o2.clip_coef()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert n.dim() == 0 and n.is_cuda and c.dim() == 0 and c.is_cuda
    assert o1._gc[0].item() == 2.0 and n.item() == pytest.approx(0.5 * math.sqrt(1003), rel=1e-6)


# ============================================================================================== 4. a small model, and the scripts
def test_small_model_through_configure_optimizer():
    from UCF_VIT.utils.misc import configure_optimizer
    m, m0 = _build(torch.bfloat16), _build(torch.bfloat16)
    plain = configure_optimizer(m0, 1e-3, 0.9, 0.95, 1e-2)
    opt = configure_optimizer(m, 1e-3, 0.9, 0.95, 1e-2, max_grad_norm=0.05)          # this model's gradient norms are 3 ... 7 at these steps
    losses, coefs = [], []
    for _ in range(3):
        losses.append(_backward(m).item())
        opt.step()
        opt.zero_grad()
        coefs.append(opt.clip_coef().item())
    _backward(m0)
    plain.step()
    print(f"losses {losses} coefficients {coefs} norm {opt.grad_norm().item():.4f}")
    assert all(math.isfinite(v) for v in losses) and min(coefs) < 1.0 and all(0.0 < c <= 1.0 for c in coefs)
    assert bool(opt._flat), "the flat one-launch path was not taken"
    sd, sd0 = opt.state_dict(), plain.state_dict()
    assert sd.keys() == sd0.keys() and sd["state"].keys() == sd0["state"].keys()
    assert all(set(e) == {"step", "exp_avg", "exp_avg_sq"} for e in sd["state"].values())
    assert [g.keys() for g in sd["param_groups"]] == [g.keys() for g in sd0["param_groups"]]
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


def _entry(script, cfg_path, port):
    env = dict(os.environ, MASTER_PORT=str(port))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "ucf-vit_amd", "training_scripts", script), str(cfg_path)],
                         capture_output=True, text=True, timeout=280, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def test_diffusion_scripts_run_the_grad_clip_smoke_config(tmp_path):
    import yaml
    lines = {}
    for name, port in (("grad_clip_smoke.yaml", 29661), ("diffusion_smoke.yaml", 29663)):
        cfg = yaml.safe_load(open(os.path.join(ROOT, "ucf-vit_amd", "configs", name)))
        cfg["trainer"]["checkpoint_path"] = str(tmp_path / name)
        os.makedirs(tmp_path / name)
        p = tmp_path / (name + ".cfg.yaml")
        p.write_text(yaml.safe_dump(cfg))
        out = _entry("train_diffusion_simple.py", p, port)
        lines[name] = [ln for ln in out.splitlines() if ln.startswith("epoch: ")]
        assert len(lines[name]) == 2, out
        if name == "grad_clip_smoke.yaml":
            assert cfg["model"]["use_grad_scaler"] is True and float(cfg["model"]["clip_grad_norm"]) > 0
            _entry("inference_diffusion_simple.py", p, port + 1)
            s = np.load(tmp_path / name / "samples.npy")
            assert s.shape == (2, 3, 32, 32) and np.isfinite(s).all()
    print("\n".join(lines["grad_clip_smoke.yaml"] + lines["diffusion_smoke.yaml"]))
    for ln in lines["grad_clip_smoke.yaml"]:
        m = re.fullmatch(r"epoch: \d+ epoch_loss ([-+.\deinfa]+) images/s [\d.]+ grad_norm ([-+.\deinfa]+)", ln)
        assert m and math.isfinite(float(m.group(1))) and math.isfinite(float(m.group(2))) and float(m.group(2)) > 0.05, ln
    for ln in lines["diffusion_smoke.yaml"]:
        assert re.fullmatch(r"epoch: \d+ epoch_loss [-+.\deinfa]+ images/s [\d.]+", ln), ln
