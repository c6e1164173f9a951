"""DDPM noise schedule (reference ddpm/ddpm.py) with what training and sampling need around it on the HIP hot path: the forward noising
(HF.q_sample), one ancestral reverse step on the image (HF.ddpm_step) and the whole reverse loop (sample); the strided DDIM sampler with its
generalised step, which can clamp the predicted x0 (ddim_timesteps, ddim_coefficients, HF.ddim_step, sample_ddim)."""
import math

import numpy as np
import torch
import torch.nn as nn

from UCF_VIT._hip import functional as HF


class DDPM_Scheduler(nn.Module):
    """beta: linear in [1e-4, 0.02]; alpha: the cumulative product of 1 - beta (the reference's name for abar).  Both are fp32 tables from
    the reference's own torch calls, kept as non-persistent buffers: .to(device) moves them, state_dict() stays empty.
    sqrt_ab = sqrt(alpha) and sqrt_1mab = sqrt(1 - alpha) are taken once in float64 from the fp32 alpha and rounded once."""

    def __init__(self, num_time_steps: int = 1000):
        super().__init__()
        beta = torch.linspace(1e-4, 0.02, num_time_steps, requires_grad=False)
        alpha = torch.cumprod(1 - beta, dim=0).requires_grad_(False)
        self.register_buffer("beta", beta, persistent=False)
        self.register_buffer("alpha", alpha, persistent=False)
        a64 = alpha.double()
        self.register_buffer("sqrt_ab", a64.sqrt().float(), persistent=False)
        self.register_buffer("sqrt_1mab", (1.0 - a64).sqrt().float(), persistent=False)
        self.num_time_steps = num_time_steps
        self._beta64 = beta.double().tolist()        # host copies for the step coefficients: the loop never reads the device
        self._alpha64 = a64.tolist()

    def forward(self, t):
        return self.beta[t], self.alpha[t]

    def q_sample(self, x0, t, eps, out=None):
        """x_t = sqrt(alpha[t]) x0 + sqrt(1 - alpha[t]) eps per sample; t int64 [B] on the device (a CPU t is moved).  A step outside
        [0, num_time_steps) is clamped by the kernel, which cannot refuse what only the device sees."""
        if not torch.is_tensor(t):
            raise TypeError("q_sample: t must be an int64 tensor of B steps")
        if not t.is_cuda:
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= self.num_time_steps):
                raise ValueError(f"q_sample: step outside [0, {self.num_time_steps})")
            t = t.to(x0.device)
        return HF.q_sample(x0, t.to(torch.int64), eps, self.sqrt_ab, self.sqrt_1mab, out=out)

    def coefficients(self, i: int):
        """(c1, c2, sigma) of reverse step i as fp32 values: c1 = 1 / sqrt(1 - beta_i), c2 = beta_i / sqrt(1 - alpha_i), sigma = sqrt(beta_i)
        (0 at i == 0), each evaluated in float64 from the fp32 tables and rounded once"""
        if not 0 <= i < self.num_time_steps:
            raise ValueError(f"step {i} outside [0, {self.num_time_steps})")
        b, ab = self._beta64[i], self._alpha64[i]
        c1 = 1.0 / math.sqrt(1.0 - b)
        c2 = b / math.sqrt(1.0 - ab)
        sigma = math.sqrt(b) if i > 0 else 0.0
        return float(np.float32(c1)), float(np.float32(c2)), float(np.float32(sigma))

    def step(self, x, pred, i: int, z, patch_size: int, out=None):
        """x_{i-1} = c1 (x_i - c2 eps_hat) + sigma_i z with eps_hat = unpatchify(pred), read in place by the kernel.  i is a host integer; z
        is the fresh noise of this step, None at i == 0.  out may be x."""
        c1, c2, sigma = self.coefficients(int(i))
        if z is None and sigma != 0.0:
            raise ValueError(f"step {i} > 0 needs noise z")
        return HF.ddpm_step(x, pred, z if sigma != 0.0 else None, patch_size, c1, c2, sigma, out=out)

    @torch.no_grad()
    def sample(self, model, shape, variables, generator=None):
        """ancestral sampling: x_T ~ N(0, I), then num_time_steps reverse steps with the model in eval().  The step index stays on the host
        and the per-step t tensors are cut from one table made before the loop: nothing inside the loop waits for the device."""
        dev = self.beta.device
        shape = tuple(shape)
        T, B = self.num_time_steps, shape[0]
        x = torch.randn(shape, dtype=torch.float32, device=dev, generator=generator)
        ts = torch.arange(T, dtype=torch.int64, device=dev).unsqueeze(1).expand(T, B).contiguous()
        was_training = model.training
        model.eval()
        try:
            for i in range(T - 1, -1, -1):
                pred = model(x, ts[i], variables)
                z = torch.randn(shape, dtype=torch.float32, device=dev, generator=generator) if i > 0 else None
                self.step(x, pred, i, z, model.patch_size, out=x)
        finally:
            model.train(was_training)
        return x

    # ---------------------------------------------------------------------------------------------- strided sampling (DDIM, Song et al.)
    def ddim_timesteps(self, num_steps: int):
        """the S = num_steps steps a strided sampler visits, increasing: tau_k = (k (T-1) + (S-1)//2) // (S-1), which is k (T-1) / (S-1)
        rounded to the nearest step; S = 1 is [T-1].  Strictly increasing, ends at T-1, and S = T is every step."""
        T, S = self.num_time_steps, int(num_steps)
        if not 1 <= S <= T:
            raise ValueError(f"num_steps {num_steps} outside [1, {T}]")
        if S == 1:
            return [T - 1]
        return [(k * (T - 1) + (S - 1) // 2) // (S - 1) for k in range(S)]

    def ddim_coefficients(self, i: int, i_prev: int, eta: float = 0.0):
        """(s_ab, s_1mab, r_ab, r_1mab, c_x0, c_eps, sigma) of the step from i to i_prev < i as fp32 values (i_prev = -1: the last step, whose
        abar_prev is 1): s_ab = sqrt(abar_i), s_1mab = sqrt(1 - abar_i), r_* their reciprocals, sigma = eta sqrt((1 - abar_prev) /
        (1 - abar_i)) sqrt(1 - abar_i / abar_prev), c_x0 = sqrt(abar_prev), c_eps = sqrt(max(1 - abar_prev - sigma^2, 0)); each evaluated in
        float64 from the fp32 alpha table and rounded once.  eta = 0 is deterministic DDIM, eta = 1 the ancestral sampler's variance."""
        if not 0 <= i < self.num_time_steps or not -1 <= i_prev < i:
            raise ValueError(f"steps ({i}, {i_prev}): need -1 <= i_prev < i < {self.num_time_steps}")
        eta = float(eta)
        if not 0.0 <= eta <= 1.0:
            raise ValueError(f"eta {eta} outside [0, 1]")
        ab = self._alpha64[i]
        ab_prev = self._alpha64[i_prev] if i_prev >= 0 else 1.0
        sigma = eta * math.sqrt((1.0 - ab_prev) / (1.0 - ab)) * math.sqrt(1.0 - ab / ab_prev)
        s_ab, s_1mab = math.sqrt(ab), math.sqrt(1.0 - ab)
        vals = (s_ab, s_1mab, 1.0 / s_ab, 1.0 / s_1mab, math.sqrt(ab_prev), math.sqrt(max(1.0 - ab_prev - sigma * sigma, 0.0)), sigma)
        return tuple(float(np.float32(v)) for v in vals)

    def ddim_step(self, x, pred, i: int, i_prev: int, z, patch_size: int, eta: float = 0.0, clip=None, out=None):
        """x_{i_prev} = c_x0 x0_hat + c_eps eps_hat + sigma z, x0_hat = (x_i - sqrt(1 - abar_i) eps_hat) / sqrt(abar_i) clamped to [-clip, clip]
        when clip is given (eps_hat is then re-derived from the clamped x0_hat); eps_hat = unpatchify(pred), read in place by the kernel.
        z is this step's noise, needed only where sigma != 0.  out may be x."""
        if clip is not None and not float(clip) >= 0.0:
            raise ValueError(f"clip must be None or >= 0, got {clip}")
        coef = self.ddim_coefficients(int(i), int(i_prev), eta)
        if z is None and coef[6] != 0.0:
            raise ValueError(f"step {i} -> {i_prev} with eta={eta} needs noise z")
        return HF.ddim_step(x, pred, z if coef[6] != 0.0 else None, patch_size, coef, clip=clip, out=out)

    @torch.no_grad()
    def sample_ddim(self, model, shape, variables, num_steps: int = 50, eta: float = 0.0, clip_denoised=None, generator=None):
        """strided sampling: x_T ~ N(0, I), then num_steps reverse steps over ddim_timesteps(num_steps) with the model in eval().  As in
        sample() the steps and their coefficients stay on the host and the t rows are cut from one table made before the loop; noise is
        drawn only for a step whose sigma is not 0 (never at eta = 0)."""
        dev = self.beta.device
        shape = tuple(shape)
        B = shape[0]
        tau = self.ddim_timesteps(num_steps)
        pairs = [(tau[k], tau[k - 1] if k else -1) for k in range(len(tau) - 1, -1, -1)]
        sigmas = [self.ddim_coefficients(i, ip, eta)[6] for i, ip in pairs]                     # refuses a bad eta before anything is drawn
        if clip_denoised is not None and not float(clip_denoised) >= 0.0:
            raise ValueError(f"clip_denoised must be None or >= 0, got {clip_denoised}")
        x = torch.randn(shape, dtype=torch.float32, device=dev, generator=generator)
        ts = torch.tensor(tau, dtype=torch.int64, device=dev).unsqueeze(1).expand(len(tau), B).contiguous()
        was_training = model.training
        model.eval()
        try:
            for k, (i, ip) in enumerate(pairs):
                pred = model(x, ts[len(tau) - 1 - k], variables)
                z = torch.randn(shape, dtype=torch.float32, device=dev, generator=generator) if sigmas[k] != 0.0 else None
                self.ddim_step(x, pred, i, ip, z, model.patch_size, eta=eta, clip=clip_denoised, out=x)
        finally:
            model.train(was_training)
        return x
