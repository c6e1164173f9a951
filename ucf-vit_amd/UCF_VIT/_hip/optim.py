"""Fused AdamW on the HIP kernel (ucfvit_adamw), a torch.optim.Optimizer so schedulers / state_dict keep working.

Semantics = torch.optim.AdamW (reference: utils/misc.py:58-84, two param groups).  When the parameters of a group
are consecutive slots of one HipParamStore and every one of them received its gradient in the store's flat gradient
buffer, the whole group is ONE launch over the flat segment (which also rewrites the bf16 shadow weights in the
same pass); otherwise it falls back to one launch per parameter.

Under a HipGradScaler (grad_scaler.py) the same two paths run ucfvit_grad_nonfinite over every gradient segment of every group first and
then ucfvit_adamw_scaled, which skips itself on the device when the check fired (step_scaled below).  The host-side step counters then
count CALLS; the number of applied steps, which the bias corrections use, lives in the scaler's device state.

With `ema_decay` the same launches (ucfvit_adamw_ema / ucfvit_adamw_scaled_ema) also keep an exponential moving average of the weights,
ema += (1 - decay) (p_new - ema): one fp32 buffer per flat run, one tensor per parameter on the fallback path, created at the first step as
a copy of the parameters before that step's update.  The average is not optimizer state in torch's sense and stays out of state_dict(),
which keeps the torch.optim.AdamW layout; ema_state_dict / load_ema_state_dict carry it as a model state_dict, and ema_weights() swaps it
into the model for evaluation.

With `max_grad_norm` the gradients are clipped by their global L2 norm, torch.nn.utils.clip_grad_norm_'s rule, without being rewritten: one
read-only pass per gradient segment (ucfvit_grad_sqnorm, which under a loss scaler is also the non-finite check and replaces
ucfvit_grad_nonfinite), one launch that folds the partial sums into the norm and the coefficient (ucfvit_grad_clip_coef), and AdamW launches
that multiply the coefficient into the factor they already apply to every gradient (ucfvit_adamw_clipped).  Norm and coefficient stay on the
device (grad_norm(), clip_coef()); neither they nor the threshold are part of state_dict().
"""
import contextlib

import torch

from . import ops
from .lib import GC_COEF as _GC_COEF, GC_MAX_NORM as _GC_MAX_NORM, GC_NORM as _GC_NORM, GC_STATE_FLOATS as _GC_FLOATS
from .lib import GS_APPLIED_STEPS as _GS_APPLIED, GS_SKIPPED_STEPS as _GS_SKIPPED


class HipAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0, ema_decay=None, max_grad_norm=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        max_grad_norm = self._checked_max_norm(max_grad_norm)
        ema_rate = None if ema_decay is None else ops.ema_rate(ema_decay)      # 1 - decay in double; refuses a decay outside [0, 1)
        super().__init__(params, defaults)
        self.grad_scale = grad_scale  # multiplies gradients inside the kernel (e.g. 1/world_size, or 1/loss_scale)
        # moving average of the weights (None: not kept).  _ema: parameter -> its average, a tensor of its own or a view into the buffer of
        # its flat run; _ema_flat: (id(store), lo, hi) -> (store, lo, hi, buffer, params).  Neither is part of state_dict().
        self.ema_decay, self._ema_rate = ema_decay, ema_rate
        self._ema, self._ema_flat = {}, {}
        # flat moment buffers of the one-launch path, keyed (id(store), lo, hi).  They live on the optimizer object, NOT in self.state:
        # state_dict() then serialises only the per-parameter {step, exp_avg, exp_avg_sq} entries (views into these buffers) — the
        # torch.optim.AdamW layout the reference's checkpoints hold (train_class_simple.py:364-388) — and nothing keyed by an id()
        self._flat = {}
        # loss-scaler binding (step_scaled): the scaler's device state, and its skipped-step count when the host counters were last equal
        # to the applied-step count (construction or load_state_dict)
        self._gs, self._gs_skip_base, self._gs_bound = None, None, False
        # clipping by global norm (None: off).  _gc: the device state block (UCFVIT_GC_*), _gc_ws: the partial sums of all gradient segments;
        # both are allocated at the first clipped step and stay out of state_dict()
        self._max_grad_norm, self._gc, self._gc_ws = max_grad_norm, None, None

    # ------------------------------------------------------------------------------------------------ clipping by global norm
    @staticmethod
    def _checked_max_norm(value):
        if value is None:
            return None
        if isinstance(value, bool) or not isinstance(value, float) or not 0.0 < value < float("inf"):       # (NaN fails the comparison)
            raise ValueError(f"max_grad_norm must be None or a positive finite float, got {value!r}")
        return value

    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        """None switches clipping off; a new threshold reaches the device by a device-side write (no synchronisation)"""
        self._max_grad_norm = self._checked_max_norm(value)
        if self._gc is not None and self._max_grad_norm is not None:
            self._gc[_GC_MAX_NORM:_GC_MAX_NORM + 1].fill_(self._max_grad_norm)

    def _clip_state(self):
        """the fp32 state block on the device (UCFVIT_GC_* layout), created on first use by device-side writes"""
        if self._max_grad_norm is None:
            raise RuntimeError("this optimizer does not clip gradients (max_grad_norm=None)")
        if self._gc is None:
            gc = torch.zeros(_GC_FLOATS, dtype=torch.float32, device=self._params()[0].device)
            gc[_GC_MAX_NORM:_GC_MAX_NORM + 1].fill_(self._max_grad_norm)
            gc[_GC_COEF:_GC_COEF + 1].fill_(1.0)
            self._gc = gc
        return self._gc

    def grad_norm(self):
        """0-d device tensor (a view of the state): the global L2 norm of the last step's gradients before clipping, as AdamW consumed them
        (times grad_scale, and under a loss scaler divided by the scale; Inf or NaN at a skipped step).  0 before the first step."""
        return self._clip_state()[_GC_NORM]

    def clip_coef(self):
        """0-d device tensor (a view of the state): the factor min(1, max_grad_norm / (norm + 1e-6)) the last step applied"""
        return self._clip_state()[_GC_COEF]

    def _clip_pass(self, gs):
        """sums of squares over ALL gradient segments of ALL groups (one flat run per group, or one launch per parameter that has a gradient),
        then the coefficient: no group updates before it is final.  Under a loss scaler (gs) the same pass is the non-finite check."""
        for group in self.param_groups:
            for p in group["params"]:
                if getattr(p, "_ucf_sharded", None):
                    raise NotImplementedError(
                        f"HipAdamW(max_grad_norm=...): a parameter is {p._ucf_sharded}-parallel: ranks hold different shards, so the global "
                        "norm would need a sum over the group; not supported")
        segs = []
        for group in self.param_groups:
            if not group["params"]:
                continue
            self._adopt_foreign_grads(group)
            run = self._flat_run(group)
            if run is not None:
                segs.append(run[0].flat_g[run[1]:run[2]])
                continue
            segs.extend(p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in group["params"] if p.grad is not None)
        counts = [ops.grad_sqnorm_partials(g.numel(), g.dtype) for g in segs]
        total = sum(counts)
        gc = self._clip_state()
        if self._gc_ws is None or self._gc_ws.numel() < total:
            self._gc_ws = torch.empty(max(total, 1), dtype=torch.float64, device=gc.device)
        off = 0
        for g, c in zip(segs, counts):
            if c:
                ops.grad_sqnorm(g, self._gc_ws[off:off + c], self.grad_scale, gs)
            off += c
        ops.grad_clip_coef(self._gc_ws, total, gc)

    def load_state_dict(self, state_dict):
        """accepts a torch.optim.AdamW / HipAdamW state_dict; the flat buffers are rebuilt from the per-parameter entries on the next
        step (the loaded tensors are copied in, so a checkpoint mapped to the CPU ends up in device memory before any kernel sees it)"""
        super().load_state_dict(state_dict)
        self._flat = {}
        self._gs_bound = False          # the next scaled step seeds the scaler's applied-step count from the loaded `step`

    def state_dict(self):
        """torch.optim.AdamW layout.  Under a loss scaler `step` is the number of APPLIED steps (calls minus the steps the device skipped):
        one synchronisation here, none on the step path."""
        sd = super().state_dict()
        if self._gs is None or not self._gs_bound:
            return sd
        skipped = float((self._gs[_GS_SKIPPED] - self._gs_skip_base).item())
        if skipped:
            sd["state"] = {k: dict(v, step=v["step"] - skipped) if "step" in v else v for k, v in sd["state"].items()}
        return sd

    def _bind_scaler(self, gs):
        """host step counters == applied steps at this point (nothing skipped yet, or a state_dict just loaded): hand that count to the
        device, where the bias corrections are formed, and remember the scaler's skipped-step count.  Device-side writes only."""
        steps = [int(s["step"]) for s in self.state.values() if "step" in s] + [e["step"] for e in self._flat.values()]
        gs[_GS_APPLIED:_GS_APPLIED + 1].fill_(float(max(steps, default=0)))
        self._gs, self._gs_skip_base, self._gs_bound = gs, gs[_GS_SKIPPED].clone(), True

    @staticmethod
    def _adopt_foreign_grads(group):
        """a gradient that torch autograd produced itself (a parameter used by a torch op: the variable embedding, a torch/MIOpen
        decoder) lives outside the flat buffer: copy it into its slot and re-point p.grad, so the group keeps its one-launch update"""
        for p in group["params"]:
            s = getattr(p, "_ucf_slot", None)
            if s is None or p.grad is None or not s[0].owns(p, s[1]):
                continue
            view = s[0].grad_view(p, s[1], s[2])
            if p.grad.data_ptr() != view.data_ptr() and p.grad.dtype == view.dtype and p.grad.device == view.device:
                view.copy_(p.grad)
                p.grad = view

    @staticmethod
    def _flat_run(group):
        """(store, start, end) if the group's params are one contiguous run of a store with grads in the flat buffer."""
        ps = group["params"]
        slot0 = getattr(ps[0], "_ucf_slot", None)
        if slot0 is None:
            return None
        st = slot0[0]
        expect = slot0[1]
        for p in ps:
            s = getattr(p, "_ucf_slot", None)
            if s is None or s[0] is not st or s[1] != expect or not st.owns(p, s[1]):
                return None
            if p.grad is None or p.grad.data_ptr() != st.flat_g.data_ptr() + 4 * s[1]:
                return None
            expect = s[1] + (s[2] + 63) // 64 * 64
        return st, slot0[1], expect

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._max_grad_norm is not None:
            self._clip_pass(None)
        self._update(None)
        return loss

    @torch.no_grad()
    def step_scaled(self, gs):
        """one step under a loss scaler whose device state is `gs` (HipGradScaler.step calls this): the non-finite check over ALL gradient
        segments of ALL groups first, then the AdamW launches, so no group updates before the flag is final.  No host synchronisation.
        With max_grad_norm the clip pass is that check (ucfvit_grad_sqnorm sets the flag): ucfvit_grad_nonfinite is not launched."""
        if self._gs is not gs or not self._gs_bound:
            self._bind_scaler(gs)
        if self._max_grad_norm is not None:
            self._clip_pass(gs)
            return self._update(gs)
        for group in self.param_groups:
            if not group["params"]:
                continue
            self._adopt_foreign_grads(group)
            run = self._flat_run(group)
            if run is not None:
                ops.grad_nonfinite(run[0].flat_g[run[1]:run[2]], gs, self.grad_scale)
                continue
            for p in group["params"]:
                if p.grad is not None:
                    ops.grad_nonfinite(p.grad if p.grad.is_contiguous() else p.grad.contiguous(), gs, self.grad_scale)
        self._update(gs)

    def _adamw(self, gs, p, g, m, v, shadow, ema, lr, b1, b2, eps, wd, step):
        if self._max_grad_norm is not None:
            ops.clipped_adamw(p, g, m, v, shadow, ema, lr, b1, b2, eps, wd, step, self._ema_rate, self._gc, gs, self.grad_scale)
        elif ema is None:
            if gs is None:
                ops.adamw(p, g, m, v, shadow, lr, b1, b2, eps, wd, step, self.grad_scale)
            else:
                ops.adamw_scaled(p, g, m, v, shadow, lr, b1, b2, eps, wd, gs, self.grad_scale)
        elif gs is None:
            ops.adamw_ema(p, g, m, v, shadow, ema, lr, b1, b2, eps, wd, step, self._ema_rate, self.grad_scale)
        else:
            ops.adamw_scaled_ema(p, g, m, v, shadow, ema, lr, b1, b2, eps, wd, gs, self._ema_rate, self.grad_scale)

    # ------------------------------------------------------------------------------------------------ moving average of the weights
    def _ema_of_run(self, group, st, lo, hi):
        """the average of a flat run: one buffer over [lo, hi), started from the parameters as they are now, or from the per-parameter
        averages where the fallback path (or load_ema_state_dict) made some before; the parameters' entries become views into it"""
        key = (id(st), lo, hi)
        ent = self._ema_flat.get(key)
        if ent is None or ent[0] is not st:
            buf = st.flat_p[lo:hi].clone()
            for p in group["params"]:
                o, n = p._ucf_slot[1] - lo, p.numel()
                if p in self._ema:
                    buf[o:o + n].copy_(self._ema[p].reshape(-1))
                self._ema[p] = buf[o:o + n].view(p.shape)
            ent = self._ema_flat[key] = (st, lo, hi, buf, list(group["params"]))
        return ent[3]

    def _ema_of_param(self, p):
        e = self._ema.get(p)
        if e is None:
            e = self._ema[p] = p.detach().clone(memory_format=torch.contiguous_format)
        return e

    def _params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def ema_state_dict(self, module):
        """module.state_dict() with every entry that is a parameter of this optimizer replaced by a clone of its average (the parameter's
        own value before the first step).  Entries are matched by identity, so two names of one parameter both get the average."""
        sd = module.state_dict()
        for k, v in module.state_dict(keep_vars=True).items():
            e = self._ema.get(v) if isinstance(v, torch.nn.Parameter) else None
            if e is not None:
                sd[k] = e.detach().clone()
        return sd

    @torch.no_grad()
    def load_ema_state_dict(self, module, sd):
        """the inverse of ema_state_dict: every parameter of this optimizer gets the average `sd` holds under its name in `module`"""
        if self._ema_rate is None:
            raise RuntimeError("load_ema_state_dict: this optimizer keeps no average (ema_decay=None)")
        mine = set(self._params())
        for k, v in module.state_dict(keep_vars=True).items():
            if not (isinstance(v, torch.nn.Parameter) and v in mine):
                continue
            if k not in sd or tuple(sd[k].shape) != tuple(v.shape):
                raise KeyError(f"load_ema_state_dict: no entry of shape {tuple(v.shape)} for {k}")
            self._ema_of_param(v).copy_(sd[k].to(v.device, torch.float32))

    @torch.no_grad()
    def _swap_ema(self):
        """exchange parameter and average contents in place (copies only: bit-exact), a flat run in three copies; the bf16 shadows and
        their transposed copies no longer match the weights afterwards and are marked stale"""
        done = set()
        for st, lo, hi, buf, params in self._ema_flat.values():
            if all(getattr(p, "_ucf_slot", None) is not None and p._ucf_slot[0] is st and st.owns(p, p._ucf_slot[1]) and
                   self._ema[p].data_ptr() == buf.data_ptr() + 4 * (p._ucf_slot[1] - lo) for p in params):
                tmp = buf.clone()
                buf.copy_(st.flat_p[lo:hi])
                st.flat_p[lo:hi].copy_(tmp)
                done.update(params)
        for p, e in self._ema.items():
            if p not in done:
                tmp = e.clone()
                e.copy_(p)
                p.copy_(tmp)
        for p in self._ema:
            slot = getattr(p, "_ucf_slot", None)
            if slot is not None:
                slot[0]._shadow_sig, slot[0]._t_fresh = None, False
            if hasattr(p, "_ucf_shadow"):
                del p._ucf_shadow

    @contextlib.contextmanager
    def ema_weights(self):
        """inside the context the model's parameters hold the averaged weights (and the averages hold the raw iterate); on exit both are
        back, bit for bit.  Before the first step there is no average yet and nothing moves.  Not for use around step()."""
        self._swap_ema()
        try:
            yield self
        finally:
            self._swap_ema()

    def _update(self, gs):
        for group in self.param_groups:
            if not group["params"]:
                continue
            b1, b2 = group["betas"]
            lr, eps, wd = group["lr"], group["eps"], group["weight_decay"]
            self._adopt_foreign_grads(group)
            run = self._flat_run(group)
            if run is not None:
                st, lo, hi = run
                fs = self._flat
                key = (id(st), lo, hi)
                ent = fs.get(key)
                if ent is None:
                    ent = fs[key] = dict(step=0, m=torch.zeros(hi - lo, dtype=torch.float32, device=st.device),
                                         v=torch.zeros(hi - lo, dtype=torch.float32, device=st.device))
                    # adopt per-parameter state if the slow path ran before
                    for p in group["params"]:
                        s = self.state.get(p)
                        if s and "exp_avg" in s:
                            o = p._ucf_slot[1] - lo
                            ent["m"][o:o + p.numel()].copy_(s["exp_avg"].reshape(-1).to(ent["m"].device, torch.float32))
                            ent["v"][o:o + p.numel()].copy_(s["exp_avg_sq"].reshape(-1).to(ent["v"].device, torch.float32))
                            ent["step"] = int(s["step"])
                    for p in group["params"]:
                        o = p._ucf_slot[1] - lo
                        self.state[p] = dict(step=torch.tensor(float(ent["step"])),
                                             exp_avg=ent["m"][o:o + p.numel()].view(p.shape),
                                             exp_avg_sq=ent["v"][o:o + p.numel()].view(p.shape))
                ent["step"] += 1
                shadow = st.flat_s[lo:hi] if st.flat_s is not None else None
                ema = self._ema_of_run(group, st, lo, hi) if self._ema_rate is not None else None
                self._adamw(gs, st.flat_p[lo:hi], st.flat_g[lo:hi], ent["m"], ent["v"], shadow, ema, lr, b1, b2, eps, wd, ent["step"])
                for p in group["params"]:
                    self.state[p]["step"] += 1
                if shadow is not None:
                    st.note_shadow_fresh()      # (also after a skipped step: the shadow still equals p, neither moved)
                continue
            if self._ema_rate is not None:
                for p in group["params"]:
                    self._ema_of_param(p)           # also of a parameter without a gradient: its average is the parameter itself
            for p in group["params"]:
                if p.grad is None:
                    continue
                s = self.state.setdefault(p, {})
                if "exp_avg" not in s:
                    s["step"] = torch.tensor(0.0)
                    s["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    s["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                s["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                self._adamw(gs, p.data, g, s["exp_avg"], s["exp_avg_sq"], None, self._ema.get(p), lr, b1, b2, eps, wd, int(s["step"]))
                p._version  # (kernel wrote p in place; bf16 shadows are re-cast lazily via the store signature)
                slot = getattr(p, "_ucf_slot", None)
                if slot is not None:
                    slot[0]._shadow_sig = None
