"""Dynamic loss scaling for HipAdamW with on-device skipping of non-finite steps.

The reference's bf16 policy pairs fp32 master weights with ShardedGradScaler(init_scale=8192, growth_interval=100) and raises a scale
below 128 back to 128 after every update (training_scripts/train_masked_fsdp.py:417-419,601-606).  HipGradScaler is that scaler for the
flat-buffer optimizer, with the part of torch.amp.GradScaler's interface a training loop uses:

    scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()

All state is one small fp32 device array (layout: UCFVIT_GS_* in include/ucfvit_hip.h).  step() runs a read-only non-finite check over
the gradients (ucfvit_grad_nonfinite), then AdamW launches that return at once when the check fired (ucfvit_adamw_scaled) and that fold
the division by the scale into their gradient read; update() is one launch (ucfvit_grad_scaler_update).  Gradients are never rewritten
and the host never reads the flag: scale(), step() and update() do not synchronise.  get_scale() and state_dict() do.
"""
import torch

from . import lib as _l
from . import ops


class HipGradScaler:
    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, min_scale=0.0, enabled=True,
                 device="cuda"):
        if enabled:
            if growth_factor <= 1.0:
                raise ValueError("HipGradScaler: the growth factor must be > 1.0")
            if not 0.0 < backoff_factor <= 1.0:
                raise ValueError("HipGradScaler: the backoff factor must be in (0, 1]")
            if init_scale <= 0.0 or min_scale < 0.0 or int(growth_interval) < 1:
                raise ValueError("HipGradScaler: init_scale > 0, min_scale >= 0 and growth_interval >= 1 are required")
        self._enabled = bool(enabled)
        self._device = torch.device(device)
        self._init = dict(scale=float(init_scale), growth_factor=float(growth_factor), backoff_factor=float(backoff_factor),
                          growth_interval=int(growth_interval), min_scale=float(min_scale), _growth_tracker=0)
        self._state = None      # allocated on first use: constructing a scaler does not initialise the GPU

    # ------------------------------------------------------------------ state block
    def _write_state(self, d, applied=0.0, skipped=0.0):
        host = torch.zeros(_l.GS_STATE_FLOATS, dtype=torch.float32)
        host[_l.GS_SCALE] = d["scale"]
        host[_l.GS_INV_SCALE] = 1.0 / float(torch.tensor(d["scale"], dtype=torch.float32))     # (float)(1.0 / scale), as the update kernel
        host[_l.GS_GROWTH_TRACKER] = d["_growth_tracker"]
        host[_l.GS_APPLIED_STEPS], host[_l.GS_SKIPPED_STEPS] = applied, skipped
        host[_l.GS_GROWTH_FACTOR], host[_l.GS_BACKOFF_FACTOR] = d["growth_factor"], d["backoff_factor"]
        host[_l.GS_GROWTH_INTERVAL], host[_l.GS_MIN_SCALE] = d["growth_interval"], d["min_scale"]
        if self._state is None:
            self._state = host.to(self._device)
        else:
            self._state.copy_(host)

    def device_state(self):
        """the fp32 state block on the device (UCFVIT_GS_* layout), created on first use"""
        if self._state is None:
            self._write_state(self._init)
        return self._state

    def is_enabled(self):
        return self._enabled

    # ------------------------------------------------------------------ training-loop API
    def scale(self, loss):
        """loss * scale, multiplied on the device (no synchronisation).  The fused loss Functions multiply their saved gradient by
        grad_output, so the factor reaches every gradient."""
        if not self._enabled:
            return loss
        return loss * self.device_state()[_l.GS_SCALE]

    def step(self, optimizer, *args, **kwargs):
        """check ALL gradient segments of ALL parameter groups, then issue the AdamW launches: no group updates before the flag is final"""
        if not self._enabled:
            return optimizer.step(*args, **kwargs)
        if not hasattr(optimizer, "step_scaled"):
            raise TypeError("HipGradScaler.step: the optimizer must be a HipAdamW (the unscaling is folded into its kernel)")
        if args or kwargs:
            raise TypeError("HipGradScaler.step: closures are not supported")
        for group in optimizer.param_groups:
            for p in group["params"]:
                if getattr(p, "_ucf_sharded", None):
                    raise NotImplementedError(
                        f"HipGradScaler.step: a parameter is {p._ucf_sharded}-parallel: ranks hold different shards, so the skip decision "
                        "would need a collective over the group; not supported")
        from . import functional as HF
        # Weight gradients may still sit in a deferred grouped launch, and a HipDataParallel wrapper reduces its buckets on another stream.
        # Both are closed by their end-of-backward callbacks (the compute stream waits for every bucket there, no host sync), so here the
        # queues are normally empty; a backward that ended some other way is flushed now (a flush also launches the waiting buckets).
        # Data parallel: the check reads the gradient buffer AFTER the all-reduce.  Inf and NaN survive SUM and AVG, and a bf16 overflow
        # in the transport becomes Inf, so a non-finite value on any rank is non-finite on every rank: all ranks take the same decision
        # without an extra collective.
        if HF.wgrads_pending():
            HF.flush_wgrads()
        return optimizer.step_scaled(self.device_state())

    def update(self):
        """torch's update rule + the floor min_scale; one launch, no synchronisation"""
        if self._enabled:
            ops.grad_scaler_update(self.device_state())

    def unscale_(self, optimizer):
        raise NotImplementedError("HipGradScaler.unscale_ is not provided: unscaling is folded into AdamW's read, and nothing here clips "
                                  "gradients; clipping by global norm is HipAdamW(max_grad_norm=...), inside the same read")

    # ------------------------------------------------------------------ host-side views (these synchronise)
    def get_scale(self):
        """the current scale as a Python float; synchronises with the device"""
        if not self._enabled:
            return 1.0
        return float(self.device_state()[_l.GS_SCALE].item())

    def counters(self):
        """(applied_steps, skipped_steps); synchronises with the device"""
        s = self.device_state()[_l.GS_APPLIED_STEPS:_l.GS_SKIPPED_STEPS + 1].tolist()
        return int(s[0]), int(s[1])

    def state_dict(self):
        """torch.amp.GradScaler's keys plus min_scale; synchronises with the device"""
        if not self._enabled:
            return {}
        s = self.device_state().tolist()
        return {"scale": s[_l.GS_SCALE], "growth_factor": s[_l.GS_GROWTH_FACTOR], "backoff_factor": s[_l.GS_BACKOFF_FACTOR],
                "growth_interval": int(s[_l.GS_GROWTH_INTERVAL]), "_growth_tracker": int(s[_l.GS_GROWTH_TRACKER]),
                "min_scale": s[_l.GS_MIN_SCALE]}

    def load_state_dict(self, state_dict):
        """accepts a HipGradScaler or torch.amp.GradScaler state_dict (without min_scale the floor of this object is kept).  The step
        counters are not part of the dict: HipAdamW.load_state_dict re-seeds the applied-step count from its own state."""
        if not self._enabled:
            return
        if not state_dict:
            raise RuntimeError("HipGradScaler.load_state_dict: the source state dict is empty (saved from a disabled scaler?)")
        d = dict(self._init)
        for k in ("scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker", "min_scale"):
            if k in state_dict:
                d[k] = state_dict[k]
        d = dict(d, scale=float(d["scale"]), growth_interval=int(d["growth_interval"]), _growth_tracker=int(d["_growth_tracker"]))
        self._init = d
        if self._state is None:
            return                       # written when the device state is first needed
        applied, skipped = self._state[_l.GS_APPLIED_STEPS:_l.GS_SKIPPED_STEPS + 1].tolist()
        self._write_state(d, applied, skipped)
