"""torch.autograd.Function wrappers that drive the HIP kernels for the UCF-VIT operator layer.

Each Function's forward/backward is a fixed sequence of libucfvit_hip.so launches (no torch math on the hot path).
Reference semantics: src/UCF_VIT/simple/building_blocks.py (PatchEmbed:78-92, Mlp:122-129, Attention:157-192,
Block:236-239) and src/UCF_VIT/simple/arch.py (_pos_embed:367-393, random_masking:663-681, mask_head:683-702).

Parameter gradients are written by the kernels straight into the flat fp32 gradient buffer of the model's
HipParamStore when there is one (see params.py); the view is handed to autograd so post-accumulate hooks (e.g. a DDP reducer) still
fire.  The gradient of a parameter with tensor hooks (register_hook) is not written there: it goes through autograd like any tensor's.
"""
import os
import weakref
from collections import namedtuple
from typing import NamedTuple, Optional

import torch

from . import ops
from .lib import ACT_GELU, ACT_GELU_SAVE_DERIV, ACT_NONE
from .params import compute_param, compute_param_t, grad_target


def _as(x, dtype):
    """x in the compute dtype, contiguous (kernel-side cast, no torch math)."""
    if x.dtype == dtype:
        return x if x.is_contiguous() else x.contiguous()
    x = x if x.is_contiguous() else x.contiguous()
    return ops.cast(x, torch.empty(x.shape, dtype=dtype, device=x.device))


def _ret_grad(g, like):
    """gradient handed back to autograd must carry the dtype of the forward input"""
    if g is None or g.dtype == like:
        return g
    return ops.cast(g, torch.empty(g.shape, dtype=like, device=g.device))


# ---------------------------------------------------------------------------------------------- param-grad helpers
_QUEUES = weakref.WeakSet()      # every live queue (one per HipParamStore + the stand-alone one): flush_wgrads() walks them


class WgradQueue:
    """Per-model backward context (one per HipParamStore: two models whose backward passes interleave — GAN-style training, tensor-
    parallel threads — never see each other's pending gradients or column sums).

    Weight gradients are off the critical path of backward: nothing reads them before the optimizer step (or a data-parallel
    all-reduce).  They are collected and issued as grouped launches (ucfvit_gemm_grouped: one persistent 256x256 ping-pong kernel
    over the union of the output tiles, no split-K partial sums).  One ViT-L Block has 192 tiles = 75 % of one round of 256 CUs,
    four Blocks have 768 = three whole rounds, so the queue keeps collecting ACROSS Blocks until the tile count fills whole
    rounds (>= 95 %) or 32 problems are pending, and the rest goes out when backward ends (autograd engine callback).

    Deferral across Blocks is only used for gradients that land in the flat gradient buffer (params.grad_target gives a view):
    autograd receives that view before the kernel has run, which is safe because AccumulateGrad adopts it without reading it and
    every reader of the buffer (optimizer, HipDataParallel bucket launch, grad clipping) comes after flush_wgrads().  A tensor hook on
    the weight would read it: grad_target gives a hooked parameter no target, so its gradient is a tensor of its own, the queue stops
    deferring (deferrable) and end_block issues the launch before the Block's backward returns."""

    MAX_PROBLEMS = 32       # GROUP_MAX of csrc/gemm2.hip
    CUS = 256

    def __init__(self):
        self.items, self.owners = [], []
        self.tiles, self.tiles_by_rows = 0, {}
        self.deferrable = True
        self.callback_armed = False
        self.listeners = []          # called after every flush (HipDataParallel launches the buckets that were waiting for it)
        # one-slot hand-over of a residual-stream gradient's column sums between two autograd Functions of the SAME model (see
        # publish_stream_colsum below): (dx tensor, fp32 [D] column sums)
        self.stream_colsum = None
        self.stream_colsum_armed = False
        # Blocks per backward pass (learnt from the first pass): with a data-parallel listener the LAST group of four Blocks is flushed in
        # pairs, so that only two Blocks' gradients (ViT-L: 50 MB of bf16) are still to be all-reduced when backward ends, not four
        self.blocks_seen = 0
        self.blocks_per_pass = 0
        _QUEUES.add(self)

    def add(self, weight, dy2, x2):
        out, acc = grad_target(weight)
        o2 = out.view(out.shape[0], -1) if out is not None else None
        if o2 is None:
            o2 = torch.empty((dy2.shape[1], x2.shape[1]), dtype=torch.float32, device=dy2.device)
            ret = o2.view(weight.shape)
            self.deferrable = False          # autograd will READ this tensor (clone / accumulate): it must be complete on return
        else:
            ret = None if acc else out
        self.items.append((dy2, x2, o2, acc))
        # (o2 is a separate view object: holding `out` itself would raise its use count and make AccumulateGrad clone it)
        self.owners.append((weight, o2) if (out is not None and not acc) else None)
        # one grouped launch takes problems of ONE reduction length (token rows): a tail Block's compact gradients (B rows) wait next to
        # the dense ones (B N rows) and ops.wgrad_grouped sends them as a launch of their own; the round count below is that of the
        # fullest launch
        rows = dy2.shape[0]
        self.tiles_by_rows[rows] = self.tiles_by_rows.get(rows, 0) + ((dy2.shape[1] + 255) // 256) * ((x2.shape[1] + 255) // 256)
        self.tiles = max(self.tiles_by_rows.values())
        return ret

    def end_block(self):
        """called when a Block's backward has queued its gradients"""
        self.blocks_seen += 1
        if not self.callback_armed:             # one callback per backward pass: flushes the rest and closes the Block count
            self.callback_armed = True
            self._arm()
        if not self.items:
            return
        rounds = -(-self.tiles // self.CUS)
        full = self.tiles >= 0.95 * rounds * self.CUS
        left = self.blocks_per_pass - self.blocks_seen           # Blocks of this pass still to come (unknown in the first pass: < 0)
        tail = bool(self.listeners) and self.blocks_per_pass > 0 and 0 <= left < 4 and left % 2 == 0
        if not (_DEFER_WGRAD and self.deferrable) or full or tail or len(self.items) + 4 > self.MAX_PROBLEMS:
            self.flush()

    def _arm(self):
        torch.autograd.Variable._execution_engine.queue_callback(self._end_of_backward)

    def _end_of_backward(self):
        self.callback_armed = False
        if self.blocks_seen:
            self.blocks_per_pass = self.blocks_seen
        self.blocks_seen = 0
        self.flush()

    def flush(self):
        items, owners = self.items, self.owners
        self.items, self.owners, self.tiles, self.tiles_by_rows, self.deferrable = [], [], 0, {}, True
        for i in range(0, len(items), self.MAX_PROBLEMS):
            ops.wgrad_grouped(items[i:i + self.MAX_PROBLEMS])
        for ow in owners:
            # a gradient handed to autograd before it was computed: if AccumulateGrad took a copy instead of the view, refresh it
            if ow is not None and ow[0].grad is not None and ow[0].grad.data_ptr() != ow[1].data_ptr():
                ow[0].grad.copy_(ow[1].view(ow[0].shape))
        for ref in list(self.listeners):
            fn = ref()
            if fn is None:
                self.listeners.remove(ref)       # its HipDataParallel wrapper is gone
            else:
                fn()


# Measured (round 1, ViT-L B=166): the four weight gradients of a Block as ONE grouped 256x256 ping-pong launch take 786 us
# (1.05 PFLOP/s on 192 of the 256 CUs) against 1142 us as four 128x128 split-K launches, +9.6 % images/s on the whole step.
# (Before the KS fragment reads moved to inline asm the grouped launch ran at 0.45-0.54 PFLOP/s: hipcc drained the LDS-DMA
# prefetch in front of every ds_read_tr builtin.)  UCFVIT_WGRAD_GROUPED=0 restores the per-GEMM launches,
# UCFVIT_WGRAD_DEFER=0 keeps one launch per Block.
_GROUP_WGRAD = os.environ.get("UCFVIT_WGRAD_GROUPED", "1") != "0"
_DEFER_WGRAD = os.environ.get("UCFVIT_WGRAD_DEFER", "1") != "0"
_STANDALONE_WQ = WgradQueue()     # modules used without a flat parameter store (single operators in tests)


def queue_of_store(store):
    q = getattr(store, "_ucf_wq", None)
    if q is None:
        q = store._ucf_wq = WgradQueue()
    return q


def _queue_for(p):
    """the backward context of the model that owns parameter `p`"""
    slot = getattr(p, "_ucf_slot", None)
    if slot is not None and slot[0].owns(p, slot[1]):
        return queue_of_store(slot[0])
    return _STANDALONE_WQ


def flush_wgrads(store=None):
    """issue every pending weight-gradient launch (of one model's store, or of every live model)"""
    if store is not None:
        queue_of_store(store).flush()
        return
    for q in list(_QUEUES):
        q.flush()


def wgrads_pending(store=None):
    if store is not None:
        return bool(queue_of_store(store).items)
    return any(q.items for q in list(_QUEUES))


def add_wgrad_flush_listener(bound_method, store=None):
    q = queue_of_store(store) if store is not None else _STANDALONE_WQ
    q.listeners.append(weakref.WeakMethod(bound_method))


def _wgrad(weight, dy2, x2, queue=None):
    if _GROUP_WGRAD and queue is not None and dy2.dtype == torch.bfloat16:
        return queue.add(weight, dy2, x2)
    out, acc = grad_target(weight)
    o2 = out.view(out.shape[0], -1) if out is not None else None
    r = ops.linear_wgrad(dy2, x2, out=o2, accumulate=acc)
    if acc:
        return None
    return out if out is not None else r.view(weight.shape)


def _bgrad(bias, dy2):
    out, acc = grad_target(bias)
    r = ops.colsum(dy2, out=out, accumulate=acc)
    return None if acc else r


def _ln_bwd(dy2, x2, gamma_c, mean, rstd, weight, bias, dres=None, dx_colsum=None, dx_colsum_accumulate=False, dres_period=1):
    ow, aw = grad_target(weight)
    ob, ab = grad_target(bias)
    if aw != ab or (ow is None) != (ob is None):  # mixed states: take the simple route
        ow = ob = None
        aw = ab = False
    dx, dg, db = ops.layernorm_bwd(dy2, x2, gamma_c, mean, rstd, dres=dres, dgamma=ow, dbeta=ob, accumulate=aw, dx_colsum=dx_colsum,
                                   dx_colsum_accumulate=dx_colsum_accumulate, dres_period=dres_period)
    return dx, (None if aw else dg), (None if ab else db)


# The gradient of the residual stream leaves a LayerNorm backward (dx + dres) and is the output gradient of the Linear that wrote
# into the stream before that norm: proj (inside the same Block) or fc2 (the Block before / the model's final norm).  Its column
# sums = that Linear's bias gradient are taken by the LayerNorm-backward kernel; across autograd Functions they travel in a
# one-slot cache of the model's backward context (WgradQueue.stream_colsum), keyed by the tensor autograd hands on (held strongly
# until consumed or until backward ends, so its address cannot be reused by another tensor in between).
def _publish_stream_colsum(q, dx, cs):
    q.stream_colsum = (dx, cs)
    if not q.stream_colsum_armed:
        q.stream_colsum_armed = True

        def clear():
            q.stream_colsum = None
            q.stream_colsum_armed = False
        torch.autograd.Variable._execution_engine.queue_callback(clear)


def _take_stream_colsum(q, dy2):
    """column sums of dy2 if the LayerNorm backward that produced exactly this tensor published them, else None"""
    ent = q.stream_colsum
    q.stream_colsum = None
    if ent is None or not _BIAS_FROM_EPILOGUE:
        return None
    dx, cs = ent
    if dx.data_ptr() == dy2.data_ptr() and dx.numel() == dy2.numel() and dx.dtype == dy2.dtype and cs.numel() == dy2.shape[-1]:
        return cs
    return None


def _bgrad_from(bias, cs):
    """bias gradient from ready column sums (fp32 [D]): written / accumulated into the gradient target without touching dy"""
    out, acc = grad_target(bias)
    if out is None:
        return cs
    ops.reduce_rows(cs.view(1, -1), out, accumulate=acc)
    return None if acc else out


def _dgrad(dy2, p_w, w, aux=None, aux_is_deriv=False, c_colsum=None, c_colsum_accumulate=False, out=None):
    """dx = dy·W (optionally x gelu'(aux), or x aux when aux already is the derivative); uses the transposed weight shadow
    when the flat store keeps one.  c_colsum: fp32 [K] that receives the column sums of dx (bias gradient of the layer before)."""
    wT = compute_param_t(p_w, dy2.dtype)
    if wT is not None:
        return ops.linear_dgrad_t(dy2, wT, act_grad_aux=aux, aux_is_deriv=aux_is_deriv, c_colsum=c_colsum,
                                  c_colsum_accumulate=c_colsum_accumulate, out=out)
    return ops.linear_dgrad(dy2, w, act_grad_aux=aux, aux_is_deriv=aux_is_deriv, c_colsum=c_colsum, c_colsum_accumulate=c_colsum_accumulate,
                            out=out)


_BIAS_FROM_EPILOGUE = os.environ.get("UCFVIT_BIAS_FROM_EPILOGUE", "1") != "0"   # A/B switch
_GELU_SAVE_DERIV = os.environ.get("UCFVIT_GELU_SAVE_DERIV", "1") != "0"     # A/B switch


def _saves_gelu_deriv(dtype):
    """bf16: the fc1 epilogue evaluates gelu' next to gelu (shared erfc) and saves it instead of the pre-activation, so the fc2
    data-gradient epilogue is a multiply; fp32 keeps the pre-activation (one formulation with the oracle, parity 1e-6)"""
    return dtype == torch.bfloat16 and _GELU_SAVE_DERIV


class TP:
    """tensor-parallel (Hybrid-OP) handle: process group, size, rank in group.  group "local" = no collective (the
    single-GPU shard-equivalence tests sum the partial results themselves)."""

    def __init__(self, group, size):
        self.group, self.size = group, size
        if hasattr(group, "tp_rank"):          # in-process stand-in used by the single-GPU equivalence tests
            self.rank = group.tp_rank
        elif group is None or isinstance(group, str):
            self.rank = 0
        else:
            self.rank = torch.distributed.get_rank(group)

    def all_reduce(self, t):
        if self.size <= 1 or self.group is None or isinstance(self.group, str):
            return t
        if hasattr(self.group, "all_reduce_sum"):
            return self.group.all_reduce_sum(t)
        if t.is_cuda and torch.distributed.get_backend(self.group) == "gloo":
            # test-only transport (several ranks sharing one GPU cannot use RCCL): stage through host memory
            h = t.detach().float().cpu()
            torch.distributed.all_reduce(h, op=torch.distributed.ReduceOp.SUM, group=self.group)
            t.copy_(h.to(t.dtype))
            return t
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.SUM, group=self.group)   # RCCL, own stream; stream-ordered
        return t


# ---------------------------------------------------------------------------------------------- raw fused sequences
# With a TP handle the weights are this rank's shards (qkv: 3*D/tp rows = H/tp heads, proj: D/tp columns, fc1: 4D/tp rows,
# fc2: 4D/tp columns; reference fsdp/building_blocks.py:123-142,169-217): the exit GEMM output is SUM-all-reduced (forward) and
# the entry gradient is SUM-all-reduced (backward).  The residual is fused on TP rank 0 only, so the sum adds it exactly once;
# the row-parallel biases are added on every rank like the reference does (bias counted tp times).
# QK-norm (the reference Attention's q_norm / k_norm): qkn = (gamma_q, beta_q, gamma_k, beta_k, eps), the four fp32 [dh] master parameters
# of the two LayerNorms and their eps, or None = exactly the launches without it.  ops.qk_norm_fwd normalises the Q and K thirds of the qkv
# buffer in place between the qkv GEMM and the attention kernels, which do not change.  For backward it keeps the un-normalised Q and K
# (saved_qk: two more D-wide token matrices per Block, the price LayerScale paid for its branch outputs) and the fp32 statistics.
def _refuse_group_qk_norm(tp, qkn):
    if tp is not None and qkn is not None:
        raise NotImplementedError(f"qk_norm under a tensor-parallel group (tp group {tp.group!r}, size {tp.size}): the heads are sharded and "
                                  "the [head_dim] parameters replicated, so their gradient would have to be summed over the group; not implemented")


def _qkn_of(qnw, qnb, knw, knb, eps):
    """the Functions' five trailing arguments -> qkn, or None without qk_norm"""
    if qnw is None and qnb is None and knw is None and knb is None:
        return None
    if qnw is None or qnb is None or knw is None or knb is None or eps is None:
        raise ValueError("qk_norm needs q_norm.weight, q_norm.bias, k_norm.weight, k_norm.bias and eps together")
    return (qnw, qnb, knw, knb, float(eps))


class _DenseCore:
    """the attention of a Block over every token: N rows per sample from the qkv GEMM to the Block's exit"""
    rows = False
    # Whether the UCFVIT_BIAS_FROM_EPILOGUE switch gates (a) the proj bias gradient taken from the LayerNorm-2 backward and (b) the V
    # third of the qkv bias gradient taken from the proj data-gradient epilogue in the qk_norm arm of _attn_bwd.  The dense core gates
    # both, the class-row core neither: they were written apart and drifted.  Kept as found: aligning them changes bits under the switch.
    bias_switch_gates = True

    @staticmethod
    def fwd(qkv, B, N, H, dh):
        return ops.attention_fwd(qkv, B, N, H, dh, dh ** -0.5)            # K5: fused softmax(QKᵀ)V over the local heads

    @staticmethod
    def bwd(qkv, o, do, lse, B, N, H, dh, **kw):
        return ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, dh ** -0.5, **kw)

    @staticmethod
    def colsum_supported(B, N, H, dh, dtype):
        return ops.attention_bwd_colsum_supported(B, N, H, dh, dtype)


class _ClassRowCore:
    """the attention of the last Block for the class token alone: one query per head and sample (token 0), so 1 row per sample from the
    attention on; the gradient turns dense again at dK / dV"""
    rows = True
    bias_switch_gates = False                                             # see _DenseCore

    @staticmethod
    def fwd(qkv, B, N, H, dh):
        return ops.attention_rows_fwd(qkv, B, N, H, dh, dh ** -0.5, 0)

    @staticmethod
    def bwd(qkv, o, do, lse, B, N, H, dh, **kw):
        return ops.attention_rows_bwd(qkv, o, do, lse, B, N, H, dh, dh ** -0.5, 0, **kw)

    @staticmethod
    def colsum_supported(B, N, H, dh, dtype):
        return True


_QKN_NAMES = ("qnw", "qnb", "knw", "knb")


def _attn_fwd(x2, B, N, H, wqkv, bqkv, wproj, bproj, residual, tp=None, qkn=None, save_qk=True, core=_DenseCore):
    """-> y, (qkv, o, lse, saved_qk, mean_qk, rstd_qk); the last three are None without qkn, or with save_qk false (no backward follows).
    With the class-row core y and the residual have one row per sample; the whole qkv buffer is normalised (its queries need every key)"""
    dh = wproj.shape[0] // H
    Hl = H // tp.size if tp else H
    qkv = ops.linear_fwd(x2, wqkv, bqkv)                               # K4: qkv GEMM + bias
    sq = (None, None, None)
    if qkn is not None:
        _refuse_group_qk_norm(tp, qkn)
        sq = ops.qk_norm_fwd(qkv, qkn[0], qkn[1], qkn[2], qkn[3], Hl, dh, qkn[4], save=save_qk)      # in place: Q, K <- LayerNorm over dh
    o, lse = core.fwd(qkv, B, N, Hl, dh)
    if tp and tp.rank != 0:
        residual = None
    y = ops.linear_fwd(o, wproj, bproj, residual=residual)             # K6: proj GEMM + bias (+ residual)
    if tp:
        tp.all_reduce(y)                                               # C3: exit all-reduce
    return y, (qkv, o, lse, *sq)


def _qkn_bwd(dqkv, sq, qkn, H, dh, qkn_needs, gb2, gb2_acc):
    """the QK-norm backward over the Q and K thirds of dqkv, in place; gb2: fp32 [2 H dh] view that receives (+)= the Q and K thirds of the
    qkv bias gradient, or None.  -> the four parameter gradients (through the path LayerScale's gamma takes)"""
    saved_qk, mean, rstd = sq
    pg = torch.empty((4, dh), dtype=torch.float32, device=dqkv.device) if any(qkn_needs) else None
    ops.qk_norm_bwd(dqkv, saved_qk, qkn[0], qkn[2], mean, rstd, H, dh, param_grads=pg, c_colsum=gb2, c_colsum_accumulate=gb2_acc)
    return tuple(_bgrad_from(qkn[i], pg[i]) if qkn_needs[i] else None for i in range(4))


def _attn_bwd(dy2, x2, saved, B, N, H, wqkv, wproj, p_qkvw, p_qkvb, p_projw, p_projb, need, tp=None, wq=None, projb_done=None, qkn=None,
              core=_DenseCore):
    """need: {forward argument name: requires a gradient} of the calling node (qkvw, qkvb, projw, projb and, with qkn, qnw, qnb, knw, knb);
    projb_done: (grad,) when the producer of dy2 (LayerNorm backward, a branch exit) has already written the proj bias gradient;
    qkn: as in _attn_fwd.  -> dx, {name: gradient} under the same names"""
    qkv, o, lse, *sq = saved
    dh = wproj.shape[0] // H
    H = H // tp.size if tp else H
    g = {}
    g["projw"] = _wgrad(p_projw, dy2, o, wq) if need["projw"] else None
    if projb_done is not None:
        g["projb"] = projb_done[0]
    else:
        g["projb"] = _bgrad(p_projb, dy2) if (p_projb is not None and need["projb"]) else None
    want_b = p_qkvb is not None and need["qkvb"]
    if qkn is not None:
        # with a LayerNorm between the bias and the scores the shortcut below does not hold for the Q and K thirds (the K third is not 0, the Q
        # third not the sum of dQ): they are the column sums of what qk_norm_bwd writes; the V third is still the column sum of dO
        Dl = H * dh
        gb, acc = grad_target(p_qkvb) if want_b else (None, False)
        if want_b and gb is None:
            gb, acc = torch.empty(3 * Dl, dtype=torch.float32, device=dy2.device), False
        from_epi = want_b and (_BIAS_FROM_EPILOGUE or not core.bias_switch_gates)
        do = _dgrad(dy2, p_projw, wproj, c_colsum=gb[2 * Dl:] if from_epi else None, c_colsum_accumulate=acc)
        dqkv = core.bwd(qkv, o, do, lse, B, N, H, dh)
        if want_b and not from_epi:
            ops.colsum(dqkv[:, 2 * Dl:], out=gb[2 * Dl:], accumulate=acc)
        g.update(zip(_QKN_NAMES, _qkn_bwd(dqkv, sq, qkn, H, dh, [need[k] for k in _QKN_NAMES], gb[:2 * Dl] if want_b else None, acc)))
        g["qkvb"] = (None if acc else gb) if want_b else None
    elif want_b and core.colsum_supported(B, N, H, dh, qkv.dtype):
        # the qkv bias gradient without a second read of dqkv (include/ucfvit_hip.h, ucfvit_attention_bwd_colsum): Q third = the per-image
        # column sums the backward kernel hands out, summed over the images; K third = 0 exactly; V third = the column sums of dO, taken in
        # the epilogue of the GEMM that produces dO
        Dl = H * dh
        gb, acc = grad_target(p_qkvb)
        if gb is None:
            gb, acc = torch.empty(3 * Dl, dtype=torch.float32, device=dy2.device), False
        do = _dgrad(dy2, p_projw, wproj, c_colsum=gb[2 * Dl:], c_colsum_accumulate=acc)
        dqkv, part = core.bwd(qkv, o, do, lse, B, N, H, dh, want_colsum=True)
        ops.reduce_rows(part, gb[:2 * Dl], accumulate=acc)
        g["qkvb"] = None if acc else gb
    else:
        do = _dgrad(dy2, p_projw, wproj)
        dqkv = core.bwd(qkv, o, do, lse, B, N, H, dh)
        g["qkvb"] = _bgrad(p_qkvb, dqkv) if want_b else None
    g["qkvw"] = _wgrad(p_qkvw, dqkv, x2, wq) if need["qkvw"] else None
    dx = _dgrad(dqkv, p_qkvw, wqkv)
    if tp:
        tp.all_reduce(dx)                                              # C2: entry gradient all-reduce
    return dx, g


def _mlp_fwd(x2, w1, b1, w2, b2, residual, tp=None, drop1=None):
    """drop1: the dropout site behind the activation (p, seed, row_step) or None; the dropped activation is what fc2 reads and what is saved"""
    h = torch.empty((x2.shape[0], w1.shape[0]), dtype=x2.dtype, device=x2.device)
    act = ACT_GELU_SAVE_DERIV if _saves_gelu_deriv(x2.dtype) else ACT_GELU
    a = ops.linear_fwd(x2, w1, b1, act=act, aux_out=h)                 # K7: fc1 GEMM + bias + erf-GELU (h: pre-activation, or gelu' of it)
    if drop1 is not None:
        _dropout(a, drop1, out=a)                                      # in place: a <- m ⊙ a / keep
    if tp and tp.rank != 0:
        residual = None
    y = ops.linear_fwd(a, w2, b2, residual=residual)                   # K7: fc2 GEMM + bias (+ residual)
    if tp:
        tp.all_reduce(y)                                               # C4: exit all-reduce
    return y, (h, a)


def _mlp_bwd(dy2, x2, saved, w1, w2, p_w1, p_b1, p_w2, p_b2, need, tp=None, wq=None, dy2_colsum=None, drop1=None):
    """need: {forward argument name: requires a gradient} of the calling node (f1w, f1b, f2w, f2b); -> dx, {name: gradient};
    dy2_colsum: column sums of dy2 when its producer (a LayerNorm backward) published them: the fc2 bias gradient;
    drop1: the dropout site behind the activation: dh is masked in place after the fused gelu' epilogue, and the column sums of the masked
    dh (the fc1 bias gradient) come from that pass, not from the epilogue"""
    h, a = saved
    g_w2 = _wgrad(p_w2, dy2, a, wq) if need["f2w"] else None
    if p_b2 is not None and need["f2b"]:
        g_b2 = _bgrad_from(p_b2, dy2_colsum) if dy2_colsum is not None else _bgrad(p_b2, dy2)
    else:
        g_b2 = None
    # dgrad fused with gelu'(pre-activation); the fc1 bias gradient = column sums of dh comes out of the same epilogue
    need_b1 = p_b1 is not None and need["f1b"]
    if drop1 is not None:
        dh = _dgrad(dy2, p_w2, w2, aux=h, aux_is_deriv=_saves_gelu_deriv(h.dtype))
        cs = torch.empty(dh.shape[1], dtype=torch.float32, device=dy2.device) if need_b1 else None
        _dropout(dh, drop1, out=dh, c_colsum=cs)
        g_b1 = _bgrad_from(p_b1, cs) if need_b1 else None
    elif need_b1 and _BIAS_FROM_EPILOGUE:
        bout, bacc = grad_target(p_b1)
        if bout is None:
            bout = torch.empty(p_b1.shape, dtype=torch.float32, device=dy2.device)
        dh = _dgrad(dy2, p_w2, w2, aux=h, aux_is_deriv=_saves_gelu_deriv(h.dtype), c_colsum=bout, c_colsum_accumulate=bacc)
        g_b1 = None if bacc else bout
    else:
        dh = _dgrad(dy2, p_w2, w2, aux=h, aux_is_deriv=_saves_gelu_deriv(h.dtype))
        g_b1 = _bgrad(p_b1, dh) if need_b1 else None
    g_w1 = _wgrad(p_w1, dh, x2, wq) if need["f1w"] else None
    dx = _dgrad(dh, p_w1, w1)
    if tp:
        tp.all_reduce(dx)                                              # C4: entry gradient all-reduce
    return dx, dict(f1w=g_w1, f1b=g_b1, f2w=g_w2, f2b=g_b2)


# ---------------------------------------------------------------------------------------------- Functions
class LinearFn(torch.autograd.Function):
    """y = x·Wᵀ + b over the last dim (nn.Linear)."""

    @staticmethod
    def forward(ctx, x, weight, bias, cdtype):
        xin = _as(x, cdtype)
        x2 = xin.reshape(-1, xin.shape[-1])
        w, b = compute_param(weight, cdtype), compute_param(bias, cdtype)
        y = ops.linear_fwd(x2, w, b)
        ctx.save_for_backward(x2, weight, bias)
        ctx.cdtype, ctx.in_dtype, ctx.in_shape = cdtype, x.dtype, x.shape
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, weight, bias = ctx.saved_tensors
        dy2 = _as(dy, ctx.cdtype).reshape(-1, dy.shape[-1])
        w = compute_param(weight, ctx.cdtype)
        gw = _wgrad(weight, dy2, x2) if ctx.needs_input_grad[1] else None
        gb = _bgrad(bias, dy2) if (bias is not None and ctx.needs_input_grad[2]) else None
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _ret_grad(_dgrad(dy2, weight, w).view(ctx.in_shape), ctx.in_dtype)
        return dx, gw, gb, None


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, cdtype):
        xin = _as(x, cdtype)
        x2 = xin.reshape(-1, xin.shape[-1])
        g, b = compute_param(weight, cdtype), compute_param(bias, cdtype)
        y, mean, rstd = ops.layernorm_fwd(x2, g, b, eps)
        ctx.save_for_backward(x2, mean, rstd, weight, bias)
        ctx.cdtype, ctx.in_dtype, ctx.in_shape = cdtype, x.dtype, x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd, weight, bias = ctx.saved_tensors
        dy2 = _as(dy, ctx.cdtype).reshape(x2.shape)
        cs = torch.empty(x2.shape[1], dtype=torch.float32, device=dy2.device) if (_BIAS_FROM_EPILOGUE and ctx.in_dtype == ctx.cdtype) else None
        dx, dg, db = _ln_bwd(dy2, x2, compute_param(weight, ctx.cdtype), mean, rstd, weight, bias, dx_colsum=cs)
        if cs is not None:
            _publish_stream_colsum(_queue_for(weight), dx, cs)      # e.g. the model's final norm: its dx is the last Block's output gradient
        return _ret_grad(dx.view(ctx.in_shape), ctx.in_dtype), dg, db, None, None


class _Slots:
    """the forward argument names of one autograd node (ctx left out), declared once: backward reads needs_input_grad and files its
    gradients under these names, so no position is counted by hand"""

    def __init__(self, *names):
        self.names = names
        self.index = {n: i for i, n in enumerate(names)}

    def needs(self, ctx):
        """{name: requires a gradient}; needs_input_grad covers the arguments apply() was given, the defaulted rest needs none"""
        given = ctx.needs_input_grad
        return dict(zip(self.names, given + (False,) * (len(self.names) - len(given))))

    def grads(self, **by_name):
        """the tuple backward returns: None but for the gradients given; a name that is no forward argument raises KeyError"""
        out = [None] * len(self.names)
        for k, g in by_name.items():
            out[self.index[k]] = g
        return tuple(out)


class AttentionFn(torch.autograd.Function):
    """Attention.forward (building_blocks.py:157-192): qkv Linear -> fused SDPA -> proj Linear."""
    ARGS = _Slots("x", "qkvw", "qkvb", "projw", "projb", "num_heads", "cdtype", "tp", "drop", "qnw", "qnb", "knw", "knb", "qk_eps", "save_qk")

    @staticmethod
    def forward(ctx, x, qkvw, qkvb, projw, projb, num_heads, cdtype, tp=None, drop=None, qnw=None, qnb=None, knw=None, knb=None, qk_eps=None,
                save_qk=None):
        """drop: (p, seed) of proj_drop in training, or None
        qnw, qnb, knw, knb, qk_eps: the weight and bias of q_norm and k_norm (fp32 [head_dim] master parameters) and their eps, or None: the
        Q and K thirds of the qkv buffer are LayerNormed per head in place before the attention kernels.  When a backward pass can follow
        the un-normalised Q and K are kept (two more D-wide token matrices) with the fp32 statistics; save_qk: whether one can (the caller
        passes torch.is_grad_enabled(), as for BlockFn's save_branch); None: decided from needs_input_grad alone"""
        ctx.exit = _Exit(site=_site(drop, tp))
        qkn = _qkn_of(qnw, qnb, knw, knb, qk_eps)
        _refuse_group_qk_norm(tp, qkn)
        keep = any(ctx.needs_input_grad) and (save_qk is None or bool(save_qk))
        xin = _as(x, cdtype)
        B, N, D = xin.shape
        x2 = xin.view(B * N, D)
        c = lambda p: compute_param(p, cdtype)
        y, saved = _attn_fwd(x2, B, N, num_heads, c(qkvw), c(qkvb), c(projw), c(projb), None, tp, qkn, keep)
        y, _ = ctx.exit.forward(None, y, False)
        ctx.save_for_backward(x2, *saved, qkvw, qkvb, projw, projb, qnw, qnb, knw, knb)
        ctx.meta = (B, N, num_heads, cdtype, x.dtype, tp, qk_eps)
        return y.view(B, N, D)

    @staticmethod
    def backward(ctx, dy):
        x2, *saved, qkvw, qkvb, projw, projb, qnw, qnb, knw, knb = ctx.saved_tensors
        B, N, H, cdtype, in_dtype, tp, qk_eps = ctx.meta
        need = AttentionFn.ARGS.needs(ctx)
        qkn = _qkn_of(qnw, qnb, knw, knb, qk_eps)
        dy2 = _as(dy, cdtype).reshape(x2.shape)
        c = lambda p: compute_param(p, cdtype)
        # behind proj_drop: the gradient of proj's output, and its column sums: proj's bias gradient
        dy2, cs, _ = ctx.exit.backward(dy2, None, projb is not None and need["projb"], False)
        projb_done = None if ctx.exit.plain else (_bgrad_from(projb, cs) if cs is not None else None,)
        dx, g = _attn_bwd(dy2, x2, saved, B, N, H, c(qkvw), c(projw), qkvw, qkvb, projw, projb, need, tp, projb_done=projb_done, qkn=qkn)
        return AttentionFn.ARGS.grads(x=_ret_grad(dx.view(B, N, -1), in_dtype), **g)


class MlpFn(torch.autograd.Function):
    """Mlp.forward (building_blocks.py:122-129): fc1 -> erf-GELU -> drop1 -> fc2 -> drop2 (norm=Identity; the drops only in training)."""
    ARGS = _Slots("x", "f1w", "f1b", "f2w", "f2b", "cdtype", "tp", "drop1", "drop2")

    @staticmethod
    def forward(ctx, x, f1w, f1b, f2w, f2b, cdtype, tp=None, drop1=None, drop2=None):
        """drop1, drop2: (p, seed) of the dropout behind the activation and behind fc2 in training, or None"""
        drop1, ctx.exit = _site(drop1, tp), _Exit(site=_site(drop2, tp))
        xin = _as(x, cdtype)
        x2 = xin.reshape(-1, xin.shape[-1])
        c = lambda p: compute_param(p, cdtype)
        y, saved = _mlp_fwd(x2, c(f1w), c(f1b), c(f2w), c(f2b), None, tp, drop1=drop1)
        y, _ = ctx.exit.forward(None, y, False)
        ctx.save_for_backward(x2, *saved, f1w, f1b, f2w, f2b)
        ctx.meta = (cdtype, x.dtype, x.shape, tp, drop1)
        return y.view(*x.shape[:-1], y.shape[-1])

    @staticmethod
    def backward(ctx, dy):
        x2, h, a, f1w, f1b, f2w, f2b = ctx.saved_tensors
        cdtype, in_dtype, in_shape, tp, drop1 = ctx.meta
        need = MlpFn.ARGS.needs(ctx)
        dy2 = _as(dy, cdtype).reshape(-1, dy.shape[-1])
        c = lambda p: compute_param(p, cdtype)
        dy2, cs, _ = ctx.exit.backward(dy2, None, f2b is not None and need["f2b"], False)
        dx, g = _mlp_bwd(dy2, x2, (h, a), c(f1w), c(f2w), f1w, f1b, f2w, f2b, need, tp, dy2_colsum=cs, drop1=drop1)
        return MlpFn.ARGS.grads(x=_ret_grad(dx.view(in_shape), in_dtype), **g)


class DropPathFn(torch.autograd.Function):
    """DropPath applied on its own: y = s ⊙ x with one fp32 scale per sample (s [B], x [B, ..., D]); backward is the same kernel on dy."""

    @staticmethod
    def forward(ctx, x, s):
        xc = x if x.is_contiguous() else x.contiguous()
        B, D = xc.shape[0], xc.shape[-1]
        x2 = xc.view(-1, D)
        y = ops.drop_path_scale(x2, s, x2.shape[0] // B)
        ctx.save_for_backward(s)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        s, = ctx.saved_tensors
        dc = dy if dy.is_contiguous() else dy.contiguous()
        d2 = dc.view(-1, dc.shape[-1])
        return ops.drop_path_scale(d2, s, d2.shape[0] // dc.shape[0]).view(dy.shape), None


# Element-wise dropout.  A site is (p, seed, row_step): the rate, the 64-bit seed of this forward pass (a host integer, HipDropout.draw)
# and the row step of the mask index (include/ucfvit_hip.h: 1 for a dense matrix, N for the class-row tail).  The mask is never stored:
# backward and a checkpoint recomputation call the same kernel with the same seed.
def _site(drop, tp=None, row_step=1):
    """(p, seed) from a module -> the site tuple, None for no dropout; refused under a tensor-parallel group"""
    if drop is None or drop[0] <= 0.0:
        return None
    if tp is not None:
        raise NotImplementedError(f"dropout under a tensor-parallel group (tp group {tp.group!r}, size {tp.size}): every rank of the group "
                                  "would need the same seed; not implemented")
    return (float(drop[0]), int(drop[1]), int(row_step))


def _dropout(x2, site, s=None, rows_per_sample=1, out=None, c_colsum=None):
    """out = s ⊙ m ⊙ x2 / keep (ops.dropout).  p == 1 needs no mask: zeros"""
    p, seed, row_step = site
    if p >= 1.0:
        out = torch.empty_like(x2) if out is None else out
        if c_colsum is not None:
            c_colsum.zero_()
        return out.zero_()
    return ops.dropout(x2, p, seed, s=s, rows_per_sample=rows_per_sample, row_step=row_step, out=out, c_colsum=c_colsum)


class _Exit(NamedTuple):
    """The exit of a residual branch: stream = res + s ⊙ m ⊙ (γ ⊙ branch) / keep, and its gradient.
    s: the drop-path scale per sample (fp32 [B]) or None; site: the dropout site (mask m, rate 1 - keep) or None; gamma: the LayerScale
    parameter (fp32 [D] master) or None; rows_per_sample: rows of the branch that share one entry of s.

    plain (none of the three): the residual stays in the epilogue of the branch's exit GEMM and there is nothing to do here, launch for
    launch a Block without any of them.  Otherwise that GEMM runs without the residual and one row pass applies what is there:
    drop path alone ops.drop_path_add, with dropout ops.dropout_add, both over the branch; with a gamma ops.layer_scale_add (the scale
    and the site riding along).  Backward of a gamma needs the UNSCALED branch output (gamma's gradient is the column sums of g ⊙ branch):
    with keep the sum goes to a new buffer and the branch output is saved; without (no_grad, nothing that requires a gradient, the first
    pass of a checkpointed Block) it overwrites the branch.  The column sums of the branch's output gradient s ⊙ m ⊙ γ ⊙ dy / keep are the
    bias gradient of proj / fc2 — not those of the stream gradient that the LayerNorm backward kernels hand out."""
    s: Optional[torch.Tensor] = None
    site: Optional[tuple] = None
    gamma: Optional[torch.Tensor] = None
    rows_per_sample: int = 1

    @property
    def plain(self):
        return self.s is None and self.site is None and self.gamma is None

    def forward(self, res, y, keep):
        """y: the exit GEMM's output (without the residual unless plain); res None: no residual (a module on its own)
        -> (the stream, the branch output to save for backward or None)"""
        if self.plain:
            return y, None
        p, seed, row_step = self.site if self.site is not None else (0.0, 0, 1)
        if self.gamma is not None:
            out = torch.empty_like(y) if keep else y
            if p >= 1.0:
                out.copy_(res)
            else:
                ops.layer_scale_add(res, y, self.gamma, s=self.s, rows_per_sample=self.rows_per_sample, p=p, seed=seed, row_step=row_step, out=out)
            return out, (y if keep else None)
        if res is None:
            _dropout(y, self.site, self.s, self.rows_per_sample, out=y)
        elif self.site is None:
            ops.drop_path_add(res, y, self.s, self.rows_per_sample)
        elif p >= 1.0:
            y.copy_(res)
        else:
            ops.dropout_add(res, y, p, seed, s=self.s, rows_per_sample=self.rows_per_sample, row_step=row_step)
        return y, None

    def backward(self, dy2, branch, want_sums, want_gamma):
        """dy2: the stream gradient; branch: what forward handed back to save
        -> (the gradient of the exit GEMM's output, its fp32 [D] column sums = that GEMM's bias gradient or None, the fp32 [D] column sums
        of g ⊙ branch = gamma's gradient or None); plain: dy2 itself and no sums"""
        if self.plain:
            return dy2, None, None
        D, dev = dy2.shape[1], dy2.device
        cs = torch.empty(D, dtype=torch.float32, device=dev) if want_sums else None
        if self.gamma is None:
            if self.site is None:
                return ops.drop_path_scale(dy2, self.s, self.rows_per_sample, c_colsum=cs), cs, None
            return _dropout(dy2, self.site, self.s, self.rows_per_sample, c_colsum=cs), cs, None
        gs = torch.empty(D, dtype=torch.float32, device=dev) if want_gamma else None
        p, seed, row_step = self.site if self.site is not None else (0.0, 0, 1)
        if p >= 1.0:
            for t in (cs, gs):
                if t is not None:
                    t.zero_()
            return torch.zeros_like(dy2), cs, gs
        d = ops.layer_scale_grad(dy2, branch if want_gamma else None, self.gamma, s=self.s, rows_per_sample=self.rows_per_sample, p=p,
                                 seed=seed, row_step=row_step, c_colsum=cs, c_gamma=gs)
        return d, cs, gs


def _refuse_group_layer_scale(tp, g1, g2):
    if tp is not None and (g1 is not None or g2 is not None):
        raise NotImplementedError(f"LayerScale under a tensor-parallel group (tp group {tp.group!r}, size {tp.size}): the row-parallel exit "
                                  "GEMM's partial outputs would have to be summed before gamma is applied; not implemented")


class LayerScaleFn(torch.autograd.Function):
    """LayerScale applied on its own: y = gamma ⊙ x over the last dimension (gamma: the fp32 parameter); backward is one layer_scale_grad."""

    @staticmethod
    def forward(ctx, x, gamma):
        xc = x if x.is_contiguous() else x.contiguous()
        x2 = xc.view(-1, xc.shape[-1])
        ctx.save_for_backward(x2, gamma)
        return _Exit(gamma=gamma).forward(None, x2, True)[0].view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, gamma = ctx.saved_tensors
        dc = dy if dy.is_contiguous() else dy.contiguous()
        want_gamma = ctx.needs_input_grad[1]
        dx, _, gs = _Exit(gamma=gamma).backward(dc.view(x2.shape), x2, False, want_gamma)
        return dx.view(dy.shape), (_bgrad_from(gamma, gs) if want_gamma else None)


def _block_sites(drop, tp, row_step):
    """BlockFn's dropout argument (p, seed_proj, seed_drop1, seed_drop2) -> the three sites (proj, drop1, drop2)"""
    if drop is None or drop[0] <= 0.0:
        return None, None, None
    p = drop[0]
    return tuple(_site((p, seed), tp, row_step) for seed in drop[1:4])


class DropoutFn(torch.autograd.Function):
    """HipDropout applied on its own: y = m ⊙ x / keep over the last dimension's rows; backward is the same kernel on dy with the same seed."""

    @staticmethod
    def forward(ctx, x, p, seed):
        xc = x if x.is_contiguous() else x.contiguous()
        ctx.site = (float(p), int(seed), 1)
        return _dropout(xc.view(-1, xc.shape[-1]), ctx.site).view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        dc = dy if dy.is_contiguous() else dy.contiguous()
        return _dropout(dc.view(-1, dc.shape[-1]), ctx.site).view(dy.shape), None, None


def _refuse_group_drop_path(tp, s1, s2):
    if tp is not None and (s1 is not None or s2 is not None):
        raise NotImplementedError(f"drop_path under a tensor-parallel group (tp group {tp.group!r}, size {tp.size}): every rank of the group "
                                  "would need the same draw; not implemented")


# ---------------------------------------------------------------------------------------------- the fused Block
# One skeleton, x1 = x + exit1(proj(attn(norm1(x)))) ; y = x1 + exit2(fc2(gelu(fc1(norm2(x1))))), for two attention cores (_DenseCore,
# _ClassRowCore).  Every token runs LayerNorm 1 and the qkv GEMM; with the class-row core everything from the attention on has one row
# per sample: the residual of branch 1 is the strided class rows of x (ldr = N D), the dropout masks are those of dense row b N (site
# row step N), and the class rows' residual gradient joins the dense dx inside the LayerNorm-1 backward (dres_period = N).
_BlockIn = namedtuple("_BlockIn", "n1w n1b qkvw qkvb projw projb n2w n2b f1w f1b f2w f2b s1 s2 gamma1 gamma2 qnw qnb knw knb")
_BlockIn.__doc__ = "the tensor arguments of a Block node besides x, under their forward names: what both nodes save whole"
_BlockSaved = namedtuple("_BlockSaved", "mean1 rstd1 ln1 qkv o lse sqk mqk rqk x1 mean2 rstd2 ln2 h a b1 b2")
_BlockSaved.__doc__ = ("what _block_forward keeps for backward (sqk, mqk, rqk: qk_norm's; b1, b2: the unscaled branch outputs under LayerScale); "
                       "not saved under recompute, rebuilt bit for bit")


def _block_exits(core, N, p, sites):
    rows_per_sample = 1 if core.rows else N
    return _Exit(p.s1, sites[0], p.gamma1, rows_per_sample), _Exit(p.s2, sites[2], p.gamma2, rows_per_sample)


def _block_forward(core, x2, B, N, H, eps, c, p, tp, sites, keep, qkn):
    """p: _BlockIn; c: parameter -> its compute-dtype tensor; sites: the dropout sites (proj, drop1, drop2); keep: a backward pass follows
    -> y, _BlockSaved"""
    exit1, exit2 = _block_exits(core, N, p, sites)
    ln1, mean1, rstd1 = ops.layernorm_fwd(x2, c(p.n1w), c(p.n1b), eps)
    # class rows of the stream: a [B, D] view, row stride N D (explicit D: an empty batch has no elements to infer it from)
    res = x2.view(B, N, x2.shape[1])[:, 0] if core.rows else x2
    x1, sa = _attn_fwd(ln1, B, N, H, c(p.qkvw), c(p.qkvb), c(p.projw), c(p.projb), res if exit1.plain else None, tp, qkn, keep, core)
    x1, b1 = exit1.forward(res, x1, keep)
    ln2, mean2, rstd2 = ops.layernorm_fwd(x1, c(p.n2w), c(p.n2b), eps)
    y, sm = _mlp_fwd(ln2, c(p.f1w), c(p.f1b), c(p.f2w), c(p.f2b), x1 if exit2.plain else None, tp, drop1=sites[1])
    y, b2 = exit2.forward(x1, y, keep)
    return y, _BlockSaved(mean1, rstd1, ln1, *sa, x1, mean2, rstd2, ln2, *sm, b1, b2)


def _block_enter(ctx, core, x, p, num_heads, eps, cdtype, tp, recompute, drop, save_branch, qk_eps):
    """forward of both Block nodes: refusals, the skeleton, what is saved -> y ([B N, D], or [B, D] with the class-row core), (B, N, D)"""
    _refuse_group_drop_path(tp, p.s1, p.s2)
    _refuse_group_layer_scale(tp, p.gamma1, p.gamma2)
    qkn = _qkn_of(p.qnw, p.qnb, p.knw, p.knb, qk_eps)
    _refuse_group_qk_norm(tp, qkn)
    xin = _as(x, cdtype)
    B, N, D = xin.shape
    ctx.sites = _block_sites(drop, tp, N if core.rows else 1)
    x2 = xin.view(B * N, D)
    keep = not recompute and any(ctx.needs_input_grad) and (save_branch is None or bool(save_branch))
    y, saved = _block_forward(core, x2, B, N, num_heads, eps, lambda t: compute_param(t, cdtype), p, tp, ctx.sites, keep, qkn)
    ctx.save_for_backward(x2, *(() if recompute else saved), *p)
    ctx.meta = (B, N, num_heads, eps, cdtype, x.dtype, tp, qk_eps)
    return y, (B, N, D)


def _block_backward(ctx, core, dy, need):
    """backward of both Block nodes; need: {forward argument name: requires a gradient} -> {name: gradient}"""
    B, N, H, eps, cdtype, in_dtype, tp, qk_eps = ctx.meta
    c = lambda t: compute_param(t, cdtype)
    x2, *saved = ctx.saved_tensors
    p = _BlockIn(*saved[-len(_BlockIn._fields):])
    qkn = _qkn_of(p.qnw, p.qnb, p.knw, p.knb, qk_eps)
    if len(saved) == len(p):                              # recompute: only the input was kept; the same launches rebuild the rest
        _, v = _block_forward(core, x2, B, N, H, eps, c, p, tp, ctx.sites, True, qkn)
    else:
        v = _BlockSaved(*saved[:-len(p)])
    exit1, exit2 = _block_exits(core, N, p, ctx.sites)
    D = x2.shape[1]
    dy2 = _as(dy, cdtype).reshape(B if core.rows else B * N, D)
    wq = _queue_for(p.qkvw)
    g = {}
    # The column sums of the stream gradient dy that its producer (a LayerNorm backward) published are fc2's bias gradient for a plain
    # exit; otherwise they are dropped (always taken: the slot is cleared) and the exit's own pass sums s ⊙ m ⊙ γ ⊙ dy / keep
    published = _take_stream_colsum(wq, dy2)
    dt2, cs2, gs2 = exit2.backward(dy2, v.b2, p.f2b is not None and need["f2b"], need["gamma2"])
    g["gamma2"] = _bgrad_from(p.gamma2, gs2) if gs2 is not None else None
    dln2, gm = _mlp_bwd(dt2, v.ln2, (v.h, v.a), c(p.f1w), c(p.f2w), p.f1w, p.f1b, p.f2w, p.f2b, need, tp, wq,
                        dy2_colsum=published if exit2.plain else cs2, drop1=ctx.sites[1])
    # LayerNorm backward also sums its output (the residual-stream gradient) over the tokens: proj's bias gradient for a plain exit ...
    want_projb = p.projb is not None and need["projb"]
    projb_done, pb_out, pb_acc = None, None, False
    if exit1.plain and want_projb and (_BIAS_FROM_EPILOGUE or not core.bias_switch_gates):
        pb_out, pb_acc = grad_target(p.projb)
        if pb_out is None:
            pb_out = torch.empty(p.projb.shape, dtype=torch.float32, device=dy2.device)
        projb_done = (None if pb_acc else pb_out,)
    dx1, g["n2w"], g["n2b"] = _ln_bwd(dln2, v.x1, c(p.n2w), v.mean2, v.rstd2, p.n2w, p.n2b, dres=dy2, dx_colsum=pb_out,     # + residual branch
                                      dx_colsum_accumulate=pb_acc)
    # ... unless the branch is scaled or masked: then the sums of the exit's pass are, and the LayerNorm backward above was not asked for any
    dt1, cs1, gs1 = exit1.backward(dx1, v.b1, want_projb, need["gamma1"])
    if not exit1.plain:
        projb_done = (_bgrad_from(p.projb, cs1) if cs1 is not None else None,)
    g["gamma1"] = _bgrad_from(p.gamma1, gs1) if gs1 is not None else None
    dln1, ga = _attn_bwd(dt1, v.ln1, (v.qkv, v.o, v.lse, v.sqk, v.mqk, v.rqk), B, N, H, c(p.qkvw), c(p.projw), p.qkvw, p.qkvb, p.projw, p.projb,
                         need, tp, wq, projb_done=projb_done, qkn=qkn, core=core)
    # ... and, published for whoever receives dx, the fc2 bias gradient of the Block before this one
    cs0 = torch.empty(D, dtype=torch.float32, device=dy2.device) if _BIAS_FROM_EPILOGUE else None
    dx, g["n1w"], g["n1b"] = _ln_bwd(dln1, x2, c(p.n1w), v.mean1, v.rstd1, p.n1w, p.n1b, dres=dx1, dx_colsum=cs0,
                                     dres_period=N if core.rows else 1)
    if cs0 is not None and in_dtype == cdtype:
        _publish_stream_colsum(wq, dx, cs0)
    wq.end_block()                                   # the Block's 4 weight gradients: grouped launch now, or with the next Blocks'
    g.update(ga, **gm, x=_ret_grad(dx.view(B, N, D), in_dtype))
    return g


class BlockFn(torch.autograd.Function):
    """Block.forward (building_blocks.py:236-239):
    x1 = x + s1 ⊙ γ1 ⊙ proj(attn(norm1(x))) ; y = x1 + s2 ⊙ γ2 ⊙ fc2(gelu(fc1(norm2(x1)))) (γ: LayerScale, absent = Identity).  Without drop path (s1 = s2 = None): 7 forward
    launches, residual adds and the activation fused into GEMM epilogues; the residual-branch gradients are fused into the LayerNorm
    backward.  With a scale a branch costs one row pass more forward (drop_path_add) and one backward (drop_path_scale)."""
    ARGS = _Slots("x", "n1w", "n1b", "qkvw", "qkvb", "projw", "projb", "n2w", "n2b", "f1w", "f1b", "f2w", "f2b", "num_heads", "eps", "cdtype",
                  "tp", "recompute", "s1", "s2", "drop", "gamma1", "gamma2", "save_branch", "qnw", "qnb", "knw", "knb", "qk_eps")

    @staticmethod
    def forward(ctx, x, n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, f1w, f1b, f2w, f2b, num_heads, eps, cdtype, tp=None, recompute=False,
                s1=None, s2=None, drop=None, gamma1=None, gamma2=None, save_branch=None, qnw=None, qnb=None, knw=None, knb=None, qk_eps=None):
        """s1, s2: the per-sample drop-path scales of the attention and the MLP branch (fp32 [B]); None = no drop path on that branch.
        qnw, qnb, knw, knb, qk_eps: the weight and bias of attn.q_norm / attn.k_norm (fp32 [head_dim]) and their eps, or None (no qk_norm:
        the launches of a Block without it).  One row pass over the qkv buffer forward, one over its gradient backward; when a gradient is
        wanted (save_branch) the un-normalised Q and K are kept: two more D-wide token matrices per Block, none under recompute, whose
        rebuilt forward gives the same bits.
        gamma1, gamma2: the LayerScale parameters of the two branches (fp32 [D], ls1.gamma / ls2.gamma) or None.  A branch with a gamma runs
        its exit GEMM without the residual and ops.layer_scale_add writes res + s ⊙ m ⊙ (gamma ⊙ branch) / keep; when a gradient is wanted
        the sum goes to a new buffer and the unscaled branch output is saved (two more token matrices per Block), else it overwrites the
        branch.  Under recompute only the input is kept, as without LayerScale.
        save_branch: whether a backward pass can follow.  Grad mode is always off in here, and needs_input_grad only says which inputs
        require a gradient, so the caller passes torch.is_grad_enabled() (as the modules do); None: decided from needs_input_grad alone,
        which keeps the branch outputs under no_grad too (the same bits, two token matrices more).
        drop: (p, seed_proj, seed_drop1, seed_drop2) = the rate of proj_drop / Mlp.drop and this pass's seeds of the three sites, or None.
        A branch with dropout runs its exit GEMM without the residual and ops.dropout_add writes res + s ⊙ m ⊙ branch / keep over it (the
        drop-path scale rides along); drop1 masks the activation in place before fc2.  The seeds are host integers kept on ctx, so the
        recomputation below regenerates the same masks.
        recompute = activation checkpointing of the Block (reference: apply_activation_checkpointing(Block),
        training_scripts/train_masked_fsdp.py:393-396): only the Block's INPUT is kept; backward re-runs the seven forward launches to
        rebuild ln1, qkv, o, lse, x1, ln2, h, a (15 of the 16 token matrices a Block otherwise keeps), then proceeds as usual.  The
        rebuilt tensors are bit-identical (no atomics, fixed reduction orders), so gradients equal the non-checkpointed ones exactly;
        the scales are kept with the input, so the rebuilt forward uses the same draw."""
        p = _BlockIn(n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, f1w, f1b, f2w, f2b, s1, s2, gamma1, gamma2, qnw, qnb, knw, knb)
        y, shape = _block_enter(ctx, _DenseCore, x, p, num_heads, eps, cdtype, tp, recompute, drop, save_branch, qk_eps)
        return y.view(shape)

    @staticmethod
    def backward(ctx, dy):
        return BlockFn.ARGS.grads(**_block_backward(ctx, _DenseCore, dy, BlockFn.ARGS.needs(ctx)))


TAIL_ROWS = os.environ.get("UCFVIT_TAIL_ROWS", "1") != "0"     # A/B switch: 0 = the last Block runs dense like every other
TAIL_ROWS_MAX_TOKENS = 8192                                    # AR_MAX_N of csrc/attention_rows.hip


class TailBlockFn(torch.autograd.Function):
    """BlockFn for the LAST Block of a model whose head reads only the class token (token 0 of every sequence; the final norm is
    row-wise): [B, N, D] -> the Block's output for those B rows, [B, D].  Everything up to the keys and values is needed for every
    token (LayerNorm 1, the qkv GEMM); from the attention on only the class rows are computed: one query per head
    (ops.attention_rows_fwd), then proj / LayerNorm 2 / fc1 / fc2 as M = B GEMMs, the proj residual read in place from the strided
    class rows of x (ldr = N D).  Backward: the same compact chain, weight gradients queued with B reduction rows; the gradient turns
    dense again at dK / dV (ops.attention_rows_bwd) and the class rows' residual gradient joins the dense dx inside the LayerNorm-1
    backward (dres_period = N), rounded once like the dense Block's."""
    ARGS = _Slots(*(n for n in BlockFn.ARGS.names if n != "tp"))

    @staticmethod
    def forward(ctx, x, n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, f1w, f1b, f2w, f2b, num_heads, eps, cdtype, recompute=False,
                s1=None, s2=None, drop=None, gamma1=None, gamma2=None, save_branch=None, qnw=None, qnb=None, knw=None, knb=None, qk_eps=None):
        """recompute: as in BlockFn, only the Block's input is kept and backward re-runs the forward launches (bit-identical);
        qnw, qnb, knw, knb, qk_eps: qk_norm as in BlockFn; the whole qkv buffer is normalised (every key is needed), then the class rows run;
        gamma1, gamma2, save_branch: the LayerScale parameters and the grad-mode flag as in BlockFn, applied to the class rows;
        s1, s2: the drop-path scales of the two branches as in BlockFn, one row per sample from the attention on;
        drop: BlockFn's dropout argument; the mask index steps by N rows, so class row b draws the mask of row b N of the dense Block"""
        p = _BlockIn(n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, f1w, f1b, f2w, f2b, s1, s2, gamma1, gamma2, qnw, qnb, knw, knb)
        return _block_enter(ctx, _ClassRowCore, x, p, num_heads, eps, cdtype, None, recompute, drop, save_branch, qk_eps)[0]

    @staticmethod
    def backward(ctx, dy):
        return TailBlockFn.ARGS.grads(**_block_backward(ctx, _ClassRowCore, dy, TailBlockFn.ARGS.needs(ctx)))


class PatchEmbedFn(torch.autograd.Function):
    """PatchEmbed.forward (building_blocks.py:78-92): conv(k=s=p) == im2col + GEMM + bias -> [B, L, D]."""

    @staticmethod
    def forward(ctx, img, weight, bias, patch, cdtype):
        if img.dtype != torch.float32:
            img = img.float()
        img = img if img.is_contiguous() else img.contiguous()
        cols = ops.im2col(img, patch, cdtype)
        w = compute_param(weight, cdtype)
        y = ops.linear_fwd(cols, w.view(w.shape[0], -1), compute_param(bias, cdtype))
        ctx.save_for_backward(cols, weight, bias)
        ctx.cdtype = cdtype
        B = img.shape[0]
        L = 1
        for d_ in img.shape[2:]:
            L *= d_ // patch
        return y.view(B, L, w.shape[0])          # (explicit L: an empty batch has no elements to infer it from)

    @staticmethod
    def backward(ctx, dy):
        cols, weight, bias = ctx.saved_tensors
        dy2 = _as(dy, ctx.cdtype).reshape(cols.shape[0], -1)
        gw = _wgrad(weight, dy2, cols) if ctx.needs_input_grad[1] else None
        gb = _bgrad(bias, dy2) if (bias is not None and ctx.needs_input_grad[2]) else None
        return None, gw, gb, None, None   # no gradient w.r.t. the image (leaf input of the training step)


def _tokens_backward(ctx, dout, cls, pos, B, Lp, D, cdtype, in_dtype, bwd_op):
    """The backward pass TokensFn and TimeTokensFn share: where dpos / dcls go (the flat gradient buffer or fresh tensors) and whether they
    accumulate, then one launch of `bwd_op` (ops.tokens_bwd | ops.time_tokens_bwd).  -> (gx, g_cls, g_pos, what bwd_op returns beyond the
    three gradients: dtemb or None)"""
    d = _as(dout, cdtype)
    want_pos = pos is not None and ctx.needs_input_grad[2]
    has_cls = cls is not None
    op = oc = None
    ap = ac = False
    if want_pos:
        op, ap = grad_target(pos)
    if has_cls:
        oc, ac = grad_target(cls)
    if (want_pos and has_cls and ap != ac) or (want_pos and has_cls and ((op is None) != (oc is None))):
        op = oc = None
        ap = ac = False
    acc = ap or ac
    dpatches, dpos, dcls, *rest = bwd_op(d, B, Lp, D, has_cls, want_pos,
                                         dpos=op.view(-1, D) if op is not None else None,
                                         dcls=oc.view(-1) if oc is not None else None, accumulate=acc,
                                         want_patches=ctx.needs_input_grad[0])
    g_pos = None if (not want_pos or acc) else (op if op is not None else dpos.view(pos.shape))
    g_cls = None if (not has_cls or acc) else (oc if oc is not None else dcls.view(cls.shape))
    gx = _ret_grad(dpatches.view(B, Lp, D), in_dtype) if dpatches is not None else None
    return gx, g_cls, g_pos, rest[0] if rest else None


class TokensFn(torch.autograd.Function):
    """VIT._pos_embed (arch.py:367-393): cat(cls, x) + pos_embed."""

    @staticmethod
    def forward(ctx, x, cls, pos, cdtype):
        xin = _as(x, cdtype)
        B, Lp, D = xin.shape
        out = ops.tokens_fwd(xin.view(B * Lp, D), compute_param(cls, cdtype), compute_param(pos, cdtype), B, Lp, D)
        ctx.save_for_backward(cls, pos)
        ctx.meta = (B, Lp, D, cdtype, x.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        cls, pos = ctx.saved_tensors
        B, Lp, D, cdtype, in_dtype = ctx.meta
        gx, g_cls, g_pos, _ = _tokens_backward(ctx, dout, cls, pos, B, Lp, D, cdtype, in_dtype, ops.tokens_bwd)
        return gx, g_cls, g_pos, None


class TimeTokensFn(torch.autograd.Function):
    """DiffusionVIT's token assembly: (cat(cls, x) + pos_embed) + temb[:, None, :], one pass (ucfvit_time_tokens_fwd).  temb [B, D] is the
    time MLP's output; its gradient (the sum of dout over a sample's rows) comes out of the same backward pass as dpatches, dpos, dcls.
    Gradient targets and accumulation of cls and pos are TokensFn's."""

    @staticmethod
    def forward(ctx, x, cls, pos, temb, cdtype):
        xin = _as(x, cdtype)
        B, Lp, D = xin.shape
        out = ops.time_tokens_fwd(xin.view(B * Lp, D), compute_param(cls, cdtype), compute_param(pos, cdtype), _as(temb, cdtype), B, Lp, D)
        ctx.save_for_backward(cls, pos)
        ctx.meta = (B, Lp, D, cdtype, x.dtype, temb.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        cls, pos = ctx.saved_tensors
        B, Lp, D, cdtype, in_dtype, temb_dtype = ctx.meta
        gx, g_cls, g_pos, dtemb = _tokens_backward(ctx, dout, cls, pos, B, Lp, D, cdtype, in_dtype, ops.time_tokens_bwd)
        return gx, g_cls, g_pos, _ret_grad(dtemb, temb_dtype) if ctx.needs_input_grad[3] else None, None


class ReluDropoutFn(torch.autograd.Function):
    """The hidden layer of DiffusionVIT's time MLP: y = m * relu(x) / keep in one pass (ucfvit_relu_dropout); p == 0 (eval) is plain ReLU.
    The mask is that of HipDropout (seed, element index) and is never stored: backward reads the pre-activation and the seed."""

    @staticmethod
    def forward(ctx, x, p, seed):
        xc = x if x.is_contiguous() else x.contiguous()
        ctx.save_for_backward(xc)
        ctx.site = (float(p), int(seed))
        return ops.relu_dropout(xc.view(-1, xc.shape[-1]), *ctx.site).view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        (xc,) = ctx.saved_tensors
        dc = dy if dy.is_contiguous() else dy.contiguous()
        dc = dc if dc.dtype == xc.dtype else _as(dc, xc.dtype)
        return ops.relu_dropout_bwd(xc.view(-1, xc.shape[-1]), dc.view(-1, dc.shape[-1]), *ctx.site).view(dy.shape), None, None


class SeqPatchesFn(torch.autograd.Function):
    """einops 'b c s p -> b s (p c)' on the adaptively patched input (arch.py:466); the input is data, no gradient."""

    @staticmethod
    def forward(ctx, x, cdtype):
        xin = x if x.dtype == torch.float32 else x.float()
        xin = xin if xin.is_contiguous() else xin.contiguous()
        B, C, S, P = xin.shape
        return ops.seq_patches(xin, cdtype).view(B, S, P * C)

    @staticmethod
    def backward(ctx, dy):
        return None, None


class AdaptivePosFn(torch.autograd.Function):
    """VIT._pos_embed with use_adaptive_pos_emb (arch.py:366-393): cat(cls, x) + cat(0, GELU(Linear(seq_ps))).  The K = 3 | 4 Linear,
    the GELU, the concatenation and the add are one kernel; backward recomputes the pre-activation from seq_ps."""

    @staticmethod
    def forward(ctx, x, seq_ps, w, bias, cls, cdtype):
        xin = _as(x, cdtype)
        B, S, D = xin.shape
        sp = seq_ps if seq_ps.dtype == torch.float32 else seq_ps.float()
        sp = sp if sp.is_contiguous() else sp.contiguous()
        out = ops.adaptive_pos_fwd(xin.view(B * S, D), sp, compute_param(w, cdtype), compute_param(bias, cdtype),
                                   compute_param(cls, cdtype).reshape(-1) if cls is not None else None, B, S, D)
        ctx.save_for_backward(sp, w, bias, cls)
        ctx.meta = (B, S, D, cdtype, x.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        sp, w, bias, cls = ctx.saved_tensors
        B, S, D, cdtype, in_dtype = ctx.meta
        d = _as(dout, cdtype)
        has_cls = cls is not None
        tw, aw = grad_target(w)
        tb, ab = grad_target(bias)
        tc, ac = grad_target(cls) if has_cls else (None, False)
        bits = (1 if aw else 0) | (2 if ab else 0) | (4 if ac else 0)
        dx, dw, db, dc = ops.adaptive_pos_bwd(d, sp, compute_param(w, cdtype), compute_param(bias, cdtype), B, S, D, has_cls,
                                              want_dx=ctx.needs_input_grad[0], dw=tw, dbias=tb,
                                              dcls=tc.view(-1) if tc is not None else None, acc_bits=bits)
        gx = _ret_grad(dx.view(B, S, D), in_dtype) if dx is not None else None
        g_w = None if aw else (tw if tw is not None else dw)
        g_b = None if ab else (tb if tb is not None else db)
        g_c = None
        if has_cls and not ac:
            g_c = tc if tc is not None else dc.view(cls.shape)
        return gx, None, g_w, g_b, g_c, None


class VarAggFn(torch.autograd.Function):
    """The attention of VariableMapping_Attention (building_blocks.py:336-366) for one aggregated variable: kv rows ordered (v, r),
    q = the projected learnt query [D] (fp32) -> [R, D]."""

    @staticmethod
    def forward(ctx, kv, q, V, head_dim, scale):
        kv = kv if kv.is_contiguous() else kv.contiguous()
        q32 = (q if q.dtype == torch.float32 else q.float()).reshape(-1).contiguous()
        D = q32.numel()
        R = kv.shape[0] // V
        out, lse = ops.varagg_fwd(kv, q32, V, R, D, head_dim, scale)
        ctx.save_for_backward(kv, q32, out, lse)
        ctx.meta = (V, R, D, head_dim, scale, q.dtype, q.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        kv, q32, out, lse = ctx.saved_tensors
        V, R, D, head_dim, scale, q_dtype, q_shape = ctx.meta
        d = _as(dout, kv.dtype)
        dkv, dq = ops.varagg_bwd(kv, q32, out, lse, d, V, R, D, head_dim, scale)
        return dkv, dq.to(q_dtype).view(q_shape), None, None, None


class CrossEntropyFn(torch.autograd.Function):
    """nn.CrossEntropyLoss()(logits, labels), mean reduction (train_class_simple.py:24-30); fp32 loss scalar."""

    @staticmethod
    def forward(ctx, logits, labels):
        l2 = logits if logits.is_contiguous() else logits.contiguous()
        loss, dl, _ = ops.cross_entropy(l2, labels, 1.0, want_grad=True)
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g.to(dl.dtype), None


class RandomMaskFn(torch.autograd.Function):
    """MAE.random_masking (arch.py:663-681) for a given noise tensor: returns (kept tokens, mask, ids_restore)."""

    @staticmethod
    def forward(ctx, x, noise, len_keep):
        B, Lp, D = x.shape
        xin = x if x.is_contiguous() else x.contiguous()
        ids_shuffle, ids_restore, mask = ops.mae_mask(noise.contiguous().float(), len_keep)
        kept = ops.gather_rows(xin, ids_shuffle, len_keep, Lp)
        ctx.save_for_backward(ids_shuffle)
        ctx.meta = (Lp, len_keep)
        ctx.mark_non_differentiable(mask, ids_restore)
        return kept, mask, ids_restore

    @staticmethod
    def backward(ctx, dkept, _dm, _di):
        (ids_shuffle,) = ctx.saved_tensors
        Lp, len_keep = ctx.meta
        d = dkept if dkept.is_contiguous() else dkept.contiguous()
        return ops.scatter_rows(d, ids_shuffle, Lp, Lp), None, None


class UnshuffleFn(torch.autograd.Function):
    """MAE.mask_head's un-shuffle (arch.py:687-697): gather(cat(x, mask_tokens), ids_restore) + decoder_pos_embed."""

    @staticmethod
    def forward(ctx, x, mask_token, ids_restore, pos, cdtype):
        xin = _as(x, cdtype)
        out = ops.unshuffle_fwd(xin, compute_param(mask_token, cdtype).reshape(-1), ids_restore, compute_param(pos, cdtype))
        ctx.save_for_backward(ids_restore, mask_token, pos)
        ctx.meta = (xin.shape[1], cdtype, x.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        ids_restore, mask_token, pos = ctx.saved_tensors
        R, cdtype, in_dtype = ctx.meta
        d = _as(dout, cdtype)
        want_pos = pos is not None and ctx.needs_input_grad[3]
        om, am = grad_target(mask_token)
        op, ap = grad_target(pos) if want_pos else (None, False)
        if want_pos and (am != ap or ((om is None) != (op is None))):
            om = op = None
            am = ap = False
        dx, dmask, dpos = ops.unshuffle_bwd(d, ids_restore, R, want_pos, dmask=om.view(-1) if om is not None else None,
                                            dpos=op.view(-1, d.shape[-1]) if op is not None else None, accumulate=am)
        g_m = None if am else (om if om is not None else dmask.view(mask_token.shape))
        g_p = None if (not want_pos or ap) else (op if op is not None else dpos.view(pos.shape))
        return _ret_grad(dx, in_dtype), g_m, None, g_p, None


class PatchMSEFn(torch.autograd.Function):
    """MSE between pred and patchify(img) (misc.py:14-33 + train_masked_simple.py:43-47), optional mask (metrics.py:11-17)."""

    @staticmethod
    def forward(ctx, pred, img, mask, patch):
        p = pred if pred.is_contiguous() else pred.contiguous()
        im = img if img.is_contiguous() else img.contiguous()
        loss, dpred = ops.patch_mse(p, im.float(), patch, mask=mask, grad_scale=1.0, want_grad=True)
        ctx.save_for_backward(dpred)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g.to(dpred.dtype), None, None, None


class InstNormActFn(torch.autograd.Function):
    """leaky_relu(instance_norm(x) [+ res], slope) — the normalisation / residual / activation chain of monai's UnetResBlock (reference
    simple/arch.py:808-940) as two HBM passes forward (statistics, apply) and two backward."""

    @staticmethod
    def forward(ctx, x, res, eps, slope):
        xin = x if x.is_contiguous() else x.contiguous()
        rin = None if res is None else (res if res.is_contiguous() else res.contiguous())
        y, mean, rstd = ops.instnorm_fwd(xin, rin, eps, slope)
        ctx.save_for_backward(xin, y, mean, rstd)
        ctx.slope, ctx.has_res = slope, res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, rstd = ctx.saved_tensors
        d = dy if dy.is_contiguous() else dy.contiguous()
        dx, dres = ops.instnorm_bwd(d.to(x.dtype), y, x, mean, rstd, ctx.slope, ctx.has_res and ctx.needs_input_grad[1])
        return dx, dres, None, None


class DiceCEFn(torch.autograd.Function):
    """monai DiceCELoss(to_onehot_y=True, softmax=True, squared_pred=True) (reference train_unetr_simple.py:38), forward + backward fused"""

    @staticmethod
    def forward(ctx, logits, labels, smooth_nr, smooth_dr):
        lb = labels if labels.is_contiguous() else labels.contiguous()
        # the HIP decoder's logits (a view at offset 0 over a [B, *spatial, ld] buffer): read in place, no N C D H W copy
        if logits.is_contiguous() or (logits.dim() >= 3 and logits.storage_offset() == 0 and ops.dice_strides(logits) is not None):
            lg = logits
        else:
            lg = logits.contiguous()
        loss, dl = ops.dice_ce(lg, lb, smooth_nr, smooth_dr, 1.0, want_grad=True)
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dice_grad_times(dl, g), None, None, None


def dice_grad_times(dl, g):
    """dl * g for a logits gradient of ops.dice_ce / dice_ce_from_stats: N C (D) H W, or a view over a padded channels-last buffer, which
    is scaled whole so that the product keeps dl's strides"""
    if dl.is_contiguous():
        return dl * g.to(dl.dtype)
    flat = dl.as_strided((dl.shape[0] * dl.stride(0),), (1,))           # the padded channels-last buffer behind the view
    return (flat * g.to(dl.dtype)).as_strided(dl.shape, dl.stride())


class SapHeadFn(torch.autograd.Function):
    """SAP.mask_head (reference simple/arch.py:523-533): ConvTranspose neck (kernel = stride = p, no bias) + 1x1 header on the token grid, as
    ONE Linear layer.  The two convolutions have no nonlinearity between them, so their weights fold into W_eff [p^nd C, D] (ops.sap_fold,
    fp32, rounded once to the compute dtype); the tokens go through ucfvit_gemm with an fp32 output and ops.sap_scatter_fwd moves the C
    channels into the [B, C, *(s p,) * nd] map.  The 256-channel map of the two-step form never exists.  Backward: inverse scatter, the data
    and weight gradient GEMMs of a Linear layer, ops.sap_unfold back to the gradients of the two convolution weights (fp32, fixed order)."""

    @staticmethod
    def forward(ctx, x, w_neck, w_head, b_head, p, s, nd, cdtype):
        B, S, D = x.shape
        if S != s ** nd:
            raise ValueError(f"SapHeadFn: {S} tokens do not fill a grid of {s}^{nd}")
        x2 = _as(x, cdtype).view(B * S, D)                       # x may be a slice (class token stripped): _as makes it dense
        wn, wh, bh = compute_param(w_neck, torch.float32), compute_param(w_head, torch.float32), compute_param(b_head, torch.float32)
        w_eff = ops.sap_fold(wn, wh, cdtype)
        N = w_eff.shape[0]
        rows = ops.gemm(x2, w_eff, B * S, N, D, ops.LAYOUT_KC, ops.LAYOUT_KC, out_dtype=torch.float32)
        out = ops.sap_scatter_fwd(rows, bh, B, p, s, nd)
        ctx.save_for_backward(x2, w_eff, w_neck, w_head)
        ctx.geom, ctx.cdtype, ctx.in_dtype, ctx.in_shape = (p, s, nd), cdtype, x.dtype, x.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        x2, w_eff, w_neck, w_head = ctx.saved_tensors
        p, s, nd = ctx.geom
        d = dout if dout.dtype == torch.float32 else dout.float()
        drows, dbias = ops.sap_scatter_bwd(d if d.is_contiguous() else d.contiguous(), p, s, nd, ctx.cdtype, want_dbias=ctx.needs_input_grad[3])
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _ret_grad(ops.linear_dgrad(drows, w_eff).view(ctx.in_shape), ctx.in_dtype)
        gn = gh = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw_eff = ops.linear_wgrad(drows, x2)
            gn, gh = ops.sap_unfold(dw_eff, compute_param(w_neck, torch.float32), compute_param(w_head, torch.float32))
        return dx, gn, gh, dbias, None, None, None, None


class DiceBCEFn(torch.autograd.Function):
    """utils/metrics.DiceBLoss with act=True (reference utils/metrics.py:95-121): one statistics pass in forward, the gradient pass in backward
    with autograd's upstream scalar read on the device.  logits fp32 or bf16 [B, C, *spatial], targets fp32 of the same shape."""

    @staticmethod
    def forward(ctx, logits, targets, weight, smooth):
        lg = logits if logits.is_contiguous() else logits.contiguous()
        tg = targets if targets.is_contiguous() else targets.contiguous()
        stats = ops.dice_bce_stats(lg, tg)
        loss, _ = ops.dice_bce_from_stats(lg, tg, stats, weight, smooth, want_grad=False)
        ctx.save_for_backward(lg, tg, stats)
        ctx.weight, ctx.smooth = weight, smooth
        return loss

    @staticmethod
    def backward(ctx, g):
        lg, tg, stats = ctx.saved_tensors
        gd = g if g.dtype == torch.float32 else g.float()
        _, dl = ops.dice_bce_from_stats(lg, tg, stats, ctx.weight, ctx.smooth, 1.0, gd.contiguous(), want_loss=False)
        return _ret_grad(dl, lg.dtype), None, None, None


class DeserializeFn(torch.autograd.Function):
    """Patchify.deserialize / Patchify_3D.deserialize with a gradient: a token sequence fp32 (the patch list [B, L, p, .., p, C] or the model
    layout [B, C, L, p^nd], read in place) painted into the image plane through the tree (ops.quadtree_deserialize / octree_deserialize); backward
    is the adjoint gather (ops.*_deserialize_bwd), deterministic, written in seq's own layout.  nodes / count carry no gradient.  Truncated
    tokens have none either, so there is no `truncate` here."""

    @staticmethod
    def forward(ctx, seq, nodes, count, size, patch, nd, mode, channels_last):
        if seq.dtype != torch.float32:
            raise TypeError(f"DeserializeFn: seq must be fp32, got {seq.dtype} (HF.deserialize casts under autograd)")
        fwd = ops.quadtree_deserialize if nd == 2 else ops.octree_deserialize
        out = fwd(seq, nodes, count, size, patch, mode=mode, channels_last=channels_last)
        ctx.save_for_backward(nodes, count)
        ctx.like = torch.empty_like(seq, device="meta")                     # shape and strides of seq, no memory
        ctx.args = (patch, nd, mode, channels_last)
        return out

    @staticmethod
    def backward(ctx, dout):
        nodes, count = ctx.saved_tensors
        patch, nd, mode, channels_last = ctx.args
        d = dout if dout.dtype == torch.float32 else dout.float()
        bwd = ops.quadtree_deserialize_bwd if nd == 2 else ops.octree_deserialize_bwd
        dseq = bwd(d if d.is_contiguous() else d.contiguous(), nodes, count, ctx.like, patch, mode=mode, channels_last=channels_last)
        return dseq, None, None, None, None, None, None, None


# ---------------------------------------------------------------------------------------------- public helpers
def instnorm_act(x, res=None, eps=1e-5, slope=0.01):
    return InstNormActFn.apply(x, res, eps, slope)


def dice_ce(logits, labels, smooth_nr=1e-5, smooth_dr=1e-5):
    return DiceCEFn.apply(logits, labels, smooth_nr, smooth_dr)


def segment(logits, labels):
    """logits [B, n, *spatial], labels int64 [B, *spatial] or [B, 1, *spatial] -> (pred uint8 [B, *spatial], counts int64 [B, 3, n]): the argmax
    label map and the per-(batch element, class) TP / PRED / LAB counts of a Dice accuracy (utils.metrics.dice_from_counts), one HIP pass
    (ops.seg_counts).  No gradient flows through either result; the inputs need none."""
    with torch.no_grad():
        return ops.seg_counts(logits.detach(), labels.detach(), want_pred=True)


def dice_bce(logits, targets, weight=0.5, smooth=1.0):
    return DiceBCEFn.apply(logits, targets, float(weight), float(smooth))


def deserialize(seq, nodes, count, size, patch, nd, mode=None, channels_last=True):
    """seq [B, L, p, .., p, C] or [B, C, L, p^nd] -> the image plane [B, *size, C] (channels_last) or [B, C, *size], differentiable in seq;
    nd = 2: size (H, W), mode 'bicubic' (default) or 'nearest'; nd = 3: size N, 'trilinear' or 'nearest'.  A seq that is not fp32 (SAP's bf16
    output) is cast here, under autograd, so its gradient comes back in its own dtype."""
    if nd not in (2, 3):
        raise ValueError(f"deserialize: nd must be 2 or 3, got {nd}")
    mode = ("bicubic" if nd == 2 else "trilinear") if mode is None else mode
    seq = seq if seq.dtype == torch.float32 else seq.float()
    return DeserializeFn.apply(seq, nodes, count, size, int(patch), nd, mode, bool(channels_last))


def cross_entropy(logits, labels):
    return CrossEntropyFn.apply(logits, labels)


def patch_mse(pred, img, patch_size, mask=None):
    return PatchMSEFn.apply(pred, img, mask, patch_size)


def q_sample(x0, t, eps, sqrt_ab, sqrt_1mab, out=None):
    """DDPM forward noising x_t = sqrt(abar_t) x0 + sqrt(1 - abar_t) eps on the device (no gradient: x0 and eps are data); t int64 [B] on the
    device, the two tables fp32 [T] (DDPM_Scheduler.sqrt_ab / sqrt_1mab)"""
    with torch.no_grad():
        x0 = x0 if x0.is_contiguous() else x0.contiguous()
        eps = eps if eps.is_contiguous() else eps.contiguous()
        return ops.ddpm_q_sample(x0, eps, t, sqrt_ab, sqrt_1mab, out=out)


def ddpm_step(x, pred, z, patch_size, c1, c2, sigma, out=None):
    """one ancestral reverse step x_{i-1} = c1 (x_i - c2 unpatchify(pred)) + sigma z on the image (no gradient)"""
    with torch.no_grad():
        pred = pred if pred.is_contiguous() else pred.contiguous()
        return ops.ddpm_step(x, pred, z, int(patch_size), c1, c2, sigma, out=out)


def ddim_step(x, pred, z, patch_size, coef, clip=None, out=None):
    """one generalised reverse step (DDIM) on the image (no gradient); coef = (s_ab, s_1mab, r_ab, r_1mab, c_x0, c_eps, sigma) of
    DDPM_Scheduler.ddim_coefficients; clip: clamp the predicted x0 to [-clip, clip] (None: no clamp)"""
    with torch.no_grad():
        pred = pred if pred.is_contiguous() else pred.contiguous()
        return ops.ddim_step(x, pred, z, int(patch_size), *coef, clip=clip, out=out)
