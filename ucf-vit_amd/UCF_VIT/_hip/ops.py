"""Tensor-level wrappers over the C ABI (no autograd here).  Every function enqueues HIP kernels on torch's
current stream and returns torch tensors that own the outputs.  PyTorch is used for device memory and streams only.
"""
import ctypes
import os
import math

import torch

from . import lib as _l
from .lib import ACT_GELU, ACT_GELU_GRAD, ACT_GELU_SAVE_DERIV, ACT_MUL_AUX, ACT_NONE, BF16, F32, LAYOUT_KC, LAYOUT_KS

_DT = {torch.float32: F32, torch.bfloat16: BF16}
_TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16}


def dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"UCF_VIT HIP ops support float32 and bfloat16 tensors, got {t.dtype}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t, name, rows_ok=False):
    """rows_ok: a 2-D matrix whose rows are contiguous but padded (stride(0) >= shape[1]) is accepted: the C ABI takes leading dimensions"""
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the MI355X (cuda) device, got {t.device}. "
                           "UCF_VIT operators run only through libucfvit_hip.so; there is no CPU path.")
    if not t.is_contiguous():
        if not (rows_ok and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
            raise RuntimeError(f"{name}: tensor must be contiguous")
    return t


def _p(t):
    return None if t is None else t.data_ptr()


_workspaces = {}


def workspace(nbytes, device):
    """fp32 scratch, cached per (device, stream): used and consumed inside one ABI call sequence on that stream."""
    key = (device.index, _stream())
    ws = _workspaces.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty(max(int(nbytes) // 4 + 1, 1 << 16), dtype=torch.float32, device=device)
        _workspaces[key] = ws
    return ws


# Dynamic tile schedule of the persistent GEMM (desc.sched_state, include/ucfvit_hip.h): off for a single process (every CU is the GEMM's,
# the static order costs nothing), switched on by HipDataParallel / the tensor-parallel blocks, whose collectives hold CUs while GEMMs run.
# UCFVIT_GEMM_DYNAMIC=1|0 forces it.  One state block per (device, stream): launches of one stream are ordered, so they can share it.
_dynamic_sched = os.environ.get("UCFVIT_GEMM_DYNAMIC", "") == "1"
_sched_states = {}


def set_dynamic_tile_schedule(on):
    global _dynamic_sched
    if os.environ.get("UCFVIT_GEMM_DYNAMIC", "") in ("0", "1"):
        return _dynamic_sched                      # forced by the environment
    _dynamic_sched = bool(on)
    return _dynamic_sched


def _sched_state(device):
    if not _dynamic_sched:
        return None
    key = (device.index, _stream())
    st = _sched_states.get(key)
    if st is None:
        st = torch.zeros(_l.GEMM_SCHED_BYTES // 4, dtype=torch.int32, device=device)     # zeroed once; every launch leaves it zeroed
        _sched_states[key] = st
    return st.data_ptr()


def mfma_probe(iters=10000):
    """diagnostic: one launch of a pure bf16 MFMA stream on the current stream; returns the FLOPs it executes"""
    L = _l.load()
    sink = workspace(1024, torch.device("cuda", torch.cuda.current_device()))
    flops = L.ucfvit_mfma_probe(sink.data_ptr(), int(iters), _stream())
    if flops < 0:
        _l.check(int(flops), "ucfvit_mfma_probe")
    return flops


# ------------------------------------------------------------------------------------------------ GEMM
def gemm(A, B, M, N, K, a_layout, b_layout, out=None, out_dtype=None, bias=None, residual=None, act=ACT_NONE,
         aux_in=None, aux_out=None, accumulate=False, alpha=1.0, c_colsum=None, c_colsum_accumulate=False, split_k_workspace=True):
    """C[M,N] = epilogue(alpha * op(A)·op(B)); A, B are 2-D row-major tensors (see include/ucfvit_hip.h).
    split_k_workspace=False withholds the split-K scratch (desc.workspace = NULL): the library then runs the problem un-split.
    c_colsum: optional fp32 [N] tensor that receives (+)= the column sums of C — as a by-product of the epilogue where the library
    has one (desc.c_colsum_partial + ucfvit_reduce_rows), else by a separate ucfvit_colsum pass over C."""
    L = _l.load()
    _chk(A, "gemm.A", rows_ok=True), _chk(B, "gemm.B", rows_ok=True)
    if A.dtype != B.dtype:
        raise TypeError("gemm: A and B must have the same dtype")
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype or A.dtype, device=A.device)
    d = _l.GemmDesc()
    d.A, d.B, d.C = A.data_ptr(), B.data_ptr(), out.data_ptr()
    d.bias, d.residual, d.aux_in, d.aux_out = _p(bias), _p(residual), _p(aux_in), _p(aux_out)
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = A.stride(0), B.stride(0), out.stride(0)
    d.ldr = residual.stride(0) if residual is not None else 0
    aux = aux_in if aux_in is not None else aux_out
    d.ldaux = aux.stride(0) if aux is not None else 0
    d.a_layout, d.b_layout = a_layout, b_layout
    d.dtype, d.out_dtype = dt(A), dt(out)
    d.act, d.accumulate, d.alpha = act, 1 if accumulate else 0, alpha
    d.workspace, d.workspace_bytes = None, 0
    d.c_colsum_partial = None
    d.sched_state = _sched_state(A.device)
    cs_rows, cs_part = 0, None
    if c_colsum is not None:
        _chk(c_colsum, "gemm.c_colsum")
        if c_colsum.dtype != torch.float32 or c_colsum.numel() != N or not c_colsum.is_contiguous():
            raise TypeError("gemm: c_colsum must be a contiguous fp32 tensor of N elements")
        cs_rows = L.ucfvit_gemm_colsum_rows(ctypes.byref(d))
        if cs_rows > 0:
            cs_part = workspace(cs_rows * N * 4, A.device)
            d.c_colsum_partial = cs_part.data_ptr()
    if split_k_workspace and act == ACT_NONE and bias is None and residual is None:      # only epilogue-free GEMMs (weight gradients) split K
        need = L.ucfvit_gemm_workspace(ctypes.byref(d))
        if need > 0:
            ws = workspace(need, A.device)
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    _l.check(L.ucfvit_gemm(ctypes.byref(d), _stream()), "ucfvit_gemm")
    if c_colsum is not None:
        if cs_rows > 0:
            _l.check(L.ucfvit_reduce_rows(cs_part.data_ptr(), c_colsum.data_ptr(), cs_rows, N, 1 if c_colsum_accumulate else 0, _stream()),
                     "ucfvit_reduce_rows")
        else:
            colsum(out, out=c_colsum, accumulate=c_colsum_accumulate)
    return out


def wgrad_grouped(items):
    """items: list of (dy2 [M,N], x2 [M,K], out [N,K] (fp32 or bf16) or None (fp32), accumulate) -> list of dW tensors; ONE launch when groupable.
    The library groups problems of one reduction length M: items of several lengths (the compact gradients of a tail Block among dense
    ones) go out as one launch per length."""
    rows = {it[0].shape[0] for it in items}
    if len(rows) > 1:
        outs = [None] * len(items)
        for r in sorted(rows, reverse=True):
            idx = [i for i, it in enumerate(items) if it[0].shape[0] == r]
            for i, o in zip(idx, wgrad_grouped([items[i] for i in idx])):
                outs[i] = o
        return outs
    L = _l.load()
    n = len(items)
    outs = []
    arr = (_l.GemmDesc * n)()
    for i, (dy2, x2, out, acc) in enumerate(items):
        _chk(dy2, "wgrad.dy", rows_ok=True), _chk(x2, "wgrad.x", rows_ok=True)
        Mtok, N = dy2.shape
        K = x2.shape[1]
        if out is None:
            out = torch.empty((N, K), dtype=torch.float32, device=dy2.device)
        outs.append(out)
        d = arr[i]
        d.A, d.B, d.C = dy2.data_ptr(), x2.data_ptr(), out.data_ptr()
        d.bias = d.residual = d.aux_in = d.aux_out = None
        d.M, d.N, d.K = N, K, Mtok
        d.lda, d.ldb, d.ldc, d.ldr, d.ldaux = dy2.stride(0), x2.stride(0), out.stride(0), 0, 0
        d.a_layout, d.b_layout = LAYOUT_KS, LAYOUT_KS
        d.dtype, d.out_dtype = dt(dy2), dt(out)
        d.act, d.accumulate, d.alpha = ACT_NONE, 1 if acc else 0, 1.0
        d.workspace, d.workspace_bytes = None, 0
        d.c_colsum_partial = None
        d.sched_state = _sched_state(dy2.device)
    _l.check(L.ucfvit_gemm_grouped(arr, n, _stream()), "ucfvit_gemm_grouped")
    return outs


def linear_fwd(x2, w, b=None, act=ACT_NONE, residual=None, aux_out=None, out=None):
    """y[M,N] = act(x2[M,K]·w[N,K]ᵀ + b) + residual   (nn.Linear forward, building_blocks.py:123,127,159,190)"""
    M, K = x2.shape
    N = w.shape[0]
    return gemm(x2, w, M, N, K, LAYOUT_KC, LAYOUT_KC, out=out, bias=b, residual=residual, act=act,
                aux_out=aux_out)


def _dgrad_act(act_grad_aux, aux_is_deriv):
    if act_grad_aux is None:
        return ACT_NONE
    return ACT_MUL_AUX if aux_is_deriv else ACT_GELU_GRAD


def linear_dgrad(dy2, w, act_grad_aux=None, out=None, aux_is_deriv=False, c_colsum=None, c_colsum_accumulate=False):
    """dx[M,K] = dy2[M,N]·w[N,K], optionally times gelu'(aux) (aux = the fc1 pre-activation) or times aux itself
    (aux_is_deriv: aux = gelu' saved by the forward epilogue, ACT_GELU_SAVE_DERIV)"""
    M, N = dy2.shape
    K = w.shape[1]
    return gemm(dy2, w, M, K, N, LAYOUT_KC, LAYOUT_KS, out=out, act=_dgrad_act(act_grad_aux, aux_is_deriv), aux_in=act_grad_aux,
                c_colsum=c_colsum, c_colsum_accumulate=c_colsum_accumulate)


def linear_wgrad(dy2, x2, out=None, accumulate=False):
    """dW[N,K] (fp32) = dy2[M,N]ᵀ·x2[M,K]"""
    M, N = dy2.shape
    K = x2.shape[1]
    return gemm(dy2, x2, N, K, M, LAYOUT_KS, LAYOUT_KS, out=out, out_dtype=torch.float32, accumulate=accumulate)


def reduce_rows(partial, out, accumulate=False):
    """out[N] (+)= sum over the rows of partial [R, N] (fp32)"""
    L = _l.load()
    R, N = partial.shape
    _l.check(L.ucfvit_reduce_rows(partial.data_ptr(), out.data_ptr(), R, N, 1 if accumulate else 0, _stream()), "ucfvit_reduce_rows")
    return out


def colsum(x2, out=None, accumulate=False):
    L = _l.load()
    _chk(x2, "colsum.x", rows_ok=True)
    M, N = x2.shape
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=x2.device)
    ws = workspace(L.ucfvit_colsum_workspace(M, N), x2.device)
    _l.check(L.ucfvit_colsum(x2.data_ptr(), out.data_ptr(), M, N, x2.stride(0), 1 if accumulate else 0, ws.data_ptr(), dt(x2),
                             _stream()), "ucfvit_colsum")
    return out


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x2, gamma, beta, eps):
    L = _l.load()
    _chk(x2, "layernorm.x")
    rows, D = x2.shape
    y = torch.empty_like(x2)
    mean = torch.empty(rows, dtype=torch.float32, device=x2.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x2.device)
    _l.check(L.ucfvit_layernorm_fwd(x2.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                    rows, D, eps, dt(x2), _stream()), "ucfvit_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy2, x2, gamma, mean, rstd, dres=None, dgamma=None, dbeta=None, accumulate=False, dx_colsum=None,
                  dx_colsum_accumulate=False, dres_period=1):
    """-> dx, dgamma, dbeta; dx_colsum: optional fp32 [D] that receives (+)= the column sums of dx (a bias gradient, see the header).
    dres_period = P > 1: dres is compact, [ceil(rows / P), D], and belongs to rows 0, P, 2 P, ... (every other row adds +0)"""
    L = _l.load()
    _chk(dy2, "layernorm_bwd.dy")
    rows, D = x2.shape
    if dres is not None:
        _chk(dres, "layernorm_bwd.dres")
        if dres_period < 1 or tuple(dres.shape) != (-(-rows // dres_period), D) or dres.dtype != x2.dtype:
            raise ValueError("layernorm_bwd: dres must be [ceil(rows / dres_period), D] of x's dtype")
    dx = torch.empty_like(x2)
    if dgamma is None:
        dgamma = torch.empty(D, dtype=torch.float32, device=x2.device)
    if dbeta is None:
        dbeta = torch.empty(D, dtype=torch.float32, device=x2.device)
    ws = workspace(L.ucfvit_layernorm_bwd_workspace(rows, D), x2.device)
    _l.check(L.ucfvit_layernorm_bwd_rows(dy2.data_ptr(), x2.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _p(dres),
                                         int(dres_period), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), rows, D, 1 if accumulate else 0,
                                         _p(dx_colsum), 1 if dx_colsum_accumulate else 0, ws.data_ptr(), dt(x2), _stream()),
             "ucfvit_layernorm_bwd_rows")
    return dx, dgamma, dbeta


# ------------------------------------------------------------------------------------------------ attention
def attention_fwd(qkv, B, N, H, dh, scale):
    """qkv: [B*N, 3*H*dh] (the qkv Linear's output) -> out [B*N, H*dh], lse [B,H,N]"""
    L = _l.load()
    _chk(qkv, "attention.qkv")
    out = torch.empty((B * N, H * dh), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
    _l.check(L.ucfvit_attention_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, N, H, dh, scale, dt(qkv), _stream()),
             "ucfvit_attention_fwd")
    return out, lse


def attention_bwd_colsum_supported(B, N, H, dh, dtype):
    return bool(_l.load().ucfvit_attention_bwd_colsum_supported(B, N, H, dh, _DT[dtype]))


def attention_bwd(qkv, out, dout, lse, B, N, H, dh, scale, want_colsum=False):
    """-> dqkv, or (dqkv, partial) with want_colsum: partial fp32 [B, 2 H dh] = the column sums of dQ over each batch element's tokens and
    zeros for dK (include/ucfvit_hip.h: the K third of the qkv bias gradient is identically 0, the V third is the column sum of dout), or
    None where the shape runs the streaming kernels (the caller sums dqkv itself)"""
    L = _l.load()
    _chk(dout, "attention_bwd.dout")
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
    if want_colsum and L.ucfvit_attention_bwd_colsum_supported(B, N, H, dh, dt(qkv)):
        part = torch.empty((B, 2 * H * dh), dtype=torch.float32, device=qkv.device)
        _l.check(L.ucfvit_attention_bwd_colsum(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), delta.data_ptr(),
                                               part.data_ptr(), B, N, H, dh, scale, dt(qkv), _stream()), "ucfvit_attention_bwd_colsum")
        return dqkv, part
    _l.check(L.ucfvit_attention_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), delta.data_ptr(),
                                    B, N, H, dh, scale, dt(qkv), _stream()), "ucfvit_attention_bwd")
    return (dqkv, None) if want_colsum else dqkv


def attention_rows_fwd(qkv, B, N, H, dh, scale, qrow=0):
    """one query (token `qrow`) per batch element against all N keys: qkv [B*N, 3*H*dh] -> out [B, H*dh] (compact), lse [B, H]"""
    L = _l.load()
    _chk(qkv, "attention_rows.qkv")
    out = torch.empty((B, H * dh), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, H), dtype=torch.float32, device=qkv.device)
    _l.check(L.ucfvit_attention_rows_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, N, H, dh, int(qrow), scale, dt(qkv), _stream()),
             "ucfvit_attention_rows_fwd")
    return out, lse


def attention_rows_bwd(qkv, out, dout, lse, B, N, H, dh, scale, qrow=0, want_colsum=False):
    """out / dout: compact [B, H*dh] -> dqkv [B*N, 3*H*dh] (Q third: token `qrow` only, zeros elsewhere), or (dqkv, partial fp32 [B, 2 H dh])
    with want_colsum (partial: dq of every batch element, then zeros; see attention_bwd)"""
    L = _l.load()
    _chk(out, "attention_rows_bwd.out"), _chk(dout, "attention_rows_bwd.dout"), _chk(qkv, "attention_rows_bwd.qkv")
    if tuple(out.shape) != (B, H * dh) or tuple(dout.shape) != (B, H * dh) or dout.dtype != qkv.dtype or out.dtype != qkv.dtype:
        raise ValueError("attention_rows_bwd: out and dout must be [B, H*dh] of qkv's dtype")
    dqkv = torch.empty_like(qkv)
    part = torch.empty((B, 2 * H * dh), dtype=torch.float32, device=qkv.device) if want_colsum else None
    _l.check(L.ucfvit_attention_rows_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), _p(part), B, N, H, dh,
                                         int(qrow), scale, dt(qkv), _stream()), "ucfvit_attention_rows_bwd")
    return (dqkv, part) if want_colsum else dqkv


def attention_cross_fwd(q, k, v, B, Nq, Nk, H, dh, scale):
    """q [B*Nq, ldq], k / v [B*Nk, ldkv] (2-D views, head h at columns h*dh..) -> (out [B*Nq, H*dh], lse [B, H, Nq] in log2 units)"""
    L = _l.load()
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _chk(t, "attention_cross_fwd." + n, rows_ok=True)
    if k.stride(0) != v.stride(0) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError("attention_cross_fwd: k and v must share their row stride, and all operands their dtype")
    out = torch.empty((B * Nq, H * dh), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    _l.check(L.ucfvit_attention_cross_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), B, Nq, Nk, H, dh, q.stride(0),
                                          k.stride(0), scale, dt(q), _stream()), "ucfvit_attention_cross_fwd")
    return out, lse


def attention_cross_bwd(q, k, v, out, dout, lse, dq, dk, dv, B, Nq, Nk, H, dh, scale, accumulate):
    """this (query block, key block) pair's gradient terms, (+)= into fp32 dq [B*Nq, H*dh], dk / dv [B*Nk, H*dh]; lse / out: of the FULL softmax"""
    L = _l.load()
    _chk(dout, "attention_cross_bwd.dout"), _chk(out, "attention_cross_bwd.out")
    for t in (dq, dk, dv):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("attention_cross_bwd: dq / dk / dv must be contiguous fp32")
    delta = workspace(B * H * Nq * 4, q.device)
    _l.check(L.ucfvit_attention_cross_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                                          dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), B, Nq, Nk, H, dh, q.stride(0), k.stride(0), scale,
                                          1 if accumulate else 0, dt(q), _stream()), "ucfvit_attention_cross_bwd")


def attention_merge(o_acc, lse_acc, o_part, lse_part, B, Nq, H, dh, first):
    L = _l.load()
    _l.check(L.ucfvit_attention_merge(o_acc.data_ptr(), lse_acc.data_ptr(), o_part.data_ptr(), lse_part.data_ptr(), B, Nq, H, dh, 1 if first else 0,
                                      dt(o_part), _stream()), "ucfvit_attention_merge")


# ------------------------------------------------------------------------------------------------ front end
def im2col(img, p, out_dtype):
    """img fp32 [B,C,H,W] or [B,C,H,W,Z] -> [B*L, C*p^nd] in out_dtype, K-order (c, ph, pw[, pd])"""
    L = _l.load()
    _chk(img, "im2col.img")
    if img.dtype != torch.float32:
        raise TypeError("im2col: image must be float32 (as the reference dataloaders deliver it)")
    B, C = img.shape[0], img.shape[1]
    sp = list(img.shape[2:])
    nd = len(sp)
    Lp = 1
    for s in sp:
        Lp *= s // p
    cols = torch.empty((B * Lp, C * p ** nd), dtype=out_dtype, device=img.device)
    dims = (ctypes.c_int64 * 3)(*(sp + [1] * (3 - nd)))
    _l.check(L.ucfvit_im2col(img.data_ptr(), cols.data_ptr(), B, C, dims, nd, p, _DT[out_dtype], _stream()), "ucfvit_im2col")
    return cols


def tokens_fwd(patches, cls, pos, B, Lp, D):
    L = _l.load()
    _chk(patches, "tokens.patches")
    pre = 0 if cls is None else 1
    out = torch.empty((B, Lp + pre, D), dtype=patches.dtype, device=patches.device)
    _l.check(L.ucfvit_tokens_fwd(patches.data_ptr(), _p(cls), _p(pos), out.data_ptr(), B, Lp, D, pre, dt(patches), _stream()),
             "ucfvit_tokens_fwd")
    return out


def tokens_bwd(dout, B, Lp, D, has_cls, want_pos, dpos=None, dcls=None, accumulate=False, want_patches=True):
    L = _l.load()
    _chk(dout, "tokens_bwd.dout")
    dev = dout.device
    dpatches = torch.empty((B * Lp, D), dtype=dout.dtype, device=dev) if want_patches else None
    pre = 1 if has_cls else 0
    if want_pos and dpos is None:
        dpos = torch.empty((Lp + pre, D), dtype=torch.float32, device=dev)
    if has_cls and dcls is None:
        dcls = torch.empty(D, dtype=torch.float32, device=dev)
    _l.check(L.ucfvit_tokens_bwd(dout.data_ptr(), _p(dpatches), _p(dpos) if want_pos else None, _p(dcls) if has_cls else None, B, Lp, D,
                                 pre, 1 if accumulate else 0, dt(dout), _stream()), "ucfvit_tokens_bwd")
    return dpatches, dpos, dcls


# ------------------------------------------------------------------------------------------------ adaptive patching
def seq_patches(x, dtype):
    """x fp32 [B, C, S, P] -> rows [B*S, P*C] in `dtype` (einops 'b c s p -> b s (p c)', arch.py:466)"""
    L = _l.load()
    _chk(x, "seq_patches.x")
    if x.dtype != torch.float32 or x.dim() != 4:
        raise TypeError("seq_patches: x must be fp32 [B, C, S, P]")
    B, C, S, P = x.shape
    out = torch.empty((B * S, P * C), dtype=dtype, device=x.device)
    _l.check(L.ucfvit_seq_patches(x.data_ptr(), out.data_ptr(), B, C, S, P, _DT[dtype], _stream()), "ucfvit_seq_patches")
    return out


def _chk_seq_ps(seq_ps, B, S, name):
    _chk(seq_ps, name)
    if seq_ps.dtype != torch.float32 or seq_ps.dim() != 3 or seq_ps.shape[0] != B or seq_ps.shape[1] != S or seq_ps.shape[2] not in (3, 4):
        raise ValueError(f"{name}: seq_ps must be fp32 [B={B}, S={S}, 3|4], got {tuple(seq_ps.shape)} {seq_ps.dtype}")
    return seq_ps.shape[2]


def adaptive_pos_fwd(x2, seq_ps, w, bias, cls, B, S, D):
    """out [B, S+pre, D] = cat(cls, x) + cat(0, GELU(seq_ps w^T + bias))"""
    L = _l.load()
    _chk(x2, "adaptive_pos.x"), _chk(w, "adaptive_pos.w"), _chk(bias, "adaptive_pos.bias")
    kin = _chk_seq_ps(seq_ps, B, S, "adaptive_pos.seq_ps")
    if tuple(x2.shape) != (B * S, D) or tuple(w.shape) != (D, kin) or bias.numel() != D or w.dtype != x2.dtype or bias.dtype != x2.dtype:
        raise ValueError("adaptive_pos_fwd: shape / dtype mismatch")
    pre = 0 if cls is None else 1
    if cls is not None and (cls.numel() != D or cls.dtype != x2.dtype):
        raise ValueError("adaptive_pos_fwd: cls must hold D values of the compute dtype")
    out = torch.empty((B, S + pre, D), dtype=x2.dtype, device=x2.device)
    _l.check(L.ucfvit_adaptive_pos_fwd(x2.data_ptr(), seq_ps.data_ptr(), w.data_ptr(), bias.data_ptr(), _p(cls), out.data_ptr(), B, S, D, kin,
                                       pre, dt(x2), _stream()), "ucfvit_adaptive_pos_fwd")
    return out


def adaptive_pos_bwd(dout, seq_ps, w, bias, B, S, D, has_cls, want_dx=True, dw=None, dbias=None, dcls=None, acc_bits=0):
    """returns (dx [B*S, D] or None, dw fp32 [D, kin], dbias fp32 [D], dcls fp32 [D] or None); given outputs are written in place,
    acc_bits (1 dw, 2 dbias, 4 dcls) selects += for them"""
    L = _l.load()
    _chk(dout, "adaptive_pos_bwd.dout")
    kin = _chk_seq_ps(seq_ps, B, S, "adaptive_pos_bwd.seq_ps")
    pre = 1 if has_cls else 0
    _chk(w, "adaptive_pos_bwd.w"), _chk(bias, "adaptive_pos_bwd.bias")
    if (tuple(dout.shape) != (B, S + pre, D) or tuple(w.shape) != (D, kin) or bias.numel() != D or w.dtype != dout.dtype
            or bias.dtype != dout.dtype):
        raise ValueError("adaptive_pos_bwd: shape / dtype mismatch")
    dev = dout.device
    dx = torch.empty((B * S, D), dtype=dout.dtype, device=dev) if want_dx else None
    if dw is None:
        dw = torch.empty((D, kin), dtype=torch.float32, device=dev)
    if dbias is None:
        dbias = torch.empty(D, dtype=torch.float32, device=dev)
    if has_cls and dcls is None:
        dcls = torch.empty(D, dtype=torch.float32, device=dev)
    for t, n in ((dw, D * kin), (dbias, D), (dcls, D)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous()):
            raise ValueError("adaptive_pos_bwd: gradient outputs must be contiguous fp32 of the parameter's size")
    ws = workspace(L.ucfvit_adaptive_pos_bwd_workspace(B, S, D, kin, pre, dt(dout)), dev)
    _l.check(L.ucfvit_adaptive_pos_bwd(dout.data_ptr(), seq_ps.data_ptr(), w.data_ptr(), bias.data_ptr(), _p(dx), dw.data_ptr(), dbias.data_ptr(),
                                       _p(dcls) if has_cls else None, B, S, D, kin, pre, acc_bits, ws.data_ptr(), dt(dout), _stream()),
             "ucfvit_adaptive_pos_bwd")
    return dx, dw, dbias, (dcls if has_cls else None)


# ------------------------------------------------------------------------------------------------ variable aggregation
def varagg_fwd(kv, q, V, R, D, head_dim, scale):
    """kv [V*R, 2D] (rows ordered (v, r)), q fp32 [D] -> (out [R, D], lse fp32 [R, H])"""
    L = _l.load()
    _chk(kv, "varagg.kv"), _chk(q, "varagg.q")
    if tuple(kv.shape) != (V * R, 2 * D) or q.dtype != torch.float32 or q.numel() != D:
        raise ValueError("varagg_fwd: kv must be [V*R, 2D] and q fp32 [D]")
    out = torch.empty((R, D), dtype=kv.dtype, device=kv.device)
    lse = torch.empty((R, D // head_dim), dtype=torch.float32, device=kv.device)
    _l.check(L.ucfvit_varagg_fwd(kv.data_ptr(), q.data_ptr(), out.data_ptr(), lse.data_ptr(), R, V, D, head_dim, scale, dt(kv), _stream()),
             "ucfvit_varagg_fwd")
    return out, lse


def varagg_bwd(kv, q, out, lse, dout, V, R, D, head_dim, scale):
    """-> (dkv [V*R, 2D], dq fp32 [D])"""
    L = _l.load()
    _chk(dout, "varagg_bwd.dout")
    dkv = torch.empty_like(kv)
    dq_rows = torch.empty((R, D), dtype=torch.float32, device=kv.device)
    _l.check(L.ucfvit_varagg_bwd(kv.data_ptr(), q.data_ptr(), out.data_ptr(), lse.data_ptr(), dout.data_ptr(), dkv.data_ptr(), dq_rows.data_ptr(),
                                 R, V, D, head_dim, scale, dt(kv), _stream()), "ucfvit_varagg_bwd")
    return dkv, colsum(dq_rows)


# ------------------------------------------------------------------------------------------------ quadtree patcher
def _tree_build(name, nd, domain, fixed_length, *rule):
    """the builder of a 2^nd-ary tree: domain uint8 [B, H, W] or cubic [B, N, N, N]; rule: what the 3-D entry point takes beside the shape"""
    L = _l.load()
    what = "edges" if nd == 2 else "domain"
    _chk(domain, f"{name}.{what}")
    if domain.dtype != torch.uint8 or domain.dim() != nd + 1 or (nd == 3 and len(set(domain.shape[1:])) != 1):
        raise TypeError(f"{name}: edges must be uint8 [B, H, W]" if nd == 2 else
                        f"{name}: domain must be a batch of cubic uint8 volumes [B, N, N, N]")
    B, dev = domain.shape[0], domain.device
    dims = tuple(domain.shape[1:3]) if nd == 2 else (domain.shape[1],)
    nodes = torch.empty((B, fixed_length, 2 * nd), dtype=torch.int32, device=dev)
    values = torch.empty((B, fixed_length), dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    seq_ps = torch.empty((B, fixed_length, nd + 1), dtype=torch.float32, device=dev)
    size, fn = (L.ucfvit_quadtree_workspace, L.ucfvit_quadtree_build) if nd == 2 else (L.ucfvit_octree_workspace, L.ucfvit_octree_build)
    ws = workspace(size(B, *dims), dev)
    _l.check(fn(domain.data_ptr(), nodes.data_ptr(), values.data_ptr(), count.data_ptr(), seq_ps.data_ptr(), B, *dims, fixed_length, *rule,
                ws.data_ptr(), _stream()), fn.__name__)
    return nodes, values, count, seq_ps


def _serialize(name, nd, img, nodes, count, patch):
    """img fp32 [B, H, W, C] or [B, N, N, N, C] -> the patch list [B, L, p, .., p, C]"""
    L = _l.load()
    _chk(img, f"{name}.img"), _chk(nodes, f"{name}.nodes"), _chk(count, f"{name}.count")
    if img.dtype != torch.float32 or img.dim() != nd + 2 or nodes.dtype != torch.int32 or count.dtype != torch.int32:
        raise TypeError(f"{name}: img fp32 [B, {'H, W' if nd == 2 else 'N, N, N'}, C], nodes int32 [B, L, {2 * nd}], count int32 [B]")
    B, C, S = img.shape[0], img.shape[-1], nodes.shape[1]
    dims = tuple(img.shape[1:3]) if nd == 2 else (img.shape[1],)
    seq = torch.empty((B, S) + (patch,) * nd + (C,), dtype=torch.float32, device=img.device)
    fn = L.ucfvit_quadtree_serialize if nd == 2 else L.ucfvit_octree_serialize
    _l.check(fn(img.data_ptr(), nodes.data_ptr(), count.data_ptr(), seq.data_ptr(), B, *dims, C, S, patch, _stream()), fn.__name__)
    return seq


def quadtree_build(edges, fixed_length):
    """edges uint8 [B, H, W] (0 / 255) -> (nodes int32 [B, L, 4] = (x1, x2, y1, y2), values int32 [B, L], count int32 [B],
    seq_ps fp32 [B, L, 3] = (size, centre x, centre y))"""
    return _tree_build("quadtree_build", 2, edges, fixed_length)


def quadtree_serialize(img, nodes, count, patch):
    """img fp32 [B, H, W, C], nodes / count from quadtree_build -> x [B, C, L, patch*patch] (the reference's plain reshape of the
    [L, p, p, C] patch list, transform.py:42-48) = the model input of adaptive_patching=True"""
    seq = _serialize("quadtree_serialize", 2, img, nodes, count, patch)
    return seq.view(seq.shape[0], seq.shape[-1], seq.shape[1], patch * patch)


def octree_build(domain, fixed_length, norm_factor=255):
    """domain uint8 [B, N, N, N] ([z][y][x]) -> (nodes int32 [B, L, 6], values int32 [B, L], count int32 [B], seq_ps fp32 [B, L, 4])"""
    return _tree_build("octree_build", 3, domain, fixed_length, int(norm_factor))


def octree_serialize(img, nodes, count, patch, flat=True):
    """img fp32 [B, N, N, N, C] -> x [B, C, L, patch**3] (Patchify_3D's plain reshape, transform.py:123-126) or, flat=False, the patch list
    [B, L, p, p, p, C]"""
    seq = _serialize("octree_serialize", 3, img, nodes, count, patch)
    return seq.view(seq.shape[0], seq.shape[-1], seq.shape[1], patch ** 3) if flat else seq


_LABEL_DT = {torch.uint8: _l.LABEL_U8, torch.int64: _l.LABEL_I64}


def _serialize_labels(name, nd, labels, nodes, count, patch, num_classes, want_idx, want_onehot):
    L = _l.load()
    _chk(labels, f"{name}.labels"), _chk(nodes, f"{name}.nodes"), _chk(count, f"{name}.count")
    if labels.dtype not in _LABEL_DT or labels.dim() != nd + 1 or nodes.dtype != torch.int32 or nodes.dim() != 3 or \
            nodes.shape[2] != 2 * nd or count.dtype != torch.int32 or count.dim() != 1:
        raise TypeError(f"{name}: labels uint8 or int64 [B, {', '.join('HW' if nd == 2 else 'NNN')}], nodes int32 [B, L, {2 * nd}], count int32 [B]")
    if nd == 3 and not (labels.shape[1] == labels.shape[2] == labels.shape[3]):
        raise TypeError(f"{name}: labels must be a batch of cubic volumes [B, N, N, N]")
    if nodes.shape[0] != labels.shape[0] or count.shape[0] != labels.shape[0]:
        raise ValueError(f"{name}: labels, nodes and count must share the batch size")
    if not (want_idx or want_onehot):
        raise ValueError(f"{name}: nothing to compute (want_idx and want_onehot are both False)")
    B, S = labels.shape[0], nodes.shape[1]
    patch, num_classes = int(patch), int(num_classes)
    if patch < 1 or not 1 <= num_classes <= 255:
        raise ValueError(f"{name}: need patch >= 1 and 1 <= num_classes <= 255 (got {patch}, {num_classes})")
    P = patch ** nd
    idx = torch.empty((B, S) + (patch,) * nd, dtype=torch.int64, device=labels.device) if want_idx else None
    onehot = torch.empty((B, num_classes, S * P), dtype=torch.float32, device=labels.device) if want_onehot else None
    dims = labels.shape[1:3] if nd == 2 else labels.shape[1:2]
    fn = L.ucfvit_quadtree_serialize_labels if nd == 2 else L.ucfvit_octree_serialize_labels
    _l.check(fn(labels.data_ptr(), nodes.data_ptr(), count.data_ptr(), _p(idx), _p(onehot), B, *dims, S, patch, num_classes,
                _LABEL_DT[labels.dtype], _stream()), fn.__name__)
    return idx, onehot


def quadtree_serialize_labels(labels, nodes, count, patch, num_classes, want_idx=True, want_onehot=True):
    """labels uint8 or int64 [B, H, W], nodes / count from quadtree_build -> (idx int64 [B, L, p, p] or None, onehot fp32 [B, nc, L * p * p] or
    None): every leaf's label region resampled to p x p with the nearest-neighbour rule (ucfvit_quadtree_serialize_labels); padding rows are class 0;
    the one-hot block is the reference's collated seq_label in the memory order training_step_adaptive reshapes"""
    return _serialize_labels("quadtree_serialize_labels", 2, labels, nodes, count, patch, num_classes, want_idx, want_onehot)


def octree_serialize_labels(labels, nodes, count, patch, num_classes, want_idx=True, want_onehot=True):
    """labels uint8 or int64 [B, N, N, N], nodes / count from octree_build -> (idx int64 [B, L, p, p, p] or None, onehot fp32 [B, nc, L * p^3] or None)"""
    return _serialize_labels("octree_serialize_labels", 3, labels, nodes, count, patch, num_classes, want_idx, want_onehot)


def _seq_strides(name, nd, seq, patch):
    """(C, L, element strides (b, c, s, e)) of a token sequence read in place: the patch list [B, L, p, .., p, C] (any strides whose patch axes are
    jointly regular, e.g. contiguous) or the model layout [B, C, L, p^nd]"""
    P = patch ** nd
    if seq.dim() == 4 and seq.shape[3] == P:                                # [B, C, L, P]
        return seq.shape[1], seq.shape[2], (seq.stride(0), seq.stride(1), seq.stride(2), seq.stride(3))
    if seq.dim() == nd + 3 and tuple(seq.shape[2:2 + nd]) == (patch,) * nd:  # [B, L, p, .., p, C]
        st = seq.stride()
        se = st[1 + nd]
        if all(st[2 + k] == se * patch ** (nd - 1 - k) for k in range(nd)):
            return seq.shape[-1], seq.shape[1], (st[0], st[-1], st[1], se)
        raise RuntimeError(f"{name}: the patch axes of seq must be regularly strided (p * stride of the next axis)")
    raise TypeError(f"{name}: seq must be [B, C, L, {P}] or [B, L, {', '.join(['p'] * nd)}, C] with p = {patch}")


def _deserialize(name, nd, seq, nodes, count, size, patch, mode, truncate, channels_last):
    L = _l.load()
    if not seq.is_cuda:
        raise RuntimeError(f"{name}.seq: expected a tensor on the MI355X (cuda) device, got {seq.device}")
    _chk(nodes, f"{name}.nodes"), _chk(count, f"{name}.count")
    if seq.dtype != torch.float32 or nodes.dtype != torch.int32 or nodes.dim() != 3 or nodes.shape[2] != 2 * nd or \
            count.dtype != torch.int32 or count.dim() != 1:
        raise TypeError(f"{name}: seq fp32, nodes int32 [B, L, {2 * nd}], count int32 [B]")
    smooth = "bicubic" if nd == 2 else "trilinear"
    if mode not in (smooth, "nearest"):
        raise ValueError(f"{name}: mode must be '{smooth}' or 'nearest', got {mode!r}")
    patch = int(patch)
    if patch < 1:
        raise ValueError(f"{name}: need patch >= 1")
    C, S, strides = _seq_strides(name, nd, seq, patch)
    B = seq.shape[0]
    if nodes.shape[0] != B or nodes.shape[1] != S or count.shape[0] != B:
        raise ValueError(f"{name}: seq, nodes and count disagree on batch size or sequence length")
    if min(strides[1:]) <= 0 or (B > 1 and strides[0] <= 0):
        raise RuntimeError(f"{name}: seq must not be an expanded (zero-stride) view")
    size = (int(size),) * nd if isinstance(size, int) else tuple(int(v) for v in size)
    if len(size) != nd or (nd == 3 and len(set(size)) != 1):
        raise ValueError(f"{name}: size must be (H, W)" if nd == 2 else f"{name}: size must be one side N or (N, N, N)")
    npix = math.prod(size)
    out = torch.empty((B, *size, C) if channels_last else (B, C, *size), dtype=torch.float32, device=seq.device)
    ostr = (npix * C, 1, C) if channels_last else (npix * C, npix, 1)
    m = _l.RESAMPLE_NEAREST if mode == "nearest" else _l.RESAMPLE_SMOOTH
    if nd == 2:
        _l.check(L.ucfvit_quadtree_deserialize(seq.data_ptr(), nodes.data_ptr(), count.data_ptr(), out.data_ptr(), B, size[0], size[1], C, S, patch,
                                               *strides, *ostr, m, int(bool(truncate)), _stream()), "ucfvit_quadtree_deserialize")
    else:
        if truncate:
            raise ValueError(f"{name}: the 3-D rule has no truncation")
        _l.check(L.ucfvit_octree_deserialize(seq.data_ptr(), nodes.data_ptr(), count.data_ptr(), out.data_ptr(), B, size[0], C, S, patch, *strides,
                                             *ostr, m, _stream()), "ucfvit_octree_deserialize")
    return out


def quadtree_deserialize(seq, nodes, count, size, patch, mode="bicubic", truncate=False, channels_last=True):
    """seq fp32, read in place: the patch list [B, L, p, p, C] or the model layout [B, C, L, p * p] (SAP logits per class); nodes / count from
    quadtree_build; size = (H, W) -> the image fp32 [B, H, W, C] (channels_last) or [B, C, H, W]: every leaf region is its patch resized to the
    leaf (ucfvit_quadtree_deserialize: 'bicubic', optionally after truncation of the tokens, or 'nearest'); pixels no leaf covers are 0"""
    return _deserialize("quadtree_deserialize", 2, seq, nodes, count, size, patch, mode, truncate, channels_last)


def octree_deserialize(seq, nodes, count, size, patch, mode="trilinear", channels_last=True):
    """seq fp32 [B, L, p, p, p, C] or [B, C, L, p^3], nodes / count from octree_build, size = N -> fp32 [B, N, N, N, C] or [B, C, N, N, N]
    (ucfvit_octree_deserialize: aligned-corner 'trilinear' or 'nearest')"""
    return _deserialize("octree_deserialize", 3, seq, nodes, count, size, patch, mode, False, channels_last)


def _deserialize_bwd(name, nd, dout, nodes, count, seq_like_or_shape, patch, mode, channels_last):
    L = _l.load()
    if not isinstance(dout, torch.Tensor) or not dout.is_cuda:
        raise RuntimeError(f"{name}.dout: expected a tensor on the MI355X (cuda) device, got {getattr(dout, 'device', type(dout))}")
    _chk(nodes, f"{name}.nodes"), _chk(count, f"{name}.count")
    if dout.dtype != torch.float32 or dout.dim() != nd + 2 or nodes.dtype != torch.int32 or nodes.dim() != 3 or nodes.shape[2] != 2 * nd or \
            count.dtype != torch.int32 or count.dim() != 1:
        raise TypeError(f"{name}: dout fp32 [B, {'H, W' if nd == 2 else 'N, N, N'}, C] or [B, C, ..], nodes int32 [B, L, {2 * nd}], count int32 [B]")
    smooth = "bicubic" if nd == 2 else "trilinear"
    if mode not in (smooth, "nearest"):
        raise ValueError(f"{name}: mode must be '{smooth}' or 'nearest', got {mode!r}")
    patch = int(patch)
    if patch < 1:
        raise ValueError(f"{name}: need patch >= 1")
    if isinstance(seq_like_or_shape, torch.Tensor):
        like = seq_like_or_shape
        if like.dtype != torch.float32:
            raise TypeError(f"{name}: the sequence the gradient is shaped like must be fp32, got {like.dtype}")
        dseq = torch.empty_like(like, device=dout.device)               # the strides of a dense seq, contiguous otherwise
    else:
        dseq = torch.empty(tuple(int(v) for v in seq_like_or_shape), dtype=torch.float32, device=dout.device)
    C, S, strides = _seq_strides(name, nd, dseq, patch)
    B = dseq.shape[0]
    size = tuple(dout.shape[1:1 + nd]) if channels_last else tuple(dout.shape[2:])
    if nd == 3 and len(set(size)) != 1:
        raise ValueError(f"{name}: dout must hold cubic volumes, got {size}")
    if dout.shape[0] != B or (dout.shape[-1] if channels_last else dout.shape[1]) != C or nodes.shape[0] != B or nodes.shape[1] != S or \
            count.shape[0] != B:
        raise ValueError(f"{name}: dout, the sequence shape, nodes and count disagree on batch size, channels or sequence length")
    if not dout.is_contiguous():
        raise RuntimeError(f"{name}: dout must be dense ({'[B, .., C]' if channels_last else '[B, C, ..]'} contiguous)")
    if min(strides[1:]) <= 0 or (B > 1 and strides[0] <= 0):
        raise RuntimeError(f"{name}: the gradient cannot be written into an expanded (zero-stride) view")
    npix = math.prod(size)
    ostr = (npix * C, 1, C) if channels_last else (npix * C, npix, 1)
    m = _l.RESAMPLE_NEAREST if mode == "nearest" else _l.RESAMPLE_SMOOTH
    dims = (size[0], size[1]) if nd == 2 else (size[0],)
    query = L.ucfvit_quadtree_deserialize_bwd_workspace if nd == 2 else L.ucfvit_octree_deserialize_bwd_workspace
    nbytes = query(B, *dims, C, S, patch)
    if nbytes < 0:
        _l.check(-1, query.__name__)
    ws = workspace(nbytes, dout.device) if nbytes else None
    fn = L.ucfvit_quadtree_deserialize_bwd if nd == 2 else L.ucfvit_octree_deserialize_bwd
    _l.check(fn(dout.data_ptr(), nodes.data_ptr(), count.data_ptr(), dseq.data_ptr(), B, *dims, C, S, patch, *strides, *ostr, m, _p(ws), _stream()),
             fn.__name__)
    return dseq


def quadtree_deserialize_bwd(dout, nodes, count, seq_like_or_shape, patch, mode="bicubic", channels_last=True):
    """the adjoint of quadtree_deserialize: dout fp32 dense [B, H, W, C] (channels_last) or [B, C, H, W] -> dseq fp32 with the shape and strides
    of the forward's seq (a tensor to be shaped like, or a shape: [B, L, p, p, C] or [B, C, L, p * p]); dseq[c, k] = sum over the leaf's pixels of
    w(x, k) dout[c, x] with the forward's weights; every row is written, padding rows and empty leaves with 0; deterministic
    (ucfvit_quadtree_deserialize_bwd).  Truncation has no gradient."""
    return _deserialize_bwd("quadtree_deserialize_bwd", 2, dout, nodes, count, seq_like_or_shape, patch, mode, channels_last)


def octree_deserialize_bwd(dout, nodes, count, seq_like_or_shape, patch, mode="trilinear", channels_last=True):
    """the adjoint of octree_deserialize: dout fp32 dense [B, N, N, N, C] or [B, C, N, N, N] -> dseq fp32 [B, L, p, p, p, C] or [B, C, L, p^3]
    (ucfvit_octree_deserialize_bwd)"""
    return _deserialize_bwd("octree_deserialize_bwd", 3, dout, nodes, count, seq_like_or_shape, patch, mode, channels_last)


def cross_entropy(logits, labels, grad_scale=1.0, want_grad=True):
    """returns (loss fp32 scalar tensor, dlogits or None, row_loss)"""
    L = _l.load()
    _chk(logits, "cross_entropy.logits"), _chk(labels, "cross_entropy.labels")
    if labels.dtype != torch.int64:
        raise TypeError("cross_entropy: labels must be int64")
    B, C = logits.shape
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    rows = torch.empty(B, dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if want_grad else None
    _l.check(L.ucfvit_cross_entropy(logits.data_ptr(), labels.data_ptr(), loss.data_ptr(), rows.data_ptr(), _p(dl), B, C, grad_scale,
                                    dt(logits), _stream()), "ucfvit_cross_entropy")
    return loss, dl, rows


# ------------------------------------------------------------------------------------------------ UNETR decoder (HBM-bound part)
def _rows_view(x):
    """N C (D) H W tensor -> (rows = N*C, S = voxels per row); contiguous"""
    _chk(x, "instnorm.x")
    if x.dim() < 3:
        raise ValueError("instnorm: expected [N, C, *spatial]")
    rows = x.shape[0] * x.shape[1]
    S = x.numel() // max(rows, 1)
    V = 16 // x.element_size()
    if S % V:
        raise ValueError(f"instnorm: the spatial size {S} must be a multiple of {V} elements (16-byte rows); there is no slow path")
    return rows, S


def instnorm_fwd(x, res=None, eps=1e-5, slope=0.01):
    """y = leaky_relu(instance_norm(x) [+ res], slope) over every (n, c) row (slope 1.0: no activation) -> (y, mean, rstd)"""
    L = _l.load()
    rows, S = _rows_view(x)
    if res is not None:
        _chk(res, "instnorm.res")
        if res.shape != x.shape or res.dtype != x.dtype:
            raise ValueError("instnorm: res must have the shape and dtype of x")
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    ws = workspace(L.ucfvit_instnorm_workspace(rows, S), x.device)
    _l.check(L.ucfvit_instnorm_fwd(x.data_ptr(), _p(res), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, S, eps, slope, ws.data_ptr(), dt(x),
                                   _stream()), "ucfvit_instnorm_fwd")
    return y, mean, rstd


def instnorm_bwd(dy, y, x, mean, rstd, slope, want_dres):
    L = _l.load()
    rows, S = _rows_view(x)
    _chk(dy, "instnorm_bwd.dy")
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    ws = workspace(L.ucfvit_instnorm_workspace(rows, S), x.device)
    _l.check(L.ucfvit_instnorm_bwd(dy.data_ptr(), y.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), _p(dres), rows, S,
                                   slope, ws.data_ptr(), dt(x), _stream()), "ucfvit_instnorm_bwd")
    return dx, dres


def dice_strides(logits):
    """(stride_b, stride_c, stride_s) of logits [B, n, *spatial] that are contiguous (N C (D) H W) or a channels-last view with contiguous
    voxel rows (over a [B, *spatial, ld >= n] buffer); None for any other layout"""
    B, n = logits.shape[0], logits.shape[1]
    S = logits.numel() // (B * n)
    if logits.is_contiguous():
        return n * S, S, 1
    cl = logits.movedim(1, -1)                           # [B, *spatial, n]
    ld = cl.stride(-2)
    ok = cl.stride(-1) == 1 and ld >= n and cl.stride(0) == S * ld
    exp = ld
    for d in range(cl.dim() - 2, 0, -1):
        ok = ok and cl.stride(d) == exp
        exp *= cl.shape[d]
    return (S * ld, 1, ld) if ok else None


def _dice_labels(logits, labels, name):
    _chk(labels, f"{name}.labels")
    if not logits.is_cuda:
        _chk(logits, f"{name}.logits")
    if labels.dtype != torch.int64:
        raise TypeError(f"{name}: labels must be int64")
    if labels.numel() * logits.shape[1] != logits.numel():
        raise ValueError(f"{name}: labels must hold one class index per voxel")


def _dice_layout(logits):
    """-> (B, n, S, (stride_b, stride_c, stride_s))"""
    strides = dice_strides(logits)
    if strides is None:
        raise RuntimeError("dice_ce: logits must be contiguous or a channels-last view with contiguous voxel rows")
    B, n = logits.shape[0], logits.shape[1]
    return B, n, logits.numel() // (B * n), strides


def _dice_grad(logits, strides):
    """dlogits with the strides of logits: N C (D) H W, or the padded channels-last buffer behind a view (padding columns zero)"""
    if logits.is_contiguous():
        return torch.empty_like(logits)
    sb, _, ld = strides
    mk = torch.empty if ld == logits.shape[1] else torch.zeros
    return mk(logits.shape[0] * sb, dtype=logits.dtype, device=logits.device).as_strided(logits.shape, logits.stride())


def dice_ce(logits, labels, smooth_nr=1e-5, smooth_dr=1e-5, grad_scale=1.0, want_grad=True):
    """logits [B, n, *spatial] (2 <= n <= 8), labels int64 [B, *spatial] (or [B, 1, *spatial]) -> (loss fp32 scalar, dlogits or None).
    logits may be contiguous (N C D H W) or a channels-last view of a [B, *spatial, ld >= n] buffer (what the HIP decoder returns)."""
    L = _l.load()
    _dice_labels(logits, labels, "dice_ce")
    B, n, S, (sb, sc, ss) = _dice_layout(logits)
    dl = _dice_grad(logits, (sb, sc, ss)) if want_grad else None
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    ws = workspace(L.ucfvit_dice_ce_workspace(B, S), logits.device)
    _l.check(L.ucfvit_dice_ce(logits.data_ptr(), labels.data_ptr(), loss.data_ptr(), _p(dl), B, n, S, sb, sc, ss, smooth_nr, smooth_dr, grad_scale,
                              ws.data_ptr(), dt(logits), _stream()), "ucfvit_dice_ce")
    return loss, dl


def dice_ce_stats(logits, labels):
    """this rank's per-(batch, class) sums of the Dice + CE loss over its slab of a sharded volume: fp32 [B, ucfvit_dice_ce_stats_floats()]
    (to be summed over the group and handed to dice_ce_from_stats)"""
    L = _l.load()
    _dice_labels(logits, labels, "dice_ce_stats")
    B, n, S, (sb, sc, ss) = _dice_layout(logits)
    stats = torch.empty((B, L.ucfvit_dice_ce_stats_floats()), dtype=torch.float32, device=logits.device)
    ws = workspace(L.ucfvit_dice_ce_workspace(B, S), logits.device)
    _l.check(L.ucfvit_dice_ce_stats(logits.data_ptr(), labels.data_ptr(), stats.data_ptr(), B, n, S, sb, sc, ss, ws.data_ptr(), dt(logits), _stream()),
             "ucfvit_dice_ce_stats")
    return stats


def dice_ce_from_stats(logits, labels, stats, S_total, smooth_nr=1e-5, smooth_dr=1e-5, grad_scale=1.0, want_grad=True):
    """stats: the per-(batch, class) sums of the WHOLE volume (dice_ce_stats summed over the group) -> (loss of the whole volume, gradient of the
    LOCAL logits or None).  S_total: voxels of the whole volume per batch element."""
    L = _l.load()
    B, n, S, (sb, sc, ss) = _dice_layout(logits)
    dl = _dice_grad(logits, (sb, sc, ss)) if want_grad else None
    stats = stats.clone()                                # rewritten in place by the fold
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    _l.check(L.ucfvit_dice_ce_from_stats(logits.data_ptr(), labels.data_ptr(), stats.data_ptr(), loss.data_ptr(), _p(dl), B, n, S, int(S_total), sb, sc, ss,
                                         smooth_nr, smooth_dr, grad_scale, dt(logits), _stream()), "ucfvit_dice_ce_from_stats")
    return loss, dl


def _seg_args(logits, labels):
    """the operands of ucfvit_seg_counts: logits read in place where dice_strides knows their layout (at storage offset 0, as DiceCEFn.forward
    takes them), else a dense copy; labels [B, *spatial] or [B, 1, *spatial] -> (logits, labels, B, n, S, strides)"""
    if logits.dim() < 3:
        raise ValueError("seg_counts: logits must be [B, n, *spatial]")
    if not (logits.is_contiguous() or (logits.storage_offset() == 0 and dice_strides(logits) is not None)):
        logits = logits.contiguous()
    if labels.dim() == logits.dim() and labels.shape[1] == 1:
        labels = labels.view(labels.shape[0], *labels.shape[2:])
    if tuple(labels.shape) != (logits.shape[0], *logits.shape[2:]):
        raise ValueError("seg_counts: labels must be [B, *spatial] or [B, 1, *spatial] of the logits' volume")
    if not labels.is_contiguous():
        labels = labels.contiguous()
    _dice_labels(logits, labels, "seg_counts")
    B, n, S, strides = _dice_layout(logits)
    return logits, labels, B, n, S, strides


def seg_counts(logits, labels, want_pred=True):
    """logits [B, n, *spatial] fp32 or bf16 (2 <= n <= 8), labels int64 [B, *spatial] or [B, 1, *spatial] ->
    (pred uint8 [B, *spatial] = torch.argmax(logits, 1), or None; counts int64 [B, 3, n] = (TP, PRED, LAB) per batch element and class).
    One pass (ucfvit_seg_counts); the HIP decoder's padded channels-last view is read in place.  A label outside [0, n) is in no LAB / TP count."""
    L = _l.load()
    logits, labels, B, n, S, (sb, sc, ss) = _seg_args(logits, labels)
    pred = torch.empty((B, *logits.shape[2:]), dtype=torch.uint8, device=logits.device) if want_pred else None
    counts = torch.empty((B, 3, 8), dtype=torch.int64, device=logits.device)
    ws = workspace(L.ucfvit_seg_counts_workspace(B, S), logits.device)
    _l.check(L.ucfvit_seg_counts(logits.data_ptr(), labels.data_ptr(), _p(pred), counts.data_ptr(), B, n, S, sb, sc, ss, ws.data_ptr(), dt(logits),
                                 _stream()), "ucfvit_seg_counts")
    return pred, counts[:, :, :n]


def seg_counts_route(logits, labels, want_pred=True):
    """the name of the kernel seg_counts takes for these operands (ucfvit_seg_counts_route); the prediction buffer is taken as torch allocates it"""
    import ctypes
    L = _l.load()
    logits, labels, B, n, S, (sb, sc, ss) = _seg_args(logits, labels)
    pred = torch.empty((B, *logits.shape[2:]), dtype=torch.uint8, device=logits.device) if want_pred else None
    buf = ctypes.create_string_buffer(96)
    rc = L.ucfvit_seg_counts_route(logits.data_ptr(), labels.data_ptr(), _p(pred), B, n, S, sb, sc, ss, dt(logits), buf, len(buf))
    if rc < 0:
        _l.check(rc, "ucfvit_seg_counts_route")
    return buf.value.decode()


# ------------------------------------------------------------------------------------------------ SAP head and Dice + BCE
def _sap_dims(p, s, nd):
    if nd not in (2, 3) or p < 1 or s < 1:
        raise ValueError(f"sap head: need nd in (2, 3), p >= 1, s >= 1 (got nd={nd}, p={p}, s={s})")
    return p ** nd, s ** nd


def sap_fold(w_neck, w_head, dtype):
    """w_neck fp32 [D, K, *(p,) * nd] (ConvTranspose weight), w_head fp32 [C, K, 1, ..] (1x1 convolution weight) -> W_eff [P C, D] in `dtype`:
    the Linear weight of header(neck(.)), rows ordered (offset in the patch, class)"""
    L = _l.load()
    _chk(w_neck, "sap_fold.w_neck"), _chk(w_head, "sap_fold.w_head")
    if w_neck.dtype != torch.float32 or w_head.dtype != torch.float32:
        raise TypeError("sap_fold: the weights are folded in fp32")
    D, K = w_neck.shape[0], w_neck.shape[1]
    P, C = w_neck.numel() // (D * K), w_head.shape[0]
    if w_head.numel() != C * K:
        raise ValueError(f"sap_fold: w_head {tuple(w_head.shape)} does not take the {K} channels of w_neck {tuple(w_neck.shape)}")
    w_eff = torch.empty((P * C, D), dtype=dtype, device=w_neck.device)
    _l.check(L.ucfvit_sap_fold(w_neck.data_ptr(), w_head.data_ptr(), w_eff.data_ptr(), D, K, P, C, dt(w_eff), _stream()), "ucfvit_sap_fold")
    return w_eff


def sap_unfold(dw_eff, w_neck, w_head):
    """dw_eff fp32 [P C, D] -> (dw_neck fp32 like w_neck, dw_head fp32 like w_head)"""
    L = _l.load()
    _chk(dw_eff, "sap_unfold.dw_eff"), _chk(w_neck, "sap_unfold.w_neck"), _chk(w_head, "sap_unfold.w_head")
    if dw_eff.dtype != torch.float32 or w_neck.dtype != torch.float32 or w_head.dtype != torch.float32:
        raise TypeError("sap_unfold: fp32 operands only")
    D, K = w_neck.shape[0], w_neck.shape[1]
    P, C = w_neck.numel() // (D * K), w_head.shape[0]
    if tuple(dw_eff.shape) != (P * C, D) or w_head.numel() != C * K:
        raise ValueError(f"sap_unfold: dw_eff {tuple(dw_eff.shape)} / w_head {tuple(w_head.shape)} do not fit w_neck {tuple(w_neck.shape)}")
    dw_neck, dw_head = torch.empty_like(w_neck), torch.empty_like(w_head)
    ws = workspace(L.ucfvit_sap_unfold_workspace(D, K, C), dw_eff.device)
    _l.check(L.ucfvit_sap_unfold(dw_eff.data_ptr(), w_neck.data_ptr(), w_head.data_ptr(), dw_neck.data_ptr(), dw_head.data_ptr(), D, K, P, C,
                                 ws.data_ptr(), _stream()), "ucfvit_sap_unfold")
    return dw_neck, dw_head


def sap_scatter_fwd(rows, bias, B, p, s, nd):
    """rows fp32 [B s^nd, p^nd C] (columns ordered (offset in the patch, class)), bias fp32 [C] -> map fp32 [B, C, *(s p,) * nd]"""
    L = _l.load()
    _chk(rows, "sap_scatter_fwd.rows"), _chk(bias, "sap_scatter_fwd.bias")
    P, S = _sap_dims(p, s, nd)
    C = bias.numel()
    if rows.dtype != torch.float32 or bias.dtype != torch.float32:
        raise TypeError("sap_scatter_fwd: rows and bias must be float32")
    if rows.dim() != 2 or tuple(rows.shape) != (B * S, P * C):
        raise ValueError(f"sap_scatter_fwd: rows must be [{B * S}, {P * C}], got {tuple(rows.shape)}")
    out = torch.empty((B, C) + (s * p,) * nd, dtype=torch.float32, device=rows.device)
    _l.check(L.ucfvit_sap_scatter_fwd(rows.data_ptr(), bias.data_ptr(), out.data_ptr(), B, s, p, C, nd, _stream()), "ucfvit_sap_scatter_fwd")
    return out


def sap_scatter_bwd(dmap, p, s, nd, dtype, want_dbias=True):
    """dmap fp32 [B, C, *(s p,) * nd] -> (drows [B s^nd, p^nd C] in `dtype`, dbias fp32 [C] or None)"""
    L = _l.load()
    _chk(dmap, "sap_scatter_bwd.dmap")
    P, S = _sap_dims(p, s, nd)
    if dmap.dtype != torch.float32:
        raise TypeError("sap_scatter_bwd: dmap must be float32")
    if dmap.dim() != nd + 2 or tuple(dmap.shape[2:]) != (s * p,) * nd:
        raise ValueError(f"sap_scatter_bwd: dmap must be [B, C, {', '.join([str(s * p)] * nd)}], got {tuple(dmap.shape)}")
    B, C = dmap.shape[0], dmap.shape[1]
    drows = torch.empty((B * S, P * C), dtype=dtype, device=dmap.device)
    dbias = torch.empty(C, dtype=torch.float32, device=dmap.device) if want_dbias else None
    ws = workspace(L.ucfvit_sap_scatter_bwd_workspace(B, s, p, C, nd), dmap.device) if want_dbias else None
    _l.check(L.ucfvit_sap_scatter_bwd(dmap.data_ptr(), drows.data_ptr(), _p(dbias), B, s, p, C, nd, _p(ws), dt(drows), _stream()),
             "ucfvit_sap_scatter_bwd")
    return drows, dbias


def _dice_bce_layout(logits, targets, name):
    _chk(logits, f"{name}.logits"), _chk(targets, f"{name}.targets")
    if targets.dtype != torch.float32:
        raise TypeError(f"{name}: targets must be float32")
    if logits.dim() < 3 or targets.shape != logits.shape or logits.shape[1] < 2:
        raise ValueError(f"{name}: logits and targets must both be [B, classes >= 2, *spatial], got {tuple(logits.shape)} and {tuple(targets.shape)}")
    B, C = logits.shape[0], logits.shape[1]
    return B, C, logits.numel() // (B * C)


def dice_bce_stats(logits, targets):
    """logits [B, C, *spatial] (fp32 or bf16), targets fp32 of the same shape -> fp32 [4]: sum p t, sum p, sum t, sum BCE over channels 1.."""
    L = _l.load()
    B, C, S = _dice_bce_layout(logits, targets, "dice_bce_stats")
    stats = torch.empty(L.ucfvit_dice_bce_stats_floats(), dtype=torch.float32, device=logits.device)
    ws = workspace(L.ucfvit_dice_bce_workspace(B, C, S), logits.device)
    _l.check(L.ucfvit_dice_bce_stats(logits.data_ptr(), targets.data_ptr(), stats.data_ptr(), B, C, S, ws.data_ptr(), dt(logits), _stream()),
             "ucfvit_dice_bce_stats")
    return stats


def dice_bce_from_stats(logits, targets, stats, weight=0.5, smooth=1.0, grad_scale=1.0, grad_scale_dev=None, want_loss=True, want_grad=True):
    """-> (loss fp32 scalar or None, dlogits fp32 or None); the gradient is scaled by grad_scale and, when given, by the fp32 device
    scalar grad_scale_dev (autograd's upstream gradient, read by the kernel)"""
    L = _l.load()
    B, C, S = _dice_bce_layout(logits, targets, "dice_bce_from_stats")
    _chk(stats, "dice_bce_from_stats.stats")
    if stats.dtype != torch.float32 or stats.numel() != L.ucfvit_dice_bce_stats_floats():
        raise TypeError("dice_bce_from_stats: stats must be the fp32 tensor dice_bce_stats returns")
    if grad_scale_dev is not None:
        _chk(grad_scale_dev, "dice_bce_from_stats.grad_scale_dev")
        if grad_scale_dev.dtype != torch.float32 or grad_scale_dev.numel() != 1:
            raise TypeError("dice_bce_from_stats: grad_scale_dev must be one float32 value")
    loss = torch.empty((), dtype=torch.float32, device=logits.device) if want_loss else None
    dl = torch.empty(logits.shape, dtype=torch.float32, device=logits.device) if want_grad else None
    _l.check(L.ucfvit_dice_bce_from_stats(logits.data_ptr(), targets.data_ptr(), stats.data_ptr(), _p(loss), _p(dl), B, C, S, float(weight),
                                          float(smooth), float(grad_scale), _p(grad_scale_dev), dt(logits), _stream()),
             "ucfvit_dice_bce_from_stats")
    return loss, dl


# ------------------------------------------------------------------------------------------------ UNETR decoder, channels-last bf16
def _chk_cl(t, name, C=None, dims=(4, 5)):
    _chk(t, name)
    if t.dtype != torch.bfloat16 or t.dim() not in dims:
        want = " or ".join("[B, X, Y, C]" if d == 4 else "[B, X, Y, Z, C]" for d in dims)
        raise TypeError(f"{name}: expected a channels-last bf16 tensor {want}, got {tuple(t.shape)} {t.dtype}")
    if C is not None and t.shape[-1] != C:
        raise ValueError(f"{name}: expected {C} channels, got {t.shape[-1]}")
    return t


def conv_packed_numel(cin, cout, ksize):
    cpc = min(cin, 32)
    tps = 32 // cpc
    return (cin // cpc) * (-(-(ksize ** 3) // tps)) * cout * 32


def conv3d_fwd(x, w_packed, cout, ksize=3, bias=None, cout_store=None, out_dtype=torch.bfloat16, accumulate_into=None, stats_eps=None, out=None):
    """x [B, X, Y, Z, Cin] bf16, w_packed from conv.pack_conv_weight (cout rows, a multiple of 16) -> y [B, X, Y, Z, cout_store] (ksize 3:
    stride 1, zero padding 1; ksize 1: pointwise).  bias: fp32 [cout] or None.  out: a bf16 channel slice of a wider channels-last buffer
    to write y into (the first half of a concatenation)."""
    L = _l.load()
    _chk_cl(x, "conv3d.x", dims=(5,)), _chk(w_packed, "conv3d.w_packed")
    B, X, Y, Z, cin = x.shape
    if w_packed.dtype != torch.bfloat16 or w_packed.numel() != conv_packed_numel(cin, cout, ksize):
        raise ValueError("conv3d: w_packed does not match (Cin, Cout, ksize)")
    if bias is not None:
        _chk(bias, "conv3d.bias")
        if bias.dtype != torch.float32 or bias.numel() != cout:
            raise ValueError("conv3d: bias must be fp32 [Cout]")
    cs = cout if cout_store is None else cout_store
    ldy = cs
    if out is not None:
        ldy = cl_row_stride(out)
        if ldy is None or tuple(out.shape) != (B, X, Y, Z, cs) or out_dtype != torch.bfloat16 or accumulate_into is not None:
            raise ValueError("conv3d: out must be a bf16 [B, X, Y, Z, cout_store] map, dense or a channel slice of a channels-last buffer")
        y = out
    elif accumulate_into is not None:                          # y += result: the second data gradient of an input two layers consume
        y = _chk(accumulate_into, "conv3d.accumulate_into")
        if tuple(y.shape) != (B, X, Y, Z, cs) or y.dtype != out_dtype:
            raise ValueError("conv3d: accumulate_into must have the output's shape and dtype")
    else:
        y = torch.empty((B, X, Y, Z, cs), dtype=out_dtype, device=x.device)
    part, rows = None, 0
    if stats_eps is not None:
        # instance-norm statistics of the output as a by-product of the epilogue where the serving kernel has one, else one pass over y
        if accumulate_into is not None or out is not None or cs != cout or out_dtype != torch.bfloat16:
            raise ValueError("conv3d: statistics need a dense bf16 output without accumulation")
        rows = L.ucfvit_conv3d_fwd_stats_rows(B, X, Y, Z, cin, cout, ksize, 0 if bias is None else 1)
        if rows:
            buf = workspace((B * rows * 3 * cout + B * 256 * 3 * cout) * 4, x.device)       # partial rows (count, mean, M2), then the first fold stage's scratch
            part, fold_ws = buf, buf[B * rows * 3 * cout:]
    _l.check(L.ucfvit_conv3d_fwd(x.data_ptr(), w_packed.data_ptr(), _p(bias), y.data_ptr(), B, X, Y, Z, cin, cout, ksize, ldy, cs, dt(y),
                                 0 if accumulate_into is None else 1, _p(part), _stream()), "ucfvit_conv3d_fwd")
    if stats_eps is None:
        return y
    if not rows:
        return (y,) + instnorm_cl_stats(y, stats_eps)
    mean = torch.empty((B, cout), dtype=torch.float32, device=x.device)
    rstd = torch.empty((B, cout), dtype=torch.float32, device=x.device)
    _l.check(L.ucfvit_instnorm_cl_stats_fold(part.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, X * Y * Z, cout, rows, stats_eps, fold_ws.data_ptr(),
                                             _stream()), "ucfvit_instnorm_cl_stats_fold")
    return y, mean, rstd


def conv3d_wgrad(x, dy, ksize=3):
    """-> packed fp32 weight gradient (conv.unpack_conv_wgrad turns it into [Cout, Cin, k, k, k])"""
    L = _l.load()
    _chk_cl(x, "conv3d_wgrad.x", dims=(5,)), _chk_cl(dy, "conv3d_wgrad.dy", dims=(5,))
    B, X, Y, Z, cin = x.shape
    cout = dy.shape[-1]
    if dy.shape[:4] != x.shape[:4]:
        raise ValueError("conv3d_wgrad: x and dy must cover the same voxels")
    n = L.ucfvit_conv3d_wgrad_size(cin, cout, ksize)
    nbytes = L.ucfvit_conv3d_wgrad_workspace(B, X, Y, Z, cin, cout, ksize)
    if n <= 0 or nbytes <= 0:
        raise ValueError(f"conv3d_wgrad: unsupported channel counts Cin={cin} Cout={cout}")
    dw = torch.empty(n, dtype=torch.float32, device=x.device)
    ws = workspace(nbytes, x.device)
    _l.check(L.ucfvit_conv3d_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), B, X, Y, Z, cin, cout, ksize, _stream()),
             "ucfvit_conv3d_wgrad")
    return dw


def cl_row_stride(t):
    """voxel-row stride (elements) of a channels-last bf16 tensor [B, X, Y, Z, C] (or [B, X, Y, C]) that is dense or a channel slice of a
    dense [B, X, Y, Z, ld] buffer (what torch.cat's backward and a pre-allocated concatenation hand around); None if it is neither"""
    if t.dim() not in (4, 5) or t.dtype != torch.bfloat16 or not t.is_cuda or t.stride(-1) != 1:
        return None
    ld = t.stride(-2)
    if ld < t.shape[-1] or ld % 8 or t.data_ptr() % 16:
        return None
    exp = ld
    for d in range(t.dim() - 2, 0, -1):
        if t.stride(d) != exp and t.shape[d] != 1:
            return None
        exp *= t.shape[d]
    if t.stride(0) != exp and t.shape[0] != 1:
        return None
    return ld


def depth_to_space2(cols, B, Xi, Yi, Zi, C, out=None, skip=None):
    """cols [B Xi Yi Zi, 8 C] (column blocks (dx, dy, dz)) -> [B, 2Xi, 2Yi, 2Zi, C]; `out` may be a channel slice of a wider channels-last
    buffer; with `skip` (dense [B, 2Xi, 2Yi, 2Zi, Cs]) the buffer behind `out` must be C + Cs wide and receives the skip behind the C channels"""
    L = _l.load()
    _chk(cols, "depth_to_space2.cols")
    if cols.dtype != torch.bfloat16 or cols.numel() != B * Xi * Yi * Zi * 8 * C:
        raise ValueError("depth_to_space2: bad operand")
    if out is None:
        out = torch.empty((B, 2 * Xi, 2 * Yi, 2 * Zi, C), dtype=torch.bfloat16, device=cols.device)
    ld = cl_row_stride(out)
    if ld is None or tuple(out.shape) != (B, 2 * Xi, 2 * Yi, 2 * Zi, C):
        raise ValueError("depth_to_space2: out must be [B, 2Xi, 2Yi, 2Zi, C], dense or a channel slice of a dense channels-last buffer")
    cs = 0
    if skip is not None:
        _chk_cl(skip, "depth_to_space2.skip", dims=(5,))
        cs = skip.shape[-1]
        if tuple(skip.shape[:4]) != tuple(out.shape[:4]) or ld < C + cs:
            raise ValueError("depth_to_space2: skip must cover the output's voxels and fit behind it in the buffer")
    _l.check(L.ucfvit_depth_to_space2(cols.data_ptr(), out.data_ptr(), B, Xi, Yi, Zi, C, ld, 1, _p(skip), cs, _stream()), "ucfvit_depth_to_space2")
    return out


def space_to_depth2(y):
    """[B, 2Xi, 2Yi, 2Zi, C] (dense or a channel slice of a dense channels-last buffer) -> [B Xi Yi Zi, 8 C]"""
    L = _l.load()
    ld = cl_row_stride(y)
    if ld is None:
        y = _chk_cl(y.contiguous(), "space_to_depth2.y", dims=(5,))
        ld = y.shape[-1]
    if y.dim() != 5:
        raise TypeError("space_to_depth2: expected [B, 2Xi, 2Yi, 2Zi, C]")
    B, X2, Y2, Z2, C = y.shape
    if X2 % 2 or Y2 % 2 or Z2 % 2:
        raise ValueError("space_to_depth2: extents must be even")
    Xi, Yi, Zi = X2 // 2, Y2 // 2, Z2 // 2
    cols = torch.empty((B * Xi * Yi * Zi, 8 * C), dtype=torch.bfloat16, device=y.device)
    _l.check(L.ucfvit_depth_to_space2(y.data_ptr(), cols.data_ptr(), B, Xi, Yi, Zi, C, ld, 0, None, 0, _stream()), "ucfvit_depth_to_space2")
    return cols


# ---- the plane: 3x3 convolution, its weight gradient and the 2x2 transposed convolution's shuffle (csrc/conv2d.hip) ----
def conv2d_packed_numel(cin, cout):
    cpc = min(cin, 32)
    tps = 32 // cpc
    return (cin // cpc) * (-(-9 // tps)) * cout * 32


def conv2d_fwd(x, w_packed, cout, bias=None, cout_store=None, out_dtype=torch.bfloat16, accumulate_into=None, out=None):
    """x [B, X, Y, Cin] bf16, w_packed from conv.pack_conv2d_weight (cout rows, a multiple of 16) -> y [B, X, Y, cout_store]: 3x3, stride 1,
    zero padding 1.  bias: fp32 [cout] or None.  out: a bf16 channel slice of a wider channels-last buffer to write y into."""
    L = _l.load()
    _chk_cl(x, "conv2d.x", dims=(4,)), _chk(w_packed, "conv2d.w_packed")
    B, X, Y, cin = x.shape
    if w_packed.dtype != torch.bfloat16 or w_packed.numel() != conv2d_packed_numel(cin, cout):
        raise ValueError("conv2d: w_packed does not match (Cin, Cout)")
    if bias is not None:
        _chk(bias, "conv2d.bias")
        if bias.dtype != torch.float32 or bias.numel() != cout:
            raise ValueError("conv2d: bias must be fp32 [Cout]")
    cs = cout if cout_store is None else cout_store
    ldy = cs
    if out is not None:
        ldy = cl_row_stride(out)
        if ldy is None or tuple(out.shape) != (B, X, Y, cs) or out_dtype != torch.bfloat16 or accumulate_into is not None:
            raise ValueError("conv2d: out must be a bf16 [B, X, Y, cout_store] map, dense or a channel slice of a channels-last buffer")
        y = out
    elif accumulate_into is not None:                          # y += result: the second data gradient of an input two layers consume
        y = _chk(accumulate_into, "conv2d.accumulate_into")
        if tuple(y.shape) != (B, X, Y, cs) or y.dtype != out_dtype:
            raise ValueError("conv2d: accumulate_into must have the output's shape and dtype")
    else:
        y = torch.empty((B, X, Y, cs), dtype=out_dtype, device=x.device)
    _l.check(L.ucfvit_conv2d_fwd(x.data_ptr(), w_packed.data_ptr(), _p(bias), y.data_ptr(), B, X, Y, cin, cout, ldy, cs, dt(y),
                                 0 if accumulate_into is None else 1, _stream()), "ucfvit_conv2d_fwd")
    return y


def conv2d_wgrad(x, dy):
    """-> packed fp32 weight gradient (conv.unpack_conv2d_wgrad turns it into [Cout, Cin, 3, 3])"""
    L = _l.load()
    _chk_cl(x, "conv2d_wgrad.x", dims=(4,)), _chk_cl(dy, "conv2d_wgrad.dy", dims=(4,))
    B, X, Y, cin = x.shape
    cout = dy.shape[-1]
    if dy.shape[:3] != x.shape[:3]:
        raise ValueError("conv2d_wgrad: x and dy must cover the same pixels")
    n = L.ucfvit_conv2d_wgrad_size(cin, cout)
    nbytes = L.ucfvit_conv2d_wgrad_workspace(B, X, Y, cin, cout)
    if n <= 0 or nbytes <= 0:
        raise ValueError(f"conv2d_wgrad: unsupported channel counts Cin={cin} Cout={cout}")
    dw = torch.empty(n, dtype=torch.float32, device=x.device)
    ws = workspace(nbytes, x.device)
    _l.check(L.ucfvit_conv2d_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), B, X, Y, cin, cout, _stream()), "ucfvit_conv2d_wgrad")
    return dw


def depth_to_space2_2d(cols, B, Xi, Yi, C, out=None, skip=None):
    """cols [B Xi Yi, 4 C] (column blocks (dx, dy)) -> [B, 2Xi, 2Yi, C]; `out` may be a channel slice of a wider channels-last buffer; with
    `skip` (dense [B, 2Xi, 2Yi, Cs]) the buffer behind `out` must be C + Cs wide and receives the skip behind the C channels"""
    L = _l.load()
    _chk(cols, "depth_to_space2_2d.cols")
    if cols.dtype != torch.bfloat16 or cols.numel() != B * Xi * Yi * 4 * C:
        raise ValueError("depth_to_space2_2d: bad operand")
    if out is None:
        out = torch.empty((B, 2 * Xi, 2 * Yi, C), dtype=torch.bfloat16, device=cols.device)
    ld = cl_row_stride(out)
    if ld is None or tuple(out.shape) != (B, 2 * Xi, 2 * Yi, C):
        raise ValueError("depth_to_space2_2d: out must be [B, 2Xi, 2Yi, C], dense or a channel slice of a dense channels-last buffer")
    cs = 0
    if skip is not None:
        _chk_cl(skip, "depth_to_space2_2d.skip", dims=(4,))
        cs = skip.shape[-1]
        if tuple(skip.shape[:3]) != tuple(out.shape[:3]) or ld < C + cs:
            raise ValueError("depth_to_space2_2d: skip must cover the output's pixels and fit behind it in the buffer")
    _l.check(L.ucfvit_depth_to_space2_2d(cols.data_ptr(), out.data_ptr(), B, Xi, Yi, C, ld, 1, _p(skip), cs, _stream()), "ucfvit_depth_to_space2_2d")
    return out


def space_to_depth2_2d(y):
    """[B, 2Xi, 2Yi, C] (dense or a channel slice of a dense channels-last buffer) -> [B Xi Yi, 4 C]"""
    L = _l.load()
    ld = cl_row_stride(y)
    if ld is None:
        y = _chk_cl(y.contiguous(), "space_to_depth2_2d.y", dims=(4,))
        ld = y.shape[-1]
    if y.dim() != 4:
        raise TypeError("space_to_depth2_2d: expected [B, 2Xi, 2Yi, C]")
    B, X2, Y2, C = y.shape
    if X2 % 2 or Y2 % 2:
        raise ValueError("space_to_depth2_2d: extents must be even")
    Xi, Yi = X2 // 2, Y2 // 2
    cols = torch.empty((B * Xi * Yi, 4 * C), dtype=torch.bfloat16, device=y.device)
    _l.check(L.ucfvit_depth_to_space2_2d(y.data_ptr(), cols.data_ptr(), B, Xi, Yi, C, ld, 0, None, 0, _stream()), "ucfvit_depth_to_space2_2d")
    return cols


def resample_trilinear(x, size, out=None, skip=None):
    """align-corners trilinear resampling (nn.Upsample(size, mode='trilinear', align_corners=True)) of a dense channels-last bf16 map
    x [B, Xi, Yi, Zi, C] (C % 8 == 0) -> [B, *size, C]; `out` may be a channel slice of a wider channels-last buffer; with `skip` (dense
    [B, *size, Cs]) the buffer behind `out` must be C + Cs wide and receives the skip behind the C channels"""
    L = _l.load()
    _chk_cl(x, "resample_trilinear.x", dims=(5,))
    B, Xi, Yi, Zi, C = x.shape
    Xo, Yo, Zo = (int(s) for s in size)
    if C % 8:
        raise ValueError(f"resample_trilinear: C must be a multiple of 8, got {C}")
    if out is None:
        out = torch.empty((B, Xo, Yo, Zo, C), dtype=torch.bfloat16, device=x.device)
    ld = cl_row_stride(out)
    if ld is None or tuple(out.shape) != (B, Xo, Yo, Zo, C):
        raise ValueError("resample_trilinear: out must be [B, *size, C], dense or a channel slice of a dense channels-last buffer")
    cs = 0
    if skip is not None:
        _chk_cl(skip, "resample_trilinear.skip")
        cs = skip.shape[-1]
        if tuple(skip.shape[:4]) != tuple(out.shape[:4]) or ld < C + cs:
            raise ValueError("resample_trilinear: skip must cover the output's voxels and fit behind it in the buffer")
    _l.check(L.ucfvit_resample_trilinear_fwd(x.data_ptr(), out.data_ptr(), B, Xi, Yi, Zi, Xo, Yo, Zo, C, ld, _p(skip), cs, _stream()),
             "ucfvit_resample_trilinear_fwd")
    return out


def resample_trilinear_bwd(dy, in_size):
    """gradient of resample_trilinear: dy [B, Xo, Yo, Zo, C] (dense or a channel slice of a dense channels-last buffer) -> dense
    dx [B, *in_size, C]"""
    L = _l.load()
    ld = cl_row_stride(dy)
    if ld is None:
        dy = _chk_cl(dy.contiguous(), "resample_trilinear_bwd.dy", dims=(5,))
        ld = dy.shape[-1]
    if dy.dim() != 5:
        raise TypeError("resample_trilinear_bwd: expected [B, Xo, Yo, Zo, C]")
    B, Xo, Yo, Zo, C = dy.shape
    Xi, Yi, Zi = (int(s) for s in in_size)
    dx = torch.empty((B, Xi, Yi, Zi, C), dtype=torch.bfloat16, device=dy.device)
    _l.check(L.ucfvit_resample_trilinear_bwd(dy.data_ptr(), dx.data_ptr(), B, Xi, Yi, Zi, Xo, Yo, Zo, C, ld, _stream()),
             "ucfvit_resample_trilinear_bwd")
    return dx


def pad_channels8(vol):
    """fp32 [B, C, X, Y, Z] (or [B, C, X, Y]) with C <= 8 -> channels-last bf16 [B, X, Y, Z, 8] ([B, X, Y, 8]), channels C..7 zero"""
    L = _l.load()
    _chk(vol, "pad_channels8.vol")
    if vol.dtype != torch.float32 or vol.dim() not in (4, 5) or vol.shape[1] > 8:
        raise TypeError("pad_channels8: expected an fp32 [B, C <= 8, X, Y, Z] volume or [B, C <= 8, X, Y] image")
    B, C = vol.shape[0], vol.shape[1]
    out = torch.empty((B,) + tuple(vol.shape[2:]) + (8,), dtype=torch.bfloat16, device=vol.device)
    _l.check(L.ucfvit_pad_channels8(vol.data_ptr(), out.data_ptr(), B, C, vol.numel() // (B * C), _stream()), "ucfvit_pad_channels8")
    return out


def pad_rows8(t):
    """[..., C <= 8] fp32 or bf16 with contiguous voxel rows (element stride 1 in the last axis, one row stride ld >= C for all the others:
    a dense tensor or a channel slice of a wider channels-last buffer) -> dense bf16 [..., 8], columns C..7 zero"""
    L = _l.load()
    if not t.is_cuda or t.dtype not in (torch.float32, torch.bfloat16) or t.shape[-1] > 8 or t.stride(-1) != 1:
        raise TypeError("pad_rows8: expected a CUDA fp32 / bf16 tensor with at most 8 contiguous channels in the last axis")
    ld = t.stride(-2) if t.dim() > 1 else t.shape[-1]
    exp = ld
    for d in range(t.dim() - 2, -1, -1):
        if t.shape[d] != 1 and t.stride(d) != exp:
            raise ValueError("pad_rows8: the leading axes must form one run of rows with a common stride")
        exp *= t.shape[d]
    V = t.numel() // t.shape[-1]
    out = torch.empty(tuple(t.shape[:-1]) + (8,), dtype=torch.bfloat16, device=t.device)
    _l.check(L.ucfvit_pad_rows8(t.data_ptr(), dt(t), out.data_ptr(), V, t.shape[-1], ld, _stream()), "ucfvit_pad_rows8")
    return out


def _bsc(x):
    """(B, S, C) of a channels-last map [B, *spatial, C]: S voxels per batch element"""
    B, C = x.shape[0], x.shape[-1]
    return B, x.numel() // (B * C), C


def _cl_dy(dy, x, name):
    """-> (dy, its row stride): read in place if it is a dense or channel-sliced map of x's shape (the skip half of a concatenation's
    gradient), else a contiguous copy"""
    ld = cl_row_stride(dy)
    if ld is None or dy.shape != x.shape:
        dy = _chk_cl(dy.contiguous(), name)
        ld = dy.shape[-1]
    return dy, ld


def instnorm_cl_stats(x, eps=1e-5):
    """-> (mean [B, C], rstd [B, C]) of a channels-last bf16 map"""
    L = _l.load()
    _chk_cl(x, "instnorm_cl_stats.x")
    B, S, C = _bsc(x)
    mean = torch.empty((B, C), dtype=torch.float32, device=x.device)
    rstd = torch.empty((B, C), dtype=torch.float32, device=x.device)
    ws = workspace(L.ucfvit_instnorm_cl_workspace(B, S, C), x.device)
    _l.check(L.ucfvit_instnorm_cl_stats(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, S, C, eps, ws.data_ptr(), _stream()), "ucfvit_instnorm_cl_stats")
    return mean, rstd


def instnorm_cl_apply(x, mean, rstd, res=None, slope=0.01):
    """y = lrelu((x - mean) rstd [+ res], slope) with the statistics given"""
    L = _l.load()
    _chk_cl(x, "instnorm_cl_apply.x")
    if res is not None:
        _chk_cl(res, "instnorm_cl_apply.res")
        if res.shape != x.shape:
            raise ValueError("instnorm_cl_apply: res must have the shape of x")
    B, S, C = _bsc(x)
    y = torch.empty_like(x)
    _l.check(L.ucfvit_instnorm_cl_apply(x.data_ptr(), _p(res), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, S, C, slope, _stream()),
             "ucfvit_instnorm_cl_apply")
    return y


def instnorm_cl_apply2(x, mean, rstd, x2, mean2, rstd2, slope):
    """y = lrelu(norm(x) + norm(x2)) with both statistics given"""
    L = _l.load()
    _chk_cl(x, "instnorm_cl_apply2.x"), _chk_cl(x2, "instnorm_cl_apply2.x2")
    if x2.shape != x.shape:
        raise ValueError("instnorm_cl_apply2: the two branches must have one shape")
    B, S, C = _bsc(x)
    y = torch.empty_like(x)
    _l.check(L.ucfvit_instnorm_cl_apply2(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), x2.data_ptr(), mean2.data_ptr(), rstd2.data_ptr(), y.data_ptr(),
                                         B, S, C, slope, _stream()), "ucfvit_instnorm_cl_apply2")
    return y


def instnorm_cl_bwd2(dy, y, x, mean, rstd, x2, mean2, rstd2, slope):
    """backward of instnorm_cl_apply2 -> (dx, dx2); dy may be a channel slice of a wider channels-last gradient"""
    L = _l.load()
    _chk_cl(x, "instnorm_cl_bwd2.x")
    dy, ld = _cl_dy(dy, x, "instnorm_cl_bwd2.dy")
    B, S, C = _bsc(x)
    dx, dx2 = torch.empty_like(x), torch.empty_like(x)
    ws = workspace(L.ucfvit_instnorm_cl_bwd2_workspace(B, S, C), x.device)
    _l.check(L.ucfvit_instnorm_cl_bwd2(dy.data_ptr(), y.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), x2.data_ptr(), mean2.data_ptr(),
                                       rstd2.data_ptr(), dx.data_ptr(), dx2.data_ptr(), B, S, C, ld, slope, ws.data_ptr(), _stream()),
             "ucfvit_instnorm_cl_bwd2")
    return dx, dx2


def instnorm_cl_bwd(dy, y, x, mean, rstd, slope, want_dres, had_res=None):
    """backward of instnorm_cl_apply: instnorm_cl_bwd_sums, m1 / m2 kept in the workspace, then instnorm_cl_bwd_apply; dy may be a channel
    slice of a wider channels-last gradient: read in place"""
    had_res = want_dres if had_res is None else had_res
    m1, m2, dy = instnorm_cl_bwd_sums(dy, y, x, mean, rstd, slope, had_res, in_workspace=True)
    return instnorm_cl_bwd_apply(dy, y, x, mean, rstd, m1, m2, slope, want_dres, had_res)


def instnorm_cl_bwd_sums(dy, y, x, mean, rstd, slope, had_res, in_workspace=False):
    """first half of instnorm_cl_bwd: (m1, m2) [B, C] = the means over the voxels of x (this rank's slab of a sharded volume) of dy' and
    dy' xhat, and dy as instnorm_cl_bwd_apply reads it.  m1 / m2 are fresh, or with in_workspace views of the workspace's last 2 B C floats,
    which the next call on the workspace may overwrite"""
    L = _l.load()
    _chk_cl(x, "instnorm_cl_bwd_sums.x")
    dy, ld = _cl_dy(dy, x, "instnorm_cl_bwd_sums.dy")
    B, S, C = _bsc(x)
    n = L.ucfvit_instnorm_cl_workspace(B, S, C) // 4
    ws = workspace(4 * n, x.device)
    m1, m2 = ws[n - 2 * B * C:n].view(2, B, C) if in_workspace else torch.empty((2, B, C), dtype=torch.float32, device=x.device)
    _l.check(L.ucfvit_instnorm_cl_bwd_sums(dy.data_ptr(), y.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), m1.data_ptr(), m2.data_ptr(),
                                           B, S, C, ld, slope, 1 if had_res else 0, ws.data_ptr(), _stream()), "ucfvit_instnorm_cl_bwd_sums")
    return m1, m2, dy


def instnorm_cl_bwd_apply(dy, y, x, mean, rstd, m1, m2, slope, want_dres, had_res):
    L = _l.load()
    dy, ld = _cl_dy(dy, x, "instnorm_cl_bwd_apply.dy")
    B, S, C = _bsc(x)
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    _l.check(L.ucfvit_instnorm_cl_bwd_apply(dy.data_ptr(), y.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), m1.data_ptr(), m2.data_ptr(),
                                            dx.data_ptr(), _p(dres), B, S, C, ld, slope, 1 if had_res else 0, _stream()), "ucfvit_instnorm_cl_bwd_apply")
    return dx, dres


# ------------------------------------------------------------------------------------------------ MAE
def mae_mask(noise, len_keep):
    L = _l.load()
    _chk(noise, "mae_mask.noise")
    if noise.dtype != torch.float32:
        raise TypeError("mae_mask: noise must be float32")
    B, Lp = noise.shape
    ids_shuffle = torch.empty((B, Lp), dtype=torch.int64, device=noise.device)
    ids_restore = torch.empty((B, Lp), dtype=torch.int64, device=noise.device)
    mask = torch.empty((B, Lp), dtype=torch.float32, device=noise.device)
    _l.check(L.ucfvit_mae_mask(noise.data_ptr(), ids_shuffle.data_ptr(), ids_restore.data_ptr(), mask.data_ptr(), B, Lp, len_keep,
                               _stream()), "ucfvit_mae_mask")
    return ids_shuffle, ids_restore, mask


def gather_rows(src, idx, R, idx_stride):
    """src [B,L,D]; idx int64 with row stride idx_stride; -> [B,R,D]"""
    L = _l.load()
    _chk(src, "gather_rows.src")
    B, Lp, D = src.shape
    out = torch.empty((B, R, D), dtype=src.dtype, device=src.device)
    _l.check(L.ucfvit_gather_rows(src.data_ptr(), idx.data_ptr(), out.data_ptr(), B, Lp, R, D, idx_stride, dt(src), _stream()),
             "ucfvit_gather_rows")
    return out


def scatter_rows(dout, idx, Lp, idx_stride):
    L = _l.load()
    _chk(dout, "scatter_rows.dout")
    B, R, D = dout.shape
    dsrc = torch.empty((B, Lp, D), dtype=dout.dtype, device=dout.device)
    _l.check(L.ucfvit_scatter_rows(dout.data_ptr(), idx.data_ptr(), dsrc.data_ptr(), B, Lp, R, D, idx_stride, dt(dout), _stream()),
             "ucfvit_scatter_rows")
    return dsrc


def unshuffle_fwd(x, mask_token, ids_restore, pos):
    """x [B,R,D], mask_token [D], ids_restore [B,L] int64, pos [L,D] or None -> [B,L,D]"""
    L = _l.load()
    _chk(x, "unshuffle.x")
    B, R, D = x.shape
    Lp = ids_restore.shape[1]
    out = torch.empty((B, Lp, D), dtype=x.dtype, device=x.device)
    _l.check(L.ucfvit_unshuffle_fwd(x.data_ptr(), mask_token.data_ptr(), ids_restore.data_ptr(), _p(pos), out.data_ptr(), B, Lp, R, D,
                                    dt(x), _stream()), "ucfvit_unshuffle_fwd")
    return out


def unshuffle_bwd(dout, ids_restore, R, want_pos, dmask=None, dpos=None, accumulate=False):
    L = _l.load()
    _chk(dout, "unshuffle_bwd.dout")
    B, Lp, D = dout.shape
    dev = dout.device
    dx = torch.empty((B, R, D), dtype=dout.dtype, device=dev)
    if dmask is None:
        dmask = torch.empty(D, dtype=torch.float32, device=dev)
    if want_pos and dpos is None:
        dpos = torch.empty((Lp, D), dtype=torch.float32, device=dev)
    ws = workspace(L.ucfvit_unshuffle_bwd_workspace(B, D), dev)
    _l.check(L.ucfvit_unshuffle_bwd(dout.data_ptr(), ids_restore.data_ptr(), dx.data_ptr(), dmask.data_ptr(), _p(dpos) if want_pos else None,
                                    B, Lp, R, D, 1 if accumulate else 0, ws.data_ptr(), dt(dout), _stream()), "ucfvit_unshuffle_bwd")
    return dx, dmask, dpos


def patch_mse(pred, img, p, mask=None, grad_scale=1.0, want_grad=True):
    """pred [B,L,P]; img fp32 NCHW(D) (p = patch size) or the adaptive token sequence [B,C,S,P] (p = None); mask fp32 [B,L] or None
    -> (loss scalar fp32, dpred or None)"""
    L = _l.load()
    _chk(pred, "patch_mse.pred"), _chk(img, "patch_mse.img")
    B, C = img.shape[0], img.shape[1]
    sp = list(img.shape[2:])
    nd = len(sp)
    if p is None:       # adaptive token sequence x [B, C, S, P]: target 'b c s p -> b s (p c)'
        if nd != 2 or tuple(pred.shape) != (B, sp[0], C * sp[1]):
            raise ValueError(f"patch_mse: sequence target [B,C,S,P]={tuple(img.shape)} does not match pred {tuple(pred.shape)}")
        nd, p, sp = 1, sp[1], [sp[0]]
    dims = (ctypes.c_int64 * 3)(*(sp + [1] * (3 - nd)))
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    ws = workspace(4 * 2049, pred.device)
    _l.check(L.ucfvit_patch_mse(pred.data_ptr(), img.data_ptr(), _p(mask), loss.data_ptr(), _p(dpred), B, C, dims, nd, p, grad_scale,
                                ws.data_ptr(), dt(pred), _stream()), "ucfvit_patch_mse")
    return loss, dpred


# ------------------------------------------------------------------------------------------------ optimizer / casts
def adamw(p, g, m, v, shadow, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    L = _l.load()
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    _l.check(L.ucfvit_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _p(shadow), p.numel(), lr, beta1, beta2, eps,
                            weight_decay, bc1, bc2, grad_scale, dt(g), _stream()), "ucfvit_adamw")


def ema_rate(decay):
    """1 - decay, formed in double (the kernel's argument is rounded from it once); decay inside [0, 1)"""
    decay = float(decay)
    if not 0.0 <= decay < 1.0:
        raise ValueError(f"ema_decay must be inside [0, 1), got {decay}")
    return 1.0 - decay


def _chk_ema(ema, p):
    _chk(p, "adamw_ema.p")
    if ema.dtype != torch.float32 or ema.numel() != p.numel() or not ema.is_contiguous():
        raise ValueError("adamw_ema: ema must be a contiguous float32 tensor of p's size")
    return _chk(ema, "adamw_ema.ema")


def adamw_ema(p, g, m, v, shadow, ema, lr, beta1, beta2, eps, weight_decay, step, rate, grad_scale=1.0):
    """adamw, and in the same pass ema += rate * (p_new - ema); rate = ema_rate(decay), a double inside (0, 1]"""
    L = _l.load()
    _chk_ema(ema, p)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    _l.check(L.ucfvit_adamw_ema(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _p(shadow), ema.data_ptr(), p.numel(), lr,
                                beta1, beta2, eps, weight_decay, bc1, bc2, grad_scale, rate, dt(g), _stream()), "ucfvit_adamw_ema")


def _gs_state(state):
    if state.dtype != torch.float32 or state.numel() < _l.GS_STATE_FLOATS or not state.is_contiguous():
        raise ValueError(f"loss-scaler state must be a contiguous float32 tensor of {_l.GS_STATE_FLOATS} elements")
    return _chk(state, "grad scaler state")


def grad_nonfinite(g, state, mult=1.0):
    """state[GS_FOUND_INF] |= any(g * mult * state[GS_INV_SCALE] is Inf or NaN); read-only over g, no host synchronisation"""
    L = _l.load()
    _chk(g, "grad_nonfinite.g")
    _l.check(L.ucfvit_grad_nonfinite(g.data_ptr(), g.numel(), dt(g), mult, _gs_state(state).data_ptr(), _stream()), "ucfvit_grad_nonfinite")


def adamw_scaled(p, g, m, v, shadow, lr, beta1, beta2, eps, weight_decay, state, grad_scale=1.0):
    """adamw under a loss scaler: skipped on the device when state[GS_FOUND_INF] is set, gradients times grad_scale * state[GS_INV_SCALE],
    bias corrections from state[GS_APPLIED_STEPS] + 1"""
    L = _l.load()
    _l.check(L.ucfvit_adamw_scaled(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _p(shadow), p.numel(), lr, beta1, beta2, eps,
                                   weight_decay, grad_scale, dt(g), _gs_state(state).data_ptr(), _stream()), "ucfvit_adamw_scaled")


def adamw_scaled_ema(p, g, m, v, shadow, ema, lr, beta1, beta2, eps, weight_decay, state, rate, grad_scale=1.0):
    """adamw_scaled with the moving average of adamw_ema; a skipped step leaves ema alone"""
    L = _l.load()
    _chk_ema(ema, p)
    _l.check(L.ucfvit_adamw_scaled_ema(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _p(shadow), ema.data_ptr(), p.numel(),
                                       lr, beta1, beta2, eps, weight_decay, grad_scale, rate, dt(g), _gs_state(state).data_ptr(), _stream()),
             "ucfvit_adamw_scaled_ema")


def grad_scaler_update(state):
    L = _l.load()
    _l.check(L.ucfvit_grad_scaler_update(_gs_state(state).data_ptr(), _stream()), "ucfvit_grad_scaler_update")


def _gc_state(state):
    if state.dtype != torch.float32 or state.numel() < _l.GC_STATE_FLOATS or not state.is_contiguous():
        raise ValueError(f"clip state must be a contiguous float32 tensor of {_l.GC_STATE_FLOATS} elements")
    return _chk(state, "clip state")


def _gc_partials(partials, need):
    if partials.dtype != torch.float64 or not partials.is_contiguous() or partials.numel() < need:
        raise ValueError(f"partials must be a contiguous float64 tensor of at least {need} elements")
    return _chk(partials, "partials")


def grad_sqnorm_partials(n, dtype):
    """how many partial sums grad_sqnorm writes for a segment of n elements of `dtype` (0 for an empty one); host only"""
    L = _l.load()
    try:
        code = _DT[dtype]
    except KeyError:
        raise TypeError(f"UCF_VIT HIP ops support float32 and bfloat16 tensors, got {dtype}")
    count = L.ucfvit_grad_sqnorm_partials(n, code)
    if count < 0:
        _l.check(-1, "ucfvit_grad_sqnorm_partials")
    return count


def grad_sqnorm(g, partials, mult=1.0, gs_state=None):
    """partials[:grad_sqnorm_partials(...)] = per-workgroup sums in double of (g * k)^2, k = mult or mult * gs_state[GS_INV_SCALE]; with
    gs_state the pass also sets gs_state[GS_FOUND_INF] as grad_nonfinite would.  Read-only over g, no host synchronisation.  Returns the
    number of partials written."""
    L = _l.load()
    _chk(g, "grad_sqnorm.g")
    count = grad_sqnorm_partials(g.numel(), g.dtype)
    _gc_partials(partials, count)
    _l.check(L.ucfvit_grad_sqnorm(g.data_ptr(), g.numel(), dt(g), mult, None if gs_state is None else _gs_state(gs_state).data_ptr(),
                                  partials.data_ptr(), _stream()), "ucfvit_grad_sqnorm")
    return count


def grad_clip_coef(partials, count, clip_state):
    """clip_state[GC_NORM] = sqrt(sum of partials[:count]), clip_state[GC_COEF] = min(1, clip_state[GC_MAX_NORM] / (norm + 1e-6))"""
    L = _l.load()
    _gc_partials(partials, count)
    _l.check(L.ucfvit_grad_clip_coef(partials.data_ptr(), count, _gc_state(clip_state).data_ptr(), _stream()), "ucfvit_grad_clip_coef")


def clipped_adamw(p, g, m, v, shadow, ema, lr, beta1, beta2, eps, weight_decay, step, rate, clip_state, gs_state=None, grad_scale=1.0):
    """adamw / adamw_ema (gs_state None) or adamw_scaled / adamw_scaled_ema with clip_state[GC_COEF] multiplied into the gradient factor; ema
    (and rate) may be None.  `step` forms the bias corrections as adamw does and is not used under a loss scaler."""
    L = _l.load()
    if ema is not None:
        _chk_ema(ema, p)
    bc1 = bc2 = 1.0
    if gs_state is None:
        bc1 = 1.0 - beta1 ** step
        bc2 = 1.0 - beta2 ** step
    _l.check(L.ucfvit_adamw_clipped(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _p(shadow), _p(ema), p.numel(), lr, beta1, beta2,
                                    eps, weight_decay, bc1, bc2, grad_scale, 0.0 if ema is None else rate, dt(g),
                                    None if gs_state is None else _gs_state(gs_state).data_ptr(), _gc_state(clip_state).data_ptr(),
                                    _stream()), "ucfvit_adamw_clipped")


def cast(src, dst, scale=1.0):
    L = _l.load()
    _l.check(L.ucfvit_cast(src.data_ptr(), dst.data_ptr(), src.numel(), dt(src), dt(dst), scale, _stream()), "ucfvit_cast")
    return dst


# ------------------------------------------------------------------------------------------------ stochastic depth
def _chk_drop_scale(s, rows, rows_per_sample, name):
    _chk(s, name + ".s")
    if rows_per_sample <= 0 or rows % rows_per_sample:
        raise ValueError(f"{name}: {rows} rows are not a multiple of rows_per_sample={rows_per_sample}")
    if s.dtype != torch.float32 or s.dim() != 1 or s.numel() != rows // rows_per_sample:
        raise TypeError(f"{name}: s must be a contiguous fp32 tensor of rows / rows_per_sample = {rows // rows_per_sample} elements")


def drop_path_add(res, branch, s, rows_per_sample, out=None):
    """out[r] = res[r] + s[r // rows_per_sample] * branch[r]; res [rows, D] may have padded rows (a strided view of the stream), out may
    be branch (the default: the branch is overwritten).  A sample with s == 0 is copied from res without reading branch."""
    L = _l.load()
    _chk(res, "drop_path_add.res", rows_ok=True), _chk(branch, "drop_path_add.branch")
    rows, D = branch.shape
    out = branch if out is None else _chk(out, "drop_path_add.out")
    if tuple(res.shape) != (rows, D) or tuple(out.shape) != (rows, D) or res.dtype != branch.dtype or out.dtype != branch.dtype:
        raise TypeError("drop_path_add: res, branch and out must be [rows, D] of one dtype")
    _chk_drop_scale(s, rows, rows_per_sample, "drop_path_add")
    _l.check(L.ucfvit_drop_path_add(res.data_ptr(), res.stride(0), branch.data_ptr(), s.data_ptr(), out.data_ptr(), rows, D,
                                    int(rows_per_sample), dt(branch), _stream()), "ucfvit_drop_path_add")
    return out


def drop_path_scale(x, s, rows_per_sample, out=None, c_colsum=None, c_colsum_accumulate=False):
    """out[r] = s[r // rows_per_sample] * x[r] for x [rows, D]; c_colsum: optional fp32 [D] that receives (+)= the column sums of the
    values written (taken in fp32 before rounding; partial sums per row chunk from the kernel, folded by ucfvit_reduce_rows)"""
    L = _l.load()
    _chk(x, "drop_path_scale.x")
    rows, D = x.shape
    out = torch.empty_like(x) if out is None else _chk(out, "drop_path_scale.out")
    if tuple(out.shape) != (rows, D) or out.dtype != x.dtype:
        raise TypeError("drop_path_scale: out must have x's shape and dtype")
    _chk_drop_scale(s, rows, rows_per_sample, "drop_path_scale")
    cs_rows, part = 0, None
    if c_colsum is not None:
        _chk(c_colsum, "drop_path_scale.c_colsum")
        if c_colsum.dtype != torch.float32 or c_colsum.numel() != D:
            raise TypeError("drop_path_scale: c_colsum must be a contiguous fp32 tensor of D elements")
        cs_rows = L.ucfvit_drop_path_colsum_rows(rows, int(rows_per_sample), D)
        if cs_rows <= 0:
            raise ValueError("drop_path_scale: no column sums of an empty input")
        part = workspace(cs_rows * D * 4, x.device)
    _l.check(L.ucfvit_drop_path_scale(x.data_ptr(), s.data_ptr(), out.data_ptr(), _p(part), rows, D, int(rows_per_sample), dt(x), _stream()),
             "ucfvit_drop_path_scale")
    if part is not None:
        _l.check(L.ucfvit_reduce_rows(part.data_ptr(), c_colsum.data_ptr(), cs_rows, D, 1 if c_colsum_accumulate else 0, _stream()),
                 "ucfvit_reduce_rows")
    return out


# ------------------------------------------------------------------------------------------------ element-wise dropout
def _chk_dropout(s, rows, rows_per_sample, row_step, p, seed, name):
    if s is not None:
        _chk_drop_scale(s, rows, rows_per_sample, name)
    elif rows_per_sample <= 0 or rows % rows_per_sample:
        raise ValueError(f"{name}: {rows} rows are not a multiple of rows_per_sample={rows_per_sample}")
    if not 0.0 < p < 1.0:
        raise ValueError(f"{name}: the kernels take 0 < p < 1, got p={p} (p == 0 is the input itself, p == 1 is zeros: no launch needs a mask)")
    if row_step < 1:
        raise ValueError(f"{name}: row_step={row_step} < 1")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"{name}: the seed must be an unsigned 64-bit integer, got {seed}")


def dropout_add(res, branch, p, seed, s=None, rows_per_sample=1, row_step=1, out=None):
    """out[r] = res[r] + s[r // rows_per_sample] * m * branch[r] / keep with the mask m of (seed, element index) that include/ucfvit_hip.h
    defines (index (r * row_step) * D + c); s: optional fp32 drop-path scale per sample (None: 1).  res [rows, D] may have padded rows, out
    may be branch (the default: the branch is overwritten).  A sample with s == 0 is copied from res without reading branch."""
    L = _l.load()
    _chk(res, "dropout_add.res", rows_ok=True), _chk(branch, "dropout_add.branch")
    rows, D = branch.shape
    out = branch if out is None else _chk(out, "dropout_add.out")
    if tuple(res.shape) != (rows, D) or tuple(out.shape) != (rows, D) or res.dtype != branch.dtype or out.dtype != branch.dtype:
        raise TypeError("dropout_add: res, branch and out must be [rows, D] of one dtype")
    _chk_dropout(s, rows, rows_per_sample, row_step, p, seed, "dropout_add")
    _l.check(L.ucfvit_dropout_add(res.data_ptr(), res.stride(0), branch.data_ptr(), _p(s), out.data_ptr(), rows, D, int(rows_per_sample),
                                  int(row_step), float(p), int(seed), dt(branch), _stream()), "ucfvit_dropout_add")
    return out


def dropout(x, p, seed, s=None, rows_per_sample=1, row_step=1, out=None, c_colsum=None, c_colsum_accumulate=False):
    """out[r] = s[r // rows_per_sample] * m * x[r] / keep for x [rows, D] (mask and s as in dropout_add; out may be x); c_colsum: optional
    fp32 [D] that receives (+)= the column sums of the values written (taken in fp32 before rounding; partial sums per row chunk from the
    kernel, sized by ucfvit_drop_path_colsum_rows, folded by ucfvit_reduce_rows)"""
    L = _l.load()
    _chk(x, "dropout.x")
    rows, D = x.shape
    out = torch.empty_like(x) if out is None else _chk(out, "dropout.out")
    if tuple(out.shape) != (rows, D) or out.dtype != x.dtype:
        raise TypeError("dropout: out must have x's shape and dtype")
    _chk_dropout(s, rows, rows_per_sample, row_step, p, seed, "dropout")
    cs_rows, part = 0, None
    if c_colsum is not None:
        _chk(c_colsum, "dropout.c_colsum")
        if c_colsum.dtype != torch.float32 or c_colsum.numel() != D:
            raise TypeError("dropout: c_colsum must be a contiguous fp32 tensor of D elements")
        cs_rows = L.ucfvit_drop_path_colsum_rows(rows, int(rows_per_sample), D)
        if cs_rows <= 0:
            raise ValueError("dropout: no column sums of an empty input")
        part = workspace(cs_rows * D * 4, x.device)
    _l.check(L.ucfvit_dropout(x.data_ptr(), _p(s), out.data_ptr(), _p(part), rows, D, int(rows_per_sample), int(row_step), float(p), int(seed),
                              dt(x), _stream()), "ucfvit_dropout")
    if part is not None:
        _l.check(L.ucfvit_reduce_rows(part.data_ptr(), c_colsum.data_ptr(), cs_rows, D, 1 if c_colsum_accumulate else 0, _stream()),
                 "ucfvit_reduce_rows")
    return out


# ------------------------------------------------------------------------------------------------ LayerScale
def _chk_layer_scale(gamma, s, rows, D, rows_per_sample, row_step, p, seed, name):
    _chk(gamma, name + ".gamma")
    if gamma.dtype != torch.float32 or gamma.numel() != D:
        raise TypeError(f"{name}: gamma must be a contiguous fp32 tensor of D = {D} elements (the master parameter)")
    if s is not None:
        _chk_drop_scale(s, rows, rows_per_sample, name)
    elif rows_per_sample <= 0 or rows % rows_per_sample:
        raise ValueError(f"{name}: {rows} rows are not a multiple of rows_per_sample={rows_per_sample}")
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{name}: the kernels take 0 <= p < 1 (0: no mask), got p={p}")
    if row_step < 1:
        raise ValueError(f"{name}: row_step={row_step} < 1")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"{name}: the seed must be an unsigned 64-bit integer, got {seed}")


def layer_scale_add(res, branch, gamma, s=None, rows_per_sample=1, p=0.0, seed=0, row_step=1, out=None):
    """out[r] = res[r] + s[r // rows_per_sample] * m * (gamma * branch[r]) / keep; gamma fp32 [D]; res None: without the residual (the
    LayerScale module on its own); s: optional fp32 drop-path scale per sample; p > 0: the dropout mask of (seed, element index) as in
    dropout_add, p == 0: no mask.  res [rows, D] may have padded rows, out may be branch (the default: the branch is overwritten)."""
    L = _l.load()
    _chk(branch, "layer_scale_add.branch")
    rows, D = branch.shape
    out = branch if out is None else _chk(out, "layer_scale_add.out")
    if tuple(out.shape) != (rows, D) or out.dtype != branch.dtype:
        raise TypeError("layer_scale_add: res, branch and out must be [rows, D] of one dtype")
    if res is not None:
        _chk(res, "layer_scale_add.res", rows_ok=True)
        if tuple(res.shape) != (rows, D) or res.dtype != branch.dtype:
            raise TypeError("layer_scale_add: res, branch and out must be [rows, D] of one dtype")
    _chk_layer_scale(gamma, s, rows, D, rows_per_sample, row_step, p, seed, "layer_scale_add")
    _l.check(L.ucfvit_layer_scale_add(_p(res), 0 if res is None else res.stride(0), branch.data_ptr(), gamma.data_ptr(), _p(s), out.data_ptr(),
                                      rows, D, int(rows_per_sample), int(row_step), float(p), int(seed), dt(branch), _stream()),
             "ucfvit_layer_scale_add")
    return out


def layer_scale_grad(dy, branch, gamma, s=None, rows_per_sample=1, p=0.0, seed=0, row_step=1, out=None, c_colsum=None,
                     c_colsum_accumulate=False, c_gamma=None, c_gamma_accumulate=False):
    """out[r] = gamma * g[r] with g[r] = s[r // rows_per_sample] * m * dy[r] / keep (s, mask as in layer_scale_add; out may be dy);
    c_colsum: optional fp32 [D] that receives (+)= the column sums of gamma * g (the exit Linear's bias gradient); c_gamma: optional fp32 [D]
    that receives (+)= the column sums of g * branch (gamma's gradient; branch, the unscaled branch output, may be None without it).  Both
    are taken in fp32 before rounding: partial sums per row chunk from the kernel, folded by ucfvit_reduce_rows."""
    L = _l.load()
    _chk(dy, "layer_scale_grad.dy")
    rows, D = dy.shape
    out = torch.empty_like(dy) if out is None else _chk(out, "layer_scale_grad.out")
    if tuple(out.shape) != (rows, D) or out.dtype != dy.dtype:
        raise TypeError("layer_scale_grad: out must have dy's shape and dtype")
    if branch is not None:
        _chk(branch, "layer_scale_grad.branch")
        if tuple(branch.shape) != (rows, D) or branch.dtype != dy.dtype:
            raise TypeError("layer_scale_grad: branch must have dy's shape and dtype")
    elif c_gamma is not None:
        raise ValueError("layer_scale_grad: the gamma sums need the branch output (branch is None)")
    _chk_layer_scale(gamma, s, rows, D, rows_per_sample, row_step, p, seed, "layer_scale_grad")
    cs_rows, parts = 0, [None, None]
    if c_colsum is not None or c_gamma is not None:
        for i, (c, nm) in enumerate(((c_colsum, "c_colsum"), (c_gamma, "c_gamma"))):
            if c is None:
                continue
            _chk(c, "layer_scale_grad." + nm)
            if c.dtype != torch.float32 or c.numel() != D:
                raise TypeError(f"layer_scale_grad: {nm} must be a contiguous fp32 tensor of D elements")
        cs_rows = L.ucfvit_drop_path_colsum_rows(rows, int(rows_per_sample), D)
        if cs_rows <= 0:
            raise ValueError("layer_scale_grad: no column sums of an empty input")
        ws = workspace(2 * cs_rows * D * 4, dy.device)
        parts = [ws[:cs_rows * D] if c_colsum is not None else None, ws[cs_rows * D:2 * cs_rows * D] if c_gamma is not None else None]
    _l.check(L.ucfvit_layer_scale_grad(dy.data_ptr(), _p(branch), gamma.data_ptr(), _p(s), out.data_ptr(), _p(parts[0]), _p(parts[1]), rows, D,
                                       int(rows_per_sample), int(row_step), float(p), int(seed), dt(dy), _stream()), "ucfvit_layer_scale_grad")
    for part, c, acc in ((parts[0], c_colsum, c_colsum_accumulate), (parts[1], c_gamma, c_gamma_accumulate)):
        if part is not None:
            _l.check(L.ucfvit_reduce_rows(part.data_ptr(), c.data_ptr(), cs_rows, D, 1 if acc else 0, _stream()), "ucfvit_reduce_rows")
    return out


# ------------------------------------------------------------------------------------------------ QK-norm
def _chk_qk_norm(t, rows, H, dh, params, name):
    _chk(t, name + ".qkv")
    if t.dim() != 2 or t.shape[1] != 3 * H * dh or H < 1:
        raise TypeError(f"{name}: qkv must be [rows, 3 H dh] = [rows, {3 * H * dh}], got {tuple(t.shape)}")
    if dh not in (32, 64, 128):
        raise ValueError(f"{name}: head width dh={dh} is not one of 32, 64, 128")
    for i, p in enumerate(params):
        _chk(p, f"{name}.param{i}")
        if p.dtype != torch.float32 or p.numel() != dh:
            raise TypeError(f"{name}: the q_norm / k_norm parameters must be contiguous fp32 tensors of dh = {dh} elements (the master parameters)")


def qk_norm_fwd(qkv, gamma_q, beta_q, gamma_k, beta_k, H, dh, eps, save=True):
    """LayerNorm over the dh elements of every (row, head) segment of the Q third (gamma_q, beta_q) and of the K third (gamma_k, beta_k) of
    qkv [rows, 3 H dh], IN PLACE (the packed layout the attention entry points take); the V third is not touched.  The parameters are fp32
    [dh].  -> (saved_qk [rows, 2 H dh] = the un-normalised Q and K, mean, rstd fp32 [rows, 2 H]) with save, else (None, None, None)."""
    L = _l.load()
    rows = qkv.shape[0]
    _chk_qk_norm(qkv, rows, H, dh, (gamma_q, beta_q, gamma_k, beta_k), "qk_norm_fwd")
    saved = mean = rstd = None
    if save:
        saved = torch.empty((rows, 2 * H * dh), dtype=qkv.dtype, device=qkv.device)
        mean = torch.empty((rows, 2 * H), dtype=torch.float32, device=qkv.device)
        rstd = torch.empty((rows, 2 * H), dtype=torch.float32, device=qkv.device)
    if rows == 0:                                                      # (an empty tensor has no address to hand over)
        return saved, mean, rstd
    _l.check(L.ucfvit_qk_norm_fwd(qkv.data_ptr(), gamma_q.data_ptr(), beta_q.data_ptr(), gamma_k.data_ptr(), beta_k.data_ptr(), _p(saved),
                                  _p(mean), _p(rstd), rows, H, dh, float(eps), dt(qkv), _stream()), "ucfvit_qk_norm_fwd")
    return saved, mean, rstd


def qk_norm_bwd(dqkv, saved_qk, gamma_q, gamma_k, mean, rstd, H, dh, param_grads=None, param_accumulate=False, c_colsum=None,
                c_colsum_accumulate=False):
    """rewrites the Q and K thirds of dqkv [rows, 3 H dh] IN PLACE from the gradient of the normalised values to the gradient of the qkv
    Linear's output (the V third stays).  param_grads: optional fp32 [4, dh] that receives (+)= dgamma_q, dbeta_q, dgamma_k, dbeta_k (sums
    over rows and heads); c_colsum: optional fp32 [2 H dh] that receives (+)= the column sums of the new Q and K thirds, taken before
    rounding (the Q and K thirds of the qkv bias gradient).  Partial sums per row chunk from the kernel, folded by ucfvit_reduce_rows."""
    L = _l.load()
    rows = dqkv.shape[0]
    _chk_qk_norm(dqkv, rows, H, dh, (gamma_q, gamma_k), "qk_norm_bwd")
    _chk(saved_qk, "qk_norm_bwd.saved_qk")
    if tuple(saved_qk.shape) != (rows, 2 * H * dh) or saved_qk.dtype != dqkv.dtype:
        raise TypeError("qk_norm_bwd: saved_qk must be [rows, 2 H dh] of dqkv's dtype")
    for t, nm in ((mean, "mean"), (rstd, "rstd")):
        _chk(t, "qk_norm_bwd." + nm)
        if t.dtype != torch.float32 or t.numel() != rows * 2 * H:
            raise TypeError(f"qk_norm_bwd: {nm} must be fp32 [rows, 2 H]")
    R, pp, cp = 0, None, None
    if rows == 0:
        if param_grads is not None or c_colsum is not None:
            raise ValueError("qk_norm_bwd: no sums of an empty input")
        return dqkv
    if param_grads is not None or c_colsum is not None:
        if param_grads is not None and (_chk(param_grads, "qk_norm_bwd.param_grads").dtype != torch.float32 or param_grads.numel() != 4 * dh):
            raise TypeError("qk_norm_bwd: param_grads must be a contiguous fp32 tensor of 4 dh elements")
        if c_colsum is not None and (_chk(c_colsum, "qk_norm_bwd.c_colsum").dtype != torch.float32 or c_colsum.numel() != 2 * H * dh):
            raise TypeError("qk_norm_bwd: c_colsum must be a contiguous fp32 tensor of 2 H dh elements")
        R = L.ucfvit_qk_norm_partial_rows(rows, H, dh)
        if R <= 0:
            raise ValueError("qk_norm_bwd: no sums of an empty input")
        np_, nc = R * 4 * dh, R * 2 * H * dh
        ws = workspace((np_ + nc) * 4, dqkv.device)
        pp = ws[:np_] if param_grads is not None else None
        cp = ws[np_:np_ + nc] if c_colsum is not None else None
    _l.check(L.ucfvit_qk_norm_bwd(dqkv.data_ptr(), saved_qk.data_ptr(), gamma_q.data_ptr(), gamma_k.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                  _p(pp), _p(cp), rows, H, dh, dt(dqkv), _stream()), "ucfvit_qk_norm_bwd")
    if pp is not None:
        _l.check(L.ucfvit_reduce_rows(pp.data_ptr(), param_grads.data_ptr(), R, 4 * dh, 1 if param_accumulate else 0, _stream()),
                 "ucfvit_reduce_rows")
    if cp is not None:
        _l.check(L.ucfvit_reduce_rows(cp.data_ptr(), c_colsum.data_ptr(), R, 2 * H * dh, 1 if c_colsum_accumulate else 0, _stream()),
                 "ucfvit_reduce_rows")
    return dqkv


def transpose_batched(src_flat, dst_flat, table, n_mats, total_tiles):
    L = _l.load()
    _l.check(L.ucfvit_transpose_batched(src_flat.data_ptr(), dst_flat.data_ptr(), table.data_ptr(), n_mats, total_tiles, _stream()),
             "ucfvit_transpose_batched")


def linear_dgrad_t(dy2, wT, act_grad_aux=None, out=None, aux_is_deriv=False, c_colsum=None, c_colsum_accumulate=False):
    """dx[M,K] = dy2[M,N]·W with W given TRANSPOSED (wT [K,N]): both operands contraction-contiguous (fast path)"""
    M, N = dy2.shape
    K = wT.shape[0]
    return gemm(dy2, wT, M, K, N, LAYOUT_KC, LAYOUT_KC, out=out, act=_dgrad_act(act_grad_aux, aux_is_deriv), aux_in=act_grad_aux,
                c_colsum=c_colsum, c_colsum_accumulate=c_colsum_accumulate)


# ------------------------------------------------------------------------------------------------ DDPM (csrc/diffusion.hip)
def _chk_f32(t, name):
    _chk(t, name)
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected a float32 tensor, got {t.dtype}")
    return t


def ddpm_q_sample(x0, eps, t, sqrt_ab, sqrt_1mab, out=None):
    """out[b] = sqrt_ab[t[b]] * x0[b] + sqrt_1mab[t[b]] * eps[b]; x0, eps fp32 [B, ...]; t int64 [B] on the device (clamped into the tables
    by the kernel); the tables fp32 [T] on the device.  out may be x0."""
    L = _l.load()
    _chk_f32(x0, "ddpm_q_sample.x0"), _chk_f32(eps, "ddpm_q_sample.eps")
    _chk_f32(sqrt_ab, "ddpm_q_sample.sqrt_ab"), _chk_f32(sqrt_1mab, "ddpm_q_sample.sqrt_1mab")
    _chk(t, "ddpm_q_sample.t")
    B = x0.shape[0]
    if t.dtype != torch.int64 or t.numel() != B:
        raise TypeError(f"ddpm_q_sample: t must be an int64 tensor of B = {B} steps, got {t.dtype} {tuple(t.shape)}")
    if eps.shape != x0.shape or sqrt_ab.dim() != 1 or sqrt_1mab.shape != sqrt_ab.shape:
        raise ValueError("ddpm_q_sample: eps must have x0's shape and the two tables one length")
    out = torch.empty_like(x0) if out is None else _chk_f32(out, "ddpm_q_sample.out")
    if out.shape != x0.shape:
        raise ValueError("ddpm_q_sample: out must have x0's shape")
    n = x0.numel() // B if B else 1
    _l.check(L.ucfvit_ddpm_q_sample(x0.data_ptr(), eps.data_ptr(), t.data_ptr(), sqrt_ab.data_ptr(), sqrt_1mab.data_ptr(), out.data_ptr(),
                                    B, n, sqrt_ab.numel(), _stream()), "ucfvit_ddpm_q_sample")
    return out


def time_tokens_fwd(patches, cls, pos, temb, B, Lp, D):
    """tokens_fwd plus the time row temb [B, D] of every sample (include/ucfvit_hip.h)"""
    L = _l.load()
    _chk(patches, "time_tokens.patches"), _chk(temb, "time_tokens.temb")
    if temb.dtype != patches.dtype or tuple(temb.shape) != (B, D):
        raise TypeError(f"time_tokens: temb must be [B={B}, D={D}] of the tokens' dtype, got {temb.dtype} {tuple(temb.shape)}")
    pre = 0 if cls is None else 1
    out = torch.empty((B, Lp + pre, D), dtype=patches.dtype, device=patches.device)
    _l.check(L.ucfvit_time_tokens_fwd(patches.data_ptr(), _p(cls), _p(pos), temb.data_ptr(), out.data_ptr(), B, Lp, D, pre, dt(patches),
                                      _stream()), "ucfvit_time_tokens_fwd")
    return out


def time_tokens_bwd(dout, B, Lp, D, has_cls, want_pos, dpos=None, dcls=None, accumulate=False, want_patches=True):
    """tokens_bwd plus dtemb fp32 [B, D] = the sum of dout over a sample's rows; -> (dpatches, dpos, dcls, dtemb)"""
    L = _l.load()
    _chk(dout, "time_tokens_bwd.dout")
    dev = dout.device
    dpatches = torch.empty((B * Lp, D), dtype=dout.dtype, device=dev) if want_patches else None
    pre = 1 if has_cls else 0
    if want_pos and dpos is None:
        dpos = torch.empty((Lp + pre, D), dtype=torch.float32, device=dev)
    if has_cls and dcls is None:
        dcls = torch.empty(D, dtype=torch.float32, device=dev)
    dtemb = torch.empty((B, D), dtype=torch.float32, device=dev)
    nbytes = L.ucfvit_time_tokens_bwd_workspace(B, Lp, D, pre)
    if nbytes <= 0 and B > 0:
        raise ValueError(f"time_tokens_bwd: sizes B={B} L={Lp} D={D} are refused by the kernel")
    ws = workspace(nbytes, dev)
    _l.check(L.ucfvit_time_tokens_bwd(dout.data_ptr(), _p(dpatches), _p(dpos) if want_pos else None, _p(dcls) if has_cls else None,
                                      dtemb.data_ptr(), B, Lp, D, pre, 1 if accumulate else 0, ws.data_ptr(), dt(dout), _stream()),
             "ucfvit_time_tokens_bwd")
    return dpatches, dpos, dcls, dtemb


def _chk_relu_dropout(p, seed, name):
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{name}: the kernels take 0 <= p < 1 (0: plain ReLU, no mask), got p={p}")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"{name}: the seed must be an unsigned 64-bit integer, got {seed}")


def relu_dropout(x, p=0.0, seed=0, out=None):
    """y = m * relu(x) / keep on x [rows, D] with the dropout mask of (seed, element index) at row_step 1; p == 0: plain ReLU.  out may be x"""
    L = _l.load()
    _chk(x, "relu_dropout.x")
    rows, D = x.shape
    out = torch.empty_like(x) if out is None else _chk(out, "relu_dropout.out")
    if out.shape != x.shape or out.dtype != x.dtype:
        raise TypeError("relu_dropout: out must have x's shape and dtype")
    _chk_relu_dropout(p, seed, "relu_dropout")
    _l.check(L.ucfvit_relu_dropout(x.data_ptr(), out.data_ptr(), rows, D, float(p), int(seed), dt(x), _stream()), "ucfvit_relu_dropout")
    return out


def relu_dropout_bwd(x, dy, p=0.0, seed=0, out=None):
    """dx = m * [x > 0] * dy / keep, the mask recomputed from the seed; x is the pre-activation.  out may be dy"""
    L = _l.load()
    _chk(x, "relu_dropout_bwd.x"), _chk(dy, "relu_dropout_bwd.dy")
    rows, D = x.shape
    out = torch.empty_like(dy) if out is None else _chk(out, "relu_dropout_bwd.out")
    if dy.shape != x.shape or dy.dtype != x.dtype or out.shape != x.shape or out.dtype != x.dtype:
        raise TypeError("relu_dropout_bwd: x, dy and out must be [rows, D] of one dtype")
    _chk_relu_dropout(p, seed, "relu_dropout_bwd")
    _l.check(L.ucfvit_relu_dropout_bwd(x.data_ptr(), dy.data_ptr(), out.data_ptr(), rows, D, float(p), int(seed), dt(x), _stream()),
             "ucfvit_relu_dropout_bwd")
    return out


def _step_args(name, x, pred, z, patch, out):
    """the tensors of a reverse step, checked: -> (out, B, C, dims, nd)"""
    _chk_f32(x, name + ".x"), _chk(pred, name + ".pred")
    if z is not None:
        _chk_f32(z, name + ".z")
        if z.shape != x.shape:
            raise ValueError(f"{name}: z must have x's shape")
    B, C = x.shape[0], x.shape[1]
    sp = list(x.shape[2:])
    nd = len(sp)
    if nd not in (2, 3):
        raise ValueError(f"{name}: x must be NCHW or NCHWD, got {tuple(x.shape)}")
    Lp = 1
    for s in sp:
        Lp *= s // patch
    if tuple(pred.shape) != (B, Lp, C * patch ** nd):
        raise ValueError(f"{name}: pred {tuple(pred.shape)} is not [B, L, p^nd C] = {(B, Lp, C * patch ** nd)} of x {tuple(x.shape)}")
    out = torch.empty_like(x) if out is None else _chk_f32(out, name + ".out")
    if out.shape != x.shape:
        raise ValueError(f"{name}: out must have x's shape")
    return out, B, C, (ctypes.c_int64 * 3)(*(sp + [1] * (3 - nd))), nd


def ddpm_step(x, pred, z, patch, c1, c2, sigma, out=None):
    """out = c1 * (x - c2 * unpatchify(pred)) + sigma * z without the unpatchified tensor: x, z, out fp32 NCHW(D), pred [B, L, p^nd C] in
    fp32 or bf16; z None: no noise (sigma must be 0).  out may be x."""
    L = _l.load()
    out, B, C, dims, nd = _step_args("ddpm_step", x, pred, z, patch, out)
    _l.check(L.ucfvit_ddpm_step(x.data_ptr(), pred.data_ptr(), _p(z), out.data_ptr(), B, C, dims, nd, int(patch), float(c1), float(c2),
                                float(sigma), dt(pred), _stream()), "ucfvit_ddpm_step")
    return out


def ddim_step(x, pred, z, patch, s_ab, s_1mab, r_ab, r_1mab, c_x0, c_eps, sigma, clip=0.0, out=None):
    """the generalised reverse step of ucfvit_ddim_step, tensors as for ddpm_step: x0 = (x - s_1mab e) r_ab, clamped to [-clip, clip] when
    clip > 0 (e then re-derived as (x - s_ab x0) r_1mab), out = c_x0 x0 + c_eps e + sigma z.  clip 0 or None: no clamp."""
    L = _l.load()
    clip = 0.0 if clip is None else float(clip)
    if not clip >= 0.0:
        raise ValueError(f"ddim_step: clip must be None, 0 or positive, got {clip}")
    out, B, C, dims, nd = _step_args("ddim_step", x, pred, z, patch, out)
    _l.check(L.ucfvit_ddim_step(x.data_ptr(), pred.data_ptr(), _p(z), out.data_ptr(), B, C, dims, nd, int(patch), float(s_ab), float(s_1mab),
                                float(r_ab), float(r_1mab), float(c_x0), float(c_eps), float(sigma), clip, dt(pred), _stream()),
             "ucfvit_ddim_step")
    return out
