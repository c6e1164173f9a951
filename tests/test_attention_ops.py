"""The attention kernels of csrc/attention.hip (streaming forward, delta, dQ, dK/dV, the ring pieces cross_fwd / cross_bwd / merge),
csrc/attention_short.hip (resident forward, three-per-CU forward, fused backward) and csrc/varagg.hip against float64 references that see
the same rounded operands, element by element.  U = 2^-24 (fp32), UB = 2^-8 (bf16), c = fl32(scale) * log2(e), all scores in log2 units.

Tier 1, exact.  One-hot rows (keys = distinct +-1 vectors, query i = cq * k[pi(i)], score gap >= 160 in log2 units, so every other
probability underflows to 0): o[i] = v[pi(i)] and dV = dO permuted by pi^-1 bit for bit in bf16 (the surviving p is 2^r with r the fma
residual of s*c - fl(s*c), |r| <= U |m|, which rounds to 1 as a bf16 operand and moves o by less than half a bf16 ulp; in fp32 it stays and
the equalities hold to (3 ln2 |lse| + 8) U); lse = c * q.k[pi] to 6 U of its magnitude; dQ and dK are scale * (dP - delta) * k (or q) with
dP and delta two fp32 dot products of the same dh terms dO.v: |dP - delta| <= (2 dh + 8) U sum|dO||v|.  Uniform rows (Q = 0 or K = 0): p = 1,
l = N exactly, lse = log2 N, o = sum(v) / N within one output rounding; the gradient through the zero operand is exactly 0; the lse rejects
N + 1 and N - 1 at every N, o only where 1 / N > 2 UB (N <= 128).  Symmetries (batch / head permutation, bwd_colsum == bwd, a second call)
are bit for bit.

Tier 2, per-element bounds.  E_ij = (dh + 4) U c (|q_i| . |k_j|) bounds the error of a score (dh fp32 accumulations of exact products, the
rounding of c, the fma), W = P o E its probability-weighted form.
  forward   |o - ref| <= t + ou (|ref| + t),  t = pu P|V| + lu |ref| + ln2 (W|V| + rowsum(W) P|V|) + (2 N + 6 T + 16) U P|V|
            pu: rounding of P as MFMA operand (UB; U for fp32), ou: output rounding, T: key tiles (online-softmax rescales: one exp2 and one
            product each), 2 N U: the fp32 sums of l and of PV.  lu: the STREAMING bf16 kernel takes the row sum from the bf16-rounded P (an
            MFMA with a ones operand), the short kernels from the unrounded fp32 P: lu = UB there, 0 elsewhere.
  lse       |lse - ref| <= rowsum(W) + (N + 6 T + 48) U / ln2 + 4 U max(1, log2 N) + 2 U |ref| + 1.45 lu
            (48 U: fma rounding of arguments above -40 and v_exp_f32; v_exp_f32 and v_log_f32 are 1 ulp instructions, allowed 4 U each.)
            lu makes the streaming bf16 lse a bf16-grade quantity (5.6e-3): it still rejects padding to a 64-key tile and natural-log units,
            a dropped key only where that key carries more than UB of a row.
  backward  every kernel (fused, streaming dQ, streaming dK/dV, cross) recomputes P = 2^(c s - lse) from the lse it is GIVEN, takes delta =
            rowsum(dO o O) in fp32 from the O it is given (the stored bf16 output), dP = dO V^T in fp32 (fused: accumulated onto -delta),
            dS = P (dP - delta) in fp32, rounds dS and P to bf16 as MFMA operands, accumulates in fp32, multiplies dQ / dK by scale and rounds
            once (self-attention) or keeps fp32 (cross_bwd, += when accumulating).  The reference is that function in float64, so the lse
            and O errors of the forward do not enter.  With EP = ln2 (E + 2 U |lse| + 40 U) + 4 U (relative error of P),
            Edp = (dh + 2) U (|dO||V|^T + |delta|) + (dh + 8) U rowsum(|dO||O|),  A = |dS| (pu + EP + N U) + P Edp,  Av = P (pu + EP + N U):
            tol dQ = scale A|K|, dK = scale A^T|Q|, dV = Av^T|dO|, each then t + ou (|ref| + t) + 2 U |ref|.
  colsum    partial[b] against the fp64 column sums of the unrounded reference dQ: sum of the dQ bounds without ou, plus (N + 8) U sum|dQ|.
  merge     against the fp64 log-sum-exp combination of its own inputs: weights are 2^(la - ln) of fp32 arguments.
  varagg    plain fp32 VALU arithmetic in natural-log units, P never rounded: U-grade bounds with (dh + V + 16) terms.
Every Tier 2 comparison goes through _check, which also requires the same bound to reject wrong references: zero-filled padding keys in the
softmax (to a 16-block / 64-key tile), a dropped last key, natural-log units, delta left out, delta of the neighbouring row, scale applied
twice or not at all, the last query row left out of dK / dV.  Comparisons are pooled over the operand families and (batch, head) pairs of a
case, because arithmetic decides which family can reject what: peaked rows and flat rows at N >= 1000 hide a padding key below the bf16
rounding of o, there the lse rejects it.

test_forward_bound_vs_float64_emulation needs no GPU: a float64 emulation of the forward roundings stays inside the forward bound for every
operand family while the wrong references fall outside.

Measured on an MI355X:
  141 GPU cases + 3 CPU cases (two of them the route query, 0.01 s), 5.5 s of test time (9 s wall with start-up; tests/test_baseline_configs.py: 15 s / 18 s in the same run).
  worst err / bound        o      lse    dQ     dK     dV     colsum
  short (bf16)             0.79   0.06   0.80   0.91   0.89   0.69
  streaming bf16           0.44   0.27   0.82   0.90   0.88   -
  streaming fp32           0.06   0.10   0.10   0.12   0.13   -
  cross bf16               0.49   0.31   0.71   0.89   0.90   -
  cross fp32               0.02   0.04   0.03   0.04   0.06   -
  uniform rows (bf16)      0.97   0.43   0.52   0.49   0.32   -
  merge: o 0.11, lse 0.17 (bf16 and fp32 alike).  varagg: out 0.99, lse 0.04, dkv 0.99, dq 0.003.
Finding: the offset family (rows whose scores are all below -128 in log2 units) made the streaming dQ kernel return NaN whenever the last
key tile was ragged: P = 2^(0 - lse) = inf on a zero-filled padding key, and inf * 0 = NaN in dQ += dS K.  The kernel now clears dS of the
padding keys in the ragged tile, as the forward and the fused backward already did."""
import math

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
UB = 2.0 ** -8
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
BF, F32 = torch.bfloat16, torch.float32


def _ops():
    from UCF_VIT._hip import ops
    return ops


def _wl(name):
    import bench
    return bench.WORKLOADS[name]


def _gen(seed, dev):
    return torch.Generator(device=dev).manual_seed(seed)


def _within(got, ref, tol):
    return bool(((got.double() - ref).abs() <= tol).all())


RATIOS = {}


def _check(got, ref, tol, wrong, what, family=None):
    """got within tol of ref everywhere, and the same tol rejects every reference in `wrong`"""
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    ratio = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    if family:
        RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    print(f"RATIO {what}: worst err/bound {ratio:.3f}")
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, "
                                 f"worst excess {float((err - tol)[bad].max()):.3e}, worst err/bound {ratio:.3f}")
    wrong = wrong if isinstance(wrong, (list, tuple)) else [wrong]
    assert len(wrong) > 0, f"{what}: no wrong reference to reject"
    for i, w in enumerate(wrong):
        assert not _within(got, w, tol), f"{what}: the bound does not reject wrong reference {i}"


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _c32(scale):
    """the kernels' constants: scale arrives as fp32, c = scale * log2(e)"""
    s32 = float(torch.tensor(scale, dtype=torch.float32))
    return s32, s32 * LOG2E


# ============================================================================================== dispatch
# attn_route() in csrc/attn_route.h; test_attention_route_query holds the library's own answer, ucfvit_attention_route, to this table.
# bf16, dh in SHORT_DH, N <= 256 -> attention_short.hip, NB = the first bucket that holds ceil(N / 16) blocks:
#   forward: the kernel named here (short: attn_s_fwd_kernel, s3: attn_s3_fwd_kernel), ucfvit_attention_bwd / _bwd_colsum: attn_g_bwd_kernel
#   of the same NB; EXACT where N fills the bucket's last block, else the masked instantiation
SHORT_DH = (32, 64)
SHORT_ROUTES = {  # NB: (forward kernel, N that run EXACT, N that run masked)
    4: ("short", (49, 50, 64), (1, 15, 16, 17)),
    8: ("short", (128,), (65,)),
    13: ("s3", (196, 197, 208), (129,)),
    16: ("short", (255, 256), (209,)),
}
#   everything else -> attention.hip streaming kernels attn_fwd_kernel / attn_delta_kernel / attn_bwd_dq_kernel / attn_bwd_dkv_kernel:
#     bf16 (Geo: QB 2, NBUF 2, 128 queries per workgroup, 64-key tiles): N > 256 at dh 32 / 64, any N at dh 128, B H >= 2^31
#     fp32 (Geo: QB 1, NBUF 1, 64 queries per workgroup): every N and dh
SHORT_N = [1, 15, 16, 17, 64, 65, 128, 129, 197, 208, 209, 255, 256]


def _short_ns():
    ns = set(SHORT_N)
    for name in ("vit_l16_224", "vit_b16_224", "vit_tiny16_224"):
        try:
            w = _wl(name)
            ns.update({(w["img"] // w["patch"]) ** 2, (w["img"] // w["patch"]) ** 2 + 1})
        except Exception:
            pass
    ns.update({49, 50, 196, 197})
    return sorted(n for n in ns if n <= 256)


def _kind(dtype, N, dh):
    """(name, pu, lu, ou, key tiles) of the kernels that (dtype, N, dh) reaches"""
    if dtype == BF and dh in (32, 64) and N <= 256:
        return "short", UB, 0.0, UB, 1
    if dtype == BF:
        return "stream", UB, UB, UB, (N + 63) // 64
    return "fp32", U, 0.0, U, (N + 63) // 64


SELF_CASES = ([(BF, N, dh) for N in (1, 15, 16, 17, 49, 50, 64, 65, 128, 129, 196, 197, 208, 209, 255, 256) for dh in (32, 64)]
              + [(BF, 257, 32), (BF, 257, 64), (BF, 257, 128), (BF, 1000, 32), (BF, 1000, 64), (BF, 1000, 128), (BF, 2048, 64),
                 (BF, 17, 128), (BF, 197, 128)]
              + [(F32, N, dh) for N in (17, 197, 257, 1000) for dh in (32, 64, 128)])
BIG_CASES = [(BF, 2048, 32), (BF, 2048, 128), (BF, 8192, 64), (BF, 8192, 128)]


def _cid(c):
    return f"{'bf16' if c[0] == BF else 'fp32'}-N{c[1]}-dh{c[2]}"


# ============================================================================================== the route query, without a GPU
def _table_route(dtype, N, dh, backward):
    """the name SHORT_ROUTES gives (dtype, N, dh); a short-sequence N the table does not list is an error of the table"""
    if dtype != BF:
        return "stream-fp32"
    if dh in SHORT_DH:
        for nb, (fwd, exact, masked) in SHORT_ROUTES.items():
            if N in exact or N in masked:
                return f"{'fused' if backward else fwd}-nb{nb}-{'exact' if N in exact else 'masked'}"
        assert N > 256, f"N = {N} is missing from SHORT_ROUTES"
    return "stream-bf16"


def _lib_route(dtype, N, dh, backward, B=2, H=3, cap=64):
    import ctypes
    from UCF_VIT._hip import lib as L
    buf = ctypes.create_string_buffer(cap)
    n = L.load().ucfvit_attention_route(B, N, H, dh, L.BF16 if dtype == BF else L.F32, int(backward), buf, cap)
    assert 0 < n < cap, f"ucfvit_attention_route returned {n}"
    assert len(buf.value) == n
    return buf.value.decode()


def test_attention_route_query():
    """no GPU: for every case of the GPU tests, forward and backward, the library routes as SHORT_ROUTES says, _kind() names the same family,
    and the column sums exist exactly where the backward is the fused kernel; a grid.x of 2^31 workgroups or more streams"""
    from UCF_VIT._hip import lib as L
    lib = L.load()
    cases = SELF_CASES + BIG_CASES + [(BF, N, dh) for N in _short_ns() for dh in SHORT_DH]
    family = {"short": "short", "s3": "short", "fused": "short", "stream-bf16": "stream", "stream-fp32": "fp32"}
    seen = set()
    for dtype, N, dh in cases:
        for backward in (False, True):
            said = _lib_route(dtype, N, dh, backward)
            assert said == _table_route(dtype, N, dh, backward), f"{_cid((dtype, N, dh))} backward={backward}: ucfvit_attention_route says {said}"
            head = said if said.startswith("stream") else said.split("-")[0]
            assert family[head] == _kind(dtype, N, dh)[0], f"{_cid((dtype, N, dh))}: _kind says {_kind(dtype, N, dh)[0]}, the library {said}"
            seen.add(said)
        sup = lib.ucfvit_attention_bwd_colsum_supported(2, N, 3, dh, L.BF16 if dtype == BF else L.F32)
        assert sup == int(_lib_route(dtype, N, dh, True).startswith("fused-")), f"{_cid((dtype, N, dh))}: bwd_colsum_supported = {sup}"
    for nb, (fwd, _, _) in SHORT_ROUTES.items():          # every instantiation the table names is asked for
        for tail in ("exact", "masked"):
            assert f"{fwd}-nb{nb}-{tail}" in seen and f"fused-nb{nb}-{tail}" in seen
    assert {"stream-bf16", "stream-fp32"} <= seen
    for backward in (False, True):
        assert _lib_route(BF, 197, 64, backward, B=65535, H=65535) == "stream-bf16"
    assert lib.ucfvit_attention_bwd_colsum_supported(65535, 197, 65535, 64, L.BF16) == 0


def test_attention_route_query_cuts_the_text_to_the_room_given():
    """the length returned is the whole name's, the text is cut to cap - 1 characters and terminated; a refused shape is an error"""
    import ctypes
    from UCF_VIT._hip import lib as L
    lib = L.load()
    name = b"fused-nb13-exact"
    for cap, want in ((4, b"fus\0x"), (1, b"\0xxxx"), (len(name), name[:-1] + b"\0x"), (len(name) + 1, name + b"\0x")):
        buf = ctypes.create_string_buffer(b"x" * 32, 32)
        assert lib.ucfvit_attention_route(2, 197, 3, 64, L.BF16, 1, buf, cap) == len(name)
        assert buf.raw[:len(want)] == want, (cap, buf.raw)
    buf = ctypes.create_string_buffer(b"x" * 32, 32)
    assert lib.ucfvit_attention_route(2, 197, 3, 64, L.BF16, 1, buf, 0) == len(name) and buf.raw == b"x" * 32
    assert lib.ucfvit_attention_route(2, 197, 3, 48, L.BF16, 0, buf, 32) < 0 and b"head dim" in lib.ucfvit_last_error()


# ============================================================================================== float64 references and bounds
def _split(t, B, N, H, dh, b, h):
    """qkv [B*N, 3*H*dh] -> q, k, v [N, dh] of (b, h) in float64"""
    x = t.view(B, N, 3, H, dh)[b, :, :, h].double()
    return x[:, 0], x[:, 1], x[:, 2]


def _fwd_ref(q, k, v, scale, pad=0, drop=0):
    _, c = _c32(scale)
    if drop:
        k, v = k[:-drop], v[:-drop]
    s = (q @ k.T) * c
    if pad:        # zero-filled padding keys that a wrong kernel leaves unmasked: score 0, value 0
        s = torch.cat([s, s.new_zeros(s.shape[0], pad)], 1)
        v = torch.cat([v, v.new_zeros(pad, v.shape[1])], 0)
    m = s.max(1).values
    p = torch.exp2(s - m[:, None])
    l = p.sum(1)
    p = p / l[:, None]
    return p @ v, m + torch.log2(l), p


def _fwd_tol(q, k, v, scale, o, lse, P, pu, lu, ou, T):
    N, dh = k.shape
    _, c = _c32(scale)
    W = P * ((dh + 4) * U * c * (q.abs() @ k.abs().T))
    Ws = W.sum(1)
    PV = P @ v.abs()
    t = pu * PV + lu * o.abs() + LN2 * (W @ v.abs() + Ws[:, None] * PV) + (2 * N + 6 * T + 16) * U * PV
    tol_o = t + ou * (o.abs() + t)
    tol_lse = Ws + (N + 6 * T + 48) * U / LN2 + 4 * U * max(1.0, math.log2(N)) + 2 * U * lse.abs() + 1.45 * lu + 1e-12
    return tol_o, tol_lse


def _fwd_wrongs(q, k, v, scale, N, block):
    """wrong references of the forward: padding keys to the next multiple of `block` (one where N is a multiple), a dropped last key"""
    pad = (-N) % block or 1
    w = [_fwd_ref(q, k, v, scale, pad=pad)]
    if N > 1:
        w.append(_fwd_ref(q, k, v, scale, drop=1))
    return w


def _bwd_ref(q, k, v, og, do, lse_g, scale, delta="ok", smode="ok", drop_q=False):
    s32, c = _c32(scale)
    P = torch.exp2((q @ k.T) * c - lse_g[:, None])
    if drop_q:
        P = P.clone()
        P[-1] = 0
    dP = do @ v.T
    d = (do * og).sum(1)
    if delta == "none":
        d = torch.zeros_like(d)
    elif delta == "roll":
        d = d.roll(1)
    dS = P * (dP - d[:, None])
    sc = {"ok": s32, "twice": s32 * s32, "never": 1.0}[smode]
    return sc * (dS @ k), sc * (dS.T @ q), P.T @ do, (P, dS, d)


def _bwd_tol(q, k, v, og, do, lse_g, scale, parts, refs, pu, ou, acc_prev=None):
    Nq, dh = q.shape
    N = max(Nq, k.shape[0])
    s32, c = _c32(scale)
    P, dS, d = parts
    EP = LN2 * ((dh + 4) * U * c * (q.abs() @ k.abs().T) + (2 * U * lse_g.abs() + 40 * U)[:, None]) + 4 * U
    Edp = (dh + 2) * U * (do.abs() @ v.abs().T + d.abs()[:, None]) + ((dh + 8) * U * (do.abs() * og.abs()).sum(1))[:, None]
    A = dS.abs() * (pu + EP + N * U) + P * Edp
    Av = P * (pu + EP + N * U)
    raw = [s32 * (A @ k.abs()), s32 * (A.T @ q.abs()), Av.T @ do.abs()]
    tols = [t + ou * (r.abs() + t) + 2 * U * r.abs() + 1e-300 for t, r in zip(raw, refs)]
    return tols, raw


def _emulate_fwd(q, k, v, scale):
    """float64 emulation of the short forward's roundings: P to bf16 as operand, row sum of the unrounded P, one output rounding"""
    _, c = _c32(scale)
    s = (q @ k.T) * c
    p = torch.exp2(s - s.max(1).values[:, None])
    l = p.sum(1)
    o = (p.float().bfloat16().double() @ v) / l[:, None]
    return o.float().bfloat16(), (s.max(1).values + torch.log2(l)).float()


# ============================================================================================== operands
def _operands(family, dtype, B, N, H, dh, seed, dev):
    """-> qkv [B*N, 3*H*dh], dO [B*N, H*dh] (mixed magnitude across rows), scale"""
    g = _gen(seed, dev)
    x = torch.randn((B, N, 3, H, dh), generator=g, device=dev)
    if family == "randn":
        scale = dh ** -0.5
    elif family == "peaked":          # natural-log scores of standard deviation 13 sqrt(2 ln(N + 1)): the two best keys of a row lie 13 apart
        scale = 1.0 / 3.0             # on average, so the best one takes more than 0.99 in most rows, not in all
        x[:, :, 0] *= 13.0 * math.sqrt(2.0 * math.log(N + 1.0)) / (scale * math.sqrt(dh))
    elif family == "offset":          # small operands, scale 1; one component shared by all keys moves a row's scores by +-50 .. +-100
        scale = 1.0
        x *= 0.3
        x[:, :, 1, :, 0] = 8.0
        sign = torch.where(torch.rand((B, N, H), generator=g, device=dev) < 0.5, -1.0, 1.0)
        x[:, :, 0, :, 0] = sign * (6.25 + 6.25 * torch.rand((B, N, H), generator=g, device=dev))
    else:
        raise ValueError(family)
    do = torch.randn((B, N, H * dh), generator=g, device=dev)
    do = do * torch.exp2(torch.randint(-6, 3, (B, N, 1), generator=g, device=dev).float())
    return x.reshape(B * N, 3 * H * dh).to(dtype), do.reshape(B * N, H * dh).to(dtype), scale


def _onehot_operands(dtype, B, N, H, dh, seed, dev, scale):
    """keys: distinct +-1 vectors; query i = cq * k[pi(i)]; returns qkv, dO, pi [B, H, N], cq.  pi sends the first rows to the last keys and
    the last rows to the first keys (the streaming kernels then meet the row's key in the last / the first tile), random in between."""
    g = _gen(seed, dev)
    _, c = _c32(scale)
    k = torch.empty((B, H, N, dh), device=dev)
    for b in range(B):
        for h in range(H):
            while True:
                kk = torch.where(torch.rand((N, dh), generator=g, device=dev) < 0.5, -1.0, 1.0)
                if torch.unique(kk, dim=0).shape[0] == N:
                    break
            k[b, h] = kk
    dots = k @ k.transpose(-1, -2) - 2.0 * dh * torch.eye(N, device=dev)       # off-diagonal k.k' (integers), diagonal pushed below
    margin = dh - float(dots.max()) if N > 1 else 2.0 * dh                      # >= 2: the keys are distinct
    cq = 2.0 ** math.ceil(math.log2(160.0 / (c * margin)))                      # smallest power of two with a score gap >= 160
    e = min(8, N // 2)
    ar = torch.arange(N, device=dev)
    pi = torch.empty((B, H, N), dtype=torch.int64, device=dev)
    for b in range(B):
        for h in range(H):
            mid = ar[e:N - e][torch.randperm(N - 2 * e, generator=g, device=dev)]
            pi[b, h] = torch.cat([ar[N - e:], mid, ar[:e]])
    q = cq * torch.gather(k, 2, pi[..., None].expand(-1, -1, -1, dh))
    v = torch.randn((B, H, N, dh), generator=g, device=dev)
    qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * dh).to(dtype)
    do = torch.randn((B * N, H * dh), generator=g, device=dev).to(dtype)
    return qkv, do, pi, cq


# ============================================================================================== CPU: the bound against an emulation
def test_forward_bound_vs_float64_emulation():
    """no GPU: the float64 emulation of the forward roundings is inside the forward bound for every operand family.  Flat rows: o and lse
    both reject the padding-key and the dropped-key reference (up to N = 197; at N = 1000 only the lse is asked to).  Peaked rows: the row maximum
    lies 20 .. 60 above the score 0 of a padding key, which no output can see, and a dropped key shows only in rows where it carries weight:
    those references are left to the flat rows.  Natural-log units are rejected by every family."""
    for N, dh in ((17, 32), (197, 64), (1000, 64)):
        for family in ("randn", "peaked", "offset"):
            qkv, _, scale = _operands(family, BF, 1, N, 1, dh, 7 * N + dh, "cpu")
            q, k, v = _split(qkv, 1, N, 1, dh, 0, 0)
            o, lse = _emulate_fwd(q, k, v, scale)
            ro, rl, P = _fwd_ref(q, k, v, scale)
            to, tl = _fwd_tol(q, k, v, scale, ro, rl, P, UB, 0.0, UB, 1)
            wr = _fwd_wrongs(q, k, v, scale, N, 16)
            assert _within(o, ro, to), f"emulated o {family} N={N}"
            print(f"RATIO emulated o {family} N={N}: {float(((o.double() - ro).abs() / to).max()):.3f}")
            if family == "randn":
                _check(lse, rl, tl, [w[1] for w in wr] + [rl * LN2], f"emulated lse {family} N={N}")
                if N <= 197:         # at N = 1000 one key in a thousand moves o by less than its bf16 rounding: the lse has to tell
                    _check(o, ro, to, [w[0] for w in wr], f"emulated o {family} N={N}")
            else:
                _check(lse, rl, tl, [rl * LN2], f"emulated lse {family} N={N}")
            if family == "peaked" and N >= 49:
                assert float((P.max(1).values > 0.99).double().mean()) > 0.5


# ============================================================================================== Tier 2: self-attention
def _self_case(dtype, N, dh, B, H, families, pairs, seed0, check_colsum=False):
    ops = _ops()
    name, pu, lu, ou, T = _kind(dtype, N, dh)
    fam = f"{name}"
    pool = {key: ([], [], [], None) for key in ("o", "lse", "dq", "dk", "dv", "cs")}
    wrongs = {key: None for key in pool}

    def add(key, got, ref, tol, wr):
        pool[key][0].append(got.double().reshape(-1))
        pool[key][1].append(ref.reshape(-1))
        pool[key][2].append(tol.expand_as(ref).reshape(-1))
        if wrongs[key] is None:
            wrongs[key] = [[] for _ in wr]
        for lst, w in zip(wrongs[key], wr):
            lst.append(w.reshape(-1))

    for fi, family in enumerate(families):
        qkv, do, scale = _operands(family, dtype, B, N, H, dh, seed0 + fi, DEV)
        o, lse = ops.attention_fwd(qkv, B, N, H, dh, scale)
        if check_colsum and ops.attention_bwd_colsum_supported(B, N, H, dh, dtype):
            dqkv, part = ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, scale, want_colsum=True)
            assert torch.equal(_bits(dqkv), _bits(ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, scale)))
            assert float(part[:, H * dh:].abs().max()) == 0.0
        else:
            dqkv, part = ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, scale), None
        assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(dqkv.float()).all()) and bool(torch.isfinite(lse).all())
        for (b, h) in pairs:
            q, k, v = _split(qkv, B, N, H, dh, b, h)
            og = o.view(B, N, H, dh)[b, :, h].double()
            dg = do.view(B, N, H, dh)[b, :, h].double()
            lg = lse[b, h].double()
            ro, rl, P = _fwd_ref(q, k, v, scale)
            to, tl = _fwd_tol(q, k, v, scale, ro, rl, P, pu, lu, ou, T)
            wr = _fwd_wrongs(q, k, v, scale, N, 16 if name == "short" else 64)
            if N == 1:
                wr = wr + [wr[0]]
            # a dropped key moves o and lse by 1 / N of a flat row: below the bf16 rounding of o beyond N = 300, and below the lu term of the
            # streaming bf16 lse at every N these kernels see; the padding keys are seen through the rows of negative common offset
            add("o", og, ro, to, [w[0] for w in (wr if N <= 300 else wr[:1])])
            add("lse", lg, rl, tl, [w[1] for w in (wr if lu == 0.0 else wr[:1])] + [rl * LN2])
            if family == "peaked" and N >= 49:
                assert float((P.max(1).values > 0.99).double().mean()) > 0.5, "premise: peaked rows"
            del P
            rq, rk, rv, parts = _bwd_ref(q, k, v, og, dg, lg, scale)
            tols, raw = _bwd_tol(q, k, v, og, dg, lg, scale, parts, (rq, rk, rv), pu, ou)
            w_none = _bwd_ref(q, k, v, og, dg, lg, scale, delta="none")
            w_roll = _bwd_ref(q, k, v, og, dg, lg, scale, delta="roll")
            w_tw = _bwd_ref(q, k, v, og, dg, lg, scale, smode="twice")
            w_nv = _bwd_ref(q, k, v, og, dg, lg, scale, smode="never")
            w_dq = _bwd_ref(q, k, v, og, dg, lg, scale, drop_q=True)
            g = dqkv.view(B, N, 3, H, dh)[b, :, :, h].double()
            add("dq", g[:, 0], rq, tols[0], [w_none[0], w_roll[0], w_tw[0], w_nv[0]])
            add("dk", g[:, 1], rk, tols[1], [w_none[1], w_roll[1], w_tw[1], w_nv[1], w_dq[1]])
            add("dv", g[:, 2], rv, tols[2], [w_dq[2]])
            if part is not None:      # column sums of the unrounded dQ of this (b, h): an fp32 sum of N fp32 values
                cs_ref = rq.sum(0)
                cs_tol = raw[0].sum(0) + (N + 8) * U * rq.abs().sum(0) + 1e-300
                add("cs", part[b, h * dh:(h + 1) * dh].double(), cs_ref, cs_tol,
                    [w_none[0].sum(0), w_tw[0].sum(0), rq[:-1].sum(0) if 1 < N <= 64 else w_nv[0].sum(0)])   # one row in N: up to N = 64
            del parts, tols, raw
    for key in ("o", "lse", "dq", "dk", "dv", "cs"):
        if not pool[key][0]:
            continue
        got, ref, tol = (torch.cat(x) for x in pool[key][:3])
        wr = [torch.cat(w) for w in wrongs[key]]
        wr = [w for w in wr if not torch.equal(w, ref)]       # e.g. N = 1: dQ = dK = 0 whatever the scale; scale 1: twice = never = once
        _check(got, ref, tol, wr, f"{key} {name} N={N} dh={dh}", f"{key}/{fam}")


@gpu
@pytest.mark.parametrize("case", SELF_CASES, ids=_cid)
def test_self_attention_vs_fp64(case):
    """o, lse, dQ, dK, dV (and the bwd_colsum partials where they exist) of every dispatch, pooled over the randn / peaked / common-offset
    families (scales dh^-0.5, 1/3, 1.0) and all (batch, head) pairs, dO of mixed magnitude across rows"""
    dtype, N, dh = case
    B, H = (2, 3) if N <= 300 else (1, 2)
    _self_case(dtype, N, dh, B, H, ("randn", "peaked", "offset"), [(b, h) for b in range(B) for h in range(H)], 1000 * N + dh,
               check_colsum=True)


@gpu
@pytest.mark.parametrize("case", BIG_CASES, ids=_cid)
def test_self_attention_long_sequences_vs_fp64(case):
    """the streaming bf16 kernels at N 2048 and 8192 (32 / 128 key tiles, 16 / 64 query workgroups), one (batch, head) pair at a time"""
    dtype, N, dh = case
    _self_case(dtype, N, dh, 1, 2, ("randn", "peaked", "offset"), [(0, 0), (0, 1)], 17 * N + dh)


@gpu
def test_self_attention_grid_wraps_over_the_cus():
    """the ViT-L batch of bench.WORKLOADS at N = 197: B * H workgroups wrap many times over the 256 CUs; first, last and inner pairs"""
    w = _wl("vit_l16_224")
    B, H = int(w["batch"]), int(w["heads"])
    dh = int(w["dim"]) // H
    N = (int(w["img"]) // int(w["patch"])) ** 2 + 1
    assert N == 197 and dh == 64 and B * H > 8 * 256
    pairs = [(0, 0), (B - 1, H - 1), (0, H - 1), (B - 1, 0), (B // 2, H // 2), (B // 3, 1)]
    _self_case(BF, N, dh, B, H, ("randn",), pairs, 4242, check_colsum=True)


# ============================================================================================== Tier 1: one-hot rows
ONEHOT_CASES = ([(BF, N, dh) for N in (1, 17, 64, 65, 128, 129, 197, 208, 209, 256) for dh in (32, 64)]
                + [(BF, 257, 64), (BF, 1000, 32), (BF, 1000, 128), (BF, 197, 128), (BF, 2048, 64)]
                + [(F32, 17, 32), (F32, 197, 64), (F32, 257, 128), (F32, 1000, 64)])


@gpu
@pytest.mark.parametrize("case", ONEHOT_CASES, ids=_cid)
def test_one_hot_rows_are_exact(case):
    dtype, N, dh = case
    ops = _ops()
    B, H = 2, 2
    scale = dh ** -0.5
    s32, c = _c32(scale)
    qkv, do, pi, cq = _onehot_operands(dtype, B, N, H, dh, 31 * N + dh, DEV, scale)
    x = qkv.view(B, N, 3, H, dh).double()
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))                 # [B, H, N, dh]
    s2 = (q @ k.transpose(-1, -2)) * c
    top = s2.topk(min(2, N), dim=-1)
    assert torch.equal(top.indices[..., 0], pi), "premise: argmax = pi"
    assert torch.equal(torch.sort(pi, -1).values, torch.arange(N, device=DEV).expand(B, H, N)), "premise: pi is a permutation"
    if N > 1:
        assert float((top.values[..., 0] - top.values[..., 1]).min()) >= 160.0, "premise: score gap"
        e = min(8, N // 2)
        assert bool((pi[..., :e] >= N - e).all()) and bool((pi[..., N - e:] < e).all()), "premise: first rows -> last keys, last -> first"
    assert float(s2.abs().max()) * U * LN2 * 3 < 2.0 ** -10, "premise: the fma residual stays below half a bf16 ulp"
    o, lse = ops.attention_fwd(qkv, B, N, H, dh, scale)
    dqkv = ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, scale)
    idx = pi[..., None].expand(-1, -1, -1, dh)
    og = o.view(B, N, H, dh).permute(0, 2, 1, 3)
    vg = torch.gather(qkv.view(B, N, 3, H, dh)[:, :, 2].permute(0, 2, 1, 3), 2, idx)             # v[pi(i)]
    dog = do.view(B, N, H, dh).permute(0, 2, 1, 3)
    g = dqkv.view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)                                         # [3, B, H, N, dh]
    dv_want = torch.zeros_like(dog).scatter(2, idx, dog)                                         # dV[pi(i)] = dO[i]
    lse_ref = top.values[..., 0]
    assert bool(((lse.double() - lse_ref).abs() <= 6 * U * lse_ref.abs()).all()), "lse = c q.k[pi]"
    if dtype == BF:
        assert torch.equal(_bits(og.contiguous()), _bits(vg.contiguous())), "o[i] = v[pi(i)] bit for bit"
        assert torch.equal(_bits(g[2].contiguous()), _bits(dv_want.contiguous())), "dV = dO permuted by pi^-1 bit for bit"
        eu = 2 * UB
    else:
        r = (3 * LN2 * lse_ref.abs()[..., None] + 8) * U
        assert bool(((og.double() - vg.double()).abs() <= r * vg.double().abs()).all())
        rj = torch.zeros_like(r).scatter(2, pi[..., None], r)
        assert bool(((g[2].double() - dv_want.double()).abs() <= rj * dv_want.double().abs()).all())
        eu = 8 * U
    # dS[i][pi(i)] = dP - delta: two fp32 dot products of the same dh terms dO[i] . v[pi(i)]; every other dS is 0 * finite = 0
    gap = (2 * dh + 8) * U * (dog.double().abs() * vg.double().abs()).sum(-1) * (1 + eu)          # [B, H, N] by query
    tol_q = (s32 * gap)[..., None] * torch.gather(k, 2, idx).abs() * (1 + eu)
    assert bool((g[0].double().abs() <= tol_q).all()), "dQ = 0 up to the difference of two fp32 dot products"
    tol_k = torch.zeros_like(tol_q).scatter(2, idx, (s32 * gap)[..., None] * q.abs() * (1 + eu))
    assert bool((g[1].double().abs() <= tol_k).all()), "dK = 0 up to the difference of two fp32 dot products"


# ============================================================================================== Tier 1: uniform rows
@gpu
@pytest.mark.parametrize("case", [(BF, 17, 32), (BF, 64, 64), (BF, 128, 32), (BF, 197, 64), (BF, 209, 64), (BF, 256, 32), (BF, 1000, 64),
                                  (BF, 197, 128), (F32, 197, 64), (F32, 257, 32)], ids=_cid)
@pytest.mark.parametrize("zero", ["q", "k"])
def test_uniform_rows(case, zero):
    """Q = 0 or K = 0: p = 1 and l = N exactly.  V in multiples of 1/4: sum(v) is exact in fp32."""
    dtype, N, dh = case
    ops = _ops()
    B, H = 2, 2
    name, pu, lu, ou, T = _kind(dtype, N, dh)
    g = _gen(N + dh, DEV)
    x = torch.randn((B, N, 3, H, dh), generator=g, device=DEV)
    x[:, :, 2] = torch.randint(-8, 9, (B, N, H, dh), generator=g, device=DEV).float() * 0.25
    x[:, :, 0 if zero == "q" else 1] = 0
    qkv = x.reshape(B * N, 3 * H * dh).to(dtype)
    do = torch.randn((B * N, H * dh), generator=g, device=DEV).to(dtype)
    scale = dh ** -0.5
    o, lse = ops.attention_fwd(qkv, B, N, H, dh, scale)
    dqkv = ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, scale)
    sv = qkv.view(B, N, 3, H, dh)[:, :, 2].double().sum(1, keepdim=True).expand(B, N, H, dh)      # exact
    og = o.view(B, N, H, dh)
    tol_l = torch.full((B, H, N), 4 * U * max(1.0, math.log2(N)), dtype=torch.float64, device=DEV)
    ref_l = torch.full((B, H, N), math.log2(N), dtype=torch.float64, device=DEV)
    _check(lse, ref_l, tol_l, [torch.full_like(ref_l, math.log2(N + 1)), torch.full_like(ref_l, math.log2(max(N - 1, 1)) if N > 1 else -1.0)],
           f"uniform lse {name} N={N}", f"lse-uniform/{name}")
    ref_o = sv / N
    tol_o = (ou + 4 * U) * ref_o.abs() + 1e-300
    wrong_o = [sv / (N + 1), sv / max(N - 1, 1)] if N <= 128 else [sv / N * (1 + 3 * UB)]          # 1 / N > 2 UB only up to N = 128
    _check(og, ref_o, tol_o, wrong_o, f"uniform o {name} N={N}", f"o-uniform/{name}")
    gz = dqkv.view(B, N, 3, H, dh)[:, :, 1 if zero == "q" else 0]
    assert float(gz.float().abs().max()) == 0.0, "the gradient through a zero operand is exactly zero"
    # dV[j] = sum_i P_ij dO[i], P = 2^(0 - lse given) = (1 / N)(1 + e): the generic backward bound.  Rejected: the lse read in natural-log
    # units, the last query row left out (one row in N: visible up to N = 300), a denominator of N + 1 (1 / N > UB: up to N = 64)
    for b, h in ((0, 0), (B - 1, H - 1)):
        q, k, v = _split(qkv, B, N, H, dh, b, h)
        ogb, dg, lg = og[b, :, h].double(), do.view(B, N, H, dh)[b, :, h].double(), lse[b, h].double()
        rq, rk, rv, parts = _bwd_ref(q, k, v, ogb, dg, lg, scale)
        tols, _ = _bwd_tol(q, k, v, ogb, dg, lg, scale, parts, (rq, rk, rv), pu, ou)
        gg = dqkv.view(B, N, 3, H, dh)[b, :, :, h]
        _check(gg[:, 2], rv, tols[2], [rv * N / N ** LN2] + ([_bwd_ref(q, k, v, ogb, dg, lg, scale, drop_q=True)[2]] if N <= 300 else [])
               + ([rv * N / (N + 1)] if N <= 64 else []), f"uniform dV {name} N={N}",
               f"dv/{name}")
        other = 1 if zero == "k" else 0
        ref_other = rk if zero == "k" else rq
        _check(gg[:, other], ref_other, tols[other], [_bwd_ref(q, k, v, ogb, dg, lg, scale, delta="none")[other]],
               f"uniform d{'k' if other else 'q'} {name} N={N}", f"{'dk' if other else 'dq'}/{name}")


# ============================================================================================== Tier 1: symmetries
@gpu
@pytest.mark.parametrize("case", [(BF, 17, 32), (BF, 50, 64), (BF, 128, 64), (BF, 197, 64), (BF, 197, 32), (BF, 256, 64), (BF, 257, 64),
                                  (BF, 197, 128), (BF, 1000, 32), (F32, 197, 64)], ids=_cid)
def test_batch_and_head_permutation_bit_for_bit(case):
    """permuting batch elements and heads permutes o, lse and the gradients; a second call and bwd_colsum return the same bits"""
    dtype, N, dh = case
    ops = _ops()
    B, H = 5, 3
    qkv, do, scale = _operands("randn", dtype, B, N, H, dh, 99 + N, DEV)
    pb = torch.randperm(B, generator=_gen(1, DEV), device=DEV)
    ph = torch.randperm(H, generator=_gen(2, DEV), device=DEV)
    qkv2 = qkv.view(B, N, 3, H, dh)[pb][:, :, :, ph].reshape(B * N, -1).contiguous()
    do2 = do.view(B, N, H, dh)[pb][:, :, ph].reshape(B * N, -1).contiguous()
    o, lse = ops.attention_fwd(qkv, B, N, H, dh, scale)
    d = ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, scale)
    o2, lse2 = ops.attention_fwd(qkv2, B, N, H, dh, scale)
    d2 = ops.attention_bwd(qkv2, o2, do2, lse2, B, N, H, dh, scale)
    assert torch.equal(_bits(o.view(B, N, H, dh)[pb][:, :, ph].contiguous()), _bits(o2.view(B, N, H, dh)))
    assert torch.equal(_bits(lse[pb][:, ph].contiguous()), _bits(lse2))
    assert torch.equal(_bits(d.view(B, N, 3, H, dh)[pb][:, :, :, ph].contiguous()), _bits(d2.view(B, N, 3, H, dh)))
    o3, lse3 = ops.attention_fwd(qkv, B, N, H, dh, scale)
    assert torch.equal(_bits(o3), _bits(o)) and torch.equal(_bits(lse3), _bits(lse))
    assert torch.equal(_bits(ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, scale)), _bits(d))
    if ops.attention_bwd_colsum_supported(B, N, H, dh, dtype):
        d4, part = ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, scale, want_colsum=True)
        assert torch.equal(_bits(d4), _bits(d)) and part is not None
    else:
        assert ops.attention_bwd(qkv, o, do, lse, B, N, H, dh, scale, want_colsum=True)[1] is None


# ============================================================================================== ring pieces
def _merge_ref(oa, la, op, lp):
    ln = torch.logaddexp(la * LN2, lp * LN2) / LN2
    wa, wp = torch.exp2(la - ln), torch.exp2(lp - ln)
    return oa * wa[..., None] + op * wp[..., None], ln, wa, wp


@gpu
@pytest.mark.parametrize("dtype,dh", [(BF, 64), (BF, 32), (BF, 128), (F32, 64), (F32, 32)], ids=lambda x: str(x).replace("torch.", ""))
def test_ring_cross_fwd_merge_cross_bwd_vs_fp64(dtype, dh):
    """cross_fwd per key block (Nq != Nk, ragged last tiles on both sides, padded leading dimensions), merge (first and later) against the
    fp64 combination of its own inputs, cross_bwd (overwrite, then accumulate) against the fp64 function of the lse / O it is given"""
    ops = _ops()
    B, Nq, H = 2, 100, 2
    Nks = [70, 130, 64]
    Wd = H * dh
    name = "cross-bf16" if dtype == BF else "cross-fp32"
    pu, lu, ou = (UB, UB, UB) if dtype == BF else (U, 0.0, U)
    g = _gen(5 + dh, DEV)
    for scale in (dh ** -0.5, 1.0 / 3.0):
        qbuf = torch.randn((B * Nq, Wd + 64), generator=g, device=DEV).to(dtype)
        q2 = qbuf[:, :Wd]
        blocks = [torch.randn((B * nk, 2 * Wd + 8), generator=g, device=DEV).to(dtype) for nk in Nks]
        do = (torch.randn((B * Nq, Wd), generator=g, device=DEV)
              * torch.exp2(torch.randint(-4, 3, (B * Nq, 1), generator=g, device=DEV).float())).to(dtype)
        o_acc = torch.full((B * Nq, Wd), float("nan"), dtype=F32, device=DEV)
        l_acc = torch.full((B, H, Nq), float("nan"), dtype=F32, device=DEV)
        for bi, (blk, nk) in enumerate(zip(blocks, Nks)):
            k2, v2 = blk[:, :Wd], blk[:, Wd:2 * Wd]
            op, lp = ops.attention_cross_fwd(q2, k2, v2, B, Nq, nk, H, dh, scale)
            G, R, TL, WR = [], [], [], [[], []]
            GL, RL, TLL, WRL = [], [], [], [[], [], []]
            for b in range(B):
                for h in range(H):
                    q = q2.view(B, Nq, Wd)[b, :, h * dh:(h + 1) * dh].double()
                    k = k2.reshape(B, nk, Wd)[b, :, h * dh:(h + 1) * dh].double()
                    v = v2.reshape(B, nk, Wd)[b, :, h * dh:(h + 1) * dh].double()
                    ro, rl, P = _fwd_ref(q, k, v, scale)
                    to, tl = _fwd_tol(q, k, v, scale, ro, rl, P, pu, lu, ou, (nk + 63) // 64)
                    wr = _fwd_wrongs(q, k, v, scale, nk, 64)
                    G.append(op.view(B, Nq, H, dh)[b, :, h].double()), R.append(ro), TL.append(to)
                    GL.append(lp[b, h].double()), RL.append(rl), TLL.append(tl)
                    for i in range(2):       # one zero-score padding key after a FULL 64-key tile carries less than UB of these rows
                        WR[i].append(wr[i if nk % 64 else 1][0]), WRL[i].append(wr[i if nk % 64 else 1][1])
                    WRL[2].append(rl * LN2)
            _check(torch.cat(G), torch.cat(R), torch.cat(TL), [torch.cat(w) for w in WR], f"cross_fwd o {name} block {bi}", f"o/{name}")
            _check(torch.cat(GL), torch.cat(RL), torch.cat(TLL), [torch.cat(w) for w in WRL], f"cross_fwd lse {name} block {bi}", f"lse/{name}")
            oa0, la0 = o_acc.clone(), l_acc.clone()
            ops.attention_merge(o_acc, l_acc, op, lp, B, Nq, H, dh, first=(bi == 0))
            if bi == 0:
                assert torch.equal(o_acc, op.float()) and torch.equal(l_acc, lp), "first merge: a plain copy"
                continue
            oa = oa0.view(B, Nq, H, dh).permute(0, 2, 1, 3).double()
            opd = op.view(B, Nq, H, dh).permute(0, 2, 1, 3).double()
            mo, ml, wa, wp = _merge_ref(oa, la0.double(), opd, lp.double())
            eps = lambda l_: LN2 * (4 * U * (l_ - ml).abs() + 2 * U * (l_.abs() + ml.abs()) + 8 * U) + 4 * U
            tol_l = 8 * U / LN2 + 6 * U * ml.abs().clamp_min(1.0)
            tol_o = ((oa.abs() * wa[..., None]) * (eps(la0.double()) + LN2 * tol_l)[..., None]
                     + (opd.abs() * wp[..., None]) * (eps(lp.double()) + LN2 * tol_l)[..., None] + 2 * U * mo.abs() + 1e-300)
            got_o = o_acc.view(B, Nq, H, dh).permute(0, 2, 1, 3)
            w_nat = torch.logaddexp(la0.double(), lp.double())
            _check(l_acc, ml, tol_l, [w_nat, torch.maximum(la0, lp).double()], f"merge lse {name} block {bi}", f"merge-lse/{name}")
            _check(got_o, mo, tol_o, [oa * wp[..., None] + opd * wa[..., None], 0.5 * (oa + opd)], f"merge o {name} block {bi}", f"merge-o/{name}")
        # backward of each block, given the FULL lse and output
        out_full = o_acc.to(dtype)
        dq = torch.full((B * Nq, Wd), float("nan"), dtype=F32, device=DEV)
        fill = lambda i, nk: torch.full((B * nk, Wd), float("nan") if i == 0 else 0.0, dtype=F32, device=DEV)   # block 0 overwrites
        dks = [fill(i, nk) for i, nk in enumerate(Nks)]
        dvs = [fill(i, nk) for i, nk in enumerate(Nks)]
        dq_ref = torch.zeros((B, H, Nq, dh), dtype=torch.float64, device=DEV)
        dq_tol = torch.zeros_like(dq_ref)
        dq_wr = [torch.zeros_like(dq_ref) for _ in range(3)]
        for bi, (blk, nk) in enumerate(zip(blocks, Nks)):
            k2, v2 = blk[:, :Wd], blk[:, Wd:2 * Wd]
            ops.attention_cross_bwd(q2, k2, v2, out_full, do, l_acc, dq, dks[bi], dvs[bi], B, Nq, nk, H, dh, scale, accumulate=(bi > 0))
            Gk, Rk, Tk, Wk, Gv, Rv, Tv, Wv = [], [], [], [[], [], []], [], [], [], [[]]
            for b in range(B):
                for h in range(H):
                    sl = slice(h * dh, (h + 1) * dh)
                    q = q2.view(B, Nq, Wd)[b, :, sl].double()
                    k = k2.reshape(B, nk, Wd)[b, :, sl].double()
                    v = v2.reshape(B, nk, Wd)[b, :, sl].double()
                    og = out_full.view(B, Nq, Wd)[b, :, sl].double()
                    dg = do.view(B, Nq, Wd)[b, :, sl].double()
                    lg = l_acc[b, h].double()
                    rq, rk, rv, parts = _bwd_ref(q, k, v, og, dg, lg, scale)
                    tols, _ = _bwd_tol(q, k, v, og, dg, lg, scale, parts, (rq, rk, rv), pu, U)
                    wn = _bwd_ref(q, k, v, og, dg, lg, scale, delta="none")
                    wt = _bwd_ref(q, k, v, og, dg, lg, scale, smode="twice")
                    wd = _bwd_ref(q, k, v, og, dg, lg, scale, drop_q=True)
                    dq_ref[b, h] += rq
                    dq_tol[b, h] += tols[0] + 2 * U * dq_ref[b, h].abs()
                    for acc, w in zip(dq_wr, (wn[0], wt[0], rq * 0 if bi == 2 else rq)):
                        acc[b, h] += w
                    mult = 1.0
                    Gk.append(dks[bi].view(B, nk, Wd)[b, :, sl].double()), Rk.append(mult * rk), Tk.append(mult * tols[1] + 2 * U * rk.abs())
                    Gv.append(dvs[bi].view(B, nk, Wd)[b, :, sl].double()), Rv.append(mult * rv), Tv.append(mult * tols[2] + 2 * U * rv.abs())
                    for i, w in enumerate((wn[1], wt[1], wd[1])):
                        Wk[i].append(mult * w)
                    Wv[0].append(mult * wd[2])
            _check(torch.cat(Gk), torch.cat(Rk), torch.cat(Tk), [torch.cat(w) for w in Wk], f"cross_bwd dK {name} block {bi}", f"dk/{name}")
            _check(torch.cat(Gv), torch.cat(Rv), torch.cat(Tv), [torch.cat(w) for w in Wv], f"cross_bwd dV {name} block {bi}", f"dv/{name}")
        _check(dq.view(B, Nq, H, dh).permute(0, 2, 1, 3), dq_ref, dq_tol, dq_wr, f"cross_bwd dQ accumulated {name}", f"dq/{name}")


@gpu
def test_ring_cross_bwd_accumulates_into_dk_dv():
    """accumulate = 1 adds onto dk / dv as well: a second, accumulating call doubles an overwriting one up to one fp32 rounding"""
    ops = _ops()
    B, Nq, Nk, H, dh = 1, 70, 90, 2, 64
    Wd = H * dh
    g = _gen(77, DEV)
    q = torch.randn((B * Nq, Wd), generator=g, device=DEV).bfloat16()
    kv = torch.randn((B * Nk, 2 * Wd), generator=g, device=DEV).bfloat16()
    do = torch.randn((B * Nq, Wd), generator=g, device=DEV).bfloat16()
    o, lse = ops.attention_cross_fwd(q, kv[:, :Wd], kv[:, Wd:], B, Nq, Nk, H, dh, 0.125)
    bufs = [torch.full((B * n, Wd), float("nan"), dtype=F32, device=DEV) for n in (Nq, Nk, Nk)]
    ops.attention_cross_bwd(q, kv[:, :Wd], kv[:, Wd:], o, do, lse, *bufs, B, Nq, Nk, H, dh, 0.125, accumulate=False)
    once = [t.clone() for t in bufs]
    ops.attention_cross_bwd(q, kv[:, :Wd], kv[:, Wd:], o, do, lse, *bufs, B, Nq, Nk, H, dh, 0.125, accumulate=True)
    for a, t in zip(once, bufs):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        assert torch.equal(t, 2 * a), "x + x is exact in fp32"


@gpu
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_ring_one_hot_rows_merge_keeps_exactly_one_block(dtype):
    """one-hot rows whose key lies in one of three key blocks: every other block's lse is more than 150 below, so the merge must return that
    block's output and lse unchanged, bit for bit, whatever the order of the blocks"""
    ops = _ops()
    B, H, dh, N = 2, 2, 64, 200
    scale = dh ** -0.5
    qkv, _, pi, cq = _onehot_operands(dtype, B, N, H, dh, 5, DEV, scale)
    x = qkv.view(B, N, 3, H, dh)
    Wd = H * dh
    q2 = x[:, :, 0].reshape(B * N, Wd).contiguous()
    cuts = [0, 70, 134, 200]
    outs = []
    for a, e in zip(cuts[:-1], cuts[1:]):
        k2 = x[:, a:e, 1].reshape(B * (e - a), Wd).contiguous()
        v2 = x[:, a:e, 2].reshape(B * (e - a), Wd).contiguous()
        outs.append(ops.attention_cross_fwd(q2, k2, v2, B, N, e - a, H, dh, scale))
    lses = torch.stack([l for _, l in outs])                                                  # [3, B, H, N]
    owner = (pi[None] >= torch.tensor(cuts[:-1], device=DEV).view(3, 1, 1, 1)).sum(0) - 1
    top2 = lses.topk(2, dim=0)
    assert torch.equal(top2.indices[0], owner) and float((top2.values[0] - top2.values[1]).min()) > 150.0, "premise: lse gap > 150"
    for order in ((0, 1, 2), (2, 0, 1)):
        o_acc = torch.empty((B * N, Wd), dtype=F32, device=DEV)
        l_acc = torch.empty((B, H, N), dtype=F32, device=DEV)
        for n, bi in enumerate(order):
            ops.attention_merge(o_acc, l_acc, outs[bi][0], outs[bi][1], B, N, H, dh, first=(n == 0))
        want_o = torch.stack([o.float().view(B, N, H, dh) for o, _ in outs])                   # [3, B, N, H, dh]
        sel = owner.permute(0, 2, 1)[None, ..., None].expand(1, B, N, H, dh)
        assert torch.equal(o_acc.view(B, N, H, dh), torch.gather(want_o, 0, sel)[0])
        assert torch.equal(l_acc, top2.values[0])
    if dtype == BF:
        vg = torch.gather(x[:, :, 2].permute(0, 2, 1, 3), 2, pi[..., None].expand(-1, -1, -1, dh))
        assert torch.equal(o_acc.view(B, N, H, dh).permute(0, 2, 1, 3), vg.float()), "merged o[i] = v[pi(i)]"


# ============================================================================================== variable aggregation
@gpu
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V,R,D,dh,peaked", [(3, 24, 64, 32, False), (5, 1000, 1024, 64, False), (2, 333, 768, 64, False), (7, 130, 256, 128, False),
                                             (1, 50, 192, 64, False), (1, 1000, 1024, 64, False), (6, 500, 512, 64, True)])
def test_varagg_vs_fp64(dtype, V, R, D, dh, peaked):
    """softmax over the V variables of each token row with one shared query: all fp32 VALU arithmetic (natural-log units, P not rounded),
    outputs rounded once.  e = (dh + 8) U scale sum|k||q| + 4 U (1 + |s - lse|) is the relative error of a probability."""
    ops = _ops()
    g = _gen(V * 1000 + R + D, DEV)
    H, scale = D // dh, dh ** -0.5
    ou = UB if dtype == BF else U
    kv = torch.randn((V, R, 2, H, dh), generator=g, device=DEV)
    qv = torch.randn((D,), generator=g, device=DEV)
    if peaked:                       # variable 2 takes nearly all the weight in every row, the others still count
        kv[2, :, 0] += 1.2 * qv.view(1, H, dh) * math.sqrt(dh) / qv.view(H, dh).norm(dim=-1, keepdim=True)
    kv = kv.reshape(V * R, 2 * D).to(dtype)
    dout = (torch.randn((R, D), generator=g, device=DEV) * torch.exp2(torch.randint(-4, 3, (R, 1), generator=g, device=DEV).float())).to(dtype)
    out, lse = ops.varagg_fwd(kv, qv, V, R, D, dh, scale)
    dkv, dq = ops.varagg_bwd(kv, qv, out, lse, dout, V, R, D, dh, scale)
    s32, _ = _c32(scale)
    k, v = kv.double().view(V, R, 2, H, dh).unbind(2)
    q = qv.double().view(1, 1, H, dh)

    def fwd(keep):
        s = (k[:keep] * q).sum(-1) * s32
        l = torch.logsumexp(s, 0)
        p = torch.exp(s - l)
        return (p[..., None] * v[:keep]).sum(0).reshape(R, D), l, p, s
    ro, rl, p, s = fwd(V)
    if peaked:
        assert float((p[2] > 0.9).double().mean()) > 0.5, "premise: a peaked variable"
    es = (dh + 8) * U * s32 * (k.abs() * q.abs()).sum(-1)
    e = es + 4 * U * (1 + (s - rl).abs()) + (V + 4) * U
    pv = (p[..., None] * v.abs()).sum(0).reshape(R, D)
    t = ((p * e)[..., None] * v.abs()).sum(0).reshape(R, D) + ((p * e).sum(0)[..., None].expand(R, H, dh).reshape(R, D) + (V + 4) * U) * pv
    tol_l = (p * es).sum(0) + (V + 8) * U + 4 * U * rl.abs() + 4 * U * s.abs().max(0).values
    if V > 1:
        wo, wl, _, _ = fwd(V - 1)
        _check(out, ro, t + ou * (ro.abs() + t), [wo], f"varagg out V={V} R={R}", f"varagg-o/{'bf16' if dtype == BF else 'fp32'}")
        _check(lse, rl, tol_l, [wl, rl * LOG2E], f"varagg lse V={V} R={R}", f"varagg-lse/{'bf16' if dtype == BF else 'fp32'}")
    else:                            # one variable: p = 1, out = v up to (the rounding of) 1 / 1, lse = s
        _check(out, ro, t + ou * (ro.abs() + t), [ro * (1 + 4 * ou) + 4 * ou], f"varagg out V=1 R={R}", None)
        _check(lse, rl, tol_l, [rl * LOG2E + 1e-3], f"varagg lse V=1 R={R}", None)
    # backward: the function of the lse and out it is given
    lg, og, dg = lse.double(), out.double().view(R, H, dh), dout.double().view(R, H, dh)

    def bwd(delta_on=True, sc=s32):
        pp = torch.exp(s - lg)
        dp = (dg[None] * v).sum(-1)
        d = (dg * og).sum(-1) if delta_on else 0.0
        ds = pp * (dp - d) * sc
        dk = ds[..., None] * q
        dvv = pp[..., None] * dg[None]
        return torch.stack([dk, dvv], 2).reshape(V * R, 2 * D), (ds[..., None] * k).sum(0).reshape(R, D).sum(0), pp, dp, d, ds
    rkv, rdq, pp, dp, d, ds = bwd()
    ep = es + 4 * U * (1 + (s - lg).abs()) + 2 * U * lg.abs()
    edp = (dh + 8) * U * ((dg[None].abs() * v.abs()).sum(-1) + (dg.abs() * og.abs()).sum(-1)[None])
    a = ds.abs() * (ep + 4 * U) + pp * edp * s32
    tk = a[..., None] * q.abs()
    tv = (pp * ep)[..., None] * dg[None].abs()
    tkv = torch.stack([tk, tv], 2).reshape(V * R, 2 * D)
    tkv = tkv + ou * (rkv.abs() + tkv) + 2 * U * rkv.abs() + 1e-300
    tdq = (a[..., None] * k.abs()).sum(0).reshape(R, D).sum(0) + (R + V + dh + 16) * U * (ds.abs()[..., None] * k.abs()).sum(0).reshape(R, D).sum(0) + 1e-300
    if V > 1:
        wkv, wdq = bwd(delta_on=False)[:2]
        wkv2, wdq2 = bwd(sc=s32 * s32)[:2]
        tag = "bf16" if dtype == BF else "fp32"
        _check(dkv, rkv, tkv, [wkv, wkv2], f"varagg dkv V={V} R={R}", f"varagg-dkv/{tag}")
        _check(dq, rdq, tdq, [wdq, wdq2], f"varagg dq V={V} R={R}", f"varagg-dq/{tag}")
    else:                            # p = 1: dp - delta is the difference of two fp32 dot products of the same terms, dv = dO exactly
        _check(dkv, rkv, tkv, [bwd(delta_on=False)[0]], f"varagg dkv V=1 R={R}", None)
        assert bool((dq.double().abs() <= tdq).all())
        assert torch.equal(_bits(dkv.view(R, 2, D)[:, 1].contiguous()), _bits(dout)) or dtype == F32


# ============================================================================================== host-side edges
@gpu
def test_empty_batch_returns_early():
    """B = 0: torch hands out NULL data pointers for empty tensors; every attention entry point returns without a launch"""
    ops = _ops()
    N, H, dh = 50, 2, 64
    for dtype in (BF, F32):
        qkv = torch.empty((0, 3 * H * dh), dtype=dtype, device=DEV)
        o, lse = ops.attention_fwd(qkv, 0, N, H, dh, 0.125)
        assert o.shape == (0, H * dh) and lse.shape == (0, H, N)
        do = torch.empty((0, H * dh), dtype=dtype, device=DEV)
        d = ops.attention_bwd(qkv, o, do, lse, 0, N, H, dh, 0.125)
        assert d.shape == qkv.shape
        if dtype == BF:
            d, part = ops.attention_bwd(qkv, o, do, lse, 0, N, H, dh, 0.125, want_colsum=True)
            assert d.shape == qkv.shape and part.shape == (0, 2 * H * dh)
        q = torch.empty((0, H * dh), dtype=dtype, device=DEV)
        oc, lc = ops.attention_cross_fwd(q, q, q, 0, N, N, H, dh, 0.125)
        f = torch.empty((0, H * dh), dtype=F32, device=DEV)
        ops.attention_cross_bwd(q, q, q, oc, q, lc, f, f, f, 0, N, N, H, dh, 0.125, accumulate=False)
        ops.attention_merge(f, lc, oc, lc, 0, N, H, dh, first=True)
    torch.cuda.synchronize()


@gpu
def test_refusals_stay_refusals():
    """head dims outside {32, 64, 128}, misaligned pointers, cross_* leading dimensions below H dh or not a multiple of 8, bwd_colsum where
    _supported says 0: an error code and message, no launch (the outputs keep their fill)"""
    ops = _ops()
    from UCF_VIT._hip import lib as L
    lib = L.load()
    B, N, H = 2, 40, 2
    for dh in (16, 48, 96, 256):
        qkv = torch.zeros((B * N, 3 * H * dh), dtype=BF, device=DEV)
        with pytest.raises(RuntimeError, match="head dim"):
            ops.attention_fwd(qkv, B, N, H, dh, 0.1)
        with pytest.raises(RuntimeError, match="head dim"):
            ops.attention_bwd(qkv, qkv[:, :H * dh].contiguous(), qkv[:, :H * dh].contiguous(), torch.zeros((B, H, N), device=DEV), B, N, H, dh, 0.1)
    dh = 64
    Wd = H * dh
    buf = torch.zeros((B * N * 3 * Wd + 8,), dtype=BF, device=DEV)
    mis = buf[1:1 + B * N * 3 * Wd].view(B * N, 3 * Wd)                      # 2 bytes off a 16-byte boundary
    with pytest.raises(RuntimeError, match="aligned"):
        ops.attention_fwd(mis, B, N, H, dh, 0.125)
    q = torch.zeros((B * N, Wd + 8), dtype=BF, device=DEV)
    kv = torch.zeros((B * N, 2 * Wd + 8), dtype=BF, device=DEV)
    odd = torch.zeros((B * N, Wd + 4), dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="row strides"):                   # leading dimension below H * dh
        ops.attention_cross_fwd(q[:, :Wd - 8], kv[:, :Wd - 8], kv[:, :Wd - 8], B, N, N, H + 1, dh, 0.125)
    with pytest.raises(RuntimeError, match="row strides"):                   # not a multiple of 8 elements
        ops.attention_cross_fwd(odd[:, :Wd], kv[:, :Wd], kv[:, Wd:2 * Wd], B, N, N, H, dh, 0.125)
    f = torch.full((B * N, Wd), 7.0, dtype=F32, device=DEV)
    o = torch.zeros((B * N, Wd), dtype=BF, device=DEV)
    l = torch.zeros((B, H, N), dtype=F32, device=DEV)
    with pytest.raises(RuntimeError, match="row strides"):
        ops.attention_cross_bwd(odd[:, :Wd], kv[:, :Wd], kv[:, Wd:2 * Wd], o, o, l, f, f, f, B, N, N, H, dh, 0.125, accumulate=False)
    torch.cuda.synchronize()
    assert float((f - 7.0).abs().max()) == 0.0
    # bwd_colsum where _supported says 0 (streaming shapes): called on the C ABI directly, ops would not ask for it
    for n_, dh_, dt_ in ((300, 64, BF), (40, 128, BF), (40, 64, F32)):
        assert not ops.attention_bwd_colsum_supported(B, n_, H, dh_, dt_)
        qkv = torch.zeros((B * n_, 3 * H * dh_), dtype=dt_, device=DEV)
        o = torch.zeros((B * n_, H * dh_), dtype=dt_, device=DEV)
        lse = torch.zeros((B, H, n_), dtype=F32, device=DEV)
        dqkv = torch.full_like(qkv, 7.0)
        part = torch.full((B, 2 * H * dh_), 7.0, dtype=F32, device=DEV)
        rc = lib.ucfvit_attention_bwd_colsum(qkv.data_ptr(), o.data_ptr(), o.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), lse.data_ptr(),
                                             part.data_ptr(), B, n_, H, dh_, 0.125, ops.dt(qkv), torch.cuda.current_stream().cuda_stream)
        assert rc != 0
        with pytest.raises(RuntimeError, match="column sums"):
            L.check(rc, "ucfvit_attention_bwd_colsum")
        torch.cuda.synchronize()
        assert float((dqkv.float() - 7.0).abs().max()) == 0.0 and float((part - 7.0).abs().max()) == 0.0
