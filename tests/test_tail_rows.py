"""The class-row tail of a classification ViT: the last Block computed for token 0 of every sequence only (HF.TailBlockFn).

1. csrc/attention_rows.hip (one query per batch element and head) against the float64 reference of the dense formulas restricted to that
   query, element by element, with the bound structure of tests/test_attention_ops.py (_fwd_tol / _bwd_tol, U = 2^-24, UB = 2^-8).  The
   kernels are plain fp32 VALU arithmetic: P is never rounded to an MFMA operand (pu = U), the row sum is taken from the fp32 P (lu = 0),
   one key tile (T = 1); ou = UB (bf16) or U (fp32) is the one output rounding.  The same bounds must reject the wrong references of the
   dense tests (padding keys, a dropped key, natural-log units, delta left out, scale twice / never, dV not written).
   Underflow: with ONE query a dK / dV element is a single product p * (...), not a sum over 197 queries that its largest terms dominate,
   and p runs down to 2^-150 and below on the keys a peaked row ignores.  The relative bounds have no room for a result below the smallest
   normal number of the output format, so dK and dV get the format's absolute rounding floor, half the spacing of its subnormals: 2^-134
   (bf16), 2^-150 (fp32).  Where the dense kernel is compared, its P = v_exp_f32(...) is flushed to 0 below 2^-126 (a property of the
   instruction): that adds 2^-126 |dP - delta| scale |q| to dK and 2^-126 |dO| to dV there.  The Q third of dqkv
   away from the query row and the K half of the bias partial are exactly +0.  dK / dV also agree with the dense kernel's, given the same
   o, lse and a dO that is zero away from the query row, within the sum of the two kernels' bounds around the same float64 reference.
2. The pruned model against the dense model (UCFVIT_TAIL_ROWS switch), both judged against the float64 CPU oracle: logits, loss and every
   parameter gradient.  The two paths round independently (the class-row GEMMs run through other kernels), so at one element either can be
   the closer one, and a tensor of few elements (the loss is one number) has no error distribution of its own to compare against.  The
   margin is therefore the dense path's error scale pooled over all tensors of the case: R = max over tensors of max|dense - oracle| /
   max|oracle|, and per element err_pruned <= err_dense + R max|oracle| of that tensor.  (A first version of this test took the width
   from each tensor alone, max|dense - oracle| over that tensor: the worst of a second, independent draw exceeds the worst of the first
   half of the time, and it did, by 9 % on one fp32 LayerNorm gradient.)
   Measured on an MI355X, dense path against the oracle: R = 1.27e-2 (bf16, N 197), 1.13e-2 (bf16, N 25), 2.3e-6 (fp32, N 197), 1.3e-6
   (fp32, N 25); the pruned path's own worst relative error in the same runs: 1.69e-2, 1.20e-2, 1.9e-6, 1.2e-6; its worst error over a
   tensor was between 0.01 and 1.40 times the dense path's.
3. LayerNorm backward with a periodic dres equals the backward with that dres expanded with zeros, bit for bit.
4. Guards: forward_features / forward_intermediates return all tokens and never run the tail; subclasses (tensor parallel models) and a
   tensor_par_size > 1 take the dense path.  Activation checkpointing does NOT: tests/test_hip_models.py requires a checkpointed model to
   be bit-identical to the plain one, which a dense last Block next to a pruned one cannot be, so the tail recomputes inside itself and the
   test here asserts that bit identity for the tail (and that the dense switch still selects the dense Block under checkpointing)."""
import pytest
import torch

from test_attention_ops import (BF, DEV, F32, LN2, U, UB, _bits, _bwd_ref, _bwd_tol, _check, _fwd_ref, _fwd_tol, _fwd_wrongs, _operands, _ops,
                                _split)

gpu = pytest.mark.gpu

ROW_CASES = [(dt, N, dh) for dt in (BF, F32) for N in (49, 197, 257) for dh in (32, 64)]


def _cid(c):
    return f"{'bf16' if c[0] == BF else 'fp32'}-N{c[1]}-dh{c[2]}"


def _cat(parts):
    return torch.cat([p.reshape(-1) for p in parts])


@gpu
@pytest.mark.parametrize("case", ROW_CASES, ids=_cid)
def test_class_row_attention_vs_fp64(case):
    dtype, N, dh = case
    ops = _ops()
    B, H = 2, 3
    qrow = N // 3                      # not the first row, not a multiple of the kernels' row groups
    ou = UB if dtype == BF else U
    floor = 2.0 ** -134 if dtype == BF else 2.0 ** -150          # half the subnormal spacing of the output format
    pool = {k: ([], [], [], None) for k in ("o", "lse", "dq", "dk", "dv", "cs", "dk_dense", "dv_dense")}

    def add(key, got, ref, tol, wr):
        g, r, t, w = pool[key]
        g.append(got.double()), r.append(ref), t.append(tol.expand_as(ref))
        if w is None:
            pool[key] = (g, r, t, [[] for _ in wr])
        for lst, x in zip(pool[key][3], wr):
            lst.append(x)

    for fi, family in enumerate(("randn", "peaked", "offset")):
        qkv, do_full, scale = _operands(family, dtype, B, N, H, dh, 1000 * N + dh + fi, DEV)
        do = do_full.view(B, N, H * dh)[:, qrow].contiguous()                       # compact [B, H dh], mixed magnitude across the batch
        o, lse = ops.attention_rows_fwd(qkv, B, N, H, dh, scale, qrow)
        assert o.shape == (B, H * dh) and lse.shape == (B, H)
        dqkv, part = ops.attention_rows_bwd(qkv, o, do, lse, B, N, H, dh, scale, qrow, want_colsum=True)
        assert torch.equal(_bits(dqkv), _bits(ops.attention_rows_bwd(qkv, o, do, lse, B, N, H, dh, scale, qrow))), "colsum variant: same dqkv"
        assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(dqkv.float()).all()) and bool(torch.isfinite(lse).all())
        g5 = dqkv.view(B, N, 3, H, dh)
        others = torch.arange(N, device=DEV) != qrow
        assert int(_bits(g5[:, others, 0].contiguous()).count_nonzero()) == 0, "Q third away from the query row: +0 bit for bit"
        assert int(part[:, H * dh:].view(torch.int32).count_nonzero()) == 0, "K third of the bias sum: +0 bit for bit"
        # the dense kernels on the same problem: dO zero away from the query row, their own o and lse handed to both backward kernels
        od, lsed = ops.attention_fwd(qkv, B, N, H, dh, scale)
        dod = torch.zeros_like(od).view(B, N, H * dh)
        dod[:, qrow] = do
        dense = ops.attention_bwd(qkv, od, dod.view(B * N, H * dh), lsed, B, N, H, dh, scale).view(B, N, 3, H, dh)
        o_in = od.view(B, N, H * dh)[:, qrow].contiguous()
        lse_in = lsed[:, :, qrow].contiguous()
        mine = ops.attention_rows_bwd(qkv, o_in, do, lse_in, B, N, H, dh, scale, qrow).view(B, N, 3, H, dh)
        dpu = UB if dtype == BF else U                                               # the dense kernels round P and dS to MFMA operands
        for b in range(B):
            for h in range(H):
                q, k, v = _split(qkv, B, N, H, dh, b, h)
                q1 = q[qrow:qrow + 1]
                ro, rl, P = _fwd_ref(q1, k, v, scale)
                to, tl = _fwd_tol(q1, k, v, scale, ro, rl, P, U, 0.0, ou, 1)
                wr = _fwd_wrongs(q1, k, v, scale, N, 32)
                sl = slice(h * dh, (h + 1) * dh)
                add("o", o[b:b + 1, sl], ro, to, [w[0] for w in wr])
                add("lse", lse[b:b + 1, h], rl, tl, [w[1] for w in wr] + [rl * LN2])
                og, dg, lg = o[b:b + 1, sl].double(), do[b:b + 1, sl].double(), lse[b:b + 1, h].double()
                rq, rk, rv, parts = _bwd_ref(q1, k, v, og, dg, lg, scale)
                tols, raw = _bwd_tol(q1, k, v, og, dg, lg, scale, parts, (rq, rk, rv), U, ou)
                w_none = _bwd_ref(q1, k, v, og, dg, lg, scale, delta="none")
                w_tw = _bwd_ref(q1, k, v, og, dg, lg, scale, smode="twice")
                w_nv = _bwd_ref(q1, k, v, og, dg, lg, scale, smode="never")
                w_nat = _bwd_ref(q1, k, v, og, dg, lg * LN2, scale)
                g = g5[b, :, :, h]
                add("dq", g[qrow:qrow + 1, 0], rq, tols[0], [w_none[0], w_tw[0], w_nv[0]])
                add("dk", g[:, 1], rk, tols[1] + floor, [w_none[1], w_tw[1], w_nv[1]])
                add("dv", g[:, 2], rv, tols[2] + floor, [torch.zeros_like(rv), w_nat[2]])
                add("cs", part[b, sl], rq[0], raw[0][0] + (N + 8) * U * rq[0].abs() + 1e-300, [w_none[0][0], w_tw[0][0], w_nv[0][0]])
                # identical inputs to both kernels: one float64 reference, each kernel inside its own bound around it
                ogd, lgd = o_in[b:b + 1, sl].double(), lse_in[b:b + 1, h].double()
                _, rk2, rv2, parts2 = _bwd_ref(q1, k, v, ogd, dg, lgd, scale)
                t_mine, _ = _bwd_tol(q1, k, v, ogd, dg, lgd, scale, parts2, (rk2[:1], rk2, rv2), U, ou)
                t_dense, _ = _bwd_tol(q1, k, v, ogd, dg, lgd, scale, parts2, (rk2[:1], rk2, rv2), dpu, ou)
                P2, dS2, d2 = parts2
                s32 = float(torch.tensor(scale, dtype=torch.float32))
                flush_k = 2.0 ** -126 * s32 * ((dg @ v.T - d2[:, None]).abs().T @ q1.abs())       # [N, dh]
                flush_v = 2.0 ** -126 * dg.abs().expand(N, dh)
                add("dk_dense", mine[b, :, 1, h], dense[b, :, 1, h].double(), t_mine[1] + t_dense[1] + 2 * floor + flush_k,
                    [w_tw[1] if family != "offset" else w_none[1]])
                add("dv_dense", mine[b, :, 2, h], dense[b, :, 2, h].double(), t_mine[2] + t_dense[2] + 2 * floor + flush_v, [torch.zeros_like(rv2)])
    for key, (got, ref, tol, wrongs) in pool.items():
        got, ref, tol = _cat(got), _cat(ref), _cat(tol)
        wr = [_cat(w) for w in wrongs]
        wr = [w for w in wr if not torch.equal(w, ref)]
        _check(got, ref, tol, wr, f"{key} rows N={N} dh={dh} {_cid(case)}")


@gpu
@pytest.mark.parametrize("dtype,rows_b,period,D", [(BF, 5, 7, 64), (BF, 3, 197, 1024), (F32, 3, 50, 1024), (BF, 450, 7, 192), (F32, 4, 1, 96)],
                         ids=lambda x: str(x).replace("torch.", ""))
@pytest.mark.parametrize("colsum", [False, True], ids=["plain", "colsum"])
def test_layernorm_bwd_periodic_dres_bit_for_bit(dtype, rows_b, period, D, colsum):
    """rows = rows_b * period (450 * 7 rows: the grid-stride loop runs more than once); dres for rows 0, period, 2 period, ..."""
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(rows_b * period + D)
    rows = rows_b * period
    x = torch.randn((rows, D), generator=g, device=DEV).to(dtype)
    dy = torch.randn((rows, D), generator=g, device=DEV).to(dtype)
    gamma = torch.randn(D, generator=g, device=DEV).to(dtype)
    beta = torch.zeros(D, device=DEV).to(dtype)
    dres = torch.randn((rows_b, D), generator=g, device=DEV).to(dtype)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, beta, 1e-6)
    dense = torch.zeros((rows, D), dtype=dtype, device=DEV)
    dense[::period] = dres
    csA = torch.full((D,), float("nan"), device=DEV) if colsum else None
    csB = torch.full((D,), float("nan"), device=DEV) if colsum else None
    dxA, dgA, dbA = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dres=dense, dx_colsum=csA)
    dxB, dgB, dbB = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dres=dres, dx_colsum=csB, dres_period=period)
    assert torch.equal(_bits(dxA), _bits(dxB))
    assert torch.equal(dgA.view(torch.int32), dgB.view(torch.int32)) and torch.equal(dbA.view(torch.int32), dbB.view(torch.int32))
    if colsum:
        assert torch.equal(csA.view(torch.int32), csB.view(torch.int32))
    dx0, _, _ = ops.layernorm_bwd(dy, x, gamma, mean, rstd)
    assert not torch.equal(_bits(dx0), _bits(dxB)), "premise: dres changes dx"


# ============================================================================================== the model, pruned against dense
def _model_case(kw, B, seed, dtype, monkeypatch):
    """-> {name: (oracle float64, dense, pruned)} for logits, loss and every parameter gradient"""
    from UCF_VIT.simple.arch import VIT
    from UCF_VIT._hip import functional as HF
    from oracle import ucf_vit_ref as R
    from det_weights import det_state_dict, det_tensor
    ref = R.VIT(**kw)
    sd = det_state_dict(ref, seed)
    ref.load_state_dict(sd)
    ref = ref.double()
    x = det_tensor((B, kw["in_chans"], *kw["img_size"]), seed + 1)
    y = torch.arange(B) % kw["num_classes"]
    out_ref = ref(x.double())
    loss_ref = torch.nn.CrossEntropyLoss()(out_ref, y)
    loss_ref.backward()
    res = {"logits": [out_ref.detach()], "loss": [loss_ref.detach().reshape(1)]}
    for n, p in ref.named_parameters():
        res["grad " + n] = [p.grad.detach()]
    calls = []
    orig = HF.TailBlockFn.apply
    monkeypatch.setattr(HF.TailBlockFn, "apply", lambda *a: (calls.append(1), orig(*a))[1])
    for tail in (False, True):
        monkeypatch.setattr(HF, "TAIL_ROWS", tail)
        m = VIT(**kw)
        m.load_state_dict(sd)
        m = m.to(DEV)
        m.set_compute_dtype(dtype)
        assert m.tail_rows_applies() == tail
        n0 = len(calls)
        out = m(x.to(DEV), ["red", "green", "blue"][:kw["in_chans"]])
        loss = HF.cross_entropy(out, y.to(DEV))
        loss.backward()
        HF.flush_wgrads()
        torch.cuda.synchronize()
        assert len(calls) - n0 == (1 if tail else 0), "the switch selects the path"
        res["logits"].append(out.detach().double().cpu())
        res["loss"].append(loss.detach().double().cpu().reshape(1))
        for n, p in m.named_parameters():
            assert p.grad is not None, n
            res["grad " + n].append(p.grad.detach().double().cpu())
    return res


MODEL_CASES = [
    dict(img_size=[224, 224], patch_size=16, in_chans=3, num_classes=7, embed_dim=192, depth=2, num_heads=3),      # N = 197, dh 64
    dict(img_size=[32, 48], patch_size=8, in_chans=3, num_classes=5, embed_dim=192, depth=2, num_heads=6),         # N = 25 (odd), dh 32
]


@gpu
@pytest.mark.parametrize("kw", MODEL_CASES, ids=["N197-dh64", "N25-dh32"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_pruned_model_vs_dense_model_vs_oracle(kw, dtype, monkeypatch):
    res = _model_case(kw, 3, 31, dtype, monkeypatch)
    R = max(float((dense - ref).abs().max()) / float(ref.abs().max()) for ref, dense, _ in res.values())
    print(f"TAIL R (dense path, worst relative error over tensors) = {R:.3e}")
    assert R <= (0.1 if dtype == BF else 1e-3), "premise: the dense path itself is close to the oracle"
    worst = 0.0
    for name, (ref, dense, pruned) in res.items():
        e_d, e_p = (dense - ref).abs(), (pruned - ref).abs()
        scale = float(ref.abs().max())
        print(f"TAIL {name}: dense max err {float(e_d.max()):.3e} pruned max err {float(e_p.max()):.3e} max|ref| {scale:.3e}")
        worst = max(worst, float(e_p.max()) / scale)
        assert bool(torch.isfinite(pruned).all()), name
        bad = e_p > e_d + R * scale
        assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {bad.numel()} elements of the pruned path are further from the oracle than "
                                     f"the dense path's error there plus {R * scale:.3e}; worst pruned error {float(e_p.max()):.3e}")
    print(f"TAIL worst relative error of the pruned path over tensors: {worst:.3e}")


# ============================================================================================== guards
def _small_vit(cls=None, **extra):
    from UCF_VIT.simple.arch import VIT
    kw = dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=64, depth=2, num_heads=2)
    kw.update(extra)
    return (cls or VIT)(**kw)


def test_tail_applies_only_to_the_plain_classifier(monkeypatch):
    """no GPU: which models may prune their last Block"""
    from UCF_VIT._hip import functional as HF
    from UCF_VIT.simple import arch as SA
    from UCF_VIT.simple.building_blocks import apply_activation_checkpointing
    from UCF_VIT.fsdp import arch as FA
    monkeypatch.setattr(HF, "TAIL_ROWS", True)
    assert _small_vit().tail_rows_applies()
    assert not _small_vit(class_token=False).tail_rows_applies(), "no class token: pooling reads every row"
    assert not _small_vit(num_classes=None).tail_rows_applies(), "no head"
    assert not _small_vit(FA.VIT).tail_rows_applies(), "the tensor-parallel model class"
    m = _small_vit()
    m.tensor_par_size = 2
    assert not m.tail_rows_applies(), "tensor parallelism"
    m = _small_vit()
    assert apply_activation_checkpointing(m) == 2
    assert m.tail_rows_applies(), "recompute stays on the tail (its own recompute mode)"
    m = _small_vit(SA.SAP)
    assert not m.tail_rows_applies(), "a subclass whose head reads every token"
    monkeypatch.setattr(HF, "TAIL_ROWS", False)
    assert not _small_vit().tail_rows_applies(), "the switch"


@gpu
def test_dense_paths_return_all_tokens_and_never_run_the_tail(monkeypatch):
    from UCF_VIT._hip import functional as HF
    from UCF_VIT.simple.arch import UNETR
    from UCF_VIT.simple.building_blocks import apply_activation_checkpointing
    monkeypatch.setattr(HF, "TAIL_ROWS", True)
    calls = []
    orig = HF.TailBlockFn.apply
    monkeypatch.setattr(HF.TailBlockFn, "apply", lambda *a: (calls.append(1), orig(*a))[1])
    V = ["red", "green", "blue"]
    x = torch.randn(2, 3, 32, 32, device=DEV)
    m = _small_vit().to(DEV)
    assert m(x, V).shape == (2, 5) and len(calls) == 1
    feats = m.forward_features(x, V, None)
    assert feats.shape == (2, 17, 64) and len(calls) == 1, "forward_features: all tokens, dense"
    assert torch.equal(m.forward_head(feats), m.forward_head(m.forward_features(x, V, None)))
    # activation checkpointing: the tail with its own recompute, bit-identical to the plain tail; the dense switch still holds
    grads = []
    for ckpt in (False, True):
        torch.manual_seed(5)
        m2 = _small_vit().to(DEV)
        if ckpt:
            apply_activation_checkpointing(m2)
        n0 = len(calls)
        out = m2(x, V)
        out.sum().backward()
        HF.flush_wgrads()
        assert out.shape == (2, 5) and len(calls) == n0 + 1
        grads.append([out.detach()] + [p.grad.detach().clone() for p in m2.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads)), "checkpointed tail == plain tail, bit for bit"
    monkeypatch.setattr(HF, "TAIL_ROWS", False)
    n0 = len(calls)
    m2(x, V)
    assert len(calls) == n0, "UCFVIT_TAIL_ROWS=0 under checkpointing: dense"
    monkeypatch.setattr(HF, "TAIL_ROWS", True)
    calls[:] = [1]
    m3 = _small_vit().to(DEV)
    m3.tensor_par_size = 2
    assert m3(x, V).shape == (2, 5) and len(calls) == 1, "tensor parallelism: dense"
    un = UNETR(num_classes=4, linear_decoder=False, feature_size=4, skip_connection=True, allow_torch_decoder=True, img_size=[32, 32, 16], patch_size=8,
               in_chans=1, embed_dim=96, depth=4, num_heads=3, class_token=False, twoD=False).to(DEV)
    f, taps = un.forward_intermediates(torch.randn(2, 1, 32, 32, 16, device=DEV), None, None, indices=un.skip_indices)
    assert f.shape == (2, 32, 96) and all(t.shape[0] == 2 for t in taps) and len(calls) == 1, "forward_intermediates: all tokens, dense"
