"""The backward glue of UCF_VIT/_hip/functional.py against float64: where each parameter gradient is written, whether it accumulates, which
launch carries it and when that launch is issued (WgradQueue, params.grad_target, _ln_bwd's mixed-state route, the stream column-sum
hand-over, the UCFVIT_* A/B switches).  The kernels have their own per-element tests; this module tests the state machine above them.

One model, the smallest at which every branch is live: VIT 32x32 / patch 8 (17 tokens), embed_dim 128, 2 heads, batch 8 = 136 token rows.
136 rows and extents >= 128 make every dense weight gradient groupable (ucfvit_gemm_grouped), width 128 gives the weights a transposed
shadow, the tail Block's three compact gradients (proj, fc1, fc2: 8 rows) wait beside the dense ones and go out one by one, depth 9
passes MAX_PROBLEMS once; a Block has 2 + 1 + 2 + 2 = 7 output tiles.  The reference is oracle.ucf_vit_ref.VIT in float64 on the CPU.

Premises (a recorder around ops.wgrad_grouped, top-level calls only): the launch pattern of every routing state is the one the policy in
WgradQueue.end_block implies — bf16 default [32, 4]; _DEFER_WGRAD off [4] * 9; CUS = 9 [8, 20, 8] and CUS = 16 [12, 24] (CUS = 14 never
fills a round at these tile counts, see test_routing_full_rounds_flush_equals_plain_route: the tail Block's qkv gradient has 136 rows and
counts with the dense ones); with a flush listener [32, 4] in the first pass (Block count unknown) and [28, 8] in the second; a hooked or
foreign-.grad weight: its Block's end flushes; fp32 [] — nothing is pending when backward() returns, and in the default state every
p.grad is the flat-buffer view.

Tier A  canonical paths against the oracle, conftest.rel_err per tensor: fp32 depth 9 < 1e-3, bf16 depth 3 plain route < 5e-2, bf16 depth 9
        default < 5e-2.
Tier B  same arithmetic, different routing: against the plain route (bf16, depth 9, one launch of four problems per Block), rel_err < 1e-5
        per tensor (tests/test_gemm_ops.py::test_gemm_grouped: a problem gives the same bits whatever shares its launch).
Tier C  different arithmetic (the A/B switches, a frozen subset): both paths against the oracle at depth 3 with the rule of
        tests/test_tail_rows.py part 2: R = the default path's worst relative error pooled over tensors (premise R <= 0.1), per element
        err_variant <= err_default + R max|oracle|; fp32: 1e-3 against the oracle.  The qkv-bias arm that UCFVIT_BIAS_FROM_EPILOGUE gates exists
        only with qk_norm, which the oracle does not model: that arm runs against the reference fixture model_vit_qknorm.npz.
Hooks   a tensor hook on a parameter sees the finished gradient and what it returns reaches p.grad, on every pass: params.grad_target
        reports "no target" for a hooked parameter, so its gradient travels through autograd and its Block's launches go out before the
        Block's backward returns.

The stream column-sum hand-over has a model of its own: a second loss term reads the first Block's output, so that Block's output gradient
is a sum autograd formed and the published sums must be refused (Tier A tolerances against an oracle with the same second term).

Measured on an MI355X (worst conftest.rel_err over logits, loss and all gradients unless said otherwise):
Tier A  fp32 depth 9 1.65e-6; bf16 depth 3 plain route 1.21e-2 (blocks.0.attn.proj.bias); bf16 depth 9 default 2.16e-2 (blocks.6.norm2.weight;
        logits 1.20e-2, loss 2.3e-4): depth 9 stays under 5e-2, so the bf16 oracle comparison is kept at depth 9.
Tier B  every variant bit-equal to the plain route (rel_err 0): default, CUS 14 / 9 / 16, listener (both passes), checkpointing, accumulate
        onto zeros, two passes (2 x), foreign .grad (both halves, both parts), autograd.grad, HipDataParallel (both passes), two models.
Tier C  bf16 depth 3: R = 1.21e-2; worst relative error of the variants: group-off 1.21e-2 (bit-equal to the default path), bias-epilogue-off
        1.17e-2, gelu-deriv-off 1.31e-2, tail-rows-off 1.29e-2 (these three not bit-equal), frozen-third 1.17e-2 (bit-equal on what it
        computes).  fp32: bias-epilogue-off 1.17e-6, tail-rows-off 1.08e-6, frozen-third 1.17e-6.  qkv bias with qk_norm, error over
        max|reference| per third: fp32 <= 7.3e-7, bf16 <= 8.8e-3, switch on and off.
Tapped  fp32 1.08e-6, bf16 1.29e-2 (blocks.0.mlp.fc2.bias, the gradient at stake: 3.0e-7 and 6.0e-3).
Hooks   bit-equal to 0.5 x / 1 x / 2 x the plain route; the recorded norms equal the finished gradients' (2.246115, 0.2018560).
        Before grad_target refused hooked parameters the hook on blocks.1.mlp.fc1.weight read the flat buffer before the launch (norm 768 of
        the fill value 3 instead of 2.246) and flush() overwrote what the hook returned (1 x instead of 0.5 x after one pass).
"""
import functools
import socket

import pytest
import torch

from conftest import load_golden, rel_err
from det_weights import det_state_dict, det_tensor

gpu = pytest.mark.gpu
DEV = "cuda"
VARS = ["red", "green", "blue"]
BF, F32 = torch.bfloat16, torch.float32
KW = dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=128, num_heads=2)
B, SEED = 8, 61
DEEP, SHALLOW = 9, 3
SAME = 1e-5                     # tests/test_hip_models.py::test_deferred_weight_gradients...: the same gradient through another route


def _hf():
    from UCF_VIT._hip import functional as HF
    return HF


def _data(flip=False):
    x = det_tensor((B, 3, 32, 32), SEED + 1)
    return (x.flip(0) if flip else x), torch.arange(B) % KW["num_classes"]


@functools.lru_cache(maxsize=None)
def _oracle(depth):
    """-> (state dict, {name: float64 tensor} for logits, loss and every parameter gradient); built once per depth"""
    from oracle import ucf_vit_ref as R
    ref = R.VIT(depth=depth, **KW)
    sd = det_state_dict(ref, SEED)
    ref.load_state_dict(sd)
    ref = ref.double()
    x, y = _data()
    out = ref(x.double())
    loss = torch.nn.CrossEntropyLoss()(out, y)
    loss.backward()
    res = {"logits": out.detach(), "loss": loss.detach().reshape(1)}
    for n, p in ref.named_parameters():
        res["grad " + n] = p.grad.detach()
    return sd, res


class _Recorder:
    """counts the problems of every top-level ops.wgrad_grouped call (the function re-enters itself once per row count)"""

    def __init__(self, mp):
        HF = _hf()
        self.calls, self.depth = [], 0
        orig = HF.ops.wgrad_grouped

        def through(items):
            if self.depth == 0:
                self.calls.append(len(items))
            self.depth += 1
            try:
                return orig(items)
            finally:
                self.depth -= 1
        mp.setattr(HF.ops, "wgrad_grouped", through)

    def take(self):
        c, self.calls = self.calls, []
        return c


@pytest.fixture
def rec(monkeypatch):
    return _Recorder(monkeypatch)


def _model(depth, dtype, ckpt=False, **extra):
    from UCF_VIT.simple.arch import VIT
    m = VIT(depth=depth, **KW, **extra)
    m.load_state_dict(_oracle(depth)[0])
    m = m.to(DEV)
    m.set_compute_dtype(dtype)
    if ckpt:
        from UCF_VIT.simple.building_blocks import apply_activation_checkpointing
        assert apply_activation_checkpointing(m) == depth
    return m


def _loss(m, flip=False, wrap=None):
    x, y = _data(flip)
    out = m(x.to(DEV), VARS) if wrap is None else wrap(x.to(DEV), VARS, None)
    return out, _hf().cross_entropy(out, y.to(DEV))


def _collect(m, out, loss):
    assert not _hf().wgrads_pending(), "backward() has returned: nothing may wait in a queue"
    torch.cuda.synchronize()
    res = {"logits": out.detach().float().cpu(), "loss": loss.detach().float().cpu().reshape(1)}
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert p.grad is not None, n
            res["grad " + n] = p.grad.detach().float().cpu()
        else:
            assert p.grad is None, n
    return res


def _once(m):
    out, loss = _loss(m)
    loss.backward()
    return _collect(m, out, loss)


def _in_flat_buffer(m):
    st = m._ucf_store
    return all(p.grad is not None and p.grad.data_ptr() == st.flat_g.data_ptr() + 4 * o for p, o in zip(st.params, st.offsets))


@functools.lru_cache(maxsize=None)
def _plain(depth):
    """the plain route: bf16, every Block's four weight gradients as one grouped launch when its backward ends; run once per depth"""
    HF = _hf()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(HF, "_DEFER_WGRAD", False)
        r = _Recorder(mp)
        res = _once(_model(depth, BF))
        assert r.take() == [4] * depth
    return res


@functools.lru_cache(maxsize=None)
def _default(depth, dtype):
    """the default state at this depth and dtype; run once, shared by the tiers that compare against it"""
    with pytest.MonkeyPatch.context() as mp:
        r = _Recorder(mp)
        m = _model(depth, dtype)
        res = _once(m)
        calls = r.take()
        assert _in_flat_buffer(m), "default state: every gradient was written into the flat buffer and adopted as a view"
    return res, calls


def _vs_oracle(res, depth, tol, what):
    ref = _oracle(depth)[1]
    worst, worst_k = 0.0, None
    errs = {}
    for k, v in res.items():
        assert bool(torch.isfinite(v).all()), k
        errs[k] = rel_err(v, ref[k])
        if errs[k] > worst:
            worst, worst_k = errs[k], k
    print(f"ROUTING {what}: worst rel_err against the oracle {worst:.3e} ({worst_k}); logits {errs['logits']:.3e} loss {errs['loss']:.3e}")
    for k, e in errs.items():
        if e >= 0.5 * tol:
            print(f"ROUTING {what}:   {k} {e:.3e}")
    bad = {k: f"{e:.3e}" for k, e in errs.items() if not e < tol}
    assert not bad, f"{what}: rel_err >= {tol} against the oracle: {bad}"
    return worst


def _same(got, want, what, scale=None, keys=None):
    """got == scale * want per tensor to SAME (scale: a number or {key: number}, default 1)"""
    worst, equal = 0.0, True
    bad = {}
    for k in (keys if keys is not None else want):
        s = scale.get(k, 1.0) if isinstance(scale, dict) else (scale or 1.0)
        w = want[k] * s
        e = rel_err(got[k], w)
        worst = max(worst, e)
        equal = equal and torch.equal(got[k], w)
        if not e < SAME:
            bad[k] = f"{e:.3e}"
    print(f"ROUTING {what}: worst rel_err against the plain route {worst:.3e}, bit-equal: {equal}")
    assert not bad, f"{what}: differs from the plain route: {bad}"


def _grads(res):
    return [k for k in res if k.startswith("grad ")]


# ============================================================================================== Tier A
@gpu
def test_routing_fp32_depth9_vs_oracle(rec):
    m = _model(DEEP, F32)
    res = _once(m)
    assert rec.take() == [], "fp32 never enters the queue"
    assert _in_flat_buffer(m)
    _vs_oracle(res, DEEP, 1e-3, "A fp32 depth 9")


@gpu
def test_routing_bf16_depth3_plain_route_vs_oracle():
    _vs_oracle(_plain(SHALLOW), SHALLOW, 5e-2, "A bf16 depth 3 plain route")


@gpu
def test_routing_bf16_depth9_default_vs_oracle():
    res, calls = _default(DEEP, BF)
    assert calls == [32, 4], "28 dense and 4 tail problems when the ninth Block would pass MAX_PROBLEMS, the first Block when backward ends"
    _vs_oracle(res, DEEP, 5e-2, "A bf16 depth 9 default")


# ============================================================================================== Tier B
@gpu
def test_routing_default_state_equals_plain_route():
    res, calls = _default(DEEP, BF)
    assert calls == [32, 4]
    _same(res, _plain(DEEP), "B1 default (deferred, flush at MAX_PROBLEMS)")


FULL_ROUNDS = [(14, [32, 4]), (9, [8, 20, 8]), (16, [12, 24])]


@gpu
@pytest.mark.parametrize("cus,pattern", FULL_ROUNDS, ids=[f"cus{c}" for c, _ in FULL_ROUNDS])
def test_routing_full_rounds_flush_equals_plain_route(rec, monkeypatch, cus, pattern):
    """The flush when the fullest launch fills whole rounds (tiles >= 95 % of a multiple of CUS).  The tail Block queues 5 tiles of 8 rows
    (proj, fc1, fc2) and 2 tiles of 136 rows (its qkv gradient is dense: every token's keys and values), a dense Block 7 tiles of 136
    rows, so the fullest launch holds 2 + 7 k tiles after k dense Blocks.
    14 CUs: 9, 16, 23, 30, 37, 44, 51 tiles never reach 95 % of 14, 28, 28, 42, 42, 56, 56: the default pattern.
    9 CUs: 9 of 9 after the first dense Block (8 problems); then 7, 14, 21, 28 miss 9, 18, 27, 36 and 35 of 36 fills (20); 8 are left.
    16 CUs: 16 of 16 after two dense Blocks (12 problems); 7 ... 42 never reach 95 % of 16, 16, 32, 32, 48, 48: 24 are left."""
    monkeypatch.setattr(_hf().WgradQueue, "CUS", cus)
    res = _once(_model(DEEP, BF))
    assert rec.take() == pattern
    _same(res, _plain(DEEP), f"B2 CUS = {cus} (flush on full rounds)")


class _Listener:
    def __init__(self):
        self.calls = 0

    def poke(self):
        self.calls += 1


@gpu
def test_routing_flush_listener_pairs_the_last_blocks(rec):
    HF = _hf()
    m = _model(DEEP, BF)
    m._prepare()
    owner = _Listener()
    HF.add_wgrad_flush_listener(owner.poke, m._ucf_store)
    first = _once(m)
    assert rec.take() == [32, 4], "first pass: the Block count is not known yet"
    n1 = owner.calls
    assert n1 >= 2
    m.zero_grad()
    second = _once(m)
    assert rec.take() == [28, 8], "second pass: the last four Blocks go out two by two (2 and 0 Blocks to come)"
    assert owner.calls > n1
    _same(first, _plain(DEEP), "B3 flush listener, first pass")
    _same(second, _plain(DEEP), "B3 flush listener, second pass")


@gpu
def test_routing_checkpointed_blocks_equal_plain_route(rec):
    res = _once(_model(DEEP, BF, ckpt=True))
    assert rec.take() == [32, 4]
    _same(res, _plain(DEEP), "B4 activation checkpointing")


@gpu
def test_routing_accumulate_onto_zeros_equals_plain_route(rec):
    m = _model(DEEP, BF)
    _once(m)
    m.zero_grad(set_to_none=False)
    assert _in_flat_buffer(m) and not bool(m._ucf_store.flat_g.count_nonzero())
    rec.take()
    res = _once(m)
    assert rec.take() == [32, 4] and _in_flat_buffer(m)
    _same(res, _plain(DEEP), "B5 zero_grad(set_to_none=False), accumulate onto zeros")


@gpu
def test_routing_two_passes_accumulate_twice_the_gradient(rec):
    m = _model(DEEP, BF)
    _once(m)
    res = _once(m)
    assert rec.take() == [32, 4, 32, 4] and _in_flat_buffer(m)
    _same(res, _plain(DEEP), "B6 two passes without zero_grad", scale=2.0, keys=_grads(res))


@gpu
@pytest.mark.parametrize("parity", [0, 1], ids=["weights-foreign", "biases-foreign"])
def test_routing_foreign_grads_on_every_second_parameter(rec, parity):
    """parity 0: cls_token, every weight and every norm weight carry a .grad that is not the flat view, the biases do not: every LayerNorm
    is in mixed state, every queued weight gradient has no target (deferrable = False: one launch per Block).  parity 1: the other half;
    the weights keep their flat-buffer target, so the launches are the default state's."""
    m = _model(DEEP, BF)
    m._prepare()                                            # the flat store exists: a .grad set now is foreign to it
    named = list(m.named_parameters())
    foreign = {n: torch.zeros_like(p) for n, p in named[parity::2]}
    assert ("blocks.0.attn.qkv.weight" in foreign) == (parity == 0) and ("blocks.0.norm1.weight" in foreign) != ("blocks.0.norm1.bias" in foreign)
    for n, p in named:
        if n in foreign:
            p.grad = foreign[n]
    res = _once(m)
    assert rec.take() == ([4] * DEEP if parity == 0 else [32, 4])
    _same(res, _plain(DEEP), f"B7 foreign .grad on parameters {parity}::2")
    st = m._ucf_store
    for (n, p), o in zip(zip(st.names, st.params), st.offsets):
        if n in foreign:                                    # (the partner of a foreign parameter in a LayerNorm left the flat buffer as well)
            assert p.grad.data_ptr() != st.flat_g.data_ptr() + 4 * o, n
    # The accumulate flag mixed in as well: after a default pass every gradient is its flat view; half of them are then replaced by a copy.
    # In the second pass that half has no target and autograd adds to the copy, the other half accumulates in the kernels, and the two
    # parameters of every LayerNorm differ in both respects.
    m = _model(DEEP, BF)
    _once(m)
    assert _in_flat_buffer(m)
    for n, p in list(m.named_parameters())[parity::2]:
        p.grad = p.grad.clone()
    rec.take()
    res = _once(m)
    assert rec.take() == ([4] * DEEP if parity == 0 else [32, 4])
    _same(res, _plain(DEEP), f"B7 copies as .grad of parameters {parity}::2, second pass", scale=2.0, keys=_grads(res))


@gpu
def test_routing_autograd_grad_equals_plain_route(rec):
    m = _model(DEEP, BF)
    out, loss = _loss(m)
    named = list(m.named_parameters())
    grads = torch.autograd.grad(loss, [p for _, p in named])
    assert not _hf().wgrads_pending()
    torch.cuda.synchronize()
    assert rec.take() == [32, 4]
    assert all(p.grad is None for _, p in named)
    res = {"grad " + n: g.detach().float().cpu() for (n, _), g in zip(named, grads)}
    _same(res, _plain(DEEP), "B8 torch.autograd.grad", keys=_grads(res))


@gpu
def test_routing_hip_data_parallel_one_nccl_rank(rec, monkeypatch):
    """HipDataParallel on the nccl backend, fp32 transport: a bucket whose gradients are complete for autograd while weight gradients still
    wait in the queue is reduced by _after_wgrad_flush; the mean over one rank is the gradient itself"""
    import os
    import torch.distributed as dist
    from UCF_VIT._hip.ddp import HipDataParallel
    launched = []
    state = {"inside": False}
    orig_after, orig_launch = HipDataParallel._after_wgrad_flush, HipDataParallel._launch

    def after(self):
        state["inside"] = True
        try:
            return orig_after(self)
        finally:
            state["inside"] = False

    def launch(self, b):
        launched.append((b, state["inside"]))
        return orig_launch(self, b)
    monkeypatch.setattr(HipDataParallel, "_after_wgrad_flush", after)
    monkeypatch.setattr(HipDataParallel, "_launch", launch)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        m = _model(DEEP, BF)
        ddp = HipDataParallel(m, bucket_mb=0.5, reduce_dtype=torch.float32)
        assert len(ddp.buckets) >= 4 and ddp.reduce_dtype() == torch.float32
        results = []
        for i in range(2):
            out, loss = _loss(m, wrap=ddp)
            loss.backward()
            results.append(_collect(m, out, loss))
            assert rec.take() == ([32, 4] if i == 0 else [28, 8])
            assert sorted(b for b, _ in launched) == list(range(len(ddp.buckets))), "every bucket reduced exactly once per pass"
            assert any(inside for _, inside in launched), "no bucket waited for the weight-gradient queue"
            launched.clear()
            m.zero_grad()
        _same(results[0], _plain(DEEP), "B9 HipDataParallel, first pass")
        _same(results[1], _plain(DEEP), "B9 HipDataParallel, second pass")
    finally:
        dist.destroy_process_group()


@gpu
def test_routing_two_models_in_one_backward(rec):
    """each model has its own queue, end-of-backward callback and column-sum slot; model b sees the batch in reverse order"""
    b_alone = _model(DEEP, BF)
    out, loss = _loss(b_alone, flip=True)
    loss.backward()
    solo_b = _collect(b_alone, out, loss)
    rec.take()
    ma, mb = _model(DEEP, BF), _model(DEEP, BF)
    oa, la = _loss(ma)
    ob, lb = _loss(mb, flip=True)
    (la + lb).backward()
    ra, rb = _collect(ma, oa, la), _collect(mb, ob, lb)
    assert sorted(rec.take()) == [4, 4, 32, 32]
    assert _in_flat_buffer(ma) and _in_flat_buffer(mb)
    _same(ra, _plain(DEEP), "B10 two models, a")
    _same(rb, solo_b, "B10 two models, b")
    assert not torch.equal(ra["grad head.weight"], rb["grad head.weight"]), "premise: the two models compute different gradients"


# ============================================================================================== the stream column-sum hand-over
@functools.lru_cache(maxsize=None)
def _tapped_oracle():
    """the depth-3 model with a second loss term that reads the first Block's output: that Block's output gradient is the SUM of the next
    Block's dx and the tap's gradient, a tensor no LayerNorm backward produced"""
    from oracle import ucf_vit_ref as R
    ref = R.VIT(depth=SHALLOW, **KW)
    ref.load_state_dict(_oracle(SHALLOW)[0])
    ref = ref.double()
    x, y = _data()
    h = ref._pos_embed(ref.token_embeds(x.double()))
    taps = []
    for blk in ref.blocks:
        h = blk(h)
        taps.append(h)
    out = ref.head(ref.norm(h)[:, 0])
    w = det_tensor(taps[0].shape, SEED + 2)
    loss = torch.nn.CrossEntropyLoss()(out, y) + (taps[0] * w.double()).sum() / (taps[0].shape[0] * taps[0].shape[1])
    loss.backward()
    res = {"logits": out.detach(), "loss": loss.detach().reshape(1)}
    for n, p in ref.named_parameters():
        res["grad " + n] = p.grad.detach()
    return w, res


@gpu
@pytest.mark.parametrize("dtype,tol", [(F32, 1e-3), (BF, 5e-2)], ids=["fp32", "bf16"])
def test_routing_stream_colsum_is_refused_for_a_summed_gradient(dtype, tol):
    """Every LayerNorm-1 backward publishes the column sums of its dx for the Block before it (that Block's fc2 bias gradient).  Here the
    first Block's output has a second reader, so autograd hands it dx + the tap's gradient: the published sums belong to another tensor
    and must be refused, while the other Blocks take theirs.  Tolerances: Tier A's for this depth."""
    HF = _hf()
    w, ref = _tapped_oracle()
    m = _model(SHALLOW, dtype)
    x, y = _data()
    taken = []
    orig = HF._take_stream_colsum

    def through(q, dy2):
        cs = orig(q, dy2)
        taken.append(cs is not None)
        return cs
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(HF, "_BIAS_FROM_EPILOGUE", True)
        mp.setattr(HF, "_take_stream_colsum", through)
        m._prepare()
        h = m._pos_embed(m._embed_tokens(x.to(DEV), VARS), None)
        taps = []
        for blk in m.blocks:
            h = blk(h)
            taps.append(h)
        out = m.head(m.norm(h)[:, 0])
        loss = HF.cross_entropy(out, y.to(DEV)) + (taps[0].float() * w.to(DEV)).sum() / (B * taps[0].shape[1])
        loss.backward()
        res = _collect(m, out, loss)
    assert taken == [True, True, False], "backward order: blocks.2 (from the final norm), blocks.1 (from blocks.2), blocks.0 (a sum: refused)"
    errs = {k: rel_err(v, ref[k]) for k, v in res.items()}
    worst = max(errs, key=errs.get)
    print(f"ROUTING tapped {dtype}: worst rel_err against the oracle {errs[worst]:.3e} ({worst}); "
          f"blocks.0.mlp.fc2.bias {errs['grad blocks.0.mlp.fc2.bias']:.3e}")
    bad = {k: f"{e:.3e}" for k, e in errs.items() if not e < tol}
    assert not bad, bad


# ============================================================================================== Tier C
def _freeze_every_third(m):
    for i, (_, p) in enumerate(m.named_parameters()):
        if i % 3 == 0:
            p.requires_grad_(False)


VARIANTS = {
    "group-off": ("_GROUP_WGRAD", False),
    "bias-epilogue-off": ("_BIAS_FROM_EPILOGUE", False),
    "gelu-deriv-off": ("_GELU_SAVE_DERIV", False),
    "tail-rows-off": ("TAIL_ROWS", False),
    "frozen-third": None,
}


def _variant(name, dtype, rec, monkeypatch):
    HF = _hf()
    if VARIANTS[name] is not None:
        monkeypatch.setattr(HF, *VARIANTS[name])
    m = _model(SHALLOW, dtype)
    rec.take()                                              # (a shared baseline computed in this test went through the recorder too)
    if name == "frozen-third":
        _freeze_every_third(m)
        frozen = [n for i, (n, _) in enumerate(m.named_parameters()) if i % 3 == 0]
        assert "blocks.0.attn.qkv.weight" in frozen and "blocks.0.attn.qkv.bias" not in frozen and "blocks.0.attn.proj.bias" in frozen
    assert m.tail_rows_applies() == (name != "tail-rows-off")
    res = _once(m)
    calls = rec.take()
    if dtype == F32 or name == "group-off":
        assert calls == []
    elif name == "frozen-third":
        assert calls == [6], "two weights of every Block are frozen, two are queued"
    else:
        assert calls == [12]
    return res


@gpu
@pytest.mark.parametrize("name", list(VARIANTS))
def test_routing_switches_bf16_vs_default_vs_oracle(name, rec, monkeypatch):
    base, calls = _default(SHALLOW, BF)
    assert calls == [12]
    ref = _oracle(SHALLOW)[1]
    R = max(float((base[k].double() - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref)
    print(f"ROUTING C bf16 depth 3: R (default path, worst relative error over tensors) = {R:.3e}")
    assert R <= 0.1, "premise: the default path itself is close to the oracle"
    res = _variant(name, BF, rec, monkeypatch)
    assert set(res) <= set(ref) and (name == "frozen-third") == (len(res) < len(ref))
    worst, equal = 0.0, True
    for k, v in res.items():
        assert bool(torch.isfinite(v).all()), k
        e_d, e_v = (base[k].double() - ref[k]).abs(), (v.double() - ref[k]).abs()
        scale = float(ref[k].abs().max())
        worst = max(worst, float(e_v.max()) / scale)
        equal = equal and torch.equal(v, base[k])
        bad = e_v > e_d + R * scale
        assert not bool(bad.any()), (f"{name} {k}: {int(bad.sum())} of {bad.numel()} elements are further from the oracle than the default path's "
                                     f"error there plus {R * scale:.3e}; worst error {float(e_v.max()):.3e}, max|oracle| {scale:.3e}")
    print(f"ROUTING C bf16 {name}: worst relative error against the oracle {worst:.3e}; bit-equal to the default path: {equal}")


@gpu
@pytest.mark.parametrize("name", ["bias-epilogue-off", "tail-rows-off", "frozen-third"])
def test_routing_switches_fp32_vs_oracle(name, rec, monkeypatch):
    res = _variant(name, F32, rec, monkeypatch)
    _vs_oracle(res, SHALLOW, 1e-3, f"C fp32 {name}")


@gpu
@pytest.mark.parametrize("dtype,tol", [(F32, 1e-3), (BF, 5e-2)], ids=["fp32", "bf16"])
@pytest.mark.parametrize("epilogue", [True, False], ids=["epilogue", "epilogue-off"])
def test_routing_qkv_bias_with_qk_norm_under_the_bias_switch(dtype, tol, epilogue, monkeypatch):
    """with qk_norm the V third of the qkv bias gradient comes from the proj data-gradient epilogue, or (switch off, dense Blocks) from a
    column sum over dqkv; the fixture and the tolerances are those of tests/test_qk_norm_models.py::test_vit_vs_reference.  The gradient
    buffer is filled with a large number first: a third that no launch writes keeps it."""
    from UCF_VIT.simple.arch import VIT
    HF = _hf()
    monkeypatch.setattr(HF, "_BIAS_FROM_EPILOGUE", epilogue)
    g = load_golden("model_vit_qknorm.npz")
    m = VIT(qk_norm=True, img_size=[32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=64, depth=2, num_heads=2)
    sd = det_state_dict(m, 77)
    sd.update({k[2:]: v for k, v in g.items() if k.startswith("w.")})
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.set_compute_dtype(dtype)
    m._prepare()
    m._ucf_store.flat_g.fill_(1e6)
    loss = HF.cross_entropy(m(g["x"].to(DEV), VARS), g["labels"].to(DEV))
    loss.backward()
    assert not HF.wgrads_pending() and _in_flat_buffer(m)
    for k, p in m.named_parameters():
        if k.endswith("qkv.bias"):
            D = p.numel() // 3
            want = g["g." + k].double()
            for i, third in enumerate("QKV"):                     # rel_err of the whole tensor, reported third by third
                e = float((p.grad.double().cpu() - want)[i * D:(i + 1) * D].abs().max() / want.abs().max())
                print(f"ROUTING qk_norm {k} {third} third: error / max|reference| {e:.3e}")
                assert e < tol, (k, third)


# ============================================================================================== hooks
HOOKED = ("blocks.1.mlp.fc1.weight", "blocks.1.mlp.fc1.bias")


@gpu
def test_routing_tensor_hook_scales_the_gradient_on_every_pass(rec):
    plain = _plain(SHALLOW)
    rec.take()
    m = _model(SHALLOW, BF)
    params = dict(m.named_parameters())
    fired = {k: 0 for k in HOOKED}

    def halve(k):
        def hook(g):
            fired[k] += 1
            return g * 0.5
        return hook
    for k in HOOKED:
        params[k].register_hook(halve(k))
    res = _once(m)
    assert fired == {k: 1 for k in HOOKED}
    assert rec.take() == [8, 4], ("the tail Block waits for the next; the hooked weight of blocks.1 has no target, so that Block's end flushes "
                                  "both; blocks.0 goes out when backward ends")
    _same(res, plain, "hook g * 0.5, first pass", scale={"grad " + k: 0.5 for k in HOOKED})
    res = _once(m)
    assert fired == {k: 2 for k in HOOKED}, "the hook fires on every pass"
    assert rec.take() == [8, 4]
    scale = {k: 2.0 for k in _grads(res)}
    scale.update({"grad " + k: 1.0 for k in HOOKED})
    _same(res, plain, "hook g * 0.5, second pass without zero_grad", scale=scale, keys=_grads(res))


@gpu
def test_routing_tensor_hook_reads_the_finished_gradient(rec):
    plain = _plain(SHALLOW)
    m = _model(SHALLOW, BF)
    m._prepare()
    m._ucf_store.flat_g.fill_(3.0)          # what a hook would read if it were handed the flat view before the launch
    params = dict(m.named_parameters())
    norms = {k: [] for k in HOOKED}

    def watch(k):
        def hook(g):
            norms[k].append(g.float().norm())
        return hook
    for k in HOOKED:
        params[k].register_hook(watch(k))
    res = _once(m)
    _same(res, plain, "hook returning None", keys=_grads(res))
    for k in HOOKED:
        want = plain["grad " + k].double().norm().item()
        assert len(norms[k]) == 1
        got = norms[k][0].item()
        print(f"ROUTING hook returning None, {k}: recorded norm {got:.6e}, finished gradient {want:.6e}")
        assert abs(got - want) <= SAME * want, k


# ============================================================================================== CPU: queue policy with faked launches
@pytest.fixture
def fake(monkeypatch):
    HF = _hf()
    launches = []
    monkeypatch.setattr(HF.ops, "wgrad_grouped", lambda items: launches.append(len(items)))
    monkeypatch.setattr(HF.WgradQueue, "_arm", lambda self: None)       # (the autograd engine takes callbacks only inside a backward pass)
    monkeypatch.setattr(HF, "_DEFER_WGRAD", True)
    return launches


class _FakeStore:
    """what params.grad_target asks of a store"""

    def __init__(self, p):
        self.flat_g = torch.zeros(p.numel())
        p._ucf_slot = (self, 0, p.numel())

    def owns(self, p, o):
        return True

    def grad_view(self, p, o, n):
        return self.flat_g[o:o + n].view(p.shape)


def _problem(rows, n=384, k=128, stored=True):
    w = torch.nn.Parameter(torch.zeros(n, k))
    if stored:
        _FakeStore(w)
    return w, torch.zeros(rows, n), torch.zeros(rows, k)


def test_flush_sends_pending_items_in_chunks_of_at_most_32(fake):
    q = _hf().WgradQueue()
    q.items += [(None, None, None, False)] * 70
    q.owners += [None] * 70
    q.flush()
    assert fake == [32, 32, 6] and not q.items and not q.owners and q.tiles == 0 and q.tiles_by_rows == {}


def test_tiles_is_the_fullest_launch_not_the_sum(fake):
    q = _hf().WgradQueue()
    q.add(*_problem(8))                           # 2 tiles of 8 rows
    assert q.tiles == 2
    q.add(*_problem(136))                         # 2 tiles of 136 rows: a launch of their own
    assert q.tiles == 2 and q.tiles_by_rows == {8: 2, 136: 2}
    q.add(*_problem(136, 512, 300))               # 2 x 2 tiles
    assert q.tiles == 6 and q.tiles_by_rows == {8: 2, 136: 6}
    q.end_block()
    assert fake == [] and len(q.items) == 3, "all three have a target in the flat buffer: deferred"


def test_add_routes_by_the_three_states_of_grad_target(fake):
    """first write: the view goes to autograd; accumulate: nothing does; no target (no store, a foreign .grad, a tensor hook): a new tensor
    does, which autograd will read, so the Block's launches may not wait"""
    HF = _hf()
    from UCF_VIT._hip.params import grad_target
    q = HF.WgradQueue()
    w, dy, x = _problem(136)
    view = w._ucf_slot[0].grad_view(w, 0, w.numel())
    ret = q.add(w, dy, x)
    assert ret.data_ptr() == view.data_ptr() and q.items[-1][3] is False and q.owners[-1][0] is w and q.deferrable
    w.grad = view
    assert q.add(w, dy, x) is None and q.items[-1][3] is True and q.items[-1][2].data_ptr() == view.data_ptr() and q.owners[-1] is None
    q.end_block()
    assert fake == [] and q.deferrable
    w.grad = torch.zeros_like(w)                                   # foreign
    assert grad_target(w) == (None, False)
    ret = q.add(w, dy, x)
    assert ret.shape == w.shape and ret.data_ptr() != view.data_ptr() and q.items[-1][2].data_ptr() == ret.data_ptr()
    assert q.items[-1][3] is False and q.owners[-1] is None and not q.deferrable
    q.end_block()
    assert fake == [3] and q.deferrable and not q.items, "an add without a target: end_block flushes, and the next Block may defer again"
    w2, dy, x = _problem(136, stored=False)                        # no store at all
    q.add(w2, dy, x)
    assert not q.deferrable
    q.end_block()
    assert fake == [3, 1]
    w3, dy, x = _problem(136)
    handle = w3.register_hook(lambda g: None)                      # a hook reads what autograd is handed
    assert grad_target(w3) == (None, False)
    q.add(w3, dy, x)
    assert not q.deferrable
    q.end_block()
    assert fake == [3, 1, 1]
    handle.remove()
    out, acc = grad_target(w3)
    assert out is not None and acc is False, "hook removed: the flat-buffer target is back"


def test_take_stream_colsum_checks_the_tensor_and_clears_the_slot(monkeypatch):
    HF = _hf()
    monkeypatch.setattr(HF, "_BIAS_FROM_EPILOGUE", True)
    q = HF.WgradQueue()
    dx, cs = torch.zeros(4, 8), torch.ones(8)

    def take(dy2):
        q.stream_colsum = (dx, cs)
        got = HF._take_stream_colsum(q, dy2)
        assert q.stream_colsum is None, "cleared either way"
        return got
    assert take(dx) is cs
    assert take(dx.view(4, 8)) is cs, "another tensor object on the same memory is the same gradient"
    assert take(dx.clone()) is None, "another address"
    assert take(dx[:2]) is None, "another element count"
    assert take(dx.view(torch.int32)) is None, "another dtype"
    assert take(dx.view(8, 4)) is None, "another width"
    assert HF._take_stream_colsum(q, dx) is None, "empty slot"
    monkeypatch.setattr(HF, "_BIAS_FROM_EPILOGUE", False)
    assert take(dx) is None, "switched off"
