"""Sequence parallelism (new capability; no reference implementation exists — SURVEY.md F4): P=2 ranks, each holding half of the
tokens, must reproduce the unsharded Block: outputs / input gradients are the token shards, parameter gradients sum to the
unsharded ones.  Two processes share the one GPU; the all-to-alls go through gloo (host-staged) in the test."""
import os
import sys
from functools import partial

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, rel_err


def _sp_worker(rank, world, port, dtype_name, tol, q):
    for p in (os.path.join(ROOT, "ucf-vit_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from UCF_VIT.simple import building_blocks as SB
        from UCF_VIT.fsdp.seq_parallel import SeqParallelBlock
        from oracle import ucf_vit_ref as R
        from det_weights import det_state_dict, det_tensor
        dtype = getattr(torch, dtype_name)
        D, H, B, N = 128, 4, 2, 96
        ref = R.Block(D, H, 4.0, True, partial(torch.nn.LayerNorm, eps=1e-6))
        sd = det_state_dict(ref, 61)
        ref.load_state_dict(sd)
        x = det_tensor((B, N, D), 62)
        gy = det_tensor((B, N, D), 63)
        xr = x.clone().requires_grad_(True)
        yr = ref(xr)
        yr.backward(gy)
        blk = SB.Block(D, H, qkv_bias=True, norm_layer=partial(SB.LayerNorm, eps=1e-6))
        blk.load_state_dict(sd)
        blk = blk.to("cuda:0")
        SB.set_compute_dtype(blk, dtype)
        sp = SeqParallelBlock(blk, dist.group.WORLD)
        Nl = N // world
        sl = slice(rank * Nl, (rank + 1) * Nl)
        xl = x[:, sl].contiguous().to("cuda:0").requires_grad_(True)
        y = sp(xl)
        y.backward(gy[:, sl].contiguous().to("cuda:0", y.dtype))
        bad = []
        if rel_err(y.float(), yr[:, sl]) >= tol:
            bad.append("y")
        if rel_err(xl.grad.float(), xr.grad[:, sl]) >= tol:
            bad.append("gx")
        for (k, p), (_, pr) in zip(blk.named_parameters(), ref.named_parameters()):
            g = p.grad.detach().float().cpu()
            dist.all_reduce(g)                                  # partial sums over the token shards
            if rel_err(g, pr.grad) >= tol:
                bad.append(k)
        q.put((rank, bad))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name,tol", [("float32", 1e-3), ("bfloat16", 5e-2)])
def test_seq_parallel_block_equals_unsharded(dtype_name, tol):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29560 + (0 if dtype_name == "float32" else 1)
    procs = [ctx.Process(target=_sp_worker, args=(r, 2, port, dtype_name, tol, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, bad in res:
        assert not bad, f"SP rank {rank}: mismatch in {bad}"


# ---------------------------------------------------------------------------------------------- cross-block attention + merge (one process)
@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name,tol", [("float32", 1e-4), ("bfloat16", 2e-2)])
@pytest.mark.parametrize("B,Nq,Nk_blocks,H,dh", [(2, 96, (64, 100), 3, 64), (1, 300, (256, 128, 77), 2, 32), (1, 130, (130,), 1, 128)])
def test_cross_block_attention_and_merge(dtype_name, tol, B, Nq, Nk_blocks, H, dh):
    """the ring building blocks: attention of Nq queries against key blocks held in OTHER buffers, folded by the log-sum-exp merge,
    equals softmax(QK^T / sqrt(dh)) V over the concatenated keys; the per-block backward, given the FULL log-sum-exp and output,
    accumulates exactly the full gradients (fp32 accumulators).
    The per-element bounds and the exact cases of these kernels live in tests/test_attention_ops.py."""
    from UCF_VIT._hip import ops
    dtype = getattr(torch, dtype_name)
    dev = "cuda"
    gen = torch.Generator().manual_seed(Nq * 7 + dh)
    W = H * dh
    qbuf = torch.randn(B * Nq, W + 64, generator=gen).to(dtype).to(dev)           # padded rows: the kernels take leading dimensions
    q = qbuf[:, :W]
    blocks = [torch.randn(B * nk, 2 * W, generator=gen).to(dtype).to(dev) for nk in Nk_blocks]
    do = torch.randn(B * Nq, W, generator=gen).to(dtype).to(dev)
    o_acc = torch.empty(B * Nq, W, dtype=torch.float32, device=dev)
    lse = torch.empty(B, H, Nq, dtype=torch.float32, device=dev)
    for i, (kv, nk) in enumerate(zip(blocks, Nk_blocks)):
        o_i, lse_i = ops.attention_cross_fwd(q, kv[:, :W], kv[:, W:], B, Nq, nk, H, dh, dh ** -0.5)
        ops.attention_merge(o_acc, lse, o_i, lse_i, B, Nq, H, dh, first=(i == 0))
    out = o_acc.to(dtype)
    # fp32 reference over the concatenated keys
    qf = q.float().view(B, Nq, H, dh).permute(0, 2, 1, 3).clone().requires_grad_(True)
    kf = [b_[:, :W].float().view(B, nk, H, dh).permute(0, 2, 1, 3).clone().requires_grad_(True) for b_, nk in zip(blocks, Nk_blocks)]
    vf = [b_[:, W:].float().view(B, nk, H, dh).permute(0, 2, 1, 3).clone().requires_grad_(True) for b_, nk in zip(blocks, Nk_blocks)]
    s = (qf @ torch.cat(kf, dim=2).transpose(-1, -2)) * dh ** -0.5
    ref = (torch.softmax(s, dim=-1) @ torch.cat(vf, dim=2)).permute(0, 2, 1, 3).reshape(B * Nq, W)
    ref.backward(do.float())
    assert rel_err(out.float(), ref.detach()) < tol
    ref_lse = torch.logsumexp(s.detach(), dim=-1) * 1.4426950408889634
    assert float((lse - ref_lse).abs().max()) < (1e-3 if dtype == torch.float32 else 2e-2)
    dq = torch.empty(B * Nq, W, dtype=torch.float32, device=dev)
    for i, (kv, nk) in enumerate(zip(blocks, Nk_blocks)):
        dk = torch.full((B * nk, W), 0.5, dtype=torch.float32, device=dev)           # accumulate = True adds to what is there
        dv = torch.full((B * nk, W), -0.25, dtype=torch.float32, device=dev)
        ops.attention_cross_bwd(q, kv[:, :W], kv[:, W:], out, do, lse, dq, dk, dv, B, Nq, nk, H, dh, dh ** -0.5, accumulate=(i > 0))
        if i == 0:            # the first call overwrote
            pass
        else:
            dk -= 0.5
            dv += 0.25
        gk = kf[i].grad.permute(0, 2, 1, 3).reshape(B * nk, W)
        gv = vf[i].grad.permute(0, 2, 1, 3).reshape(B * nk, W)
        assert rel_err(dk, gk) < tol, f"dk block {i}"
        assert rel_err(dv, gv) < tol, f"dv block {i}"
    assert rel_err(dq, qf.grad.permute(0, 2, 1, 3).reshape(B * Nq, W)) < tol


# ---------------------------------------------------------------------------------------------- UNETR encoder, 2-D sequence parallelism
def _unetr_sp_worker(rank, world, port, dtype_name, tol, ulysses, q):
    for p in (os.path.join(ROOT, "ucf-vit_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from UCF_VIT.fsdp.arch import UNETR
        from UCF_VIT.fsdp.seq_parallel import make_seq_parallel_groups, gather_tokens
        from UCF_VIT.simple.arch import UNETR as UNETR1
        from det_weights import det_state_dict, det_tensor
        dtype = getattr(torch, dtype_name)
        img = [128, 128, 128]                                    # p 16 -> 8 x 8 x 8 = 512 tokens; 12 heads like the 512x512x128 config
        kw = dict(img_size=img, patch_size=16, in_chans=1, embed_dim=384, depth=4, num_heads=12, class_token=False, twoD=False, num_classes=4,
                  linear_decoder=False, feature_size=16, skip_connection=True)
        base = UNETR1(**kw)
        sd = det_state_dict(base, 71)
        base.load_state_dict(sd)
        base = base.to("cuda:0")
        base.set_compute_dtype(dtype)
        x = det_tensor((1, 1, *img), 72).to("cuda:0")
        gy = [det_tensor((1, 512, 384), 73 + i).to("cuda:0") for i in range(4)]
        feats_r, taps_r = base.forward_intermediates(x, None, None, indices=base.skip_indices)
        (sum((a.float() * g_).sum() for a, g_ in zip([feats_r] + taps_r, gy)) / world).backward()
        spg = make_seq_parallel_groups([list(range(world))], 12, ulysses_size=ulysses)
        m = UNETR(seq_par_size=world, seq_par_group=spg, shard_decoder=False, **kw)     # (the whole-model leg below checks the REPLICATED decoder)
        m.load_state_dict(sd)
        m = m.to("cuda:0")
        m.set_compute_dtype(dtype)
        feats, taps = m.forward_intermediates(x, None, None, indices=m.skip_indices)
        n = 512 // world
        sl = slice(rank * n, (rank + 1) * n)
        sum((a.float() * g_[:, sl]).sum() for a, g_ in zip([feats] + taps, gy)).backward()
        bad = []
        full = [gather_tokens(t.detach(), spg) for t in [feats] + taps]
        for name, a, b in zip(["feats", "tap0", "tap1", "tap2"], full, [feats_r] + taps_r):
            if tuple(a.shape) != (1, 512, 384) or rel_err(a.float(), b.detach().float()) >= tol:
                bad.append(name)
        enc = ("blocks.", "patch_embed.", "norm.", "pos_embed")
        for (k, p), (_, pr) in zip(m.named_parameters(), base.named_parameters()):
            if not k.startswith(enc):
                continue
            g = p.grad.detach().float().cpu()
            dist.all_reduce(g)                                   # sum over the token shards ...
            g /= world                                           # ... the mean over ranks = gradient of the mean objective
            if rel_err(g, pr.grad.detach().float().cpu()) >= tol:
                bad.append(k)
        if world == 2 and dtype_name == "float32":
            # the whole model: token shards gathered (differentiably) in front of the replicated convolutional decoder (HIP kernels)
            from UCF_VIT._hip import functional as HF
            lab = (det_tensor((1, *img), 79) * 2).long().clamp_(0, 3).to("cuda:0")
            for mod in (base, m):
                for p_ in mod.parameters():
                    p_.grad = None
            assert base.hip_decoder() and m.hip_decoder()
            lo_r = base(x, None)
            HF.dice_ce(lo_r, lab).backward()
            lo = m(x, None)
            HF.dice_ce(lo, lab).backward()
            if rel_err(lo.detach().float(), lo_r.detach().float()) >= 2e-2:
                bad.append("whole-model logits")
            for (k, p), (_, pr) in zip(m.named_parameters(), base.named_parameters()):
                g = p.grad.detach().float().cpu()
                dist.all_reduce(g)                               # the MEAN over the group (what HipDataParallel takes) is right for the
                g /= world                                       # sharded encoder AND the replicated decoder: GatherTokensFn scales by P
                rn = ((g - pr.grad.detach().float().cpu()).norm() / pr.grad.detach().float().norm().cpu().clamp_min(1e-20)).item()
                if rn >= 0.25:                                   # bf16 decoder: gradient noise of tests/test_unetr_decoder_model.py
                    bad.append("whole-model grad " + k + f" {rn:.3f}")
        q.put((rank, bad, (spg.pu, spg.pr)))
        dist.barrier()
    except Exception as e:      # the parent must not sit out its queue timeout on a GPU box
        import traceback
        q.put((rank, ["EXCEPTION " + repr(e) + " " + traceback.format_exc()[-1500:]], (-1, -1)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world,ulysses,dtype_name,tol", [(2, 1, "float32", 1e-3), (4, 2, "float32", 1e-3), (2, 1, "bfloat16", 6e-2)])
def test_unetr_encoder_sequence_parallel_equals_unsharded(world, ulysses, dtype_name, tol):
    """UNETR encoder (3-D patch embedding, 12 heads, taps) at N = 512 tokens sharded over `world` ranks that share the one GPU (gloo,
    host-staged transport): pure ring (P_u = 1) and the 2-D grid P_u = 2 x P_r = 2 — the layout class of 12 heads on 8 GPUs (4 x 2) —
    reproduce the unsharded features, taps and parameter gradients (pure Ulysses: test_seq_parallel_block_equals_unsharded; all five
    combinations incl. P_u = 4 passed on the box when this test was written)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29570 + world * 3 + ulysses + (0 if dtype_name == "float32" else 40)
    procs = [ctx.Process(target=_unetr_sp_worker, args=(r, world, port, dtype_name, tol, ulysses, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    for _ in range(world):
        res.append(q.get(timeout=300))
        if res[-1][2] == (-1, -1):                  # a rank raised: do not wait for the others (they hang in a collective)
            for p in procs:
                p.kill()
            raise AssertionError(f"SP rank {res[-1][0]}: {res[-1][1]}")
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, bad, grid in res:
        assert grid == (ulysses, world // ulysses)
        assert not bad, f"SP rank {rank}: mismatch in {bad}"


# ------------------------------------------------------------------------- the whole sequence-parallel UNETR under HipDataParallel
def _unetr_sp_ddp_worker(rank, world, port, shard, q):
    for p in (os.path.join(ROOT, "ucf-vit_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from UCF_VIT.fsdp.arch import UNETR
        from UCF_VIT.fsdp.seq_parallel import make_seq_parallel_groups
        from UCF_VIT.simple.arch import UNETR as UNETR1
        from UCF_VIT._hip import functional as HF
        from UCF_VIT._hip.ddp import HipDataParallel
        from UCF_VIT.utils.misc import configure_optimizer
        from det_weights import det_state_dict, det_tensor
        img = [64, 64, 64]                                       # p 16 -> 64 tokens, 32 per rank
        kw = dict(img_size=img, patch_size=16, in_chans=1, embed_dim=192, depth=4, num_heads=6, class_token=False, twoD=False, num_classes=4,
                  linear_decoder=False, feature_size=16, skip_connection=True)
        x = det_tensor((1, 1, *img), 82).to("cuda:0")
        lab = (det_tensor((1, *img), 83) * 2).long().clamp_(0, 3).to("cuda:0")
        base = UNETR1(**kw)
        sd = det_state_dict(base, 81)
        base.load_state_dict(sd)
        base = base.to("cuda:0")
        opt_b = configure_optimizer(base, 1e-3, 0.9, 0.95, 0.0)
        lo_b = base(x, None)
        loss_b = HF.dice_ce(lo_b, lab)
        loss_b.backward()
        ref_logits, ref_loss = lo_b.detach().float().clone(), loss_b.item()
        g_ref = {k: p.grad.detach().float().cpu().clone() for k, p in base.named_parameters()}
        opt_b.step()
        w_ref = {k: p.detach().float().cpu().clone() for k, p in base.named_parameters()}
        spg = make_seq_parallel_groups([list(range(world))], 6)  # 2 ranks: pure Ulysses; 4 ranks: the 2 x 2 Ulysses x ring grid
        m = UNETR(seq_par_size=world, seq_par_group=spg, shard_decoder=shard, **kw)
        m.load_state_dict(sd)
        m = m.to("cuda:0")
        assert m.shard_decoder() == shard
        ddp = HipDataParallel(m, bucket_mb=0.25)                 # the documented reducer: a MEAN over the dp x sp ranks (here 1 x P)
        opt = configure_optimizer(m, 1e-3, 0.9, 0.95, 0.0)
        bad = []
        if shard:
            # every rank decodes its X-slab (halo exchange + group-wide normalisation statistics) and holds its slab of the logits
            from UCF_VIT.fsdp import sharded_decoder as SD
            lo = ddp(x, None)
            ref_lo = SD.local_slab(ref_logits, spg, 2)
            if tuple(lo.shape) != tuple(ref_lo.shape):
                bad.append(f"local logits shape {tuple(lo.shape)} vs {tuple(ref_lo.shape)}")
            else:
                rn = ((lo.detach().float() - ref_lo.float()).norm() / ref_lo.float().norm()).item()
                if rn >= 3e-2:
                    bad.append(f"local logits {rn:.4f}")
            loss = SD.sharded_dice_ce(lo, SD.local_slab(lab, spg, 1), spg)
            if abs(loss.item() - ref_loss) > 2e-2 * abs(ref_loss):
                bad.append(f"loss {loss.item():.5f} vs {ref_loss:.5f}")
            loss.backward()
        else:
            HF.dice_ce(ddp(x, None), lab).backward()
        torch.cuda.synchronize()
        for k, p in m.named_parameters():
            g = p.grad.detach().float().cpu()
            rn = ((g - g_ref[k]).norm() / g_ref[k].norm().clamp_min(1e-20)).item()
            if rn >= 0.25:                                       # bf16 decoder on both sides: the gradient noise of tests/test_unetr_decoder_model.py
                bad.append(f"grad {k} {rn:.3f}")
        # the scale is what the advisor's finding was about: a gradient 1/P of the right size would show as a norm ratio of 0.5
        enc = [k for k in g_ref if k.startswith(("blocks.", "patch_embed.", "pos_embed"))]
        ratio = sum(m.get_parameter(k).grad.float().norm().item() for k in enc) / sum(g_ref[k].norm().item() for k in enc)
        if not 0.9 < ratio < 1.1:
            bad.append(f"encoder gradient scale {ratio:.3f}")
        opt.step()
        for k, p in m.named_parameters():
            d = (p.detach().float().cpu() - w_ref[k]).abs().max().item()
            if d > 2.5e-3:                                       # Adam's first step moves every weight by ~lr = 1e-3 in the gradient's sign
                bad.append(f"weight {k} {d:.2e}")
        w = m._ucf_store.flat_p.detach().cpu()
        w0 = w.clone()
        dist.broadcast(w0, 0)
        q.put((rank, bad, bool(torch.equal(w, w0))))
        dist.barrier()
    except Exception as e:
        import traceback
        q.put((rank, ["EXCEPTION " + repr(e) + " " + traceback.format_exc()[-1500:]], False))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world,shard", [(2, False), (2, True), (4, True)])
def test_unetr_sequence_parallel_under_data_parallel_steps_like_the_unsharded_model(world, shard):
    """fsdp.arch.UNETR(seq_par_size=P) wrapped in HipDataParallel — the reducer DESIGN §7 prescribes — takes one optimiser step: every
    gradient and every post-step weight matches the unsharded model, and all ranks end with identical weights.
    shard=False: the decoder replicated behind an all-gather (round-2 advisor finding: the encoder gradients came out 1 / P).
    shard=True: the decoder SHARDED into X-slabs (fsdp/sharded_decoder.py: halo exchange in front of every 3x3x3 layer, instance-norm
    statistics and the Dice + CE sums all-reduced over the group): local logits = the unsharded logits' slab, same loss, same gradients —
    on 2 ranks (two token slabs each) and on 4 ranks (the 2 x 2 Ulysses x ring grid, one token slab each)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_unetr_sp_ddp_worker, args=(r, world, 29611 + 2 * world + int(shard), shard, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    for _ in range(world):
        res.append(q.get(timeout=300))
        if res[-1][1] and res[-1][1][0].startswith("EXCEPTION"):
            for p in procs:
                p.kill()
            raise AssertionError(f"rank {res[-1][0]}: {res[-1][1]}")
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, bad, same in res:
        assert not bad, f"rank {rank}: {bad}"
        assert same, "ranks diverged after the step"


def _sharded_stats_worker(rank, world, port, q):
    for p in (os.path.join(ROOT, "ucf-vit_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from UCF_VIT._hip import ops
        from UCF_VIT.fsdp import sharded_decoder as SD
        from UCF_VIT.fsdp.seq_parallel import _PlainGroup
        spg = _PlainGroup(dist.group.WORLD)
        g = torch.Generator(device="cuda:0").manual_seed(4)
        # a volume whose channels have |mean| / sigma ~1300: bf16 steps are 8 wide at 1024, so 1024 + 8 with p = 1 % (sigma ~0.8); the two
        # slabs get different means (the second one 8 higher in channels 8..15) so that the fold's between-slab term matters too
        x = 1024.0 + 8.0 * (torch.rand(2, 16, 32, 16, 16, device="cuda:0", generator=g) < 0.01).float()
        x[:, 8:, 16:] += 8.0
        x = x.permute(0, 2, 3, 4, 1).contiguous().bfloat16()          # channels-last [B, X, Y, Z, C]
        m_ref, r_ref = ops.instnorm_cl_stats(x, 1e-5)                    # single rank, whole volume
        xl = SD.local_slab(x, spg, 1).contiguous()
        mean, rstd = SD.sharded_instnorm_stats(xl, 1e-5, spg)
        ref64 = x.double().reshape(2, -1, 16)
        sd = ref64.var(1, unbiased=False).sqrt()
        bad = []
        if float((rstd.double() / r_ref.double() - 1).abs().max()) >= 1e-3:
            bad.append(f"rstd {float((rstd.double() / r_ref.double() - 1).abs().max()):.2e}")
        if float(((mean.double() - m_ref.double()).abs() / sd).max()) >= 1e-3:
            bad.append("mean")
        y = SD.sharded_instnorm_act(xl, None, 1e-5, 1.0, spg)
        yr = SD.local_slab(ops.instnorm_cl_apply(x, m_ref, r_ref, None, 1.0), spg, 1)
        if float((y.float() - yr.float()).abs().max()) >= 0.15:            # two bf16 steps (1 / 16) of values up to ~10 sigma
            bad.append("y")
        q.put((rank, bad))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_instance_norm_statistics_keep_their_variance_when_the_mean_is_large():
    """ShardedInstNormActFn's group-wide statistics (2 gloo ranks on the one GPU) against single-rank ucfvit_instnorm_cl_stats of the whole
    volume on channels whose |mean| is ~1300 standard deviations: averaging E[x^2] over the ranks and subtracting mean^2 in fp32 loses the
    variance there; the parallel-variance fold keeps it"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sharded_stats_worker, args=(r, 2, 29597, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, bad in res:
        assert not bad, f"rank {rank}: {bad}"
