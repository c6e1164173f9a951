"""The UNETR geometry of the reference's basic_ct/unetr config (64^3 tile, patch 4, adaptive patching with fixed_length 729 -> a 9^3 token
grid, embed_dim 768, feature_size 16) built WITHOUT allow_torch_decoder: the whole convolutional decoder, including the resampling of dec1
(72^3 -> 64^3) and decoder2's pointwise transposed convolution, runs on the HIP kernels.  It is held against the SAME model and weights with
the decoder on torch's fp32 convolutions and nn.Upsample (allow_torch_decoder + force_torch_decoder).  Reference:
src/UCF_VIT/simple/arch.py:757-1113, 887-906, 942-943, 989-991.

Yardstick of the gradients (as in tests/test_unetr_decoder_model.py): through ~25 normalised layers at random initialisation the gradient is
sensitive to WHERE values are rounded to bf16 — torch's own fp32 decoder with bf16 rounding hooks at the convolution boundaries (what
autocast does in the reference's training script) moves the parameter gradients by several per cent of their norm against the pure fp32
run.  The HIP decoder rounds at comparable points, so it is held to that: against the fp32 gradients its error may be at most 1.25 x the
hooked torch run's in the median over the parameter tensors and 2.5 x (+ 1 %) for any single one.  The 1x1x1 projection of the one-channel
input inside encoder1 (every output channel is the same normalised map: its gradient is what the eps in rstd leaves of an exact
cancellation) gets an absolute floor of 6 % instead."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
VARS = ["ct_res1"]


class _RoundBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.bfloat16().float()

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().float()


def _bf16_boundary_hooks(m):
    hooks = []
    for mod in m.modules():
        if isinstance(mod, (torch.nn.Conv3d, torch.nn.ConvTranspose3d)):
            hooks.append(mod.register_forward_pre_hook(lambda md, inp: (_RoundBf16.apply(inp[0]),)))
            hooks.append(mod.register_forward_hook(lambda md, inp, out: _RoundBf16.apply(out)))
    return hooks


def _run(m, args, lab, decoder):
    from UCF_VIT._hip import functional as HF
    from UCF_VIT._hip.functional import flush_wgrads
    allow = m.allow_torch_decoder
    m.allow_torch_decoder = decoder == "torch"
    m.force_torch_decoder = decoder == "torch"
    try:
        for p in m.parameters():
            p.grad = None
        # torch's decoder on its native convolutions, not MIOpen: the same fp32 arithmetic without a kernel build for every new shape
        with torch.backends.cudnn.flags(enabled=decoder != "torch"):
            logits = m(*args)
            loss = HF.dice_ce(logits, lab)
            loss.backward()
        flush_wgrads()
        return logits.detach().float().contiguous(), loss.item(), {n: p.grad.detach().float().clone() for n, p in m.named_parameters() if p.grad is not None}
    finally:
        m.allow_torch_decoder, m.force_torch_decoder = allow, False


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


def _check_against_torch_decoder(m, args, lab, img):
    assert m.hip_decoder() and m.resamples_dec1() and not m.allow_torch_decoder
    lo_h, loss_h, g_h = _run(m, args, lab, "hip")
    assert tuple(lo_h.shape) == (lab.shape[0], 4, *img)
    lo_t, loss_t, g_t = _run(m, args, lab, "torch")
    assert _rel(lo_h, lo_t) < 3e-2
    assert abs(loss_h - loss_t) < 2e-2 * abs(loss_t)
    assert set(g_h) == set(g_t)
    hooks = _bf16_boundary_hooks(m)
    try:
        _, _, g_q = _run(m, args, lab, "torch")
    finally:
        for h in hooks:
            h.remove()
    ratios = []
    for n in g_h:
        assert g_h[n].shape == g_t[n].shape and torch.isfinite(g_h[n]).all(), n
        if g_t[n].norm() > 0:
            e_h, e_q = _rel(g_h[n], g_t[n]), _rel(g_q[n], g_t[n])
            if n == "encoder1.layer.conv3.conv.weight":
                assert e_h < max(6e-2, 2.5 * e_q + 1e-2), (n, e_h, e_q)
                continue
            assert e_h < 2.5 * e_q + 1e-2, (n, e_h, e_q)
            ratios.append(e_h / max(e_q, 1e-3))
    assert sorted(ratios)[len(ratios) // 2] < 1.25, sorted(ratios)
    assert _rel(g_h["out.conv.conv.weight"], g_t["out.conv.conv.weight"]) < 5e-3
    assert g_h["decoder2.transp_conv.conv.weight"].norm() > 0
    return lo_h, loss_h, g_h


def test_reference_geometry_decoder_on_hip_equals_torch_decoder():
    """B = 2, depth 4 (the encoder's depth is not what is tested), the reference's adaptive front end with positions from seq_ps"""
    from UCF_VIT.simple.arch import UNETR
    torch.manual_seed(0)
    m = UNETR(img_size=[64, 64, 64], patch_size=4, in_chans=1, embed_dim=768, depth=4, num_heads=12, mlp_ratio=4, twoD=False, default_vars=VARS,
              single_channel=True, adaptive_patching=True, fixed_length=729, use_adaptive_pos_emb=True, num_classes=4, class_token=False,
              linear_decoder=False, feature_size=16, skip_connection=True, sqrt_len=9, sqrt_len_method=True).to(DEV)
    m.set_compute_dtype(torch.bfloat16)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 1, 64, 64, 64, generator=g).to(DEV)
    x_seq = torch.rand(2, 1, 36, 36, 36, generator=g).to(DEV)              # the 729 resized 4^3 patches as a pseudo volume
    seq_ps = (torch.rand(2, 729, 4, generator=g) * 64).to(DEV)
    lab = torch.randint(0, 4, (2, 64, 64, 64), generator=g).to(DEV)
    lo_h, loss_h, g_h = _check_against_torch_decoder(m, (x, VARS, seq_ps, x_seq), lab, [64, 64, 64])
    lo_2, loss_2, g_2 = _run(m, (x, VARS, seq_ps, x_seq), lab, "hip")     # deterministic, the resampling's gather backward included
    assert torch.equal(lo_h, lo_2) and loss_h == loss_2
    assert all(torch.equal(g_h[n], g_2[n]) for n in g_h if n.startswith(("encoder", "decoder", "out.")))


def test_non_adaptive_resampling_geometry():
    """img 48^3, patch 4: 12^3 tokens -> decoder3 at 96^3 -> resampled DOWN by 2 to 48^3"""
    from UCF_VIT.simple.arch import UNETR
    torch.manual_seed(2)
    m = UNETR(img_size=[48, 48, 48], patch_size=4, in_chans=1, embed_dim=96, depth=4, num_heads=3, twoD=False, num_classes=4, class_token=False,
              linear_decoder=False, feature_size=16, skip_connection=True).to(DEV)
    m.set_compute_dtype(torch.bfloat16)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 1, 48, 48, 48, generator=g).to(DEV)
    lab = torch.randint(0, 4, (2, 48, 48, 48), generator=g).to(DEV)
    _check_against_torch_decoder(m, (x, None), lab, [48, 48, 48])


def test_train_unetr_script_runs_the_reference_config(tmp_path):
    """train_unetr_simple.py on the basic_ct/unetr key set (re-typed here; depth reduced, 2 short epochs on synthetic data) with NO
    allow_torch_decoder key: the run goes through the HIP decoder and gives finite losses"""
    import os
    import subprocess
    import sys
    import yaml
    from conftest import ROOT
    cfg = {
        "trainer": {"max_epochs": 2, "data_type": "float32", "checkpoint_path": str(tmp_path), "checkpoint_filename": "multi_last",
                    "checkpoint_filename_for_loading": "multi_last_odd", "resume_from_checkpoint": False, "use_pretrained_mae_model": False},
        "parallelism": {"fsdp_size": 1, "simple_ddp_size": 1, "tensor_par_size": 1, "seq_par_size": 1},
        "model": {"lr": 1e-5, "beta_1": 0.9, "beta_2": 0.95, "weight_decay": 1e-5, "warmup_steps": 1000, "max_steps": 20000,
                  "warmup_start_lr": 1e-8, "eta_min": 1e-8,
                  "net": {"init_args": {"default_vars": ["ct_res1"], "tile_size": [64, 64, 64], "patch_size": 4, "embed_dim": 768, "depth": 4,
                                        "num_heads": 12, "mlp_ratio": 4, "drop_path": 0.0, "linear_decoder": False, "twoD": False,
                                        "use_varemb": False, "adaptive_patching": True, "fixed_length": 729, "separate_channels": False,
                                        "use_adaptive_pos_emb": True, "feature_size": 16, "skip_connection": True, "decoder_embed_dim": 576,
                                        "decoder_depth": 8, "decoder_num_heads": 16, "mlp_ratio_decoder": 4, "mask_ratio": 0.75}}},
        "data": {"dataset": "basic_ct", "num_channels_used": {"basic_ct": 1}, "dict_in_variables": {"basic_ct": ["ct_res1"]}, "batch_size": 2,
                 "single_channel": True, "tile_overlap": 0.0, "use_all_data": False, "num_classes": 4},
        "load_balancing": {"auto_load_balancing": True, "batches_per_rank_epoch": {"basic_ct": 2}},
    }
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, MASTER_PORT="29591")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "ucf-vit_amd", "training_scripts", "train_unetr_simple.py"), str(p)],
                         capture_output=True, text=True, timeout=280, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    losses = [float(l.split("epoch_loss")[1].split()[0]) for l in out.stdout.splitlines() if "epoch_loss" in l]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses), out.stdout
