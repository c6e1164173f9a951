"""Pins the CPU oracle (oracle/ucf_vit_ref.py) and the host-side tables/schedules of the product against golden vectors
generated from the reference implementation itself (tests/golden/make_golden.py).  CPU only."""
import math
from functools import partial

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from det_weights import det_state_dict, proj_vector

from oracle import ucf_vit_ref as R

torch.set_num_threads(4)


def load_w(mod, g, prefix="w."):
    sd = {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}
    mod.load_state_dict(sd)
    return mod


def run_op(mod, g):
    x = g["x"].clone().requires_grad_(True)
    y = mod(x)
    y.backward(g["gy"])
    return x, y


@pytest.mark.parametrize("name,make", [
    ("op_mlp.npz", lambda: R.Mlp(64, 256)),
    ("op_attn_none.npz", lambda: R.Attention(64, 2, True, sdpa=False)),
    ("op_attn_default.npz", lambda: R.Attention(64, 2, True, sdpa=True)),
    ("op_attn_n197_dh64.npz", lambda: R.Attention(128, 2, True, sdpa=False)),
    ("op_block.npz", lambda: R.Block(64, 2, 4.0, True, partial(torch.nn.LayerNorm, eps=1e-6))),
    ("op_layernorm.npz", lambda: torch.nn.LayerNorm(64, eps=1e-6)),
])
def test_oracle_operator(name, make):
    g = load_golden(name)
    mod = load_w(make(), g)
    x, y = run_op(mod, g)
    assert rel_err(y, g["y"]) < 1e-5
    assert rel_err(x.grad, g["gx"]) < 1e-5
    for k, p in mod.named_parameters():
        assert rel_err(p.grad, g["g." + k]) < 1e-5, k


@pytest.mark.parametrize("name,kw", [
    ("op_patch2d.npz", dict(img_size=[32, 32], patch_size=8, in_chans=3, embed_dim=64, twoD=True)),
    ("op_patch3d.npz", dict(img_size=[16, 16, 8], patch_size=4, in_chans=1, embed_dim=48, twoD=False)),
])
def test_oracle_patch_embed(name, kw):
    g = load_golden(name)
    mod = load_w(R.PatchEmbed(**kw), g)
    y = mod(g["x"])
    y.backward(g["gy"])
    assert rel_err(y, g["y"]) < 1e-5
    for k, p in mod.named_parameters():
        assert rel_err(p.grad, g["g." + k]) < 1e-5, k


def test_pos_tables_oracle_and_product():
    g = load_golden("pos_tables.npz")
    from UCF_VIT.utils import pos_embed as P
    for mod2d, mod3d in ((R.sincos_2d, R.sincos_3d), (P.get_2d_sincos_pos_embed, P.get_3d_sincos_pos_embed)):
        assert np.array_equal(mod2d(32, 3, 5, True), g["t2d_32_3x5_cls"].numpy())
        assert np.array_equal(mod2d(64, 4, 4, False), g["t2d_64_4x4"].numpy())
        assert np.array_equal(mod3d(48, 2, 3, 4), g["t3d_48_2x3x4"].numpy())
        t = mod2d(1024, 14, 14, True)
        assert np.allclose([t.sum(), np.abs(t).sum()], g["vitl_sum"].numpy(), rtol=1e-12)


def test_mae_masking_bit_exact():
    g = load_golden("mae_masking.npz")
    m = R.MAE([32, 32], patch_size=8, embed_dim=64, depth=1, num_heads=2, class_token=False, decoder_depth=1,
              decoder_embed_dim=32, decoder_num_heads=1)
    kept, mask, ids = m.random_masking(g["seq"], g["noise"])
    assert torch.equal(ids, g["ids_restore"]) and torch.equal(mask, g["mask"]) and torch.equal(kept, g["kept"])


def test_oracle_vit_small():
    g = load_golden("model_vit_small.npz")
    m = R.VIT([32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=64, depth=2, num_heads=2)
    m.load_state_dict(det_state_dict(m, 21))
    out = m(g["x"])
    loss = torch.nn.CrossEntropyLoss()(out, g["labels"])
    loss.backward()
    assert rel_err(out, g["logits"]) < 1e-5 and abs(loss.item() - g["loss"].item()) < 1e-6
    for k, p in m.named_parameters():
        assert rel_err(p.grad, g["g." + k]) < 2e-5, k


ADAPTIVE_CASES = [("model_vit_adaptive.npz", dict(patch_size=8, in_chans=3, twoD=True, use_adaptive_pos_emb=True), 52),
                  ("model_vit_adaptive_learnpos.npz", dict(patch_size=8, in_chans=3, twoD=True, use_adaptive_pos_emb=False), 53),
                  ("model_vit_adaptive_3d.npz", dict(patch_size=4, in_chans=1, twoD=False, use_adaptive_pos_emb=True), 56)]


@pytest.mark.parametrize("name,kw,seed", ADAPTIVE_CASES)
def test_oracle_vit_adaptive_patching(name, kw, seed):
    """VIT(adaptive_patching=True): LayerNorm-Linear-LayerNorm token embedding of pre-cut patches + position embedding from seq_ps"""
    g = load_golden(name)
    m = R.AdaptiveVIT(num_classes=5, embed_dim=64, depth=2, num_heads=2, fixed_length=12, **kw)
    m.load_state_dict(det_state_dict(m, seed, keep=()))
    out = m(g["x"], None, g["seq_ps"])
    loss = torch.nn.CrossEntropyLoss()(out, g["labels"])
    loss.backward()
    assert rel_err(out, g["logits"]) < 1e-5 and abs(loss.item() - g["loss"].item()) < 1e-6
    for k, p in m.named_parameters():
        ref = g["g." + k]
        if p.grad is None:
            assert float(ref.abs().max()) == 0.0, k        # pos_embed is unused when the position embedding comes from seq_ps
        else:
            assert rel_err(p.grad, ref) < 2e-5, k


@pytest.mark.parametrize("name,adaptive_pos,seed", [("model_mae_adaptive.npz", True, 58), ("model_mae_adaptive_learnpos.npz", False, 59)])
def test_oracle_mae_adaptive_patching(name, adaptive_pos, seed):
    """MAE(adaptive_patching=True): encoder and decoder positions from seq_ps (or learnt tables), target = the rearranged sequence"""
    g = load_golden(name)
    m = R.AdaptiveMAE(patch_size=8, in_chans=3, embed_dim=64, depth=2, num_heads=2, fixed_length=12, use_adaptive_pos_emb=adaptive_pos,
                      mask_ratio=0.5, decoder_depth=1, decoder_embed_dim=32, decoder_num_heads=1)
    m.load_state_dict(det_state_dict(m, seed, keep=()))
    pred, mask = m(g["x"], None, g["seq_ps"], g["noise"])
    target = g["x"].permute(0, 2, 3, 1).flatten(2)
    loss = torch.nn.MSELoss()(pred, target)
    loss.backward()
    assert torch.equal(mask, g["mask"])
    assert rel_err(pred, g["pred"]) < 1e-5 and abs(loss.item() - g["loss"].item()) < 1e-6
    assert abs(R.masked_mse(pred, target, mask).item() - g["loss_masked"].item()) < 1e-6
    for k, p in m.named_parameters():
        ref = g["g." + k]
        if p.grad is None:
            assert float(ref.abs().max()) == 0.0, k
        else:
            assert rel_err(p.grad, ref) < 2e-5, k


def _check_grads(m, g):
    for k, p in m.named_parameters():
        ref = g["g." + k]
        if p.grad is None:
            assert float(ref.abs().max()) == 0.0, k
        else:
            assert rel_err(p.grad, ref) < 2e-5, k


def test_oracle_vit_sqrt_len_method_3d():
    """adaptive patching as the UNETR / SAP scripts use it: pseudo-volume through the patch-embedding convolution + seq_ps positions"""
    g = load_golden("model_vit_sqrtlen_3d.npz")
    m = R.SqrtLenVIT([16, 16, 16], patch_size=4, in_chans=1, num_classes=5, embed_dim=96, depth=2, num_heads=3, class_token=False, twoD=False)
    m.load_state_dict(det_state_dict(m, 62, keep=()))
    out = m(g["x"], None, g["seq_ps"])
    loss = torch.nn.CrossEntropyLoss()(out.flatten(0, 1), g["labels"])
    loss.backward()
    assert rel_err(out, g["logits"]) < 1e-5 and abs(loss.item() - g["loss"].item()) < 1e-6
    _check_grads(m, g)


def test_oracle_sap_adaptive():
    g = load_golden("model_sap_adaptive.npz")
    m = R.SAP([64, 64], patch_size=8, in_chans=3, embed_dim=64, depth=2, num_heads=2, twoD=True, sqrt_len=4, num_classes=3)
    m.load_state_dict(det_state_dict(m, 65, keep=()))
    out = m(g["x"], None, g["seq_ps"])
    loss = torch.nn.MSELoss()(out, g["target"])
    loss.backward()
    assert rel_err(out, g["out"]) < 1e-5 and abs(loss.item() - g["loss"].item()) < 1e-6
    _check_grads(m, g)


@pytest.mark.parametrize("name,single,variables,seed", [("model_vit_varemb.npz", False, ["v", "q", "u"], 81), ("model_vit_varemb_single.npz", True, ["t"], 83)])
def test_oracle_vit_variable_aggregation(name, single, variables, seed):
    """VIT(use_varemb=True) on adaptively patched input: per-variable token embeddings + variable embedding + VariableMapping_Attention"""
    g = load_golden(name)
    m = R.VarembVIT(patch_size=8, num_classes=5, embed_dim=64, depth=2, num_heads=2, fixed_length=12, default_vars=["u", "v", "t", "q"],
                    single_channel=single)
    m.load_state_dict(det_state_dict(m, seed, keep=()))
    out = m(g["x"], variables, g["seq_ps"])
    loss = torch.nn.CrossEntropyLoss()(out, g["labels"])
    loss.backward()
    assert rel_err(out, g["logits"]) < 1e-5 and abs(loss.item() - g["loss"].item()) < 1e-6
    _check_grads(m, g)


def test_oracle_vit_tiny_config_T():
    """BASELINE configs[0]: ViT-Tiny/16, catsdogs tile 256x256, 2 classes (un-normalised 0..255 pixels)"""
    g = load_golden("model_vit_tiny_catsdogs.npz")
    m = R.VIT([256, 256], patch_size=16, in_chans=3, num_classes=2, embed_dim=192, depth=12, num_heads=3, sdpa=True)
    m.load_state_dict(det_state_dict(m, 23))
    out = m(g["x"])
    loss = torch.nn.CrossEntropyLoss()(out, g["labels"])
    loss.backward()
    assert rel_err(out, g["logits"]) < 1e-4
    assert abs(loss.item() - g["loss"].item()) < 1e-4 * max(1.0, abs(g["loss"].item()))
    for i, (k, p) in enumerate(m.named_parameters()):
        gn = p.grad.double().norm().item()
        assert abs(gn - g["gn." + k].item()) <= 2e-4 * max(g["gn." + k].item(), 1e-12), k
        gp = (p.grad.double() * proj_vector(p.shape, i).double()).sum().item()
        assert abs(gp - g["gp." + k].item()) <= 5e-4 * max(gn * math.sqrt(p.numel()), 1e-12), k


def test_oracle_mae_small():
    g = load_golden("model_mae_small.npz")
    m = R.MAE([32, 32], patch_size=8, in_chans=3, embed_dim=64, depth=2, num_heads=2, class_token=False, mask_ratio=0.75,
              decoder_depth=1, decoder_embed_dim=32, decoder_num_heads=1, mlp_ratio_decoder=4.0)
    m.load_state_dict(det_state_dict(m, 26))
    pred, mask = m(g["x"], noise=g["noise"])
    tgt = R.patchify(g["x"], 8)
    loss = torch.nn.MSELoss()(pred, tgt)
    assert torch.equal(mask, g["mask"])
    assert rel_err(pred, g["pred"]) < 1e-5 and abs(loss.item() - g["loss"].item()) < 1e-6
    assert abs(R.masked_mse(pred, tgt, mask).item() - g["loss_masked"].item()) < 1e-6
    loss.backward()
    for k, p in m.named_parameters():
        assert rel_err(p.grad, g["g." + k]) < 2e-5, k


def test_lr_schedule_oracle_and_product():
    g = load_golden("lr_schedule.npz")
    from UCF_VIT.utils.lr_scheduler import LinearWarmupCosineAnnealingLR as Prod
    for cls in (R.WarmupCosineLR, Prod):
        for key, (w, T, n) in {"lrs_5_20": (5, 20, 30), "lrs_1000_20000": (1000, 20000, 40)}.items():
            p = torch.nn.Parameter(torch.zeros(1))
            opt = torch.optim.SGD([p], lr=1e-4)
            sch = cls(opt, w, T, 1e-8, 1e-8)
            lrs = []
            for _ in range(n):
                lrs.append(opt.param_groups[0]["lr"])
                opt.step()
                sch.step()
            ref = g[key].numpy()
            # the reference's recursive cosine form and the closed form agree until the schedule passes max_epochs (the
            # reference then keeps recursing); compare on t <= T
            upto = min(n, T + 1)
            assert np.allclose(np.array(lrs)[:upto], ref[:upto], rtol=1e-6, atol=1e-15), (cls.__name__, key)


def test_oracle_adamw_trajectory():
    g = load_golden("traj_vit_small.npz")
    m = R.VIT([32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=64, depth=2, num_heads=2)
    sd0 = det_state_dict(m, 31)
    m.load_state_dict(sd0)
    opt = R.configure_optimizer(m, 1e-3, 0.9, 0.95, 1e-2)
    sch = R.WarmupCosineLR(opt, 2, 10, 1e-5, 1e-6)
    lrs = []
    for i in range(5):
        lrs.append(opt.param_groups[0]["lr"])
        loss, _ = R.train_step_class(m, opt, sch, g["x%d" % i], g["labels"][i])
        assert abs(loss.item() - g["losses"][i].item()) < 1e-5
    for k, v in m.state_dict().items():
        if k.startswith("token_embeds"):
            continue
        ref = g["final." + k]
        if k.endswith("attn.qkv.bias"):
            # d(loss)/d(k-bias) is exactly zero in exact arithmetic (softmax shift invariance): its computed gradient is pure
            # rounding noise, different on every CPU, which Adam normalises to steps of up to lr each (1 - beta1 <= sqrt(1 - beta2)).
            # The q and v thirds are compared as everything else; the k third of both trajectories stays within those steps of its start
            D = ref.numel() // 3
            bound = 1.05 * sum(lrs)
            for w_ in (v, ref):
                assert float((w_[D:2 * D] - sd0[k][D:2 * D]).abs().max()) <= bound, k
            v, ref = torch.cat([v[:D], v[2 * D:]]), torch.cat([ref[:D], ref[2 * D:]])
        assert rel_err(v, ref) < 1e-5, k
