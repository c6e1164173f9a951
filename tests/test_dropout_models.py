"""Element-wise dropout through the models and the training script: VIT (class token, so the last Block runs as the class-row tail and the
head dropout sits on the pooled [B, D]), MAE (encoder and decoder Blocks), SAP and the UNETR encoder at the tiny shapes of
tests/test_drop_path_models.py, one training step with each of drop_rate, pos_drop_rate and proj_drop_rate; reproducibility under
torch.manual_seed; eval() equal to the model without dropout; attn_drop_rate / patch_drop_rate still refused; the config keys."""
import math

import pytest
import torch

from det_weights import det_state_dict, det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
VARS = ["red", "green", "blue"]
RATE = 0.3

VIT_KW = dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=64, depth=3, num_heads=2)
MAE_KW = dict(img_size=[32, 32], patch_size=8, in_chans=3, embed_dim=64, depth=2, num_heads=2, class_token=False, weight_init='skip',
              mask_ratio=0.75, linear_decoder=False, decoder_depth=2, decoder_embed_dim=32, decoder_num_heads=1, mlp_ratio_decoder=4.0)
SAP_KW = dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=3, embed_dim=64, depth=2, num_heads=2, class_token=False, sqrt_len=4)
UNETR_KW = dict(num_classes=4, linear_decoder=False, feature_size=4, skip_connection=True, allow_torch_decoder=True, img_size=[32, 32, 16],
                patch_size=8, in_chans=1, embed_dim=96, depth=4, num_heads=3, class_token=False, twoD=False)
MODELS = ["vit", "mae", "sap", "unetr"]
RATES = ["drop_rate", "pos_drop_rate", "proj_drop_rate"]


def _build(name, **rates):
    from UCF_VIT.simple import arch
    cls, kw = {"vit": (arch.VIT, VIT_KW), "mae": (arch.MAE, MAE_KW), "sap": (arch.SAP, SAP_KW), "unetr": (arch.UNETR, UNETR_KW)}[name]
    torch.manual_seed(0)                                              # entries det_state_dict keeps as initialised (position tables)
    m = cls(**rates, **kw)
    m.load_state_dict(det_state_dict(m, 31))
    return m.to(DEV)


def _loss(name, m):
    """one forward of the model on fixed data -> a scalar"""
    if name == "vit":
        from UCF_VIT.utils.metrics import cross_entropy_loss
        return cross_entropy_loss(m(det_tensor((4, 3, 32, 32), 1).to(DEV), VARS), torch.tensor([1, 3, 0, 2], device=DEV))
    if name == "mae":
        from UCF_VIT.utils.metrics import patch_mse_loss
        x = det_tensor((4, 3, 32, 32), 2).to(DEV)
        pred, _ = m(x, VARS, noise=torch.rand(4, 16, generator=torch.Generator().manual_seed(3)).to(DEV))
        return patch_mse_loss(pred, x, 8)
    if name == "sap":
        return m(det_tensor((4, 3, 32, 32), 4).to(DEV), None).float().square().mean()
    feats, taps = m.forward_intermediates(det_tensor((4, 1, 32, 32, 16), 5).to(DEV), None, None, indices=m.skip_indices)
    return feats.float().square().mean() + sum(t.float().square().mean() for t in taps)


def _drawn(m):
    from UCF_VIT.simple.building_blocks import HipDropout
    return {k: d.last_seed for k, d in m.named_modules() if isinstance(d, HipDropout) and d.last_seed is not None}


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", MODELS)
def test_training_step_runs_with_each_rate(name, rate):
    m = _build(name, **{rate: RATE}).train()
    torch.manual_seed(11)
    loss = _loss(name, m)
    loss.backward()
    assert math.isfinite(loss.item())
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), k
    assert all(p.grad is not None for k, p in m.named_parameters() if k.startswith("blocks."))
    drawn = _drawn(m)
    if rate == "proj_drop_rate":                                     # three sites per Block, the MAE decoder Blocks included
        n_blocks = len(m.blocks) + (len(m.decoder_blocks) if name == "mae" else 0)
        assert len(drawn) == 3 * n_blocks and len(set(drawn.values())) == len(drawn)
        assert all(k.endswith(("attn.proj_drop", "mlp.drop1", "mlp.drop2")) for k in drawn)
    elif rate == "pos_drop_rate":
        assert list(drawn) == ["pos_drop"]
    else:                                                            # head dropout: only the classifier has the head it sits in front of
        assert list(drawn) == (["head_drop"] if name == "vit" else [])


@pytest.mark.parametrize("name", ["vit", "mae"])
def test_same_seed_same_masks_same_loss(name):
    m = _build(name, drop_rate=RATE, pos_drop_rate=RATE, proj_drop_rate=RATE).train()
    out = []
    for _ in range(2):
        torch.manual_seed(123)
        loss = _loss(name, m)
        loss.backward()
        out.append((loss.detach().clone(), dict(_drawn(m)), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
        m.zero_grad(set_to_none=True)
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32))
    assert len(out[0][1]) > 0 and out[0][1] == out[1][1]
    assert all(torch.equal(g, out[1][2][k]) for k, g in out[0][2].items())
    torch.manual_seed(124)
    other = _loss(name, m).detach()
    assert _drawn(m) != out[0][1] and not torch.equal(other, out[0][0])


@pytest.mark.parametrize("name", MODELS)
def test_eval_is_the_model_without_dropout(name):
    a, b = _build(name, drop_rate=RATE, pos_drop_rate=RATE, proj_drop_rate=RATE).eval(), _build(name).eval()
    with torch.no_grad():
        assert torch.equal(_loss(name, a), _loss(name, b))
    assert _drawn(a) == {}


@pytest.mark.parametrize("rate", ["attn_drop_rate", "patch_drop_rate"])
def test_attention_and_patch_dropout_are_still_refused(rate):
    m = _build("vit", **{rate: 0.1})
    with torch.no_grad():
        m.eval()
        _loss("vit", m)                                              # building and eval() are fine
    m.train()
    with pytest.raises(NotImplementedError, match=rate.replace("_rate", "") if rate == "attn_drop_rate" else "patch_drop_rate"):
        _loss("vit", m)


def test_head_dropout_masks_the_pooled_rows():
    """VIT.forward with the class-row tail: head_drop sees the [B, D] rows the final norm returns; the logits equal the head applied to
    the masked rows"""
    import dropout_ref as R
    m = _build("vit", drop_rate=RATE).train()
    seen = {}
    h = m.head_drop.register_forward_hook(lambda mod, inp, out: seen.update(x=inp[0].detach(), y=out.detach()))
    torch.manual_seed(5)
    x = det_tensor((4, 3, 32, 32), 1).to(DEV)
    logits = m(x, VARS)
    h.remove()
    assert tuple(seen["x"].shape) == (4, 64)
    mask = torch.from_numpy(R.keep_mask(m.head_drop.last_seed, 4, 64, RATE)).to(DEV)
    want = seen["x"].double() * mask * R.inv_keep(RATE)
    assert float((seen["y"].double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())
    assert torch.equal(seen["y"] == 0, ~mask)
    with torch.no_grad():
        assert torch.equal(logits, m.head(seen["y"]))


def test_train_class_script_reads_the_dropout_keys(tmp_path):
    """train_class_simple.py as in tests/test_drop_path_models.py, with drop_rate, pos_drop_rate and proj_drop_rate 0.1 in the config: two
    epochs, finite loss"""
    import os
    import re
    import subprocess
    import sys
    import yaml
    from conftest import ROOT
    cfg = yaml.safe_load(open(os.path.join(ROOT, "ucf-vit_amd", "configs", "catsdogs_vit_tiny_smoke.yaml")))
    cfg["trainer"]["checkpoint_path"] = str(tmp_path)
    cfg["model"]["net"]["init_args"].update(drop_rate=0.1, pos_drop_rate=0.1, proj_drop_rate=0.1)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, MASTER_PORT="29592")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "ucf-vit_amd", "training_scripts", "train_class_simple.py"), str(p)],
                         capture_output=True, text=True, timeout=280, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    losses = [float(v) for v in re.findall(r"epoch_loss ([-+0-9.einfa]+)", out.stdout)]
    assert "epoch: 1" in out.stdout and len(losses) == 2 and all(math.isfinite(v) for v in losses)
