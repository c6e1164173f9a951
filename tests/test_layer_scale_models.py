"""LayerScale through the models and the training script: VIT against the reference fixture model_vit_layerscale.npz (class token, so
the last Block runs as the class-row tail), MAE (encoder and decoder Blocks), UNETR and SAP at the tiny shapes of
tests/test_drop_path_models.py with init_values = 0.1, and the `init_values` key of the YAML config."""
import math

import pytest
import torch

from conftest import load_golden, rel_err
from det_weights import det_state_dict, det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
VARS = ["red", "green", "blue"]

VIT_KW = dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=64, depth=2, num_heads=2)
MAE_KW = dict(img_size=[32, 32], patch_size=8, in_chans=3, embed_dim=64, depth=2, num_heads=2, class_token=False, weight_init='skip',
              mask_ratio=0.75, linear_decoder=False, decoder_depth=2, decoder_embed_dim=32, decoder_num_heads=1, mlp_ratio_decoder=4.0)
SAP_KW = dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=3, embed_dim=64, depth=2, num_heads=2, class_token=False, sqrt_len=4)
UNETR_KW = dict(num_classes=4, linear_decoder=False, feature_size=4, skip_connection=True, allow_torch_decoder=True, img_size=[32, 32, 16],
                patch_size=8, in_chans=1, embed_dim=96, depth=4, num_heads=3, class_token=False, twoD=False)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (torch.bfloat16, 5e-2)])
def test_vit_vs_reference(dtype, tol):
    """the tolerances tests/test_hip_models.py applies to model_vit_small.npz; the gammas are the det_state_dict values the fixture was
    generated with (N(0, 0.05) per column)"""
    from UCF_VIT.simple.arch import VIT
    from UCF_VIT.utils.metrics import cross_entropy_loss
    g = load_golden("model_vit_layerscale.npz")
    m = VIT(init_values=0.1, **VIT_KW)
    m.load_state_dict(det_state_dict(m, 63))
    m = m.to(DEV).train()
    m.set_compute_dtype(dtype)
    out = m(g["x"].to(DEV), VARS)
    loss = cross_entropy_loss(out, g["labels"].to(DEV))
    loss.backward()
    assert out.dtype == dtype
    assert rel_err(out.float(), g["logits"]) < tol
    assert abs(loss.item() - g["loss"].item()) < tol * max(1.0, abs(g["loss"].item()))
    gammas = 0
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        assert rel_err(p.grad, g["g." + k]) < tol, k
        gammas += k.endswith(".gamma")
    assert gammas == 4
    st = m._ucf_store                                                # the gamma gradients too were written straight into the flat buffer
    for p, o in zip(st.params, st.offsets):
        assert p.grad.data_ptr() == st.flat_g.data_ptr() + 4 * o


def _build(name):
    from UCF_VIT.simple import arch
    cls, kw = {"mae": (arch.MAE, MAE_KW), "sap": (arch.SAP, SAP_KW), "unetr": (arch.UNETR, UNETR_KW)}[name]
    torch.manual_seed(0)                                              # entries det_state_dict keeps as initialised (position tables)
    m = cls(init_values=0.1, **kw)
    sd = det_state_dict(m, 31)
    for k in sd:
        if k.endswith(".gamma"):
            sd[k] = sd[k] + 0.1                                       # around init_values, different per column
    m.load_state_dict(sd)
    return m.to(DEV)


def _loss(name, m):
    """one forward of the model on fixed data -> a scalar"""
    if name == "mae":
        from UCF_VIT.utils.metrics import patch_mse_loss
        x = det_tensor((4, 3, 32, 32), 2).to(DEV)
        pred, _ = m(x, VARS, noise=torch.rand(4, 16, generator=torch.Generator().manual_seed(3)).to(DEV))
        return patch_mse_loss(pred, x, 8)
    if name == "sap":
        return m(det_tensor((4, 3, 32, 32), 4).to(DEV), None).float().square().mean()
    feats, taps = m.forward_intermediates(det_tensor((4, 1, 32, 32, 16), 5).to(DEV), None, None, indices=m.skip_indices)
    return feats.float().square().mean() + sum(t.float().square().mean() for t in taps)


def _gamma_params(m):
    return {k: p for k, p in m.named_parameters() if k.endswith(".gamma")}


@pytest.mark.parametrize("name", ["mae", "unetr", "sap"])
def test_training_step_checkpointing_optimizer_and_state_dict(name):
    from UCF_VIT.simple.building_blocks import apply_activation_checkpointing
    from UCF_VIT.utils.misc import configure_optimizer
    m = _build(name).train()
    loss = _loss(name, m)
    loss.backward()
    assert math.isfinite(loss.item())
    gammas = _gamma_params(m)
    n_blocks = len(m.blocks) + (len(m.decoder_blocks) if name == "mae" else 0)
    assert len(gammas) == 2 * n_blocks
    for k, p in gammas.items():
        assert p.dtype == torch.float32 and p.grad is not None and p.grad.dtype == torch.float32, k
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    # a checkpointed model: the same loss and gradients, bit for bit
    m2 = _build(name).train()
    assert apply_activation_checkpointing(m2) == n_blocks
    loss2 = _loss(name, m2)
    loss2.backward()
    assert torch.equal(loss2, loss)
    for k, p in m2.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, grads[k]), k
    # the state_dict round trip is exact
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m3 = _build(name)
    with torch.no_grad():
        for p in _gamma_params(m3).values():
            p.zero_()
    m3.load_state_dict(sd)
    for k, v in m3.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # a HipAdamW step moves every gamma
    before = {k: p.detach().clone() for k, p in gammas.items()}
    opt = configure_optimizer(m, 1e-2, 0.9, 0.95, 0.0)
    opt.step()
    torch.cuda.synchronize()
    for k, p in gammas.items():
        assert not torch.equal(p.detach(), before[k]), k
        assert bool(torch.isfinite(p).all()), k


def test_train_class_script_reads_the_init_values_key(tmp_path):
    """train_class_simple.py as in tests/test_drop_path_models.py, with init_values: 1e-5 and drop_path: 0.1 in the config: two epochs,
    finite losses"""
    import os
    import re
    import subprocess
    import sys
    import yaml
    from conftest import ROOT
    cfg = yaml.safe_load(open(os.path.join(ROOT, "ucf-vit_amd", "configs", "catsdogs_vit_tiny_smoke.yaml")))
    cfg["trainer"]["checkpoint_path"] = str(tmp_path)
    cfg["model"]["net"]["init_args"]["init_values"] = 1e-5
    cfg["model"]["net"]["init_args"]["drop_path"] = 0.1
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, MASTER_PORT="29593")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "ucf-vit_amd", "training_scripts", "train_class_simple.py"), str(p)],
                         capture_output=True, text=True, timeout=280, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    losses = [float(v) for v in re.findall(r"epoch_loss ([-+0-9.einfa]+)", out.stdout)]
    assert "epoch: 1" in out.stdout and len(losses) == 2 and all(math.isfinite(v) for v in losses)
