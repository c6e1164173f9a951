"""qk_norm through the models and the training script: VIT against the reference fixture model_vit_qknorm.npz (class token, so the last
Block runs as the class-row tail), MAE (encoder and decoder Blocks), SAP and UNETR at the tiny shapes of tests/test_layer_scale_models.py
with qk_norm=True (every parameter receives a finite gradient, checkpointing reproduces the bits, an optimizer step moves q_norm.weight),
and the `qk_norm` key of the YAML config."""
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


def _is_qk(k):
    return ".q_norm." in k or ".k_norm." in k


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (torch.bfloat16, 5e-2)])
def test_vit_vs_reference(dtype, tol):
    """the tolerances tests/test_hip_models.py applies to model_vit_small.npz; the weights are det_state_dict(model, 77) with the recorded
    q_norm / k_norm parameters, as the fixture was generated.  k_norm.bias (gradient mathematically 0) is judged against the scale of the
    q_norm.bias gradient of its Block."""
    from UCF_VIT.simple.arch import VIT
    from UCF_VIT.utils.metrics import cross_entropy_loss
    g = load_golden("model_vit_qknorm.npz")
    m = VIT(qk_norm=True, **VIT_KW)
    sd = det_state_dict(m, 77)
    sd.update({k[2:]: v for k, v in g.items() if k.startswith("w.")})
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.set_compute_dtype(dtype)
    out = m(g["x"].to(DEV), VARS)
    loss = cross_entropy_loss(out, g["labels"].to(DEV))
    loss.backward()
    assert out.dtype == dtype
    assert rel_err(out.float(), g["logits"]) < tol
    assert abs(loss.item() - g["loss"].item()) < tol * max(1.0, abs(g["loss"].item()))
    seen = 0
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        if k.endswith("k_norm.bias"):
            scale = g["g." + k[:-len("k_norm.bias")] + "q_norm.bias"].abs().max().item()
            assert (p.grad.cpu() - g["g." + k]).abs().max().item() < tol * scale, k
        else:
            assert rel_err(p.grad, g["g." + k]) < tol, k
        seen += _is_qk(k)
    assert seen == 8
    st = m._ucf_store                                                # the new gradients too were written straight into the flat buffer
    for p, o in zip(st.params, st.offsets):
        assert p.grad.data_ptr() == st.flat_g.data_ptr() + 4 * o


def _build(name, qk_norm=True):
    from UCF_VIT.simple import arch
    cls, kw = {"mae": (arch.MAE, MAE_KW), "sap": (arch.SAP, SAP_KW), "unetr": (arch.UNETR, UNETR_KW)}[name]
    torch.manual_seed(0)
    m = cls(qk_norm=qk_norm, **kw)
    sd = det_state_dict(m, 31)
    for i, k in enumerate(sorted(sd)):
        if _is_qk(k):                                                 # of order 1 (weights) / 0.1 (biases), different per element, q and k
            sd[k] = det_tensor(sd[k].shape, 5000 + i, 0.3, 1.0 if k.endswith("weight") else 0.1)
    m.load_state_dict(sd)
    return m.to(DEV)


def _loss(name, m):
    if name == "mae":
        from UCF_VIT.utils.metrics import patch_mse_loss
        x = det_tensor((4, 3, 32, 32), 2).to(DEV)
        pred, _ = m(x, VARS, noise=torch.rand(4, 16, generator=torch.Generator().manual_seed(3)).to(DEV))
        return patch_mse_loss(pred, x, 8)
    if name == "sap":
        return m(det_tensor((4, 3, 32, 32), 4).to(DEV), None).float().square().mean()
    feats, taps = m.forward_intermediates(det_tensor((4, 1, 32, 32, 16), 5).to(DEV), None, None, indices=m.skip_indices)
    return feats.float().square().mean() + sum(t.float().square().mean() for t in taps)


@pytest.mark.parametrize("name", ["mae", "unetr", "sap"])
def test_training_step_checkpointing_and_optimizer(name):
    from UCF_VIT.simple.building_blocks import apply_activation_checkpointing
    from UCF_VIT.utils.misc import configure_optimizer
    m = _build(name).train()
    loss = _loss(name, m)
    loss.backward()
    assert math.isfinite(loss.item())
    n_blocks = len(m.blocks) + (len(m.decoder_blocks) if name == "mae" else 0)
    qk = {k: p for k, p in m.named_parameters() if _is_qk(k)}
    assert len(qk) == 4 * n_blocks
    # every parameter receives a finite gradient, but for the ones this loss does not reach at all (UNETR's convolution decoder: the loss
    # is taken on the encoder's taps): exactly the parameters that receive none in the same model built without qk_norm, none of them in
    # a Block
    plain = _build(name, qk_norm=False).train()
    _loss(name, plain).backward()
    unreached = {k for k, p in plain.named_parameters() if p.grad is None}
    assert not any(k.startswith(("blocks.", "decoder_blocks.")) for k in unreached)
    assert (name == "unetr") == bool(unreached), sorted(unreached)
    assert {k for k, p in m.named_parameters() if p.grad is None} == unreached
    for k, p in m.named_parameters():
        if k not in unreached:
            assert bool(torch.isfinite(p.grad).all()), k
    for k, p in qk.items():
        assert p.dtype == torch.float32 and p.grad.dtype == torch.float32, k
        if not k.endswith("k_norm.bias"):                             # that one is mathematically 0
            assert float(p.grad.abs().max()) > 0, k
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m2 = _build(name).train()                                         # a checkpointed model: the same loss and gradients, bit for bit
    assert apply_activation_checkpointing(m2) == n_blocks
    loss2 = _loss(name, m2)
    loss2.backward()
    assert torch.equal(loss2, loss)
    for k, p in m2.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, grads[k]), k
    before = {k: p.detach().clone() for k, p in qk.items()}          # one HipAdamW step moves q_norm.weight (and its three siblings' values stay finite)
    opt = configure_optimizer(m, 1e-2, 0.9, 0.95, 0.0)
    opt.step()
    torch.cuda.synchronize()
    for k, p in qk.items():
        assert bool(torch.isfinite(p).all()), k
        if k.endswith("q_norm.weight"):
            assert not torch.equal(p.detach(), before[k]), k


def test_train_class_script_reads_the_qk_norm_key(tmp_path):
    """train_class_simple.py with qk_norm: True in the config, in a child process: two epochs, finite losses"""
    import os
    import re
    import subprocess
    import sys
    import yaml
    from conftest import ROOT
    cfg = yaml.safe_load(open(os.path.join(ROOT, "ucf-vit_amd", "configs", "catsdogs_vit_tiny_smoke.yaml")))
    cfg["trainer"]["checkpoint_path"] = str(tmp_path)
    cfg["model"]["net"]["init_args"]["qk_norm"] = True
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, MASTER_PORT="29594")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "ucf-vit_amd", "training_scripts", "train_class_simple.py"), str(p)],
                         capture_output=True, text=True, timeout=280, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    losses = [float(v) for v in re.findall(r"epoch_loss ([-+0-9.einfa]+)", out.stdout)]
    assert "epoch: 1" in out.stdout and len(losses) == 2 and all(math.isfinite(v) for v in losses)
