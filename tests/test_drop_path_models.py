"""Stochastic depth through the models and the training script: VIT (class token, so the last Block runs as the class-row tail), MAE
(encoder and decoder Blocks), SAP and the UNETR encoder at the tiny shapes of tests/test_hip_models.py with drop_path_rate = 0.5; the
draw's statistics and seeding; the `drop_path` key of the YAML config."""
import math

import pytest
import torch

from det_weights import det_state_dict, det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
VARS = ["red", "green", "blue"]
RATE = 0.5

VIT_KW = dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=64, depth=3, num_heads=2)
MAE_KW = dict(img_size=[32, 32], patch_size=8, in_chans=3, embed_dim=64, depth=2, num_heads=2, class_token=False, weight_init='skip',
              mask_ratio=0.75, linear_decoder=False, decoder_depth=2, decoder_embed_dim=32, decoder_num_heads=1, mlp_ratio_decoder=4.0)
SAP_KW = dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=3, embed_dim=64, depth=2, num_heads=2, class_token=False, sqrt_len=4)
UNETR_KW = dict(num_classes=4, linear_decoder=False, feature_size=4, skip_connection=True, allow_torch_decoder=True, img_size=[32, 32, 16],
                patch_size=8, in_chans=1, embed_dim=96, depth=4, num_heads=3, class_token=False, twoD=False)


def _build(name, rate):
    from UCF_VIT.simple import arch
    cls, kw = {"vit": (arch.VIT, VIT_KW), "mae": (arch.MAE, MAE_KW), "sap": (arch.SAP, SAP_KW), "unetr": (arch.UNETR, UNETR_KW)}[name]
    torch.manual_seed(0)                                              # entries det_state_dict keeps as initialised (position tables)
    m = cls(drop_path_rate=rate, **kw)
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


def _block_lists(name, m):
    """(Blocks, drop_path_rate of the linspace they were built from) per stack"""
    stacks = [list(m.blocks)]
    if name == "mae":
        stacks.append(list(m.decoder_blocks))
    return stacks


MODELS = ["vit", "mae", "sap", "unetr"]


@pytest.mark.parametrize("name", MODELS)
def test_training_step_runs_and_records_the_draw(name):
    from UCF_VIT.simple.building_blocks import DropPath
    m = _build(name, RATE).train()
    torch.manual_seed(11)
    loss = _loss(name, m)
    loss.backward()
    assert math.isfinite(loss.item())
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), k
    assert all(p.grad is not None for k, p in m.named_parameters() if k.startswith("blocks."))
    for blocks in _block_lists(name, m):
        rates = torch.linspace(0, RATE, len(blocks)).tolist()
        assert isinstance(blocks[0].drop_path1, torch.nn.Identity)              # rate 0: no module, today's launches
        for blk, rate in zip(blocks[1:], rates[1:]):
            for d in (blk.drop_path1, blk.drop_path2):
                assert isinstance(d, DropPath) and abs(d.drop_prob - rate) < 1e-6
                s = d.last_scale
                assert s is not None and s.dtype == torch.float32 and tuple(s.shape) == (4,)
                kept = (torch.ones(1) / (1.0 - d.drop_prob)).item()
                assert set(s.tolist()) <= {0.0, kept}
            assert blk.drop_path1.last_scale is not blk.drop_path2.last_scale


@pytest.mark.parametrize("name", MODELS)
def test_eval_is_the_model_without_drop_path(name):
    a, b = _build(name, RATE).eval(), _build(name, 0.0).eval()
    with torch.no_grad():
        assert torch.equal(_loss(name, a), _loss(name, b))


@pytest.mark.parametrize("name", ["vit", "mae"])
def test_same_seed_same_draw_same_loss(name):
    m = _build(name, RATE).train()
    out = []
    for _ in range(2):
        torch.manual_seed(123)
        loss = _loss(name, m).detach()
        out.append((loss.clone(), [d.last_scale.clone() for d in m.modules() if getattr(d, "last_scale", None) is not None]))
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32))
    assert len(out[0][1]) > 0 and all(torch.equal(p, q) for p, q in zip(out[0][1], out[1][1]))
    torch.manual_seed(124)
    _loss(name, m)
    other = [d.last_scale for d in m.modules() if getattr(d, "last_scale", None) is not None]
    assert any(not torch.equal(p, q) for p, q in zip(out[0][1], other))


def test_draw_statistics():
    """4096 Bernoulli(0.75) draws: the kept fraction within 5 standard deviations (sqrt(0.75 * 0.25 / 4096) = 0.00677) of 0.75"""
    from UCF_VIT.simple.building_blocks import DropPath
    torch.manual_seed(7)
    d = DropPath(0.25)
    s = d.draw(4096, DEV)
    assert s.is_cuda and s.dtype == torch.float32 and d.last_scale is s
    kept = torch.tensor(1.0 / 0.75, dtype=torch.float32).item()
    assert set(s.unique().tolist()) == {0.0, kept}
    frac = (s != 0).float().mean().item()
    assert abs(frac - 0.75) <= 0.034
    assert set(DropPath(0.25, scale_by_keep=False).draw(4096, DEV).unique().tolist()) == {0.0, 1.0}


def test_train_class_script_reads_the_drop_path_key(tmp_path):
    """train_class_simple.py as in tests/test_hip_models.py::test_train_class_simple_entry_point_runs, with drop_path: 0.1 in the config:
    two epochs, finite loss"""
    import os
    import re
    import subprocess
    import sys
    import yaml
    from conftest import ROOT
    cfg = yaml.safe_load(open(os.path.join(ROOT, "ucf-vit_amd", "configs", "catsdogs_vit_tiny_smoke.yaml")))
    cfg["trainer"]["checkpoint_path"] = str(tmp_path)
    cfg["model"]["net"]["init_args"]["drop_path"] = 0.1
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, MASTER_PORT="29591")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "ucf-vit_amd", "training_scripts", "train_class_simple.py"), str(p)],
                         capture_output=True, text=True, timeout=280, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    losses = [float(v) for v in re.findall(r"epoch_loss ([-+0-9.einfa]+)", out.stdout)]
    assert "epoch: 1" in out.stdout and len(losses) == 2 and all(math.isfinite(v) for v in losses)
