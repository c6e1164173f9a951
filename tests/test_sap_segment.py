"""SAP on a label map that lives in the image plane (GPU): train_sap_simple.py with `data: labels_from_image: True` (labels through the image's own
tree, Patchify.serialize_labels; full-resolution Dice through Patchify.deserialize + HF.segment) and inference_sap_simple.py on its checkpoint,
on the smoke config of tests/test_hip_models.py::test_train_sap_and_unetr_scripts_run_adaptive_configs (64 x 64, patch 8, fixed_length 16, 3 classes)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import yaml

from conftest import ROOT

gpu = pytest.mark.gpu


def _cfg():
    cfg = yaml.safe_load(open(os.path.join(ROOT, "ucf-vit_amd", "configs", "catsdogs_vit_tiny_smoke.yaml")))
    a = cfg["model"]["net"]["init_args"]
    a.update(tile_size=[64, 64], patch_size=8, embed_dim=96, depth=2, num_heads=3, adaptive_patching=True, fixed_length=16, use_adaptive_pos_emb=True)
    cfg["data"]["num_classes"] = 3
    cfg["data"]["batch_size"] = 4
    cfg["model"]["lr"] = 1e-3
    cfg["model"]["warmup_steps"] = 2
    cfg["load_balancing"]["batches_per_rank_epoch"]["catsdogs"] = 6
    return cfg


def _run(script, cfg, tmp_path, port):
    cfg["trainer"]["checkpoint_path"] = str(tmp_path)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "ucf-vit_amd", "training_scripts", script), str(p)], capture_output=True, text=True,
                         timeout=280, env=dict(os.environ, MASTER_PORT=str(port)))
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


EPOCH_LINE = r"epoch: \d+ epoch_loss -?\d+\.\d{4} images/s \d+\.\d"


@gpu
def test_train_and_infer_sap_on_image_plane_labels(tmp_path):
    cfg = _cfg()
    cfg["data"]["labels_from_image"] = True
    out = _run("train_sap_simple.py", cfg, tmp_path, 29591)
    lines = [l for l in out.splitlines() if "epoch_loss" in l]
    assert len(lines) == 2 and all(re.fullmatch(EPOCH_LINE + r" dice \d\.\d{4}", l) for l in lines), out
    losses = [float(l.split("epoch_loss")[1].split()[0]) for l in lines]
    dices = [float(l.split(" dice ")[1]) for l in lines]
    assert all(math.isfinite(v) for v in losses) and losses[1] < losses[0], out
    assert all(0.0 <= d <= 1.0 for d in dices), out
    # inference on the checkpoint of the second epoch
    cfg["trainer"]["resume_from_checkpoint"] = True
    cfg["trainer"]["checkpoint_filename_for_loading"] = cfg["trainer"]["checkpoint_filename"] + "_odd"
    out = _run("inference_sap_simple.py", cfg, tmp_path, 29592)
    dice = [float(l.split()[1]) for l in out.splitlines() if l.startswith("dice ")]
    acc = [l for l in out.splitlines() if l.startswith("acc ")]
    assert len(dice) == 1 and 0.0 <= dice[0] <= 1.0 and len(acc) == 1 and len(acc[0].split()) == 3, out
    pred, true = np.load(tmp_path / "pred_map0.npy"), np.load(tmp_path / "true_map0.npy")
    assert pred.shape == (64, 64) and true.shape == (64, 64) and pred.dtype == np.uint8 and true.dtype == np.uint8
    assert pred.max() <= 2 and true.max() <= 2 and len(np.unique(true)) > 1
    # the printed Dice is the Dice of the two maps (classes 1 and 2, mean over the classes the label map has)
    d = [2.0 * ((pred == k) & (true == k)).sum() / ((pred == k).sum() + (true == k).sum()) for k in (1, 2) if (true == k).any()]
    assert abs(dice[0] - float(np.mean(d))) < 1e-3, (dice, d)


@gpu
def test_train_sap_without_the_key_prints_the_usual_lines(tmp_path):
    out = _run("train_sap_simple.py", _cfg(), tmp_path, 29593)
    lines = [l for l in out.splitlines() if "epoch_loss" in l]
    assert len(lines) == 2 and all(re.fullmatch(EPOCH_LINE, l) for l in lines), out
