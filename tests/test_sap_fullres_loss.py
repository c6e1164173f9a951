"""SAP trained on a loss taken at full resolution (GPU): `data: loss_at_full_resolution: True` of train_sap_simple.py paints the logits per class
through the image's tree under autograd (HF.deserialize, backward = ucfvit_quadtree_deserialize_bwd) and takes the Dice+BCE loss in the image
plane.  On the tiny SAP of tests/test_sap_segment.py (64 x 64, patch 8, fixed_length 16, 3 classes): the gradient with respect to the model's
output against the per-leaf F.interpolate loop under torch autograd, within loop_tolerance of tests/test_patcher_label_bwd_ops.py evaluated on
the loss's own gradient in the image plane (both sides' fp32 summation bounds, the distance of two fp32 evaluations of the weights, and the
difference of the two upstream gradients carried through |w|); thirty AdamW steps on one batch; the script with and without its keys."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_patcher_label_bwd_ops import _interp_loop, loop_tolerance  # noqa: E402
from test_sap_segment import EPOCH_LINE, _cfg, _run  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda"
SCRIPTS = os.path.join(ROOT, "ucf-vit_amd", "training_scripts")


def _setup(seed=0):
    """the model, one batch and the step arguments, as train_sap_simple.main builds them (without the data-parallel wrapper)"""
    for q in (SCRIPTS, os.path.join(ROOT, "ucf-vit_amd")):
        if q not in sys.path:
            sys.path.insert(0, q)
    import _common
    import train_sap_simple as T
    from UCF_VIT.simple.arch import SAP
    from UCF_VIT.utils.fused_attn import FusedAttn
    conf = _cfg()
    margs, a, d = _common.model_args(conf)
    nc, L = d["num_classes"], margs["fixed_length"]
    sqrt_len = _common.sqrt_len_of(L, margs["twoD"])
    torch.manual_seed(seed)
    model = SAP(num_classes=nc, sqrt_len=sqrt_len, sqrt_len_method=True, class_token=False, weight_init='skip', FusedAttn_option=FusedAttn.HIP,
                **margs).to(DEV)
    model.set_compute_dtype(torch.float32)
    loader = _common.SyntheticSeqLoader(d["batch_size"], margs["in_chans"], margs["img_size"], margs["patch_size"], L, nc, 1, DEV, 1234,
                                        labels_from_image=True)
    seq, seq_ps, (seq_label, label_map, nodes, count) = next(iter(loader))
    step = dict(variables=d["dict_in_variables"][d["dataset"]], net=model, patch_size=margs["patch_size"], twoD=margs["twoD"], num_classes=nc,
                sqrt_len=sqrt_len, seq_ps=seq_ps, in_chans=margs["in_chans"], fixed_length=L)
    return T, conf, model, seq / 255.0, label_map, nodes, count, step


@gpu
def test_full_resolution_loss_gradient_matches_the_interpolate_loop():
    from UCF_VIT.dataloaders.transform import Patchify
    from UCF_VIT.utils.metrics import DiceBLoss
    T, _, model, seq, label_map, nodes, count, step = _setup()
    nc, L, p = step["num_classes"], step["fixed_length"], step["patch_size"]
    n = label_map.shape[1]
    loss, output = T.training_step_full_resolution(seq, label_map, nodes, count, **step)
    assert loss.requires_grad and math.isfinite(loss.item())
    target = torch.nn.functional.one_hot(label_map.long(), nc).movedim(-1, 1).float().contiguous()
    grads, fulls = [], []
    for path in ("hip", "loop"):
        o = output.detach().float().clone().requires_grad_(True)
        logits = o.reshape(o.shape[0], nc, L, -1)
        full = Patchify(L, p, nc).deserialize(logits, nodes, count, (n, n), channels_last=False) if path == "hip" else \
            _interp_loop(2, logits, nodes, count, n)
        full.retain_grad()
        l2 = DiceBLoss(num_class=nc)(full, target)
        if path == "hip":
            assert l2.item() == loss.item(), "the step's loss is not the loss of its parts"
        l2.backward()
        grads.append(o.grad.reshape(o.shape[0], nc, L, -1))
        fulls.append(full.grad)
    tol = loop_tolerance(2, fulls[0], nodes, count, n, p, g_other=fulls[1])
    err = (grads[0] - grads[1]).abs().double().cpu().numpy()
    q = np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))
    print(f"RATIO d loss / d output, HIP against the interpolate loop: worst err/bound {q.max():.3f}")
    assert (err <= tol).all(), f"worst err/bound {q.max():.3g}"
    assert float(grads[1].abs().max()) > 100 * float(tol.max()), "the bound is vacuous against the gradient"


@gpu
def test_thirty_steps_on_one_batch_lower_the_full_resolution_loss():
    from UCF_VIT.utils.misc import configure_optimizer
    T, conf, model, seq, label_map, nodes, count, step = _setup(seed=3)
    m = conf["model"]
    opt = configure_optimizer(model, 1e-3, float(m["beta_1"]), float(m["beta_2"]), float(m["weight_decay"]))
    model.train()
    losses = []
    for _ in range(30):
        loss, _ = T.training_step_full_resolution(seq, label_map, nodes, count, **step)
        losses.append(loss.item())
        loss.backward()
        opt.step()
        opt.zero_grad()
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses


@gpu
def test_train_sap_with_the_loss_at_full_resolution(tmp_path):
    cfg = _cfg()
    cfg["data"]["labels_from_image"] = True
    cfg["data"]["loss_at_full_resolution"] = True
    out = _run("train_sap_simple.py", cfg, tmp_path, 29594)
    lines = [l for l in out.splitlines() if "epoch_loss" in l]
    assert len(lines) == 2 and all(re.fullmatch(EPOCH_LINE + r" dice \d\.\d{4}", l) for l in lines), out
    assert all(math.isfinite(float(l.split("epoch_loss")[1].split()[0])) and 0.0 <= float(l.split(" dice ")[1]) <= 1.0 for l in lines), out


@gpu
def test_loss_at_full_resolution_needs_labels_from_image(tmp_path):
    cfg = _cfg()
    cfg["data"]["loss_at_full_resolution"] = True
    cfg["trainer"]["checkpoint_path"] = str(tmp_path)
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    out = subprocess.run([sys.executable, os.path.join(SCRIPTS, "train_sap_simple.py"), str(path)], capture_output=True, text=True, timeout=280,
                         env=dict(os.environ, MASTER_PORT="29595"))
    assert out.returncode != 0 and "labels_from_image" in out.stderr, out.stderr[-2000:]
    assert "epoch_loss" not in out.stdout
