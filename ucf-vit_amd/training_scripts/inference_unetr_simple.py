#!/usr/bin/env python3
"""UNETR segmentation inference — entry point compatible with the reference's training_scripts/inference_unetr_simple.py: the same config keys,
the model built as train_unetr_simple.py builds it, `checkpoint_path/checkpoint_filename_for_loading.ckpt` loaded when
`resume_from_checkpoint` is true, batch size forced to 1, model.eval(), ONE sample under torch.no_grad() (synthetic loaders, as in every
entry point here: the reference dataloaders are out of scope).  The logits never leave the decoder's channels-last buffer: one HIP pass
(HF.segment -> ucfvit_seg_counts) writes the uint8 label volume and the counts of the Dice accuracy (reference :383-385,418-424: argmax,
one-hot, monai DiceMetric(include_background=False, MEAN, get_not_nans); parity unpinned, monai is not vendored).

Prints `acc` (Dice per non-background class; nan where the label volume lacks the class) and the aggregate, and writes
pred_volume0.npy / true_volume0.npy (uint8, the tile's shape: a 2-D array for a `twoD: True` config such as configs/unetr2d_smoke.yaml, whose
decoder runs on csrc/conv2d.hip) into checkpoint_path.

Deliberate departure: the reference always writes one matplotlib PNG per slice for prediction and label (2 Z figures at 200 dpi, minutes for
a 128-slice volume, into the working directory).  Here the volumes go to the two .npy files and the PNG slices are written (into
checkpoint_path, same file names) only with `trainer: dump_png: True`; the default is off.

The no-grad forward keeps no activations: every autograd Function of the HIP path stores tensors through ctx only, which torch drops when
gradients are off, and the weight-gradient queue is filled in backward only."""
import os
import sys

import numpy as np
import torch

from _common import SyntheticLoader, SyntheticSeqLoader, init_distributed, load_config, maybe_resume, model_args, seq_to_pseudo_image, sqrt_len_of
from UCF_VIT.simple.arch import UNETR
from UCF_VIT.utils.fused_attn import FusedAttn
from UCF_VIT.utils.metrics import DiceMetric
from UCF_VIT.utils.misc import configure_optimizer, configure_scheduler
from UCF_VIT._hip.ddp import HipDataParallel
from UCF_VIT._hip import functional as HF


def dump_png(pred, true, num_classes, twoD, out_dir, i):
    """the reference's per-slice figures (:426-457)"""
    from matplotlib import pyplot as plt
    slices = [(pred, true, str(i))] if twoD else [(pred[..., j], true[..., j], f"{i}{j}") for j in range(pred.shape[-1])]
    for p, t, tag in slices:
        for img, name in ((p, "pred_image"), (t, "true_image")):
            fig, ax = plt.subplots()
            im = ax.imshow(np.squeeze(img), vmin=0, vmax=num_classes - 1)
            fig.colorbar(im, cax=fig.add_axes([0.85, 0.15, 0.03, 0.7]))
            plt.savefig(os.path.join(out_dir, f"{name}{tag}.png"), bbox_inches='tight', dpi=200)
            plt.close(fig)


def main(device, local_rank, rank, world):
    conf = load_config(sys.argv[1])
    margs, a, d = model_args(conf)
    t = conf["trainer"]
    adaptive = margs["adaptive_patching"]
    sqrt_len = sqrt_len_of(margs["fixed_length"], margs["twoD"]) if adaptive else None
    m = conf["model"]
    model = UNETR(num_classes=d["num_classes"], class_token=False, weight_init='', linear_decoder=a.get("linear_decoder", False),
                  feature_size=a.get("feature_size", 16), skip_connection=a.get("skip_connection", True), sqrt_len=sqrt_len,
                  allow_torch_decoder=bool(a.get("allow_torch_decoder", False)),
                  sqrt_len_method=adaptive, FusedAttn_option=FusedAttn.HIP, **margs).to(device)
    model.set_compute_dtype(torch.bfloat16 if t.get("data_type", "float32") == "bfloat16" else torch.float32)
    net = HipDataParallel(model)
    optimizer = configure_optimizer(model, float(m["lr"]), float(m["beta_1"]), float(m["beta_2"]), float(m["weight_decay"]))
    scheduler = configure_scheduler(optimizer, int(m["warmup_steps"]), int(m["max_steps"]), float(m["warmup_start_lr"]), float(m["eta_min"]))
    maybe_resume(conf, net, optimizer, scheduler)                     # (the reference restores optimizer and scheduler too, :332-338)
    variables = d["dict_in_variables"][d["dataset"]]
    batch_size = 1                                                    # reference :160
    loader = SyntheticLoader(batch_size, margs["in_chans"], margs["img_size"], d["num_classes"], 1, device, 1234 + rank, volumetric_labels=True)
    seq_loader = SyntheticSeqLoader(batch_size, margs["in_chans"], margs["img_size"], margs["patch_size"], margs["fixed_length"], 0, 1, device,
                                    4321 + rank) if adaptive else None
    dice_acc = DiceMetric(include_background=False)
    model.eval()
    os.makedirs(t["checkpoint_path"], exist_ok=True)
    seqs = iter(seq_loader) if adaptive else None
    for i, (data, label) in enumerate(loader):                        # num_samples = 1 (reference :391)
        with torch.no_grad():
            if adaptive:
                seq, seq_ps, _ = next(seqs)
                output = net(data / 255.0, variables, seq_ps, seq_to_pseudo_image(seq / 255.0, sqrt_len, margs["patch_size"], margs["twoD"]))
            else:
                output = net(data / 255.0, variables, None, None)
            pred, counts = HF.segment(output, label)
            del output
            acc = dice_acc.update(counts)
        mean, not_nans = dice_acc.aggregate()
        if rank == 0:
            print("acc", " ".join(f"{v:.4f}" for v in acc[0].tolist()), flush=True)
            print(f"dice {mean.item():.4f} not_nans {int(not_nans.item())}", flush=True)
            pred_np = pred[0].cpu().numpy()
            true_np = label.view(label.shape[0], *label.shape[2:])[0].to(torch.uint8).cpu().numpy()
            np.save(os.path.join(t["checkpoint_path"], f"pred_volume{i}.npy"), pred_np)
            np.save(os.path.join(t["checkpoint_path"], f"true_volume{i}.npy"), true_np)
            if t.get("dump_png", False):
                dump_png(pred_np, true_np, d["num_classes"], margs["twoD"], t["checkpoint_path"], i)
        torch.distributed.barrier()


if __name__ == "__main__":
    dev, lr_, r, w = init_distributed(sys.argv[2] if len(sys.argv) > 2 else None)
    main(dev, lr_, r, w)
    torch.distributed.destroy_process_group()
