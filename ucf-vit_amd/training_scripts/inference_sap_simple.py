#!/usr/bin/env python3
"""SAP segmentation inference on adaptively patched input: the model built as train_sap_simple.py builds it,
`checkpoint_path/checkpoint_filename_for_loading.ckpt` loaded when `resume_from_checkpoint` is true, batch size forced to 1, model.eval(),
ONE sample under torch.no_grad() (synthetic data, as in every entry point here: the reference dataloaders are out of scope).

The sample is one synthetic image, a label map in the image plane (brightness bands of the image) and a synthetic edge map.  The image goes
through the GPU quadtree / octree patcher, SAP predicts logits per class in sequence layout, the same tree paints them back into the image
plane (Patchify.deserialize, reading the model's output in place, [1, nc, *img]) and one HIP pass (HF.segment -> ucfvit_seg_counts) writes
the uint8 label map and the counts of the Dice accuracy against the full-resolution labels (DiceMetric(include_background=False)).

Prints `acc` (Dice per non-background class; nan where the label map lacks the class) and the aggregate, and writes pred_map0.npy /
true_map0.npy (uint8, the tile's shape) into checkpoint_path."""
import os
import sys

import numpy as np
import torch

from _common import SyntheticSeqLoader, init_distributed, load_config, maybe_resume, model_args, sqrt_len_of
from UCF_VIT.dataloaders.transform import Patchify, Patchify_3D
from UCF_VIT.simple.arch import SAP
from UCF_VIT.utils.fused_attn import FusedAttn
from UCF_VIT.utils.metrics import DiceMetric
from UCF_VIT.utils.misc import configure_optimizer, configure_scheduler
from UCF_VIT._hip.ddp import HipDataParallel
from UCF_VIT._hip import functional as HF


def main(device, local_rank, rank, world):
    conf = load_config(sys.argv[1])
    margs, a, d = model_args(conf)
    t = conf["trainer"]
    if not margs["adaptive_patching"]:
        raise ValueError("inference_sap_simple.py runs on adaptively patched input: set adaptive_patching True")
    m = conf["model"]
    twoD, p, S, nc = margs["twoD"], margs["patch_size"], margs["fixed_length"], d["num_classes"]
    sqrt_len = sqrt_len_of(S, twoD)
    model = SAP(num_classes=nc, sqrt_len=sqrt_len, sqrt_len_method=True, class_token=False, weight_init='skip', FusedAttn_option=FusedAttn.HIP,
                **margs).to(device)
    model.set_compute_dtype(torch.bfloat16 if t.get("data_type", "float32") == "bfloat16" else torch.float32)
    net = HipDataParallel(model)
    optimizer = configure_optimizer(model, float(m["lr"]), float(m["beta_1"]), float(m["beta_2"]), float(m["weight_decay"]))
    scheduler = configure_scheduler(optimizer, int(m["warmup_steps"]), int(m["max_steps"]), float(m["warmup_start_lr"]), float(m["eta_min"]))
    maybe_resume(conf, net, optimizer, scheduler)
    variables = d["dict_in_variables"][d["dataset"]]
    loader = SyntheticSeqLoader(1, margs["in_chans"], margs["img_size"], p, S, nc, 1, device, 4321 + rank, labels_from_image=True)
    patcher = (Patchify if twoD else Patchify_3D)(S, p, nc)
    side = (p * sqrt_len,) * (2 if twoD else 3)
    dice_acc = DiceMetric(include_background=False)
    model.eval()
    os.makedirs(t["checkpoint_path"], exist_ok=True)
    for i, (seq, seq_ps, (_, label_map, nodes, count)) in enumerate(loader):
        with torch.no_grad():
            output = net(torch.reshape(seq / 255.0, (-1, margs["in_chans"]) + side), variables, seq_ps)
            logits = output.float().reshape(output.shape[0], nc, S, -1)          # the pseudo image's memory is [B, nc, S, P]
            size = tuple(label_map.shape[1:]) if twoD else label_map.shape[1]
            full = patcher.deserialize(logits, nodes, count, size, channels_last=False)
            pred, counts = HF.segment(full, label_map)
            del output, logits, full
            acc = dice_acc.update(counts)
        mean, not_nans = dice_acc.aggregate()
        if rank == 0:
            print("acc", " ".join(f"{v:.4f}" for v in acc[0].tolist()), flush=True)
            print(f"dice {mean.item():.4f} not_nans {int(not_nans.item())}", flush=True)
            np.save(os.path.join(t["checkpoint_path"], f"pred_map{i}.npy"), pred[0].cpu().numpy())
            np.save(os.path.join(t["checkpoint_path"], f"true_map{i}.npy"), label_map[0].to(torch.uint8).cpu().numpy())
        torch.distributed.barrier()


if __name__ == "__main__":
    dev, lr_, r, w = init_distributed(sys.argv[2] if len(sys.argv) > 2 else None)
    main(dev, lr_, r, w)
    torch.distributed.destroy_process_group()
