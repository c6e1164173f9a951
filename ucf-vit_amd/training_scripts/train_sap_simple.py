#!/usr/bin/env python3
"""SAP segmentation training on adaptively patched input — entry point compatible with the reference's
training_scripts/train_sap_simple.py:  python train_sap_simple.py <config.yaml> [MPI]
The whole step runs on the HIP kernels: the ViT encoder (patch-embedding convolution on the pseudo image, position embedding from
seq_ps, Blocks), the transposed-convolution neck and the 1x1 header folded into one Linear layer plus a scatter (HF.SapHeadFn), and the
Dice+BCE loss (HF.DiceBCEFn behind utils/metrics.DiceBLoss)."""
import sys

import torch

from _common import (GradNormMeter, SyntheticSeqLoader, StepTimer, clip_grad_norm_of, init_distributed, iters_per_epoch, load_config,
                     maybe_resume, model_args, save_checkpoint, seed_drop_path, seed_dropout, sqrt_len_of)
from UCF_VIT.simple.arch import SAP
from UCF_VIT.utils.fused_attn import FusedAttn
from UCF_VIT.utils.metrics import DiceBLoss
from UCF_VIT.utils.misc import configure_optimizer, configure_scheduler
from UCF_VIT._hip.ddp import HipDataParallel


def training_step_adaptive(seq, seq_label, variables, net, patch_size, twoD, num_classes, sqrt_len, seq_ps, in_chans):
    """reference :28-46 (plain reshape of the token sequence into the pseudo image, as there)"""
    side = (patch_size * sqrt_len,) * (2 if twoD else 3)
    seq = torch.reshape(seq, (-1, in_chans) + side)
    seq_label = torch.reshape(seq_label, (-1, num_classes) + side)
    output = net(seq, variables, seq_ps)
    return DiceBLoss(num_class=num_classes)(output, seq_label), output


def training_step_full_resolution(seq, label_map, nodes, count, variables, net, patch_size, twoD, num_classes, sqrt_len, seq_ps, in_chans,
                                  fixed_length):
    """data: loss_at_full_resolution: the logits per class [B, nc, S, P] (the pseudo image's plain memory) are painted through the image's tree
    into [B, nc, *img] under autograd (HF.deserialize) and the Dice+BCE loss is taken there against the one-hot of the label map, so that a
    leaf weighs what it covers; the gradient comes back through the tree (ops.*_deserialize_bwd) into the head"""
    from UCF_VIT.dataloaders.transform import Patchify, Patchify_3D
    side = (patch_size * sqrt_len,) * (2 if twoD else 3)
    output = net(torch.reshape(seq, (-1, in_chans) + side), variables, seq_ps)
    logits = output.reshape(output.shape[0], num_classes, fixed_length, -1)
    patcher = (Patchify if twoD else Patchify_3D)(fixed_length, patch_size, num_classes)
    size = tuple(label_map.shape[1:]) if twoD else label_map.shape[1]
    full = patcher.deserialize(logits, nodes, count, size, channels_last=False)
    target = torch.nn.functional.one_hot(label_map.long(), num_classes).movedim(-1, 1).float().contiguous()
    return DiceBLoss(num_class=num_classes)(full, target), output


def full_resolution_dice(output, label_map, nodes, count, patch_size, num_classes, fixed_length, twoD):
    """Dice of a SAP prediction against the label map in the image plane: the pseudo image's plain memory is the logits per class in
    sequence layout [B, nc, S, P]; the tree paints them back (read in place) into [B, nc, *img] and one HIP pass takes argmax and counts"""
    from UCF_VIT.dataloaders.transform import Patchify, Patchify_3D
    from UCF_VIT.utils.metrics import DiceMetric
    from UCF_VIT._hip import functional as HF
    with torch.no_grad():
        logits = output.detach().float().reshape(output.shape[0], num_classes, fixed_length, -1)
        patcher = (Patchify if twoD else Patchify_3D)(fixed_length, patch_size, num_classes)
        size = tuple(label_map.shape[1:]) if twoD else label_map.shape[1]
        full = patcher.deserialize(logits, nodes, count, size, channels_last=False)
        pred, counts = HF.segment(full, label_map)
        metric = DiceMetric(include_background=False)
        metric.update(counts)
        return metric.aggregate()[0], pred


def main(device, local_rank, rank, world):
    conf = load_config(sys.argv[1])
    margs, a, d = model_args(conf)
    if not margs["adaptive_patching"]:
        raise ValueError("train_sap_simple.py trains on adaptively patched input (the reference script has no other path): set adaptive_patching True")
    m = conf["model"]
    sqrt_len = sqrt_len_of(margs["fixed_length"], margs["twoD"])
    nc = d["num_classes"]
    model = SAP(num_classes=nc, sqrt_len=sqrt_len, sqrt_len_method=True, class_token=False, weight_init='skip', FusedAttn_option=FusedAttn.HIP,
                **margs).to(device)
    model.set_compute_dtype(torch.bfloat16 if conf["trainer"].get("data_type", "float32") == "bfloat16" else torch.float32)
    seed_drop_path(model, device, rank)                                      # stochastic depth: ranks must not share a draw
    seed_dropout(model, device, rank)                                        # dropout: neither ranks nor modules share a seed
    net = HipDataParallel(model)
    optimizer = configure_optimizer(model, float(m["lr"]), float(m["beta_1"]), float(m["beta_2"]), float(m["weight_decay"]),
                                    max_grad_norm=clip_grad_norm_of(conf))
    scheduler = configure_scheduler(optimizer, int(m["warmup_steps"]), int(m["max_steps"]), float(m["warmup_start_lr"]), float(m["eta_min"]))
    epoch_start, loss_list = maybe_resume(conf, net, optimizer, scheduler)
    variables = d["dict_in_variables"][d["dataset"]]
    # data: labels_from_image: True -- the label map lives in the image plane and reaches the sequence through the image's own tree
    # (Patchify.serialize_labels), and the epoch line reports the full-resolution Dice of the last batch (deserialize + segment)
    from_image = bool(d.get("labels_from_image", False))
    # data: loss_at_full_resolution: True -- the loss itself is taken in the image plane (training_step_full_resolution), not on the token grid
    full_loss = bool(d.get("loss_at_full_resolution", False))
    if full_loss and not from_image:
        raise ValueError("data: loss_at_full_resolution needs the label map and the tree of the image: set data: labels_from_image: True")
    loader = SyntheticSeqLoader(d["batch_size"], margs["in_chans"], margs["img_size"], margs["patch_size"], margs["fixed_length"], nc,
                                iters_per_epoch(conf), device, 1234 + rank, labels_from_image=from_image)
    for epoch in range(epoch_start, conf["trainer"]["max_epochs"]):
        model.train()
        epoch_loss = torch.zeros((), device=device)
        timer = StepTimer()
        gnorm = GradNormMeter(optimizer, device)                              # `model: clip_grad_norm` only
        for seq, seq_ps, extra in loader:
            if from_image:
                seq_label, label_map, nodes, count = extra
            else:
                # synthetic per-pixel labels from the data itself (brightness bands), one-hot over the classes, in sequence layout
                band = torch.clamp((seq.mean(dim=1, keepdim=True) / 256.0 * nc).long(), 0, nc - 1)
                seq_label = torch.zeros(seq.shape[0], nc, *seq.shape[2:], device=device).scatter_(1, band, 1.0)
            if full_loss:
                loss, output = training_step_full_resolution(seq / 255.0, label_map, nodes, count, variables, net, margs["patch_size"], margs["twoD"],
                                                             nc, sqrt_len, seq_ps, margs["in_chans"], margs["fixed_length"])
            else:
                loss, output = training_step_adaptive(seq / 255.0, seq_label, variables, net, margs["patch_size"], margs["twoD"], nc, sqrt_len,
                                                      seq_ps, margs["in_chans"])
            epoch_loss += loss.detach()
            loss.backward()
            optimizer.step()
            gnorm.update()
            optimizer.zero_grad()
            scheduler.step()
            timer.tick(seq.shape[0] * world)
        loss_list.append(epoch_loss)
        dice = ""
        if from_image:
            mean, _ = full_resolution_dice(output, label_map, nodes, count, margs["patch_size"], nc, margs["fixed_length"], margs["twoD"])
            dice = f" dice {mean.item():.4f}"
        if rank == 0:
            print(f"epoch: {epoch} epoch_loss {epoch_loss.item():.4f} images/s {timer.rate():.1f}{dice}{gnorm.suffix()}", flush=True)
        save_checkpoint(conf, epoch, net, optimizer, scheduler, loss_list, rank)


if __name__ == "__main__":
    dev, lr_, r, w = init_distributed(sys.argv[2] if len(sys.argv) > 2 else None)
    main(dev, lr_, r, w)
    torch.distributed.destroy_process_group()
