#!/usr/bin/env python3
"""UNETR segmentation training — entry point compatible with the reference's training_scripts/train_unetr_simple.py.
The ViT encoder, the convolutional decoder (3x3x3 / transposed / 1x1x1 convolutions on csrc/conv3d.hip, channels-last instance-norm /
LeakyReLU / residual chains on csrc/unetr_decoder.hip) and the Dice+CE loss (monai DiceCELoss(to_onehot_y, softmax, squared_pred) in the
reference, :38; parity unpinned: monai is not vendored) all run on the HIP kernels — the reference's basic_ct/unetr key set (64^3 tile,
patch 4, adaptive patching with fixed_length 729) included: its 9^3 token grid times 16 is not the tile size, so dec1 is resampled to the
tile (csrc/resample.hip) in front of decoder2's pointwise transposed convolution, and the config runs as it is, without extra keys.  A
`twoD: True` config whose token grid times 16 is the tile (configs/unetr2d_smoke.yaml: 32 x 32, patch 16) runs the same decoder in the plane
(3x3 / 2x2 convolutions on csrc/conv2d.hip): labels [B, 1, X, Y], the same loss and accuracy calls.  A configuration those kernels do not
cover (2-D resampling geometries, feature sizes other than 16 / 32 k, ...) needs `allow_torch_decoder: True` in model.net.init_args, else
UNETR.forward raises.
Every step also feeds the raw logits and the labels to a Dice accuracy (reference :399-401,453-460: argmax, one-hot, monai DiceMetric(
include_background=False, MEAN, get_not_nans)): one HIP pass over the logits in place (ucfvit_seg_counts), accumulated on the device and read
with the loss once per epoch: `... epoch_loss L volumes/s R dice D`."""
import sys

import torch
import torch.nn.functional as F

from _common import (GradNormMeter, SyntheticLoader, SyntheticSeqLoader, StepTimer, clip_grad_norm_of, init_distributed, iters_per_epoch,
                     load_config, maybe_resume, model_args, save_checkpoint, seed_drop_path, seed_dropout, seq_to_pseudo_image, sqrt_len_of)
from UCF_VIT.simple.arch import UNETR
from UCF_VIT.utils.fused_attn import FusedAttn
from UCF_VIT.utils.metrics import DiceMetric
from UCF_VIT.utils.misc import configure_optimizer, configure_scheduler
from UCF_VIT._hip.ddp import HipDataParallel
from UCF_VIT._hip import functional as HF


def label_view(logits, label):
    """the loader's [B, 1, *spatial] labels as the [B, *spatial] class-index volume the loss and the accuracy take"""
    return label.view(label.shape[0], *label.shape[2:]) if label.dim() == logits.dim() else label


def dice_ce_loss(logits, label, smooth=1e-5):
    """monai DiceCELoss(to_onehot_y, softmax, squared_pred) (reference :38): DiceLoss over softmax probabilities with the squared-prediction
    denominator, mean over batch and classes, + CrossEntropy — one HIP call (ucfvit_dice_ce: loss and gradient, the decoder's channels-last logits read in place)"""
    return HF.dice_ce(logits.float(), label_view(logits, label), smooth, smooth)


def training_step(data, variables, label, net):
    output = net(data, variables, None, None)
    return dice_ce_loss(output, label), output


def training_step_adaptive(data, seq, label, variables, net, patch_size, twoD, seq_ps, sqrt_len):
    """reference :43-52: the full-resolution volume feeds the first conv encoder, the token sequence (as a pseudo volume) the ViT"""
    output = net(data, variables, seq_ps, seq_to_pseudo_image(seq, sqrt_len, patch_size, twoD))
    return dice_ce_loss(output, label), output


def main(device, local_rank, rank, world):
    conf = load_config(sys.argv[1])
    margs, a, d = model_args(conf)
    adaptive = margs["adaptive_patching"]
    sqrt_len = sqrt_len_of(margs["fixed_length"], margs["twoD"]) if adaptive else None
    m = conf["model"]
    model = UNETR(num_classes=d["num_classes"], class_token=False, weight_init='', linear_decoder=a.get("linear_decoder", False),
                  feature_size=a.get("feature_size", 16), skip_connection=a.get("skip_connection", True), sqrt_len=sqrt_len,
                  allow_torch_decoder=bool(a.get("allow_torch_decoder", False)),   # explicit opt-in for configurations the HIP decoder does not cover
                  sqrt_len_method=adaptive, FusedAttn_option=FusedAttn.HIP, **margs).to(device)
    model.set_compute_dtype(torch.bfloat16 if conf["trainer"].get("data_type", "float32") == "bfloat16" else torch.float32)
    seed_drop_path(model, device, rank)                                      # stochastic depth: ranks must not share a draw
    seed_dropout(model, device, rank)                                        # dropout: neither ranks nor modules share a seed
    net = HipDataParallel(model)
    optimizer = configure_optimizer(model, float(m["lr"]), float(m["beta_1"]), float(m["beta_2"]), float(m["weight_decay"]),
                                    max_grad_norm=clip_grad_norm_of(conf))   # PyYAML reads "1e-5" as str
    scheduler = configure_scheduler(optimizer, int(m["warmup_steps"]), int(m["max_steps"]), float(m["warmup_start_lr"]), float(m["eta_min"]))
    extras = {"dice_list": []}
    epoch_start, loss_list = maybe_resume(conf, net, optimizer, scheduler, extras=extras)
    dice_list = extras["dice_list"]
    variables = d["dict_in_variables"][d["dataset"]]
    loader = SyntheticLoader(d["batch_size"], margs["in_chans"], margs["img_size"], d["num_classes"], iters_per_epoch(conf), device,
                             1234 + rank, volumetric_labels=True)
    seq_loader = SyntheticSeqLoader(d["batch_size"], margs["in_chans"], margs["img_size"], margs["patch_size"], margs["fixed_length"], 0,
                                    iters_per_epoch(conf), device, 4321 + rank) if adaptive else None
    dice_acc = DiceMetric(include_background=False)
    for epoch in range(epoch_start, conf["trainer"]["max_epochs"]):
        model.train()
        epoch_loss = torch.zeros((), device=device)
        dice_acc.reset()
        timer = StepTimer()
        gnorm = GradNormMeter(optimizer, device)                              # `model: clip_grad_norm` only
        seqs = iter(seq_loader) if adaptive else None
        for data, label in loader:
            if adaptive:
                seq, seq_ps, _ = next(seqs)
                loss, output = training_step_adaptive(data / 255.0, seq / 255.0, label, variables, net, margs["patch_size"], margs["twoD"], seq_ps, sqrt_len)
            else:
                loss, output = training_step(data / 255.0, variables, label, net)       # basic_ct volumes are min-max normalised
            epoch_loss += loss.detach()
            with torch.no_grad():
                dice_acc(output, label_view(output, label))      # the raw logits (no fp32 copy): argmax + counts in one pass, state on the device
            del output                                           # (backward needs the gradient the loss kept, not the logits)
            loss.backward()
            optimizer.step()
            gnorm.update()
            optimizer.zero_grad()
            scheduler.step()
            timer.tick(data.shape[0] * world)
        loss_list.append(epoch_loss)
        dice_list.append(dice_acc.aggregate()[0])
        if rank == 0:
            print(f"epoch: {epoch} epoch_loss {epoch_loss.item():.4f} volumes/s {timer.rate():.2f} dice {dice_list[-1].item():.4f}{gnorm.suffix()}", flush=True)
        save_checkpoint(conf, epoch, net, optimizer, scheduler, loss_list, rank, extra={"dice_list": dice_list})


if __name__ == "__main__":
    dev, lr_, r, w = init_distributed(sys.argv[2] if len(sys.argv) > 2 else None)
    main(dev, lr_, r, w)
    torch.distributed.destroy_process_group()
