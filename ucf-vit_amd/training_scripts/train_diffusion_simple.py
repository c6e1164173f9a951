#!/usr/bin/env python3
"""DDPM noise-prediction training on the MI355X hot path — entry point compatible with the reference's
training_scripts/train_diffusion_simple.py:  python train_diffusion_simple.py <config.yaml> [MPI]

Per batch (reference :322-344): t ~ U{0..T-1} per sample, e ~ N(0, I), x_t = sqrt(abar_t) x + sqrt(1 - abar_t) e, loss =
MSE(unpatchify(model(x_t, t)), e).  Here t and e are drawn on the device from a per-rank generator, the noising is HF.q_sample, and the loss
kernel reads e in place (HF.patch_mse without a mask is MSELoss(unpatchify(pred), e)); unpatchify(pred) is never materialised.

`model: ema_decay` (absent: off) keeps an exponential moving average of the weights inside the AdamW pass; the checkpoint then also holds
`model_ema_state_dict`, which inference_diffusion_simple.py samples from and a resumed run continues."""
import sys

import torch

from _common import (GradNormMeter, SyntheticLoader, StepTimer, init_distributed, iters_per_epoch, load_config, maybe_resume, model_args, save_checkpoint,
                     clip_grad_norm_of, seed_drop_path, seed_dropout)
from UCF_VIT.simple.arch import DiffusionVIT
from UCF_VIT.ddpm.ddpm import DDPM_Scheduler
from UCF_VIT.utils.fused_attn import FusedAttn
from UCF_VIT.utils.misc import configure_grad_scaler, configure_optimizer, configure_scheduler
from UCF_VIT._hip import functional as HF
from UCF_VIT._hip.ddp import HipDataParallel


def diffusion_args(conf):
    """the DiffusionVIT keywords of the reference's script (:206-229) from the config, `num_time_steps` among them"""
    margs, a, d = model_args(conf)
    margs.pop("use_adaptive_pos_emb")                              # the reference's script does not pass it
    margs.update(linear_decoder=a["linear_decoder"], decoder_depth=a["decoder_depth"], decoder_embed_dim=a["decoder_embed_dim"],
                 decoder_num_heads=a["decoder_num_heads"], mlp_ratio_decoder=a["mlp_ratio_decoder"], time_steps=int(a["num_time_steps"]),
                 class_token=False)
    return margs, a, d


def build_model(conf, device):
    margs, a, d = diffusion_args(conf)
    model = DiffusionVIT(weight_init='skip', FusedAttn_option=FusedAttn.HIP, **margs).to(device)
    model.set_compute_dtype(torch.bfloat16 if conf["trainer"].get("data_type", "float32") == "bfloat16" else torch.float32)
    return model, margs, a, d


def training_step(data, variables, t, e, net, ddpm, patch_size, loss_fn):
    if loss_fn != "MSE":
        raise ValueError(f"loss_fn={loss_fn!r}: the diffusion script knows \"MSE\"")
    x_t = ddpm.q_sample(data, t, e)
    return HF.patch_mse(net(x_t, t, variables), e, patch_size)


def resume(conf, net, optimizer, scheduler, scaler):
    """maybe_resume, and under `model: ema_decay` the weights' moving average from the checkpoint's `model_ema_state_dict`; a checkpoint
    written without one resumes with the average restarted from the loaded weights"""
    extras = {"model_ema_state_dict": None}
    epoch_start, loss_list = maybe_resume(conf, net, optimizer, scheduler, scaler, extras=extras)
    if optimizer.ema_decay is not None and extras["model_ema_state_dict"] is not None:
        optimizer.load_ema_state_dict(net, extras["model_ema_state_dict"])
    return epoch_start, loss_list


def main(device, local_rank, rank, world):
    conf = load_config(sys.argv[1])
    model, margs, a, d = build_model(conf, device)
    m = conf["model"]
    ddpm = DDPM_Scheduler(num_time_steps=margs["time_steps"]).to(device)
    seed_drop_path(model, device, rank)                                      # stochastic depth: ranks must not share a draw
    gen = torch.Generator(device=device)                                     # t and e: one device stream per rank

    def reseed():
        gen.manual_seed(torch.initial_seed() + 7919 * (rank + 1))
        seed_dropout(model, device, rank)                                    # the time MLP's dropout: neither ranks nor modules share a seed

    reseed()                                                                 # once: every visit of an image meets fresh t, noise and mask
    # `trainer: replay_noise_per_epoch: True` (off by default; configs/diffusion_smoke.yaml sets it) restarts these streams at every epoch.
    # It is meant for the synthetic loader, which replays the same batches every epoch: the epoch losses then differ by the weights alone
    # and can be compared.  It is not DDPM training: each image would meet one (t, noise, mask) for the whole run.
    replay = bool(conf["trainer"].get("replay_noise_per_epoch", False))
    net = HipDataParallel(model)
    ema_decay = m.get("ema_decay")
    optimizer = configure_optimizer(model, float(m["lr"]), float(m["beta_1"]), float(m["beta_2"]), float(m["weight_decay"]),
                                    ema_decay=None if ema_decay is None else float(ema_decay), max_grad_norm=clip_grad_norm_of(conf))
    scheduler = configure_scheduler(optimizer, int(m["warmup_steps"]), int(m["max_steps"]), float(m["warmup_start_lr"]), float(m["eta_min"]))
    scaler = configure_grad_scaler(bool(m.get("use_grad_scaler", False)))
    epoch_start, loss_list = resume(conf, net, optimizer, scheduler, scaler)
    variables = d["dict_in_variables"][d["dataset"]]
    loss_fn = m.get("loss_fn", "MSE")
    loader = SyntheticLoader(d["batch_size"], margs["in_chans"], margs["img_size"], 0, iters_per_epoch(conf), device, 1234 + rank)
    for epoch in range(epoch_start, conf["trainer"]["max_epochs"]):
        model.train()
        if replay and epoch > epoch_start:
            reseed()
        epoch_loss = torch.zeros((), device=device)
        timer = StepTimer()
        gnorm = GradNormMeter(optimizer, device)                              # `model: clip_grad_norm` only
        for data, _ in loader:
            data = data / 255.0
            t = torch.randint(0, margs["time_steps"], (data.shape[0],), device=device, generator=gen)
            e = torch.randn(data.shape, dtype=torch.float32, device=device, generator=gen)
            loss = training_step(data, variables, t, e, net, ddpm, margs["patch_size"], loss_fn)
            epoch_loss += loss.detach()
            if scaler.is_enabled():
                scaler.scale(loss).backward()
                scaler.step(optimizer)
                scaler.update()
            else:
                loss.backward()
                optimizer.step()
            gnorm.update()
            optimizer.zero_grad()
            scheduler.step()
            timer.tick(data.shape[0] * world)
        loss_list.append(epoch_loss)
        if rank == 0:
            print(f"epoch: {epoch} epoch_loss {epoch_loss.item():.4f} images/s {timer.rate():.1f}{gnorm.suffix()}", flush=True)
        save_checkpoint(conf, epoch, net, optimizer, scheduler, loss_list, rank, scaler,
                        extra=None if ema_decay is None else {"model_ema_state_dict": optimizer.ema_state_dict(net)})


if __name__ == "__main__":
    dev, lr_, r, w = init_distributed(sys.argv[2] if len(sys.argv) > 2 else None)
    main(dev, lr_, r, w)
    torch.distributed.destroy_process_group()
