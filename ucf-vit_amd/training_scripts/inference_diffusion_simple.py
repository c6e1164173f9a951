#!/usr/bin/env python3
"""DDPM sampling with a trained DiffusionVIT:  python inference_diffusion_simple.py <config.yaml> [MPI]

Builds the model as train_diffusion_simple.py does, loads `checkpoint_path/checkpoint_filename_for_loading.ckpt`, draws
`trainer: num_samples` (default 4) images and writes them to checkpoint_path/samples.npy (fp32 [n, C, *tile_size]).  Every reverse step
runs on the HIP kernels, with no device-to-host synchronisation inside the loop.

`trainer:` keys: `sampler` "ddpm" (default: DDPM_Scheduler.sample, ancestral, one model forward per time step) or "ddim"
(DDPM_Scheduler.sample_ddim over `sampler_steps` (default 50) strided steps with `sampler_eta` (default 0: deterministic) and `clip_denoised`
(default none: the bound the predicted x0 is clamped to)); `use_ema` (default: true when the checkpoint holds `model_ema_state_dict`): sample
from the averaged weights."""
import os
import sys

import numpy as np
import torch

from _common import init_distributed, load_config
from train_diffusion_simple import build_model
from UCF_VIT.ddpm.ddpm import DDPM_Scheduler


def main(device, local_rank, rank, world):
    conf = load_config(sys.argv[1])
    t = conf["trainer"]
    model, margs, a, d = build_model(conf, device)
    ck = torch.load(os.path.join(t["checkpoint_path"], t["checkpoint_filename_for_loading"] + ".ckpt"), map_location="cpu", weights_only=True)
    strip = lambda k: k[len("module."):] if k.startswith("module.") else k
    use_ema = bool(t.get("use_ema", "model_ema_state_dict" in ck))
    if use_ema and "model_ema_state_dict" not in ck:
        raise KeyError("use_ema: the checkpoint holds no model_ema_state_dict (train with `model: ema_decay`)")
    model.load_state_dict({strip(k): v for k, v in ck["model_ema_state_dict" if use_ema else "model_state_dict"].items()})
    ddpm = DDPM_Scheduler(num_time_steps=margs["time_steps"]).to(device)
    n = int(t.get("num_samples", 4))
    gen = torch.Generator(device=device)
    gen.manual_seed(torch.initial_seed() + 104729 * (rank + 1))
    variables = d["dict_in_variables"][d["dataset"]]
    shape = (n, margs["in_chans"], *margs["img_size"])
    sampler = t.get("sampler", "ddpm")
    if sampler == "ddpm":
        steps = ddpm.num_time_steps
        x = ddpm.sample(model, shape, variables, generator=gen)
    elif sampler == "ddim":
        steps = int(t.get("sampler_steps", 50))
        clip = t.get("clip_denoised")
        x = ddpm.sample_ddim(model, shape, variables, num_steps=steps, eta=float(t.get("sampler_eta", 0.0)),
                             clip_denoised=None if clip is None else float(clip), generator=gen)
    else:
        raise ValueError(f"trainer: sampler={sampler!r}: \"ddpm\" or \"ddim\"")
    if rank == 0:
        out = x.cpu().numpy()
        np.save(os.path.join(t["checkpoint_path"], "samples.npy"), out)
        print(f"sampler {sampler} steps {steps} weights {'ema' if use_ema else 'raw'} samples {tuple(out.shape)} mean {out.mean():.4f} std {out.std():.4f} finite {bool(np.isfinite(out).all())}", flush=True)
    torch.distributed.barrier()


if __name__ == "__main__":
    dev, lr_, r, w = init_distributed(sys.argv[2] if len(sys.argv) > 2 else None)
    main(dev, lr_, r, w)
    torch.distributed.destroy_process_group()
