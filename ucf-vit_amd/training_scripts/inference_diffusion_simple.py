#!/usr/bin/env python3
"""DDPM sampling with a trained DiffusionVIT:  python inference_diffusion_simple.py <config.yaml> [MPI]

Builds the model as train_diffusion_simple.py does, loads `checkpoint_path/checkpoint_filename_for_loading.ckpt`, draws
`trainer: num_samples` (default 4) images with DDPM_Scheduler.sample (ancestral sampling, every reverse step on the HIP kernels, no
device-to-host synchronisation inside the loop) and writes them to checkpoint_path/samples.npy (fp32 [n, C, *tile_size])."""
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
    model.load_state_dict({strip(k): v for k, v in ck["model_state_dict"].items()})
    ddpm = DDPM_Scheduler(num_time_steps=margs["time_steps"]).to(device)
    n = int(t.get("num_samples", 4))
    gen = torch.Generator(device=device)
    gen.manual_seed(torch.initial_seed() + 104729 * (rank + 1))
    variables = d["dict_in_variables"][d["dataset"]]
    x = ddpm.sample(model, (n, margs["in_chans"], *margs["img_size"]), variables, generator=gen)
    if rank == 0:
        out = x.cpu().numpy()
        np.save(os.path.join(t["checkpoint_path"], "samples.npy"), out)
        print(f"samples {tuple(out.shape)} mean {out.mean():.4f} std {out.std():.4f} finite {bool(np.isfinite(out).all())}", flush=True)
    torch.distributed.barrier()


if __name__ == "__main__":
    dev, lr_, r, w = init_distributed(sys.argv[2] if len(sys.argv) > 2 else None)
    main(dev, lr_, r, w)
    torch.distributed.destroy_process_group()
