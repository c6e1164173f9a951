#!/usr/bin/env python3
"""GPU quadtree patcher vs the CPU oracle (the reference's per-image Python loop restated): images/s at 256^2, fixed_length 196, p 16; and the
GPU octree patcher at the basic_ct/sap shape: B = 2, 64^3, fixed_length 512, p = 4, the contour volumes of tools/patcher_labels_bench.py."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from UCF_VIT.dataloaders.transform import Patchify, Patchify_3D  # noqa: E402
from patcher_labels_bench import contours  # noqa: E402
from oracle import quadtree_ref as QR  # noqa: E402

B, H, L, p = 166, 256, 196, 16      # a power of two: every leaf stays square (the reference asserts that, quadtree.py:157)
rng = np.random.Generator(np.random.PCG64(0))
yy, xx = np.ogrid[:H, :H]
maps = []
for b in range(B):                                   # a few circle outlines per image, like object contours
    m = np.zeros((H, H), dtype=bool)
    for _ in range(6):
        cy, cx, r = rng.integers(0, H), rng.integers(0, H), rng.integers(8, 80)
        m |= np.abs(np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2) - r) < 1.0
    maps.append(m.astype(np.uint8) * 255)
maps = np.stack(maps)
imgs = rng.random((B, H, H, 3)).astype(np.float32) * 255
e, x = torch.from_numpy(maps).cuda(), torch.from_numpy(imgs).cuda()


def timed(pt, x, e, reps=20):
    """ms per call of the module: device events around `reps` back-to-back calls after three warm-up calls"""
    for _ in range(3):
        pt(x, e)
    torch.cuda.synchronize()
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        pt(x, e)
    t.record()
    torch.cuda.synchronize()
    return s.elapsed_time(t) / reps


ms = timed(Patchify(L, p, 3), x, e)
print(f"HIP  : batch {B} x {H}^2 -> {L} tokens of {p}^2: {ms:.3f} ms per batch = {B / ms * 1e3:.0f} images/s")
B3, N3, L3, p3 = 2, 64, 512, 4
rng3 = np.random.Generator(np.random.PCG64(0))
dom = torch.from_numpy(np.stack([contours((N3,) * 3, rng3)[0] for _ in range(B3)])).cuda()
vol = torch.from_numpy(rng3.random((B3, N3, N3, N3, 1)).astype(np.float32) * 255).cuda()
ms = timed(Patchify_3D(L3, p3, 1), vol, dom)
print(f"HIP 3-D: batch {B3} x {N3}^3 -> {L3} tokens of {p3}^3: {ms:.3f} ms per batch = {B3 / ms * 1e3:.0f} volumes/s")
t0 = time.perf_counter()
n = 8
for b in range(n):
    nodes, _ = QR.build_tree(maps[b], L)
    QR.serialize(imgs[b], nodes, L, p)
dt = time.perf_counter() - t0
print(f"CPU oracle (1 thread Python, {n} images): {n / dt:.1f} images/s")
