#!/usr/bin/env python3
"""Every output of the eight patcher ops on seeded inputs, written as .npy: the material of a bit-for-bit comparison of two builds of the library.

    UCFVIT_HIP_LIB=<build A> python tools/patcher_dump.py DIR_A          (one process per library)
    UCFVIT_HIP_LIB=<build B> python tools/patcher_dump.py DIR_B
    python tools/patcher_dump.py --compare DIR_A DIR_B                   (no GPU: raw 32-bit words; exit status 1 if a file differs)

Cases: the contour maps of tools/patcher_labels_bench.py at its two shapes, and 12x20 / L = 100 and 12^3 / L = 120 with all-zero maps, where every
refinement step is a tie.  Images and token sequences are randn.  Per case: build, serialize, serialize_labels (uint8 and int64 labels),
deserialize in both modes (2-D: also with truncation), both output layouts and both sequence layouts.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compare(dir_a, dir_b):
    names_a, names_b = sorted(os.listdir(dir_a)), sorted(os.listdir(dir_b))
    bad = names_a != names_b
    if bad:
        print("file lists differ:", sorted(set(names_a) ^ set(names_b)))
    for name in sorted(set(names_a) & set(names_b)):
        a, b = np.load(os.path.join(dir_a, name)), np.load(os.path.join(dir_b, name))
        if a.shape != b.shape or a.dtype != b.dtype:
            print(f"{name}: {a.dtype}{a.shape} against {b.dtype}{b.shape}")
            bad = True
            continue
        wa, wb = np.frombuffer(a.tobytes(), np.uint32), np.frombuffer(b.tobytes(), np.uint32)
        diff = int((wa != wb).sum())
        bad |= diff > 0
        print(f"{name}: {a.dtype}{a.shape} {'EQUAL' if not diff else f'{diff} of {wa.size} words DIFFER'}")
    print("RESULT:", "a file differs" if bad else f"all {len(names_a)} files equal")
    return int(bad)


def dump(out_dir):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from UCF_VIT._hip import ops
    from patcher_labels_bench import contours
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.Generator(np.random.PCG64(0))
    gen = torch.Generator().manual_seed(0)

    def save(case, name, t):
        np.save(os.path.join(out_dir, f"{case}.{name}.npy"), t.cpu().numpy())

    # (case, nd, B, image side(s), L, p, classes, channels, contour maps | all zero)
    cases = (("ct3d", 3, 2, (64,) * 3, 512, 4, 4, 2, True), ("img2d", 2, 8, (512,) * 2, 1024, 8, 4, 3, True),
             ("tie2d", 2, 2, (12, 20), 100, 4, 4, 3, False), ("tie3d", 3, 2, (12,) * 3, 120, 2, 4, 2, False))
    for case, nd, B, shape, L, p, nc, C, contour in cases:
        if contour:
            maps, labs = zip(*[contours(shape, rng) for _ in range(B)])
            maps, labs = np.stack(maps), np.stack(labs)
        else:
            maps, labs = np.zeros((B,) + shape, np.uint8), rng.integers(0, nc, (B,) + shape).astype(np.uint8)
        edges, labels = torch.from_numpy(maps).cuda(), torch.from_numpy(labs).cuda()
        img = torch.randn((B,) + shape + (C,), generator=gen).cuda()
        if nd == 2:
            nodes, values, count, seq_ps = ops.quadtree_build(edges, L)
            seq_img = ops.quadtree_serialize(img, nodes, count, p)
            ser, des, size, smooth = ops.quadtree_serialize_labels, ops.quadtree_deserialize, shape, "bicubic"
        else:
            nodes, values, count, seq_ps = ops.octree_build(edges, L)
            seq_img = ops.octree_serialize(img, nodes, count, p)
            ser, des, size, smooth = ops.octree_serialize_labels, ops.octree_deserialize, shape[0], "trilinear"
        for name, t in (("nodes", nodes), ("values", values), ("count", count), ("seq_ps", seq_ps), ("seq_img", seq_img)):
            save(case, name, t)
        for tag, lab in (("u8", labels), ("i64", labels.long())):
            idx, onehot = ser(lab, nodes, count, p, nc)
            save(case, f"labels_{tag}.idx", idx)
            save(case, f"labels_{tag}.onehot", onehot)
        logits = torch.randn((B, nc, L, p ** nd), generator=gen).cuda() * 3                          # the model layout [B, C, L, p^nd]
        patches = torch.randn((B, L) + (p,) * nd + (nc,), generator=gen).cuda() * 3                  # the patch list [B, L, p, .., p, C]
        for lay, seq in (("model", logits), ("list", patches)):
            for mode, trunc in ((smooth, False), ("nearest", False)) + (((smooth, True),) if nd == 2 else ()):
                for cl in (True, False):
                    kw = dict(mode=mode, channels_last=cl, **({"truncate": trunc} if nd == 2 else {}))
                    save(case, f"des_{lay}_{mode}{'_trunc' if trunc else ''}_{'cl' if cl else 'planar'}", des(seq, nodes, count, size, p, **kw))
        torch.cuda.synchronize()
        print(f"{case}: count {count.tolist()}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(sys.argv[1])
