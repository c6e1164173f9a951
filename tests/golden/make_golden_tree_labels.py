"""Generates tests/golden/tree_labels.npz from the REFERENCE's FixedOctTree.serialize_labels / deserialize (octree.py:152-213 + Cube.set_area):

    cd tests/golden && python make_golden_tree_labels.py <checkout of the reference>

src/UCF_VIT/dataloaders/octree.py is loaded from its file with an EMPTY stand-in module for `cv2` (octree.py imports it but never calls
it); scipy (RegularGridInterpolator: method='nearest' for the labels, the default linear for set_area) is the real package.  Recorded for
N = 16 and 32 (one tree each) at p = 2, 4, 8: the label volume (4 classes, blobs; uint8), the edge volume and the node list, the output of
serialize_labels (uint8 [n, p, p, p]), a random patch list (fp32, integers 0..255, [L, p, p, p, 1]) and the float64 volume deserialize paints
from it.  Even p only: the reference's nearest rule has no exact ties there (odd p: scipy's double arithmetic sends some midpoints up).
The 2-D reference needs cv2.resize, which is not available: nothing 2-D is recorded.  Data only.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
spec = importlib.util.spec_from_file_location("ref_octree", os.path.join(sys.argv[1], "src", "UCF_VIT", "dataloaders", "octree.py"))
O = importlib.util.module_from_spec(spec)
spec.loader.exec_module(O)

rec = {}
cases = [(16, 15), (32, 64)]                                  # (side, fixed_length)
for i, (n, L) in enumerate(cases):
    rng = np.random.Generator(np.random.PCG64(700 + i))
    # blobs: the class of the nearest of a few random centres, background beyond a radius
    zz, yy, xx = np.meshgrid(*[np.arange(n)] * 3, indexing="ij")
    centres = rng.integers(0, n, (7, 3))
    d = np.stack([(zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 for c in centres])
    labels = np.where(d.min(0) < (n / 3.5) ** 2, 1 + d.argmin(0) % 3, 0).astype(np.uint8)
    dom = ((labels != np.roll(labels, 1, 0)) | (labels != np.roll(labels, 1, 1)) | (labels != np.roll(labels, 1, 2))).astype(np.uint8) * 255
    t = O.FixedOctTree(domain=dom, fixed_length=L, norm_factor=255)
    nodes = np.array([list(c.get_coord()) for c, _ in t.nodes], dtype=np.int32)
    rec[f"labels{i}"], rec[f"domain{i}"], rec[f"nodes{i}"], rec[f"L{i}"] = labels, dom, nodes, np.int32(L)
    print(i, "N", n, "fixed_length", L, "-> nodes", len(nodes), "classes", np.unique(labels).tolist())
    for p in (2, 4, 8):
        seq, _, _ = t.serialize_labels(labels[..., None].astype(np.float64), size=(p, p, p, 1))
        seq = np.asarray(seq)[:len(nodes), ..., 0]
        assert (seq == np.round(seq)).all()
        rec[f"seq_labels{i}_p{p}"] = seq.astype(np.uint8)
        patches = rng.integers(0, 256, (L, p, p, p, 1)).astype(np.float32)
        rec[f"patches{i}_p{p}"] = patches
        rec[f"painted{i}_p{p}"] = t.deserialize(patches.astype(np.float64), p, 1)[..., 0]            # float64 [N, N, N]
        print("   p", p, "serialize_labels", seq.shape, "deserialize", rec[f"painted{i}_p{p}"].shape)
rec["n_cases"] = np.int32(len(cases))
np.savez_compressed(os.path.join(HERE, "tree_labels.npz"), **rec)
print("done", os.path.getsize(os.path.join(HERE, "tree_labels.npz")), "bytes")
