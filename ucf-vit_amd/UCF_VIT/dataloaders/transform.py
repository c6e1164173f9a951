"""Adaptive patching on the GPU (reference: src/UCF_VIT/dataloaders/transform.py:9-55 `Patchify`, quadtree.py:84-174 `FixedQuadTree`).

The reference patches ONE image per call on the host: cv2 edge detection -> greedy fixed-length quadtree -> cv2 bicubic resize of every
leaf to patch_size x patch_size -> `np.reshape([S, p, p, C] -> [C, S, p*p])`.  This class does the tree and the resampling for a
whole batch on the MI355X (libucfvit_hip.so: ucfvit_quadtree_build / ucfvit_quadtree_serialize) and returns tensors in exactly the
layout VIT / MAE (adaptive_patching=True) consume.  Edge detection is NOT included (cv2.Canny has no counterpart here): the caller
passes the edge maps, e.g. computed by the reference's own transform on the host or by any detector that emits 0 / 255.
"""
import torch

from .._hip import functional as HF
from .._hip import ops


class _TreePatchify(torch.nn.Module):
    """What the 2-D and the 3-D patcher share: a 2^nd-ary tree of fixed_length = (2^nd - 1) n + 1 leaves, each resampled to patch_size^nd."""
    nd = None                                   # 2 | 3

    def __init__(self, fixed_length, patch_size, num_channels, refusal):
        super().__init__()
        if fixed_length < 1 or fixed_length % (2 ** self.nd - 1) != 1:          # -2 % 3 == 1 in Python: the sign is checked apart
            raise ValueError(refusal)
        self.fixed_length, self.patch_size, self.num_channels = fixed_length, patch_size, num_channels

    @torch.no_grad()
    def forward(self, img, domain):
        nd = self.nd
        if img.dim() != nd + 2 or img.shape[-1] != self.num_channels:
            raise ValueError(f"{type(self).__name__}: {'img' if nd == 2 else 'vol'} must be [B, {'H, W' if nd == 2 else 'N, N, N'}, "
                             f"C={self.num_channels}], got {tuple(img.shape)}")
        img = img if img.dtype == torch.float32 else img.float()
        img = img if img.is_contiguous() else img.contiguous()
        domain = domain if domain.is_contiguous() else domain.contiguous()
        if nd == 2:
            nodes, _, count, seq_ps = ops.quadtree_build(domain, self.fixed_length)
            seq_img = ops.quadtree_serialize(img, nodes, count, self.patch_size)
        else:
            nodes, _, count, seq_ps = ops.octree_build(domain, self.fixed_length, self.norm_factor)
            seq_img = ops.octree_serialize(img, nodes, count, self.patch_size)
        return seq_img, seq_ps[..., 0], seq_ps[..., 1:], nodes, count

    @torch.no_grad()
    def serialize_labels(self, labels, nodes, count, num_classes, one_hot=True):
        """labels uint8 or int64 [B, H, W] / [B, N, N, N] through the tree `forward` built (reference quadtree.py:176-207, nearest neighbour per
        leaf; octree.py:152-199, scipy's nearest rule, ties to the lower index) -> one_hot: fp32 [B, num_classes, fixed_length * patch_size**nd],
        the collated `seq_label` training_step_adaptive reshapes (datamodule.py:40-51); else the class indices int64 [B, fixed_length, p, .., p].
        Padding rows are class 0."""
        labels = labels if labels.is_contiguous() else labels.contiguous()
        fn = ops.quadtree_serialize_labels if self.nd == 2 else ops.octree_serialize_labels
        idx, onehot = fn(labels, nodes, count, self.patch_size, num_classes, want_idx=not one_hot, want_onehot=one_hot)
        return onehot if one_hot else idx

    def deserialize(self, seq, nodes, count, size, mode, truncate, channels_last):
        """a token sequence painted back into the image plane, read in place, uncovered pixels 0.
        2-D (reference quadtree.py:209-221 + Rect.set_area): seq fp32 [B, L, p, p, C] or the model layout [B, C, L, p*p], size = (H, W) -> fp32
        [B, H, W, C] (channels_last) or [B, C, H, W]; mode 'bicubic' is the reference's resize (truncate=True applies its seq.astype(int)
        first), 'nearest' keeps class maps exact.
        3-D (octree.py:201-213 + Cube.set_area): seq fp32 [B, L, p, p, p, C] or [B, C, L, p**3], size = N -> fp32 [B, N, N, N, C] or
        [B, C, N, N, N]; mode 'trilinear' (aligned corners) or 'nearest'; no truncation (commented out in the reference)."""
        if torch.is_grad_enabled() and seq.requires_grad:
            # a loss at full resolution: the differentiable path (HF.deserialize, backward = the adjoint gather)
            if truncate:
                raise ValueError(f"{type(self).__name__}.deserialize: truncate=True has no gradient (truncf is flat almost everywhere), but seq "
                                 "requires grad; detach seq or drop truncate")
            return HF.deserialize(seq, nodes, count, size, self.patch_size, self.nd, mode=mode, channels_last=channels_last)
        with torch.no_grad():
            if self.nd == 2:
                return ops.quadtree_deserialize(seq, nodes, count, size, self.patch_size, mode=mode, truncate=truncate, channels_last=channels_last)
            if truncate:
                raise ValueError("Patchify_3D.deserialize: the 3-D rule has no truncation")
            return ops.octree_deserialize(seq, nodes, count, size, self.patch_size, mode=mode, channels_last=channels_last)


class Patchify(_TreePatchify):
    """forward(img, edges) -> (seq_img, seq_size, seq_pos, nodes, count)
       img   fp32 [B, H, W, C] (channels last like the reference's numpy images; square images for square patches)
       edges uint8 [B, H, W], 0 / 255
       seq_img  fp32 [B, C, fixed_length, patch_size**2]      (the reference's per-image [C, S, p*p], transform.py:44-48)
       seq_size fp32 [B, fixed_length]    width of every leaf (0 = padding)
       seq_pos  fp32 [B, fixed_length, 2] leaf centres (x, y) ((-1, -1) = padding)
       nodes int32 [B, fixed_length, 4] = (x1, x2, y1, y2), count int32 [B]
    The training scripts feed the model `seq_ps = cat([seq_size[..., None], seq_pos], -1)` (train_class_simple.py:325-337)."""
    nd = 2

    def __init__(self, fixed_length=196, patch_size=16, num_channels=3):
        super().__init__(fixed_length, patch_size, num_channels,
                         "Quadtree fixed length needs to be 3n+1, where n is some integer")      # train_unetr_simple.py:214

    def deserialize(self, seq, nodes, count, size, mode="bicubic", truncate=False, channels_last=True):
        return super().deserialize(seq, nodes, count, size, mode, truncate, channels_last)


class Patchify_3D(_TreePatchify):
    """3-D counterpart (reference transform.py:57-132 + octree.py:66-151): forward(vol, domain) -> (seq_img, seq_size, seq_pos, nodes, count)
       vol    fp32 [B, N, N, N, C] (cubic, channels last), domain uint8 [B, N, N, N] = the reference's `edges` volume
              (edge counter * norm_factor, norm_factor = int(255 / num_channels), transform.py:118-121)
       seq_img fp32 [B, C, fixed_length, patch_size**3], seq_size [B, fixed_length], seq_pos [B, fixed_length, 3]
       nodes int32 [B, fixed_length, 6] = (x1, x2, y1, y2, z1, z2); leaves are resampled with the reference's aligned-corner linear rule."""
    nd = 3

    def __init__(self, fixed_length=729, patch_size=8, num_channels=1):
        super().__init__(fixed_length, patch_size, num_channels,
                         "Octtree fixed length needs to be 7n+1, where n is some integer")       # train_unetr_simple.py:218
        self.norm_factor = int(255 / num_channels)

    def deserialize(self, seq, nodes, count, size, mode="trilinear", truncate=False, channels_last=True):
        return super().deserialize(seq, nodes, count, size, mode, truncate, channels_last)
