"""Losses on the hot path (reference: src/UCF_VIT/utils/metrics.py:11-17 masked_mse; nn.MSELoss / nn.CrossEntropyLoss
call sites in training_scripts/train_masked_simple.py:43-47 and train_class_simple.py:24-30), running on the HIP kernels, and the Dice
accuracy of the UNETR scripts (monai DiceMetric in the reference, train_unetr_simple.py:399-401,453-460) on the counts of the HIP segmentation pass."""
import torch

from .._hip import functional as HF


def masked_mse(pred, y, mask):
    """mean over the patch dim of (pred-y)^2, then sum(loss*mask)/sum(mask).  `y` is the patchified target
    [B, L, P]; prefer patch_mse_loss(), which reads the image directly and fuses forward+backward."""
    loss = ((pred.float() - y.float()) ** 2).mean(dim=-1)
    return (loss * mask).sum() / mask.sum()


def patch_mse_loss(pred, data, patch_size, mask=None):
    """MSE(pred, patchify(data)) without materialising the target; mask=None -> plain MSE over all patches
    (config loss_fn "MSE"), mask given -> masked_mse semantics ("maskMSE")."""
    return HF.patch_mse(pred, data, patch_size, mask)


def seq_mse_loss(pred, seq, mask=None):
    """MSE(pred, rearrange(seq, 'b c s p -> b s (p c)')) for adaptively patched input (reference train_masked_simple.py:24-32),
    target never materialised; mask given -> masked_mse semantics."""
    return HF.patch_mse(pred, seq, None, mask)


def cross_entropy_loss(logits, labels):
    return HF.cross_entropy(logits, labels)


class DiceBLoss(torch.nn.Module):
    """Dice + binary cross-entropy over the non-background channels of a segmentation map (reference utils/metrics.py:95-121, the
    loss of train_sap_simple.py:44-46): sigmoid, channels 1.. flattened, loss = w * BCE + (1 - w) * (1 - dice).  On GPU tensors with
    act=True the loss and its gradient are two HIP passes over the map (HF.DiceBCEFn: ucfvit_dice_bce_stats / _from_stats; targets are
    cast to fp32, soft targets allowed).  CPU tensors, or act=False (inputs that are probabilities already), keep the torch arithmetic below
    (a checker for the kernels; no training path uses it)."""

    def __init__(self, weight=0.5, num_class=2, size_average=True):
        super().__init__()
        self.weight, self.num_class = weight, num_class

    def forward(self, inputs, targets, smooth=1, act=True):
        if act and inputs.is_cuda:
            if inputs.dtype not in (torch.float32, torch.bfloat16):
                inputs = inputs.float()
            return HF.dice_bce(inputs, targets.float().contiguous(), self.weight, smooth)
        inputs = inputs.float()
        if act:
            inputs = torch.sigmoid(inputs)
        pred = torch.flatten(inputs[:, 1:])
        true = torch.flatten(targets[:, 1:].float())
        inter = (pred * true).sum()
        dice_loss = 1 - (2. * inter + smooth) / (pred.sum() + true.sum() + smooth)
        bce = torch.nn.functional.binary_cross_entropy(pred, true, reduction='mean')
        return self.weight * bce + (1 - self.weight) * dice_loss


def dice_from_counts(counts, include_background=False, group=None):
    """Dice accuracy per batch element and class from the integer counts of HF.segment / ops.seg_counts (int64 [B, 3, n] = TP, PRED, LAB):
    2 TP / (PRED + LAB) where the class occurs in the labels (LAB > 0), NaN where it does not — monai's DiceMetric / DiceHelper with
    ignore_empty=True on one-hot argmax predictions (reference train_unetr_simple.py:399-401,453-460).  monai is not installed here and is not
    vendored: PARITY UNPINNED against it; the tests hold this to a plain restatement of the published formulas.  Evaluated in float64 on the
    counts' device (CPU tensors work: this is tensor arithmetic only) and rounded once -> fp32 [B, n], or [B, n - 1] without the background
    class 0.  group: the counts are summed over the process group first — the X-slabs of fsdp/sharded_decoder.py add up to the counts of the
    whole volume (the predictions stay local slabs).  Nothing here synchronises with the host."""
    if counts.dim() != 3 or counts.shape[1] != 3 or counts.dtype != torch.int64:
        raise ValueError("dice_from_counts: counts must be int64 [B, 3, n]")
    if group is not None:
        counts = counts.clone()
        torch.distributed.all_reduce(counts, op=torch.distributed.ReduceOp.SUM, group=group)
    c = counts.double()
    tp, pr, lb = c[:, 0], c[:, 1], c[:, 2]
    d = torch.where(lb > 0, 2.0 * tp / (pr + lb), torch.full_like(tp, float("nan")))
    return (d if include_background else d[:, 1:]).float()


class DiceMetric:
    """monai.metrics.DiceMetric(include_background, reduction=MEAN, get_not_nans=True) in its call shape, on the HIP segmentation pass:
    metric(logits, labels) takes the RAW logits [B, n, *spatial] and integer labels (argmax and one-hot happen inside ucfvit_seg_counts, not
    in the caller), returns the per-item Dice fp32 [B, n or n - 1] and adds it to a running state on the device; aggregate() -> (mean,
    not_nans) by monai's MEAN reduction: per item the mean over its non-NaN classes, then the mean over the items that had at least one
    such class, not_nans the number of those items (mean is 0 where there is none, as monai's do_metric_reduction leaves it); reset() clears
    the state.  No call synchronises with the host.  Parity with monai is unpinned (see dice_from_counts)."""

    def __init__(self, include_background=False, group=None):
        self.include_background, self.group = include_background, group
        self.reset()

    def reset(self):
        self._sum, self._items = None, None

    def update(self, counts):
        """counts int64 [B, 3, n] of one batch (any device) -> its per-item Dice; added to the running state"""
        d = dice_from_counts(counts, self.include_background, self.group)
        valid = ~torch.isnan(d)
        k = valid.sum(dim=1)
        item = torch.where(k > 0, torch.where(valid, d, torch.zeros_like(d)).double().sum(dim=1) / k.clamp_min(1), torch.zeros_like(k, dtype=torch.float64))
        s, m = item.sum(), (k > 0).sum()
        self._sum = s if self._sum is None else self._sum + s
        self._items = m if self._items is None else self._items + m
        return d

    @torch.no_grad()
    def __call__(self, logits, labels):
        from .._hip import ops
        _, counts = ops.seg_counts(logits.detach(), labels, want_pred=False)
        return self.update(counts)

    def aggregate(self):
        if self._sum is None:
            raise RuntimeError("DiceMetric.aggregate: nothing was added since reset()")
        m = self._items
        mean = torch.where(m > 0, self._sum / m.clamp_min(1), torch.zeros_like(self._sum))
        return mean.float(), m.float()
