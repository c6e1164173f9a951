"""Hybrid-OP model layer — drop-in for the reference's src/UCF_VIT/fsdp/arch.py: the `simple` models plus
tensor_par_size / tensor_par_group (reference :137-138), tensor-parallel Blocks, the activation broadcast that makes all
ranks of a TP group work on the TP-source rank's tokens (reference :476-486: dist.broadcast before `blocks`,
F_Identity_B_Broadcast after `norm`) and the TP-synchronised MAE mask noise (:682-689).

Deviations from the reference's fsdp copy, which carries known defects: the image path follows the `simple`
condition (`adaptive_patching and not sqrt_len_method`), and VIT.forward_head applies `head`.
"""
from functools import partial

import torch
import torch.distributed as dist

from UCF_VIT.simple import arch as _S
from UCF_VIT.simple.arch import (  # noqa: F401
    feature_take_indices, init_weights_vit_timm, get_init_weights_vit, global_pool_nlc, named_apply)
from UCF_VIT.utils.dist_functions import F_Identity_B_Broadcast
from UCF_VIT.utils.fused_attn import FusedAttn
from .building_blocks import Block, Mlp


class _TPMixin:
    def _tp_setup(self, kwargs):
        self.tensor_par_size = kwargs.pop('tensor_par_size', 1)
        self.tensor_par_group = kwargs.pop('tensor_par_group', None)
        kwargs.setdefault('block_fn', partial(Block, tensor_par_size=self.tensor_par_size, tensor_par_group=self.tensor_par_group))
        kwargs.setdefault('mlp_layer', Mlp)
        return kwargs

    def _tp_src(self):
        return dist.get_rank() - dist.get_rank(group=self.tensor_par_group)

    def _tp_enter(self, x):
        """all ranks of the TP group continue with the source rank's tokens (C5, reference :476-479)"""
        if self.tensor_par_size > 1:
            x = x.contiguous()
            dist.broadcast(x, self._tp_src(), group=self.tensor_par_group)
        return x

    def _tp_exit(self, x):
        if self.tensor_par_size > 1:
            x = F_Identity_B_Broadcast(x, self._tp_src(), group=self.tensor_par_group)
        return x


class VIT(_TPMixin, _S.VIT):
    def __init__(self, *args, **kwargs):
        kwargs = self._tp_setup(kwargs)
        super().__init__(*args, **kwargs)

    def forward_features(self, x, variables, seq_ps):
        self._prepare()
        x = self._embed_tokens(x, variables)
        x = self._pos_embed(x, seq_ps)
        x = self.patch_drop(x)
        x = self._tp_enter(x)
        x = self.norm(self.blocks(x))
        return self._tp_exit(x)


class MAE(_TPMixin, _S.MAE):
    def __init__(self, *args, **kwargs):
        kwargs = self._tp_setup(kwargs)
        super().__init__(*args, **kwargs)

    def random_masking(self, sequence, noise=None):
        if noise is None and self.tensor_par_size > 1:
            noise = torch.rand(sequence.shape[0], sequence.shape[1], device=sequence.device)
            dist.broadcast(noise, src=self._tp_src(), group=self.tensor_par_group)    # C6: same mask on every TP rank
        return super().random_masking(sequence, noise)

    def forward_features(self, x, variables, seq_ps, noise=None):
        self._prepare()
        x = self._embed_tokens(x, variables)
        x = self._pos_embed(x, seq_ps)
        x, mask, ids_restore = self.random_masking(x, noise)
        x = self.patch_drop(x)
        x = self._tp_enter(x)
        x = self.norm(self.blocks(x))
        return self._tp_exit(x), mask, ids_restore

    def mask_head(self, x, ids_restore, seq_ps):
        if self.tensor_par_size <= 1 or self.linear_decoder:
            return super().mask_head(x, ids_restore, seq_ps)
        from UCF_VIT._hip import functional as HF
        from UCF_VIT.simple.building_blocks import _cd
        x = self.decoder_embed(x)
        x = HF.UnshuffleFn.apply(x, self.mask_token, ids_restore, self.decoder_pos_embed, _cd(self))
        x = self._tp_enter(x)
        x = self.decoder_norm(self.decoder_blocks(x))
        x = self._tp_exit(x)
        return self.decoder_pred(x)


class UNETR(_TPMixin, _S.UNETR):
    """UNETR with the Hybrid-OP arguments of the reference's fsdp copy (src/UCF_VIT/fsdp/arch.py:1093-1130: tensor_par_size / _group, the
    activation broadcast round the Blocks) plus SEQUENCE parallelism for the 8192-token volumes, under the names the reference already
    plumbs but asserts off (seq_par_size / seq_par_group, utils/misc.py:147-160, train_masked_fsdp.py:220):

        seq_par_group = UCF_VIT.fsdp.seq_parallel.make_seq_parallel_groups(...)   (a 2-D Ulysses x ring view of the group), or a plain
                        process group (pure Ulysses, num_heads % seq_par_size == 0)

    With seq_par_size > 1 every rank embeds and encodes its contiguous shard of the token sequence: forward_intermediates returns the
    LOCAL shards [B, N / P, D] of the final features and of the taps.  The convolutional decoder then runs SHARDED as well
    (shard_decoder=True, the default whenever the HIP decoder applies, the token grid's first axis divides by P and the geometry does not
    resample dec1 — the slab decoder has no resampling step, so patch-4 style geometries decode gathered): a token shard is an
    X-slab of the token grid, every rank decodes its slab of the volume with one-plane halo exchanges in front of the 3x3x3 layers and
    group-wide instance-norm statistics (fsdp/sharded_decoder.py), and forward() returns the LOCAL slab of the logits
    [B, classes, X / P, Y, Z] — pair it with sharded_decoder.sharded_dice_ce and sharded_decoder.local_slab(labels, ...).
    shard_decoder=False keeps the round-2 form: the shards are all-gathered and the decoder runs replicated on every rank."""

    def __init__(self, *args, **kwargs):
        self.seq_par_size = kwargs.pop('seq_par_size', 1)
        seq_par_group = kwargs.pop('seq_par_group', None)
        self._shard_decoder_arg = kwargs.pop('shard_decoder', None)
        kwargs = self._tp_setup(kwargs)
        super().__init__(*args, **kwargs)
        object.__setattr__(self, '_spg', None)
        object.__setattr__(self, '_sp_blocks', None)
        if self.seq_par_size > 1:
            from .seq_parallel import SeqParallelBlock, SeqParallelGroups, _PlainGroup
            assert self.tensor_par_size == 1, "tensor and sequence parallelism are not combined inside one Block"
            assert not self.class_token and not self.adaptive_patching, "sequence parallelism shards a plain token grid (no class token)"
            spg = seq_par_group if isinstance(seq_par_group, SeqParallelGroups) else _PlainGroup(seq_par_group)
            assert spg.size == self.seq_par_size
            object.__setattr__(self, '_spg', spg)
            object.__setattr__(self, '_sp_blocks', [SeqParallelBlock(b, spg) for b in self.blocks])   # wrappers, not registered twice

    def _embed_local_tokens(self, x):
        """tokens [lo, hi) of the (h, w[, d]) row-major grid: whole slabs along the first spatial axis when the grid allows it (every rank
        then reads 1 / P of the volume), else the full embedding sliced"""
        self._refuse_group_pos_drop()
        spg, p = self._spg, self.patch_size
        n = self.num_patches // spg.size
        lo = spg.rank * n
        g0 = self.grid_size[0]
        rows = self.num_patches // g0                       # tokens per slab of one patch thickness
        from UCF_VIT._hip import functional as HF
        from UCF_VIT.simple.building_blocks import _cd
        if n % rows == 0:
            s0, s1 = (lo // rows) * p, ((lo + n) // rows) * p
            pe = self.token_embeds                              # the slab through the same im2col + GEMM as PatchEmbed.forward
            tok = HF.PatchEmbedFn.apply(x[:, :, s0:s1].contiguous(), pe.proj.weight, pe.proj.bias, p, _cd(self))
        else:
            tok = self.token_embeds(x)[:, lo:lo + n]
        pos = self.pos_embed[:, lo:lo + n] if self.pos_embed is not None else None
        return HF.TokensFn.apply(tok.contiguous(), None, pos, _cd(self)) if pos is not None else tok

    def forward_intermediates(self, x, variables, seq_ps, indices=None, return_prefix_tokens=False, norm=False, stop_early=False,
                              intermediates_only=False):
        if self.seq_par_size <= 1:
            if self.tensor_par_size <= 1:
                return super().forward_intermediates(x, variables, seq_ps, indices, return_prefix_tokens, norm, stop_early, intermediates_only)
            take, max_index = feature_take_indices(len(self.blocks), indices)
            self._prepare()
            x = self._tp_enter(self.patch_drop(self._pos_embed(self._embed_tokens(x, variables), seq_ps)))
            intermediates = []
            for i, blk in enumerate(self.blocks if not stop_early else self.blocks[:max_index + 1]):
                x = blk(x)
                if i in take:
                    intermediates.append(self._tp_exit(self.norm(x) if norm else x))
            if self.num_prefix_tokens:
                intermediates = [y[:, self.num_prefix_tokens:] for y in intermediates]
            return intermediates if intermediates_only else (self._tp_exit(self.norm(x)), intermediates)
        take, max_index = feature_take_indices(len(self.blocks), indices)
        self._prepare()
        x = self._embed_local_tokens(x)
        intermediates = []
        blocks = self._sp_blocks if not stop_early else self._sp_blocks[:max_index + 1]
        for i, blk in enumerate(blocks):
            x = blk(x)
            if i in take:
                intermediates.append(self.norm(x) if norm else x)
        return intermediates if intermediates_only else (self.norm(x), intermediates)


    def forward(self, x, variables, seq_ps=None, x_seq=None):
        """sequence-parallel whole model: the encoder runs on token shards (every rank receives the whole volume and embeds its slab), the
        shards of the final features and of the taps are all-gathered, and the convolutional decoder runs replicated on every rank of the
        group (its gradients are rank-identical; the encoder's are sums over the shards, as in forward_intermediates)"""
        if self.seq_par_size <= 1:
            return super().forward(x, variables, seq_ps, x_seq)
        assert self.skip_connection and not self.linear_decoder, "sequence parallelism is wired for the skip-connection decoder"
        if self.shard_decoder():
            return self._forward_sharded_decoder(x, variables, seq_ps)
        from .seq_parallel import gather_tokens_autograd
        feats, taps = self.forward_intermediates(x, variables, seq_ps, indices=self.skip_indices)
        feats = gather_tokens_autograd(feats, self._spg)
        taps = [gather_tokens_autograd(t, self._spg) for t in taps]
        if self.hip_decoder():
            from UCF_VIT._hip import ops as _ops
            enc1 = self.encoder1.forward_cl(_ops.pad_channels8(x.float().contiguous()))
            return self._unetr_head_cl(self.pool(feats), taps, enc1)
        return self.forward_head(feats, taps, self.encoder1(x))


    # -------------------------------------------------------------------------------------------- sharded decoder (fsdp/sharded_decoder.py)
    def shard_decoder(self):
        """True when forward() decodes only this rank's X-slab (see the class docstring)"""
        if self.seq_par_size <= 1:
            return False
        can = (self.hip_decoder() and len(self.feat_size) == 3 and self.feat_size[0] % self.seq_par_size == 0
               and not self.resamples_dec1())             # sharded_decoder.py has no resampling step: the gathered path (_unetr_head_cl) has
        if self._shard_decoder_arg is None:
            return can
        if self._shard_decoder_arg and not can:
            raise ValueError("UNETR: shard_decoder=True needs the HIP decoder, a token grid whose first axis divides by seq_par_size and a "
                             "geometry without the resampling of dec1 (token grid x 16 = img_size)")
        return bool(self._shard_decoder_arg)

    def _tokens_cl_local(self, t):
        fx, fy, fz = self.feat_size
        return t.to(torch.bfloat16).reshape(t.size(0), fx // self.seq_par_size, fy, fz, self.embed_dim)

    def _forward_sharded_decoder(self, x, variables, seq_ps):
        from . import sharded_decoder as SD
        from UCF_VIT._hip import ops as _ops
        spg = self._spg
        feats, taps = self.forward_intermediates(x, variables, seq_ps, indices=self.skip_indices)       # local token shards = X-slabs
        xl = SD.local_slab(x, spg, 2).float().contiguous()                                              # [B, C, X / P, Y, Z]
        enc1 = SD.sharded_basic_block(self.encoder1, _ops.pad_channels8(xl), spg)
        tok = self._tokens_cl_local
        n = len(taps)
        dec3 = SD.sharded_up_block(self.decoder5, tok(self.pool(feats)), SD.sharded_prup_block(self.encoder4, tok(taps[n - 1]), spg), spg)
        dec2 = SD.sharded_up_block(self.decoder4, dec3, SD.sharded_prup_block(self.encoder3, tok(taps[n - 2]), spg), spg)
        dec1 = SD.sharded_up_block(self.decoder3, dec2, SD.sharded_prup_block(self.encoder2, tok(taps[n - 3]), spg), spg)
        logits = self.out.forward_cl(SD.sharded_up_block(self.decoder2, dec1, enc1, spg))                # [B, X / P, Y, Z, classes] fp32
        return logits.permute(0, 4, 1, 2, 3)


class SAP(_TPMixin, _S.SAP):
    """SAP with the Hybrid-OP arguments (reference fsdp/arch.py:1311-1338: tensor-parallel Blocks inside the broadcast bracket)"""

    def __init__(self, *args, **kwargs):
        kwargs = self._tp_setup(kwargs)
        super().__init__(*args, **kwargs)

    def forward_features(self, x, variables, seq_ps):
        self._prepare()
        x = self._embed_tokens(x, variables)
        x = self._pos_embed(x, seq_ps)
        x = self.patch_drop(x)
        x = self._tp_enter(x)
        x = self.norm(self.blocks(x))
        return self._tp_exit(x)
