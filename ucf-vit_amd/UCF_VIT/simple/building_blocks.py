"""Operator layer of the MI355X build — drop-in for the reference's src/UCF_VIT/simple/building_blocks.py
(PatchEmbed:30, Mlp:94, Attention:131, Block:194, MyUnetBlock:241, EmbeddingDenseLayer:286,
VariableMapping_Attention:301): same class names, constructor arguments, forward signatures and state_dict keys.

The modules only HOLD parameters (ordinary nn.Linear / nn.Conv / nn.LayerNorm children, so checkpoints interchange);
their forward/backward run exclusively on the hand-written gfx950 kernels of libucfvit_hip.so through
UCF_VIT._hip.functional.  There is no PyTorch fallback: CPU tensors or a missing library raise.

compute_dtype (torch.float32 | torch.bfloat16) selects the arithmetic: float32 = the reference's `simple` mode
(exact-fp32 MFMA), bfloat16 = the reference's fsdp MixedPrecision(bf16) semantics with fp32 master weights.
Set it with set_compute_dtype(model, dtype).
"""
from functools import partial
from itertools import repeat
from typing import Callable, Optional
import collections.abc

import torch
import torch.nn as nn

from UCF_VIT.utils.fused_attn import FusedAttn
from UCF_VIT._hip import functional as HF


def _ntuple(n):
    def parse(x):
        if isinstance(x, collections.abc.Iterable) and not isinstance(x, str):
            return tuple(x)
        return tuple(repeat(x, n))
    return parse


to_2tuple, to_3tuple = _ntuple(2), _ntuple(3)
LayerType = object


def _assert(cond, msg):
    if not cond:
        raise AssertionError(msg)


def trunc_normal_(tensor, mean=0.0, std=1.0, a=-2.0, b=2.0):
    return nn.init.trunc_normal_(tensor, mean=mean, std=std, a=a, b=b)


def get_act_layer(x):
    return x


def get_norm_layer(x):
    return x


def set_compute_dtype(module: nn.Module, dtype: torch.dtype):
    """Select fp32 (reference `simple` mode) or bf16 (reference fsdp MixedPrecision semantics) arithmetic for a model."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("compute dtype must be torch.float32 or torch.bfloat16")
    for m in module.modules():
        m.compute_dtype = dtype
    return module


def _cd(m):
    return getattr(m, "compute_dtype", torch.float32)


def _no_dropout(p, training, what):
    """attn_drop (inside the LDS-resident attention kernels) and patch_drop_rate (changes the token count) are not on the HIP hot path"""
    if p > 0.0 and training:
        raise NotImplementedError(f"{what}={p}: not on the HIP hot path (head, position and projection / MLP dropout are)")


class LayerNorm(nn.LayerNorm):
    """nn.LayerNorm parameters, HIP kernel arithmetic (ucfvit_layernorm_fwd/bwd)."""

    def forward(self, x):
        return HF.LayerNormFn.apply(x, self.weight, self.bias, self.eps, _cd(self))


class Linear(nn.Linear):
    """nn.Linear parameters, HIP MFMA GEMM arithmetic (ucfvit_gemm)."""

    def forward(self, x):
        return HF.LinearFn.apply(x, self.weight, self.bias, _cd(self))


class DropPath(nn.Module):
    """Stochastic depth per sample (timm's DropPath, which the reference imports): in training sample b keeps its residual branch with
    probability keep = 1 - drop_prob, and a kept branch is multiplied by 1 / keep (scale_by_keep).  The draw is B floats of host
    plumbing on the device (it follows torch.manual_seed, no synchronisation); applying it is HIP (csrc/drop_path.hip).  Inside a fused
    Block the module only draws: HF.BlockFn / HF.TailBlockFn take the scales."""

    def __init__(self, drop_prob: float = 0.0, scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob = drop_prob
        self.scale_by_keep = scale_by_keep
        self.last_scale = None           # the scale tensor of the latest draw (fp32 [B]): for tests and inspection
        self.generator = None            # None: torch's default generator of the device (torch.manual_seed); the training scripts set
                                         # one per rank so that data-parallel ranks do not share a draw

    def active(self):
        return self.training and self.drop_prob > 0.0

    def draw(self, B, device):
        """fp32 [B] on `device`: 0 for a dropped sample, 1 / keep (1 without scale_by_keep, 0 when keep == 0) for a kept one"""
        keep = 1.0 - self.drop_prob
        s = torch.empty(B, dtype=torch.float32, device=device).bernoulli_(keep, generator=self.generator)
        if keep > 0.0 and self.scale_by_keep:
            s.div_(keep)
        self.last_scale = s
        return s

    def forward(self, x):
        if not self.active():
            return x
        if not x.is_cuda:
            raise RuntimeError(f"DropPath: expected a tensor on the MI355X (cuda) device, got {x.device}. "
                               "UCF_VIT operators run only through libucfvit_hip.so; there is no CPU path.")
        return HF.DropPathFn.apply(x, self.draw(x.shape[0], x.device))

    def extra_repr(self):
        return f"drop_prob={round(self.drop_prob, 3):0.3f}"


def _draw_drop_path(d, x):
    """the scale tensor of one residual branch of a fused Block, or None when the branch has no drop path to apply"""
    return d.draw(x.shape[0], x.device) if isinstance(d, DropPath) and d.active() else None


class HipDropout(nn.Dropout):
    """nn.Dropout(p) whose training arithmetic is HIP (csrc/dropout.hip): no parameters, the same state_dict.  The mask is a function of
    (seed, element index) defined in include/ucfvit_hip.h and never stored; the module only draws one 64-bit seed per forward pass, on the
    host: a Python int from a CPU generator (self.generator, else torch's default one, so it follows torch.manual_seed), no device work
    and no synchronisation.  Inside a fused Block / Attention / Mlp the module only draws: the autograd Functions take (p, seed)."""

    def __init__(self, p: float = 0.0, inplace: bool = False):
        super().__init__(p, False)       # the kernels decide where they write; `inplace` is accepted for the signature only
        self.last_seed = None            # the seed of the latest draw: for tests and inspection
        self.generator = None            # None: torch's default CPU generator; the training scripts set one per rank and module

    def active(self):
        return self.training and self.p > 0.0

    def draw(self):
        """a fresh seed in [0, 2^64): two 32-bit halves, since torch draws int64 below 2^63"""
        hi, lo = torch.randint(0, 1 << 32, (2,), dtype=torch.int64, generator=self.generator).tolist()
        self.last_seed = (hi << 32) | lo
        return self.last_seed

    def forward(self, x):
        if not self.active():
            return x
        if not x.is_cuda:
            raise RuntimeError(f"HipDropout: expected a tensor on the MI355X (cuda) device, got {x.device}. "
                               "UCF_VIT operators run only through libucfvit_hip.so; there is no CPU path.")
        return HF.DropoutFn.apply(x, self.p, self.draw())


def _draw_dropout(d):
    """(p, seed) of one dropout site for the autograd Functions, or None when the site has nothing to apply"""
    return (d.p, d.draw()) if isinstance(d, HipDropout) and d.active() else None


def _block_dropout(attn, mlp):
    """BlockFn's dropout argument (p, seed_proj, seed_drop1, seed_drop2) from the three modules a Block builds with one rate, or None.
    Three draws, proj first."""
    sites = [_draw_dropout(attn.proj_drop), _draw_dropout(mlp.drop1), _draw_dropout(mlp.drop2)]
    if all(s is None for s in sites):
        return None
    if any(s is None for s in sites) or len({s[0] for s in sites}) != 1:
        raise NotImplementedError("the fused Block takes one rate for proj_drop, Mlp.drop1 and Mlp.drop2 (Block(proj_drop=p) builds them so)")
    return (sites[0][0],) + tuple(s[1] for s in sites)


class LayerScale(nn.Module):
    """timm's LayerScale: y = gamma ⊙ x with one learned fp32 factor per channel (state_dict key `gamma`).  Applying it is HIP
    (csrc/layer_scale.hip); `inplace` is accepted for the signature only.  Inside a fused Block the module only holds the parameter:
    HF.BlockFn / HF.TailBlockFn take the gammas and fold them into the branch-exit row pass."""

    def __init__(self, dim, init_values=1e-5, inplace=False):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError(f"LayerScale: expected a tensor on the MI355X (cuda) device, got {x.device}. "
                               "UCF_VIT operators run only through libucfvit_hip.so; there is no CPU path.")
        return HF.LayerScaleFn.apply(x, self.gamma)


def _block_gammas(block):
    """(gamma1, gamma2) of a fused Block: both LayerScale parameters, or (None, None) when ls1 / ls2 are Identity"""
    if isinstance(block.ls1, LayerScale):
        return block.ls1.gamma, block.ls2.gamma
    return None, None


def _qk_norm_problem(attn):
    """None when attn.q_norm / attn.k_norm are something the HIP hot path runs (both Identity, or both a plain affine LayerNorm over
    head_dim with one eps), else the condition that failed"""
    q, k = attn.q_norm, attn.k_norm
    if isinstance(q, nn.Identity) and isinstance(k, nn.Identity):
        return None
    for name, m in (("q_norm", q), ("k_norm", k)):
        if not isinstance(m, nn.LayerNorm):
            return f"{name} is {type(m).__name__}; the HIP hot path runs nn.Identity or nn.LayerNorm (both norms alike)"
        if tuple(m.normalized_shape) != (attn.head_dim,):
            return f"{name} normalises over {tuple(m.normalized_shape)}, not over (head_dim,) = ({attn.head_dim},)"
        if not m.elementwise_affine or m.weight is None or m.bias is None:
            return f"{name} has no affine weight and bias"
    if q.eps != k.eps:
        return f"q_norm.eps = {q.eps} differs from k_norm.eps = {k.eps}"
    return None


def _qk_norm_args(attn):
    """the qk_norm arguments of the fused Functions: (q_norm.weight, q_norm.bias, k_norm.weight, k_norm.bias, eps), five Nones without
    qk_norm; raises with the failed condition for norms the hot path does not run"""
    why = _qk_norm_problem(attn)
    if why is not None:
        raise NotImplementedError(f"qk_norm is not on the HIP hot path for this Attention: {why}")
    if isinstance(attn.q_norm, nn.Identity):
        return (None,) * 5
    tps = getattr(attn, "tensor_par_size", 1)
    if tps > 1:
        raise NotImplementedError(f"Attention(qk_norm=True) under a tensor-parallel group (tensor_par_group={getattr(attn, 'tensor_par_group', None)!r}, "
                                  f"tensor_par_size={tps}): the heads are sharded and the [head_dim] parameters replicated, so their gradient "
                                  "would have to be summed over the group; not implemented")
    return (attn.q_norm.weight, attn.q_norm.bias, attn.k_norm.weight, attn.k_norm.bias, attn.q_norm.eps)


class PatchDropout(nn.Module):
    def __init__(self, prob=0.0, num_prefix_tokens=1):
        super().__init__()
        self.prob = prob

    def forward(self, x):
        _no_dropout(self.prob, self.training, "patch_drop_rate")
        return x


AttentionPoolLatent = None
resample_patch_embed = None
resample_abs_pos_embed = None


class PatchEmbed(nn.Module):
    """2-D / 3-D image -> patch tokens [B, L, D]; `proj` is a Conv2d/Conv3d parameter holder (weight [D,C,p,p(,p)])."""

    def __init__(self, img_size: Optional[int] = 224, patch_size: int = 16, in_chans: int = 3, embed_dim: int = 768,
                 twoD: Optional[bool] = True, norm_layer: Optional[Callable] = None, bias: bool = True,
                 sqrt_len_method: bool = False):
        super().__init__()
        self.twoD = twoD
        self.sqrt_len_method = sqrt_len_method
        nd = 2 if twoD else 3
        self.patch_size = _ntuple(nd)(patch_size)
        if img_size is None:
            self.img_size = self.grid_size = self.num_patches = None
        else:
            self.img_size = _ntuple(nd)(img_size)
            self.grid_size = tuple(s // p for s, p in zip(self.img_size, self.patch_size))
            n = 1
            for g in self.grid_size:
                n *= g
            self.num_patches = n
        conv = nn.Conv2d if twoD else nn.Conv3d
        self.proj = conv(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size, bias=bias)
        self.norm = norm_layer(embed_dim) if norm_layer else nn.Identity()

    def forward(self, x):
        if self.img_size is not None and not self.sqrt_len_method:
            for i, name in enumerate(("height", "width", "depth")[: len(self.img_size)]):
                _assert(x.shape[2 + i] == self.img_size[i], f"Input {name} ({x.shape[2 + i]}) doesn't match model ({self.img_size[i]}).")
        p = self.patch_size[0]
        _assert(all(q == p for q in self.patch_size), "HIP patch embedding needs a cubic/square patch")
        x = HF.PatchEmbedFn.apply(x, self.proj.weight, self.proj.bias, p, _cd(self))
        return self.norm(x)


class Mlp(nn.Module):
    """fc1 -> erf-GELU -> fc2 as two MFMA GEMMs with fused bias/activation epilogues."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, norm_layer=None, bias=True,
                 drop=0.0, use_conv=False):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        bias = to_2tuple(bias)
        drop_probs = to_2tuple(drop)
        if use_conv:
            raise NotImplementedError("Mlp(use_conv=True) is not used by the reference models")
        self.fc1 = nn.Linear(in_features, hidden_features, bias=bias[0])
        self.act = act_layer()
        self.drop1 = HipDropout(drop_probs[0])
        self.norm = norm_layer(hidden_features) if norm_layer is not None else nn.Identity()
        self.fc2 = nn.Linear(hidden_features, out_features, bias=bias[1])
        self.drop2 = HipDropout(drop_probs[1])

    def _fusable(self):
        return (isinstance(self.act, nn.GELU) and getattr(self.act, "approximate", "none") == "none"
                and isinstance(self.norm, nn.Identity))

    def _tp(self):
        """the tensor-parallel handle of HF.MlpFn: none here, fsdp.Mlp has one"""
        return None

    def forward(self, x):
        if not self._fusable():
            raise NotImplementedError("HIP Mlp implements fc1 -> exact GELU -> fc2 (the reference configuration)")
        d1, d2 = _draw_dropout(self.drop1), _draw_dropout(self.drop2)           # two seeds, drop1 first
        return HF.MlpFn.apply(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, _cd(self), self._tp(), d1, d2)


def _attention_apply(attn, x, tp):
    """HF.AttentionFn for simple.Attention (tp None) and fsdp.Attention (its tensor-parallel handle): one spelling of the call"""
    _no_dropout(attn.attn_drop.p, attn.training, "attn_drop")
    qk = _qk_norm_args(attn)                                           # raises, naming the condition, for norms the hot path does not run
    return HF.AttentionFn.apply(x, attn.qkv.weight, attn.qkv.bias, attn.proj.weight, attn.proj.bias, attn.num_heads, _cd(attn), tp,
                                _draw_dropout(attn.proj_drop), *qk, torch.is_grad_enabled())


class Attention(nn.Module):
    """Multi-head self-attention; every FusedAttn member runs the fused gfx950 kernel (see utils/fused_attn.py).  qk_norm: q_norm / k_norm
    are norm_layer(head_dim) (LayerNorm; eps 1e-5 for a bare Attention, the Block's norm_layer eps inside a Block) and one row pass over the
    qkv buffer normalises Q and K per head before the attention kernels (HF.AttentionFn); training keeps the un-normalised Q and K for
    backward, two more D-wide token matrices."""

    def __init__(self, dim: int, fused_attn: FusedAttn = FusedAttn.NONE, num_heads: int = 8, qkv_bias: bool = False,
                 qk_norm: bool = False, attn_drop: float = 0.0, proj_drop: float = 0.0, norm_layer: nn.Module = nn.LayerNorm) -> None:
        super().__init__()
        assert dim % num_heads == 0, 'dim should be divisible by num_heads'
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.fused_attn = fused_attn
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.q_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.k_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.attn_drop = HipDropout(attn_drop)      # still refused when active: it lives inside the LDS-resident attention kernels
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = HipDropout(proj_drop)

    def _fusable(self):
        return _qk_norm_problem(self) is None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _attention_apply(self, x, None)


class Block(nn.Module):
    """Pre-LN transformer block.  With standard Attention/Mlp the whole block is ONE
    autograd node running a fixed sequence of fused HIP launches (HF.BlockFn).  drop_path > 0 in training: the two DropPath modules
    draw their per-sample scales and the node applies them (one row pass per branch and direction); proj_drop > 0 in training: the
    three HipDropout modules draw their seeds and the same row passes apply the masks (plus one pass over the activation).  Eval or
    rates 0 run the very launches of a Block without either.  init_values: ls1 / ls2 are LayerScale modules and the node folds their
    gammas into the same row passes (a branch with a gamma always takes one); without it the launches are those of a Block without.
    qk_norm: attn.q_norm / attn.k_norm are norm_layer(head_dim) and the node runs one row pass over the qkv buffer per direction
    (ops.qk_norm_fwd / qk_norm_bwd); it acts inside the branch, so it composes with the three options above, which act at its exit."""

    def __init__(self, dim: int, num_heads: int, fused_attn: FusedAttn = FusedAttn.NONE, mlp_ratio: float = 4.0,
                 qkv_bias: bool = False, qk_norm: bool = False, proj_drop: float = 0.0, attn_drop: float = 0.0,
                 init_values: Optional[float] = None, drop_path: float = 0.0, act_layer: nn.Module = nn.GELU,
                 norm_layer: nn.Module = LayerNorm, mlp_layer: nn.Module = Mlp) -> None:
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, fused_attn=fused_attn, num_heads=num_heads, qkv_bias=qkv_bias, qk_norm=qk_norm,
                              attn_drop=attn_drop, proj_drop=proj_drop, norm_layer=norm_layer)
        self.ls1 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path1 = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = mlp_layer(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=proj_drop)
        self.ls2 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path2 = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.activation_checkpointing = False      # set by apply_activation_checkpointing(): keep only the Block's input for backward

    def _fusable(self):
        return (isinstance(self.norm1, nn.LayerNorm) and isinstance(self.norm2, nn.LayerNorm)
                and self.norm1.elementwise_affine and self.norm2.elementwise_affine and self.norm1.eps == self.norm2.eps
                and ((isinstance(self.ls1, nn.Identity) and isinstance(self.ls2, nn.Identity))
                     or (type(self.ls1) is LayerScale and type(self.ls2) is LayerScale))
                and type(self.attn) is Attention and self.attn._fusable()
                and type(self.mlp) is Mlp and self.mlp._fusable()
                and self.mlp.fc1.out_features % 8 == 0)

    def _fused_args(self, x, tail, tp=None):
        """the argument list of HF.TailBlockFn (tail) or of HF.BlockFn (tp: its tensor-parallel handle, fsdp.Block passes one).  This
        pass's draws are made here, in a fixed order: the drop-path scales s1, s2, then the seeds of proj_drop, Mlp.drop1, Mlp.drop2"""
        a, m = self.attn, self.mlp
        _no_dropout(a.attn_drop.p, self.training, "attn_drop")
        recompute = getattr(self, "activation_checkpointing", False) and torch.is_grad_enabled()
        s1, s2 = _draw_drop_path(self.drop_path1, x), _draw_drop_path(self.drop_path2, x)      # two independent draws, s1 first
        drop = _block_dropout(a, m)
        return ((x, self.norm1.weight, self.norm1.bias, a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias,
                 self.norm2.weight, self.norm2.bias, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, a.num_heads, self.norm1.eps, _cd(self))
                + (() if tail else (tp,)) + (recompute, s1, s2, drop, *_block_gammas(self), torch.is_grad_enabled(), *_qk_norm_args(a)))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._fusable() and x.dim() == 3:
            return HF.BlockFn.apply(*self._fused_args(x, False))
        x = x + self.drop_path1(self.ls1(self.attn(self.norm1(x))))
        x = x + self.drop_path2(self.ls2(self.mlp(self.norm2(x))))
        return x

    def forward_class_rows(self, x: torch.Tensor) -> torch.Tensor:
        """forward(x)[:, 0] computed without the other rows (HF.TailBlockFn); the caller checked _fusable()"""
        return HF.TailBlockFn.apply(*self._fused_args(x, True))


class MyUnetBlock(nn.Module):
    """Transposed-conv upsampling stage of the skip-less UNETR decoder (reference :241-284; monai get_conv_layer(conv_only,
    is_transposed) == a bias-free ConvTranspose).  Not covered by the HIP convolution kernels: a model that uses it must be built with
    UNETR(allow_torch_decoder=True) (torch's own convolutions; UNETR.forward raises otherwise)."""

    def __init__(self, spatial_dims: int, in_channels: int, out_channels: int, upsample_kernel_size: int, res_block: bool = False) -> None:
        super().__init__()
        conv = nn.ConvTranspose3d if spatial_dims == 3 else nn.ConvTranspose2d
        self.transp_conv = nn.Sequential()
        self.transp_conv.add_module("conv", conv(in_channels, out_channels, kernel_size=upsample_kernel_size,
                                                 stride=upsample_kernel_size, bias=False))

    def forward(self, inp):
        return self.transp_conv(inp.float())


class EmbeddingDenseLayer(nn.Module):
    """time-embedding MLP of DiffusionVIT (reference :286-299): linear -> ReLU -> dropout -> linear.  The two Linears are HIP GEMMs, ReLU
    and dropout one pass (HF.ReluDropoutFn); `dropout` holds the rate and draws the seed (HipDropout), `relu` is kept for the module
    list.  In eval() no mask is generated."""

    def __init__(self, c_in: int, c_out: int, dropout_prob: float):
        super().__init__()
        if not 0.0 <= dropout_prob < 1.0:
            raise ValueError(f"EmbeddingDenseLayer: dropout_prob={dropout_prob} is not inside [0, 1)")
        self.linear1 = Linear(c_in, c_out)
        self.linear2 = Linear(c_out, c_out)
        self.relu = nn.ReLU()
        self.dropout = HipDropout(p=dropout_prob)

    def forward(self, x):
        site = _draw_dropout(self.dropout) or (0.0, 0)
        return self.linear2(HF.ReluDropoutFn.apply(self.linear1(x), *site))


class VariableMapping_Attention(nn.Module):
    """Cross-attention that aggregates the per-variable tokens of every position with a learnt query (reference :301-373).
    forward(var_query [1, N_a = 1, D], x [V, R, D]) -> [R, D]: the q / kv / proj Linears are MFMA GEMMs, the softmax over the V
    variables and the weighted sum are one HBM-bound kernel (csrc/varagg.hip).  One aggregated variable (the reference's
    `aggregated_variables = 1`); x is laid out variable-major instead of [R, V, D] so that no permuted copy is needed."""

    def __init__(self, dim: int, fused_attn: FusedAttn = FusedAttn.NONE, num_heads: int = 8, qkv_bias: bool = False,
                 qk_norm: bool = False, proj_bias: bool = True, attn_drop: float = 0.0, proj_drop: float = 0.0,
                 norm_layer: nn.Module = nn.LayerNorm) -> None:
        super().__init__()
        assert dim % num_heads == 0, 'dim should be divisible by num_heads'
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.fused_attn = fused_attn
        self.q = Linear(dim, dim, bias=qkv_bias)
        self.kv = Linear(dim, dim * 2, bias=qkv_bias)
        self.q_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.k_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = Linear(dim, dim, bias=proj_bias)
        self.proj_drop = nn.Dropout(proj_drop)
        self.qk_norm = qk_norm

    def forward(self, var_query: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        if self.qk_norm or (self.training and (self.attn_drop.p > 0.0 or self.proj_drop.p > 0.0)):
            raise NotImplementedError("qk_norm / dropout inside the variable aggregation are not on the HIP hot path")
        if var_query.shape[1] != 1:
            raise NotImplementedError("aggregated_variables > 1 is not on the HIP hot path")
        V, R, D = x.shape
        q = self.q(var_query.reshape(1, D))                       # [1, D], the same query for every token
        kv = self.kv(x.reshape(V * R, D))                         # [V * R, 2 D]
        out = HF.VarAggFn.apply(kv, q, V, self.head_dim, self.scale)
        return self.proj(out)


def apply_activation_checkpointing(model, check_fn=None):
    """the reference's `apply_activation_checkpointing(model, checkpoint_wrapper_fn=checkpoint_wrapper, check_fn=lambda m: isinstance(m, Block))`
    (training_scripts/train_masked_fsdp.py:393-396) for the HIP Blocks: every Block (or every module check_fn accepts) keeps only its input
    and re-runs its forward launches inside backward (HF.BlockFn recompute).  Returns the number of Blocks switched."""
    n = 0
    for mod in model.modules():
        if isinstance(mod, Block) and (check_fn is None or check_fn(mod)):
            mod.activation_checkpointing = True
            n += 1
    return n
