"""qk_norm without a GPU: the binding of the entry points of csrc/qk_norm.hip, their argument validation (which happens before any HIP
call), the _fusable decisions and messages of the Attention / Block modules, the tensor- and sequence-parallel refusals, the config key,
the state_dict layout, and the float64 restatements of tests/qk_norm_ref.py pinned to the three reference fixtures."""
import ctypes
import importlib
import re
import subprocess

import pytest
import torch
import torch.nn as nn

from conftest import load_golden, rel_err

NEW = ("ucfvit_qk_norm_fwd", "ucfvit_qk_norm_bwd", "ucfvit_qk_norm_partial_rows")
QK_KEYS = {"q_norm.weight", "q_norm.bias", "k_norm.weight", "k_norm.bias"}


def _lib():
    from UCF_VIT._hip import lib
    return lib, lib.load()


def test_binding_and_abi_version():
    lib, L = _lib()
    for name in NEW:
        assert name in lib.SIGNATURES
    assert len(lib.SIGNATURES["ucfvit_qk_norm_fwd"][1]) == 14 and len(lib.SIGNATURES["ucfvit_qk_norm_bwd"][1]) == 13
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (ucfvit_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
    assert lib.ABI_VERSION == L.ucfvit_abi_version() == 24


def test_argument_validation_needs_no_gpu():
    lib, L = _lib()
    raw = (ctypes.c_float * 260)()
    p = (ctypes.addressof(raw) + 15) & ~15                                     # 16-byte aligned
    err = lambda: L.ucfvit_last_error().decode()

    def fwd(qkv=p, gq=p, bq=p, gk=p, bk=p, saved=p, mean=p, rstd=p, rows=4, H=2, dh=32, eps=1e-6, dtype=lib.F32):
        return L.ucfvit_qk_norm_fwd(qkv, gq, bq, gk, bk, saved, mean, rstd, rows, H, dh, eps, dtype, None)

    def bwd(dqkv=p, saved=p, gq=p, gk=p, mean=p, rstd=p, pp=None, cp=None, rows=4, H=2, dh=32, dtype=lib.F32):
        return L.ucfvit_qk_norm_bwd(dqkv, saved, gq, gk, mean, rstd, pp, cp, rows, H, dh, dtype, None)

    assert fwd(qkv=None) == -1 and "ucfvit_qk_norm_fwd" in err() and "null pointer" in err()
    for k in ("gq", "bq", "gk", "bk"):
        assert fwd(**{k: None}) == -1 and "null parameter" in err(), k
    assert fwd(mean=None, rstd=None) == -1 and "go together" in err()
    assert fwd(saved=None) == -1 and "go together" in err()
    assert fwd(rstd=None) == -1 and "go together" in err()
    for dh in (0, 16, 48, 96, 256):
        assert fwd(dh=dh) == -1 and f"dh={dh}" in err()
    assert fwd(H=0) == -1 and "H=0" in err()
    assert fwd(rows=-1) == -1 and "bad row count -1" in err()
    assert fwd(rows=1 << 31) == -1 and "bad row count" in err()
    assert fwd(eps=-1.0) == -1 and "bad eps" in err()
    assert fwd(eps=float("nan")) == -1 and "bad eps" in err()
    assert fwd(dtype=7) == -1 and "dtype" in err()
    assert fwd(qkv=p + 4) == -1 and "16-byte aligned" in err()
    assert fwd(saved=p + 8) == -1 and "16-byte aligned" in err()
    assert fwd(rows=0) == 0 and fwd(rows=0, saved=None, mean=None, rstd=None, dtype=lib.BF16, dh=128, H=16) == 0      # no rows: no launch

    assert bwd(dqkv=None) == -1 and "ucfvit_qk_norm_bwd" in err() and "null pointer" in err()
    for k in ("saved", "mean", "rstd"):
        assert bwd(**{k: None}) == -1 and "null pointer" in err(), k
    assert bwd(gq=None) == -1 and "null parameter" in err()
    assert bwd(gk=None) == -1 and "null parameter" in err()
    assert bwd(dh=40) == -1 and "dh=40" in err()
    assert bwd(H=-3) == -1 and "H=-3" in err()
    assert bwd(rows=-2) == -1 and "bad row count -2" in err()
    assert bwd(dtype=9) == -1 and "dtype" in err()
    assert bwd(dqkv=p + 4) == -1 and "16-byte aligned" in err()
    assert bwd(rows=0, pp=p) == -1 and "empty input" in err()
    assert bwd(rows=0, cp=p) == -1 and "empty input" in err()
    assert bwd(rows=0) == 0

    R = L.ucfvit_qk_norm_partial_rows
    assert R(0, 2, 32) == 0 and R(4, 0, 32) == 0 and R(4, 2, 33) == 0 and R(1 << 31, 2, 32) == 0
    assert R(1, 1, 32) == 1 and R(16, 3, 64) == 1 and R(17, 3, 64) == 2 and 1 < R(3 * 197, 16, 64) < 3 * 197
    assert R(665 * 197, 16, 64) <= 1024


def test_ops_refuse_cpu_tensors():
    from UCF_VIT._hip import ops
    qkv, g = torch.zeros(4, 3 * 2 * 32), torch.ones(32)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ops.qk_norm_fwd(qkv, g, g, g, g, 2, 32, 1e-6)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ops.qk_norm_bwd(qkv, torch.zeros(4, 2 * 2 * 32), g, g, torch.zeros(4, 4), torch.zeros(4, 4), 2, 32)


@pytest.mark.parametrize("pkg", ["simple", "fsdp"])
def test_fusable_decisions_and_messages(pkg):
    BB = importlib.import_module(f"UCF_VIT.{pkg}.building_blocks")
    att = BB.Attention(64, num_heads=2, qkv_bias=True, qk_norm=True)
    assert att._fusable() and att.q_norm.eps == att.k_norm.eps == 1e-5                # a bare Attention: nn.LayerNorm's default
    assert QK_KEYS <= set(att.state_dict()) and att.q_norm.weight.shape == (32,)
    assert BB.Attention(64, num_heads=2)._fusable()                                    # both Identity
    blk = BB.Block(64, 2, qkv_bias=True, qk_norm=True, init_values=0.1, norm_layer=lambda d: BB.LayerNorm(d, eps=1e-6))
    assert blk._fusable() and blk.attn.q_norm.eps == 1e-6                              # the Block hands its norm_layer down
    x = torch.zeros(1, 3, 64)

    def refused(mod, pattern):
        assert not mod._fusable()
        with pytest.raises(NotImplementedError, match=pattern):
            mod(x)

    a = BB.Attention(64, num_heads=2, qk_norm=True)
    a.k_norm = nn.Identity()
    refused(a, "k_norm is Identity")
    a = BB.Attention(64, num_heads=2, qk_norm=True)
    a.q_norm = nn.GroupNorm(1, 32)
    refused(a, "q_norm is GroupNorm")
    a = BB.Attention(64, num_heads=2, qk_norm=True)
    a.q_norm = nn.LayerNorm(32, elementwise_affine=False)
    refused(a, "q_norm has no affine weight and bias")
    a = BB.Attention(64, num_heads=2, qk_norm=True)
    a.k_norm = nn.LayerNorm(32, bias=False)
    refused(a, "k_norm has no affine weight and bias")
    a = BB.Attention(64, num_heads=2, qk_norm=True)
    a.k_norm = nn.LayerNorm(32, eps=1e-6)
    refused(a, "q_norm.eps = 1e-05 differs from k_norm.eps = 1e-06")
    a = BB.Attention(64, num_heads=2, qk_norm=True)
    a.q_norm = nn.LayerNorm(64)
    refused(a, r"q_norm normalises over \(64,\), not over \(head_dim,\) = \(32,\)")
    blk.attn.k_norm = nn.LayerNorm(32, eps=1e-3)
    assert not blk._fusable()
    with pytest.raises(NotImplementedError, match="differs from k_norm.eps"):        # what the unfused line of the Block then reaches
        blk.attn(x)


def test_parallel_groups_and_variable_aggregation_refuse(monkeypatch):
    from UCF_VIT.fsdp import building_blocks as F
    from UCF_VIT.fsdp import seq_parallel as SP
    from UCF_VIT.simple import building_blocks as S
    with pytest.raises(NotImplementedError, match="qk_norm=True.*tensor-parallel group.*my_tp_group.*tensor_par_size=2"):
        F.Block(64, 2, qk_norm=True, tensor_par_size=2, tensor_par_group="my_tp_group")
    with pytest.raises(NotImplementedError, match="qk_norm=True.*tensor-parallel group.*my_tp_group"):
        F.Attention(64, num_heads=2, qk_norm=True, tensor_par_size=2, tensor_par_group="my_tp_group")
    F.Block(64, 2, tensor_par_size=2, tensor_par_group="my_tp_group")

    class Group:                                                    # stands in for a SeqParallelGroups
        size, rank, sp_group = 2, 0, "my_sp_group"
    monkeypatch.setattr(SP, "SeqParallelGroups", Group)
    with pytest.raises(NotImplementedError, match="qk_norm=True.*sequence-parallel group of 2 ranks.*my_sp_group"):
        SP.SeqParallelBlock(F.Block(64, 2, qk_norm=True), Group())
    SP.SeqParallelBlock(F.Block(64, 2), Group())

    # the raw sequences refuse a group too (a caller that bypasses the modules)
    from UCF_VIT._hip import functional as HF
    g = torch.ones(32)
    with pytest.raises(NotImplementedError, match="qk_norm under a tensor-parallel group.*'local'.*size 2"):
        HF._refuse_group_qk_norm(HF.TP("local", 2), (g, g, g, g, 1e-6))
    HF._refuse_group_qk_norm(HF.TP("local", 2), None)
    with pytest.raises(ValueError, match="together"):
        HF._qkn_of(g, g, g, None, 1e-6)

    v = S.VariableMapping_Attention(64, num_heads=2, qk_norm=True)
    with pytest.raises(NotImplementedError, match="qk_norm"):
        v(torch.zeros(1, 1, 64), torch.zeros(1, 3, 64))


MODEL_KW = {
    "VIT": dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=64, depth=2, num_heads=2),
    "MAE": dict(img_size=[32, 32], patch_size=8, in_chans=3, embed_dim=64, depth=2, num_heads=2, class_token=False, weight_init='skip',
                mask_ratio=0.75, linear_decoder=False, decoder_depth=2, decoder_embed_dim=32, decoder_num_heads=1, mlp_ratio_decoder=4.0),
    "UNETR": dict(num_classes=4, linear_decoder=False, feature_size=4, skip_connection=True, allow_torch_decoder=True, img_size=[32, 32, 16],
                  patch_size=8, in_chans=1, embed_dim=96, depth=4, num_heads=3, class_token=False, twoD=False),
    "SAP": dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=3, embed_dim=64, depth=2, num_heads=2, class_token=False, sqrt_len=4),
    "DiffusionVIT": dict(img_size=[32, 32], patch_size=8, in_chans=3, embed_dim=64, depth=2, num_heads=2, class_token=False,
                         linear_decoder=False, decoder_depth=2, decoder_embed_dim=32, decoder_num_heads=1, mlp_ratio_decoder=4.0, time_steps=10),
}


@pytest.mark.parametrize("name", list(MODEL_KW))
def test_models_hand_qk_norm_down(name):
    from UCF_VIT.simple import arch
    kw = MODEL_KW[name]
    m = getattr(arch, name)(qk_norm=True, **kw)
    sd = m.state_dict()
    stacks = [("blocks", kw["depth"], kw["embed_dim"] // kw["num_heads"])]
    if "decoder_depth" in kw:
        stacks.append(("decoder_blocks", kw["decoder_depth"], kw["decoder_embed_dim"] // kw["decoder_num_heads"]))
    for stack, depth, dh in stacks:
        for i in range(depth):
            for k in QK_KEYS:
                t = sd[f"{stack}.{i}.attn.{k}"]
                assert t.dtype == torch.float32 and t.shape == (dh,), (stack, i, k)
        for b in getattr(m, stack):
            assert b._fusable() and b.attn.q_norm.eps == b.norm1.eps == 1e-6       # the models' norm_layer, handed down by the Block
    plain = getattr(arch, name)(**kw).state_dict()
    assert not any("q_norm" in k or "k_norm" in k for k in plain) and set(plain) < set(sd)


def test_state_dict_keys_match_the_fixtures():
    from UCF_VIT.simple import arch
    from UCF_VIT.simple import building_blocks as S
    g = load_golden("op_attn_qknorm.npz")
    att = S.Attention(64, num_heads=2, qkv_bias=True, qk_norm=True)
    assert {k[2:] for k in g if k.startswith("w.")} == set(att.state_dict())
    assert {k[2:]: tuple(v.shape) for k, v in g.items() if k.startswith("w.")} == {k: tuple(v.shape) for k, v in att.state_dict().items()}
    g = load_golden("op_block_qknorm.npz")
    blk = S.Block(64, 2, qkv_bias=True, qk_norm=True, init_values=0.5)
    assert {k[2:] for k in g if k.startswith("w.")} == set(blk.state_dict())
    g = load_golden("model_vit_qknorm.npz")
    m = arch.VIT(qk_norm=True, **MODEL_KW["VIT"])
    assert {k[2:] for k in g if k.startswith("g.")} == {k for k, _ in m.named_parameters()}
    assert {k[2:] for k in g if k.startswith("w.")} == {k for k in m.state_dict() if "q_norm" in k or "k_norm" in k}


def test_model_args_reads_the_config_key():
    import os
    import sys
    import yaml
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd", "training_scripts"))
    try:
        from _common import model_args
    finally:
        sys.path.pop(0)
    conf = yaml.safe_load(open(os.path.join(ROOT, "ucf-vit_amd", "configs", "catsdogs_vit_tiny_smoke.yaml")))
    assert model_args(conf)[0]["qk_norm"] is False
    conf["model"]["net"]["init_args"]["qk_norm"] = True
    margs = model_args(conf)[0]
    assert margs["qk_norm"] is True and "init_values" in margs


def _check(y, x, P, g, bound=1e-5):
    worst = max(rel_err(y, g["y"]), rel_err(x.grad, g["gx"]))
    assert worst < bound
    for k, v in P.items():
        e = _grad_err(k, v.grad, g)
        worst = max(worst, e)
        assert e < bound, k
    return worst


def _grad_err(k, grad, g):
    """conftest.rel_err of one parameter gradient against the fixture's.  k_norm.bias is the exception: a key bias shifts every score of a
    query alike, so its gradient is mathematically 0 and the reference records only the round-off of a cancelling sum whose terms are those
    of q_norm.bias's gradient: the difference is measured against THAT gradient's largest entry."""
    if k.endswith("k_norm.bias"):
        ref = g["g." + k[:-len("k_norm.bias")] + "q_norm.bias"]
        return ((grad.detach().double() - g["g." + k].double()).abs().max() / ref.double().abs().max()).item()
    return rel_err(grad, g["g." + k])


def test_fp64_restatement_reproduces_the_reference_attention():
    """qk_norm_ref.attn64_qkn against the reference Attention(qk_norm=True) of op_attn_qknorm.npz (fp32, CPU, eps 1e-5): y, gx and every
    parameter gradient, conftest.rel_err < 1e-5."""
    import qk_norm_ref as QR
    g = load_golden("op_attn_qknorm.npz")
    P = QR.p64((k[2:], v) for k, v in g.items() if k.startswith("w."))
    assert QK_KEYS <= set(P)
    x = g["x"].double().requires_grad_(True)
    y = QR.attn64_qkn(x, P, 2, 1e-5, pre="")
    y.backward(g["gy"].double())
    print("worst rel_err", _check(y, x, P, g))
    # the parameters matter at this tolerance: swapped between q and k, or left out, the restatement is far off
    Q = dict(P)
    Q["q_norm.weight"], Q["k_norm.weight"] = P["k_norm.weight"], P["q_norm.weight"]
    assert rel_err(QR.attn64_qkn(g["x"].double(), Q, 2, 1e-5, pre=""), g["y"]) > 1e-3
    Q = {k: v for k, v in P.items() if "_norm" not in k}
    assert rel_err(QR.attn64_qkn(g["x"].double(), Q, 2, 1e-5, pre=""), g["y"]) > 1e-3


def test_fp64_restatement_reproduces_the_reference_block():
    """qk_norm_ref.block64_qkn against the reference Block(qk_norm=True, init_values=0.5) of op_block_qknorm.npz (eps 1e-6)."""
    import qk_norm_ref as QR
    g = load_golden("op_block_qknorm.npz")
    P = QR.p64((k[2:], v) for k, v in g.items() if k.startswith("w."))
    assert "ls1.gamma" in P and "attn.q_norm.weight" in P
    x = g["x"].double().requires_grad_(True)
    y = QR.block64_qkn(x, P, 2, 1e-6)
    y.backward(g["gy"].double())
    print("worst rel_err", _check(y, x, P, g))
    Q = {k: v for k, v in P.items() if "_norm." not in k or k.startswith("norm")}
    assert rel_err(QR.block64_qkn(g["x"].double(), Q, 2, 1e-6), g["y"]) > 1e-3
    # the second recorded backward: an output gradient that is zero outside the class row
    P = QR.p64((k[2:], v) for k, v in g.items() if k.startswith("w."))
    x = g["x"].double().requires_grad_(True)
    QR.block64_qkn(x, P, 2, 1e-6)[:, 0].backward(g["gy"][:, 0].double())
    gc = {"g." + k[5:]: v for k, v in g.items() if k.startswith("gcls.")}
    assert rel_err(x.grad, g["gx_cls"]) < 1e-5
    for k, v in P.items():
        assert _grad_err(k, v.grad, gc) < 1e-5, k


def vit_qknorm_state_dict(model, g):
    """the weights model_vit_qknorm.npz was generated with: det_state_dict(model, 77), then the recorded q_norm / k_norm parameters"""
    from det_weights import det_state_dict
    sd = det_state_dict(model, 77)
    for k, v in g.items():
        if k.startswith("w."):
            assert k[2:] in sd
            sd[k[2:]] = v.clone()
    return sd


def test_fp64_restatement_reproduces_the_reference_model():
    """The torch oracle's small VIT in float64 with its Blocks replaced by qk_norm_ref.block64_qkn, against the reference
    VIT(qk_norm=True) of model_vit_qknorm.npz: logits, loss and every parameter gradient, conftest.rel_err < 1e-5."""
    import qk_norm_ref as QR
    from oracle import ucf_vit_ref as R
    from UCF_VIT.simple import arch
    g = load_golden("model_vit_qknorm.npz")
    sd = vit_qknorm_state_dict(arch.VIT(qk_norm=True, **MODEL_KW["VIT"]), g)
    m = R.VIT([32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=64, depth=2, num_heads=2).double()
    qk = {k: v.double().requires_grad_(True) for k, v in sd.items() if "q_norm" in k or "k_norm" in k}
    assert len(qk) == 8
    m.load_state_dict({k: v.double() for k, v in sd.items() if k not in qk})

    class Block64(torch.nn.Module):
        def __init__(self, inner, i):
            super().__init__()
            self.inner, self.i = inner, i

        def forward(self, x):
            P = dict(self.inner.named_parameters())
            P.update({k[len(f"blocks.{self.i}."):]: v for k, v in qk.items() if k.startswith(f"blocks.{self.i}.")})
            return QR.block64_qkn(x, P, 2, 1e-6)

    m.blocks = torch.nn.Sequential(*[Block64(b, i) for i, b in enumerate(m.blocks)])
    out = m(g["x"].double())
    loss = torch.nn.CrossEntropyLoss()(out, g["labels"])
    loss.backward()
    assert rel_err(out, g["logits"]) < 1e-5 and abs(loss.item() - g["loss"].item()) < 1e-5 * max(1.0, abs(g["loss"].item()))
    worst = 0.0
    for k, p in list(m.named_parameters()) + list(qk.items()):
        k = k.replace(".inner.", ".")
        e = _grad_err(k, p.grad, g)
        worst = max(worst, e)
        assert e < 1e-5, k
    print("worst rel_err", worst)
    # a key bias shifts every score of a query alike: the softmax does not see it
    for i in range(2):
        assert g[f"g.blocks.{i}.attn.k_norm.bias"].abs().max() < 1e-3 * g[f"g.blocks.{i}.attn.q_norm.bias"].abs().max()
