"""LayerScale without a GPU: the binding of the two entry points of csrc/layer_scale.hip, their argument validation (which happens before
any HIP call), what the LayerScale / Block modules and the models do off the device, the config key, and the float64 Block restatement of
tests/layer_scale_ref.py pinned to the reference fixture."""
import ctypes
import re
import subprocess

import pytest
import torch

from conftest import load_golden, rel_err

NEW = ("ucfvit_layer_scale_add", "ucfvit_layer_scale_grad")


def _lib():
    from UCF_VIT._hip import lib
    return lib, lib.load()


def test_binding_and_abi_version():
    lib, L = _lib()
    for name in NEW:
        assert name in lib.SIGNATURES
    assert len(lib.SIGNATURES["ucfvit_layer_scale_add"][1]) == 14 and len(lib.SIGNATURES["ucfvit_layer_scale_grad"][1]) == 15
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (ucfvit_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
    assert lib.ABI_VERSION == L.ucfvit_abi_version() == 24


def test_argument_validation_needs_no_gpu():
    lib, L = _lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    err = lambda: L.ucfvit_last_error().decode()

    def add(res=p, ldr=8, br=p, gamma=p, s=None, out=p, rows=4, D=8, rps=2, step=1, prob=0.0, seed=0, dtype=lib.F32):
        return L.ucfvit_layer_scale_add(res, ldr, br, gamma, s, out, rows, D, rps, step, prob, seed, dtype, None)

    def grad(dy=p, br=p, gamma=p, s=None, out=p, pc=None, pg=None, rows=4, D=8, rps=2, step=1, prob=0.0, seed=0, dtype=lib.F32):
        return L.ucfvit_layer_scale_grad(dy, br, gamma, s, out, pc, pg, rows, D, rps, step, prob, seed, dtype, None)

    assert add(br=None) == -1 and "ucfvit_layer_scale_add" in err() and "null pointer" in err()
    assert add(out=None) == -1 and "null pointer" in err()
    assert add(gamma=None) == -1 and "null gamma" in err()
    assert add(D=0, ldr=0) == -1 and "D=0" in err()
    assert add(rps=0) == -1 and "rows_per_sample=0" in err()
    assert add(rows=-1) == -1 and "bad row count -1" in err()
    assert add(rows=5) == -1 and "not a multiple" in err() and "rows=5" in err()
    assert add(ldr=7) == -1 and "ldr=7" in err()
    assert add(res=None, ldr=0, rows=0) == 0                                   # without a residual ldr is ignored; no rows: no launch
    assert add(prob=1.0) == -1 and "p=1" in err() and "[0, 1)" in err()
    assert add(prob=-0.25) == -1 and "p=-0.25" in err()
    assert add(prob=float("nan")) == -1 and "[0, 1)" in err()
    assert add(step=0) == -1 and "row_step=0" in err()
    assert add(step=1 << 31) == -1 and "row_step" in err()
    assert add(dtype=7) == -1 and "dtype" in err()

    assert grad(dy=None) == -1 and "ucfvit_layer_scale_grad" in err() and "null pointer" in err()
    assert grad(out=None) == -1 and "null pointer" in err()
    assert grad(gamma=None) == -1 and "null gamma" in err()
    assert grad(br=None, pg=p) == -1 and "branch is null" in err()
    assert grad(br=None, rows=0) == 0                                          # allowed without the gamma sums
    assert grad(D=0) == -1 and "D=0" in err()
    assert grad(rps=-1) == -1 and "rows_per_sample=-1" in err()
    assert grad(rows=7) == -1 and "not a multiple" in err()
    assert grad(prob=1.0) == -1 and "[0, 1)" in err()
    assert grad(prob=-1e-9) == -1 and "[0, 1)" in err()
    assert grad(step=0) == -1 and "row_step=0" in err()
    assert grad(dtype=3) == -1 and "dtype" in err()
    assert grad(rows=0, pc=p) == -1 and "empty input" in err()
    assert grad(rows=0, pg=p) == -1 and "empty input" in err()


def test_module_off_the_device():
    from UCF_VIT.simple import building_blocks as S
    from UCF_VIT.fsdp import building_blocks as F
    ls = S.LayerScale(8, init_values=0.25)
    assert F.LayerScale is S.LayerScale
    assert list(ls.state_dict()) == ["gamma"] and torch.equal(ls.gamma.detach(), torch.full((8,), 0.25))
    assert ls.gamma.dtype == torch.float32 and ls.gamma.requires_grad
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ls(torch.randn(4, 5, 8))


@pytest.mark.parametrize("pkg", ["simple", "fsdp"])
def test_block_with_init_values_is_fusable(pkg):
    import importlib
    BB = importlib.import_module(f"UCF_VIT.{pkg}.building_blocks")
    blk = BB.Block(64, 2, qkv_bias=True, init_values=0.1)
    assert blk._fusable()
    assert isinstance(blk.ls1, BB.LayerScale) and isinstance(blk.ls2, BB.LayerScale)
    assert {"ls1.gamma", "ls2.gamma"} <= set(blk.state_dict())
    assert BB.Block(64, 2, qkv_bias=True)._fusable()
    blk.ls2 = torch.nn.Identity()                                  # one branch only: not what Block builds, not fused
    assert not blk._fusable()


def test_block_under_a_parallel_group_is_refused(monkeypatch):
    from UCF_VIT.fsdp import building_blocks as F
    from UCF_VIT.fsdp import seq_parallel as SP
    with pytest.raises(NotImplementedError, match="init_values=0.1.*tensor-parallel group.*my_tp_group"):
        F.Block(64, 2, init_values=0.1, tensor_par_size=2, tensor_par_group="my_tp_group")
    F.Block(64, 2, tensor_par_size=2, tensor_par_group="my_tp_group")

    class Group:                                                    # stands in for a SeqParallelGroups
        size, rank, sp_group = 2, 0, "my_sp_group"
    monkeypatch.setattr(SP, "SeqParallelGroups", Group)
    with pytest.raises(NotImplementedError, match="sequence-parallel group of 2 ranks.*my_sp_group"):
        SP.SeqParallelBlock(F.Block(64, 2, init_values=0.1), Group())
    SP.SeqParallelBlock(F.Block(64, 2), Group())


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
def test_models_build_layer_scale_with_the_reference_keys(name):
    from UCF_VIT.simple import arch
    kw = MODEL_KW[name]
    m = getattr(arch, name)(init_values=0.1, **kw)
    sd = m.state_dict()
    stacks = [("blocks", kw["depth"], kw["embed_dim"])]
    if "decoder_depth" in kw:
        stacks.append(("decoder_blocks", kw["decoder_depth"], kw["decoder_embed_dim"]))
    for stack, depth, dim in stacks:
        for i in range(depth):
            for ls in ("ls1", "ls2"):
                g = sd[f"{stack}.{i}.{ls}.gamma"]
                assert g.dtype == torch.float32 and torch.equal(g, torch.full((dim,), 0.1)), (stack, i, ls)
        assert all(b._fusable() for b in getattr(m, stack))
    plain = getattr(arch, name)(**kw).state_dict()
    assert not any("gamma" in k for k in plain) and set(plain) < set(sd)


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
    assert model_args(conf)[0]["init_values"] is None
    conf["model"]["net"]["init_args"]["init_values"] = 1e-5
    margs = model_args(conf)[0]
    assert margs["init_values"] == 1e-5 and "drop_path_rate" in margs


def test_fp64_restatement_reproduces_the_reference_block():
    """tests/layer_scale_ref.block64 against the reference Block(init_values) recorded in op_block_layerscale.npz (fp32, CPU): y, gx and
    every parameter gradient, conftest.rel_err < 1e-5.  Measured: at most 3.7e-7 (fp32 round-off of the reference's own 64-wide
    Block), twenty-seven times below the bound."""
    import layer_scale_ref as LR
    g = load_golden("op_block_layerscale.npz")
    P = LR.p64((k[2:], v) for k, v in g.items() if k.startswith("w."))
    assert "ls1.gamma" in P and "ls2.gamma" in P
    x = g["x"].double().requires_grad_(True)
    y = LR.block64(x, P, 2, 1e-6)
    y.backward(g["gy"].double())
    worst = max(rel_err(y, g["y"]), rel_err(x.grad, g["gx"]))
    assert worst < 1e-5
    for k, v in P.items():
        e = rel_err(v.grad, g["g." + k])
        worst = max(worst, e)
        assert e < 1e-5, k
    print("worst rel_err", worst)
    # the gammas matter at this tolerance: without them the restatement is far off
    Q = {k: v for k, v in P.items() if "gamma" not in k}
    assert rel_err(LR.block64(g["x"].double(), Q, 2, 1e-6), g["y"]) > 1e-2
