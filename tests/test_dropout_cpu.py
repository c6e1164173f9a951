"""Element-wise dropout without a GPU: the binding of the two entry points of csrc/dropout.hip, their argument validation (before any HIP
call), the numpy restatement of the mask definition of include/ucfvit_hip.h (tests/dropout_ref.py) against the Random123 known answers
of Philox4x32-10 and against its own statistics, and what HipDropout and the modules that hold one do off the device."""
import ctypes
import math
import re
import subprocess

import numpy as np
import pytest
import torch

import dropout_ref as R

NEW = ("ucfvit_dropout", "ucfvit_dropout_add")


def _lib():
    from UCF_VIT._hip import lib
    return lib, lib.load()


def test_binding_and_abi_version():
    lib, L = _lib()
    for name in NEW:
        assert name in lib.SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (ucfvit_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
    assert lib.ABI_VERSION == L.ucfvit_abi_version() == 24          # symbols were only added


def test_argument_validation_needs_no_gpu():
    lib, L = _lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def add(res=p, ldr=8, br=p, s=p, out=p, rows=4, D=8, rps=2, step=1, prob=0.5, dtype=lib.F32):
        return L.ucfvit_dropout_add(res, ldr, br, s, out, rows, D, rps, step, prob, 7, dtype, None)

    def drop(x=p, s=p, out=p, part=None, rows=4, D=8, rps=2, step=1, prob=0.5, dtype=lib.F32):
        return L.ucfvit_dropout(x, s, out, part, rows, D, rps, step, prob, 7, dtype, None)

    err = lambda: L.ucfvit_last_error().decode()
    assert add(res=None) == -1 and "ucfvit_dropout_add" in err() and "null pointer" in err()
    assert add(br=None) == -1 and "null pointer" in err()
    assert add(out=None) == -1 and "null pointer" in err()
    assert add(D=0, ldr=0) == -1 and "D=0" in err()
    assert add(rows=-1) == -1 and "row count -1" in err()
    assert add(rps=0) == -1 and "rows_per_sample=0" in err()
    assert add(rows=5) == -1 and "not a multiple" in err() and "rows=5" in err()
    assert add(ldr=7) == -1 and "ldr=7" in err()
    assert add(prob=0.0) == -1 and "p=0" in err() and "(0, 1)" in err()
    assert add(prob=1.0) == -1 and "p=1" in err()
    assert add(prob=float("nan")) == -1 and "(0, 1)" in err()
    assert add(step=0) == -1 and "row_step=0" in err()
    assert add(dtype=7) == -1 and "dtype" in err()
    assert drop(x=None) == -1 and "ucfvit_dropout:" in err() and "null pointer" in err()
    assert drop(out=None) == -1 and "null pointer" in err()
    assert drop(D=0) == -1 and "D=0" in err()
    assert drop(rps=-1) == -1 and "rows_per_sample=-1" in err()
    assert drop(rows=7) == -1 and "not a multiple" in err()
    assert drop(prob=-0.1) == -1 and "(0, 1)" in err()
    assert drop(prob=1.5) == -1 and "(0, 1)" in err()
    assert drop(step=-3) == -1 and "row_step=-3" in err()
    assert drop(step=1 << 31, rows=4) == -1 and "row_step" in err()
    assert drop(dtype=-1) == -1 and "dtype" in err()
    assert drop(rows=0, part=p) == -1 and "empty input" in err()
    assert drop(rows=0) == 0 and add(rows=0) == 0                   # nothing to do, no launch


def test_ops_wrappers_refuse_before_the_device():
    from UCF_VIT._hip import ops
    x = torch.zeros(10, 64)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ops.dropout(x, 0.5, 1)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ops.dropout_add(x, x.clone(), 0.5, 1)


KNOWN_ANSWERS = [                                                   # Random123 kat_vectors, philox4x32 10 rounds: counter, key, result
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10(*[np.array([c], dtype=np.uint64) for c in ctr], *key)
    assert tuple(int(g[0]) for g in got) == want


def test_mask_function_is_the_header_definition():
    """words() feeds the counter (lo32(i >> 2), hi32(i >> 2), 0, 0) and the key (lo32(seed), hi32(seed)) and takes word i & 3"""
    assert R.words(0, np.arange(4, dtype=np.uint64)).tolist() == list(KNOWN_ANSWERS[0][2])
    seed = (0x299f31d0 << 32) | 0xa4093822
    i = (0x15a308d3 << 34) | (0x243f6a88 << 2)                       # below 2^64
    blk = R.philox4x32_10(*[np.array([c], dtype=np.uint64) for c in (0x243f6a88, 0x15a308d3, 0, 0)], 0xa4093822, 0x299f31d0)
    assert R.words(seed, np.array([i + j for j in range(4)], dtype=np.uint64)).tolist() == [int(b[0]) for b in blk]
    assert R.threshold(0.5) == 2 ** 31 and R.threshold(0.1) == math.floor(0.1 * 2 ** 32) and R.threshold(1.0 - 2.0 ** -40) == 2 ** 32 - 1
    # row_step: row b of the class-row tail draws the mask of dense row b * N
    dense, tail = R.keep_mask(5, 3 * 7, 12, 0.3), R.keep_mask(5, 3, 12, 0.3, row_step=7)
    assert np.array_equal(tail, dense[::7])


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("seed", [1, 0x9E3779B97F4A7C15, 2 ** 64 - 1])
def test_drop_fraction(seed, p):
    """n = 2^20 elements: the dropped fraction within 4 sqrt(p (1 - p) / n) of p (the nine cases stay within 1.9 sigma)"""
    n = 1 << 20
    frac = 1.0 - R.keep_mask(seed, 1024, 1024, p).mean()
    assert abs(frac - p) <= 4.0 * math.sqrt(p * (1.0 - p) / n), (frac, p)


def test_module_off_the_device():
    from UCF_VIT.simple import building_blocks as S
    from UCF_VIT.fsdp import building_blocks as F
    assert F.HipDropout is S.HipDropout and issubclass(S.HipDropout, torch.nn.Dropout)
    x = torch.randn(4, 5, 8)
    d = S.HipDropout(0.3)
    assert d.p == 0.3 and list(d.parameters()) == [] and d.state_dict() == {}
    assert S.HipDropout(0.0)(x) is x and not S.HipDropout(0.0).active()
    assert d.eval()(x) is x and not d.active()
    d.train()
    assert d.active()
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        d(x)
    # the seed: a 64-bit Python int from the default CPU generator (follows torch.manual_seed) or from a private one
    torch.manual_seed(3)
    a = [d.draw(), d.draw()]
    assert all(isinstance(v, int) and 0 <= v < 2 ** 64 for v in a) and a[0] != a[1] and d.last_seed == a[1]
    torch.manual_seed(3)
    assert [d.draw(), d.draw()] == a
    d.generator = torch.Generator().manual_seed(11)
    torch.manual_seed(3)
    b = [d.draw(), d.draw()]
    assert b != a
    d.generator.manual_seed(11)
    torch.manual_seed(4)                                             # the private generator does not follow the default one
    assert [d.draw(), d.draw()] == b
    assert any(S.HipDropout(0.5).draw() >> 63 for _ in range(64))    # the top bit is drawn too


def test_modules_hold_hip_dropout_and_keep_their_state_dict():
    from UCF_VIT.simple import building_blocks as S
    from UCF_VIT.simple.arch import VIT
    blk = S.Block(64, 2, proj_drop=0.1, attn_drop=0.2)
    for d, p in ((blk.attn.proj_drop, 0.1), (blk.mlp.drop1, 0.1), (blk.mlp.drop2, 0.1), (blk.attn.attn_drop, 0.2)):
        assert isinstance(d, S.HipDropout) and d.p == p
    kw = dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=64, depth=2, num_heads=2)
    plain = VIT(**kw)
    m = VIT(drop_rate=0.1, pos_drop_rate=0.2, proj_drop_rate=0.3, attn_drop_rate=0.4, **kw)
    assert list(m.state_dict()) == list(plain.state_dict())
    assert (m.head_drop.p, m.pos_drop.p, m.blocks[0].attn.proj_drop.p, m.blocks[1].mlp.drop1.p, m.blocks[0].attn.attn_drop.p) == (0.1, 0.2, 0.3, 0.3, 0.4)
    m.eval()
    assert not any(d.active() for d in m.modules() if isinstance(d, S.HipDropout))
    m.train()
    assert sum(d.active() for d in m.modules() if isinstance(d, S.HipDropout)) == 2 + 4 * 2
    with pytest.raises(NotImplementedError, match="attn_drop"):     # still refused, before any device work
        m.blocks[0](torch.zeros(2, 17, 64))


def test_parallel_groups_refuse_active_dropout(monkeypatch):
    from UCF_VIT.fsdp import building_blocks as F
    from UCF_VIT.fsdp import seq_parallel as SP
    from UCF_VIT.simple.arch import VIT
    x = torch.zeros(2, 5, 64)
    blk = F.Block(64, 2, proj_drop=0.2, tensor_par_size=2, tensor_par_group="my_tp_group")      # building it is fine, as it was
    with pytest.raises(NotImplementedError, match="proj_drop=0.2 under a tensor-parallel group.*my_tp_group.*same seed"):
        blk.train()(x)

    class Group:                                                    # stands in for a SeqParallelGroups: only its size is read
        size, rank = 2, 0
    monkeypatch.setattr(SP, "SeqParallelGroups", Group)
    sp = SP.SeqParallelBlock(F.Block(64, 2, proj_drop=0.2), Group())
    with pytest.raises(NotImplementedError, match="proj_drop=0.2 under a sequence-parallel group of 2 ranks.*same seed"):
        sp.train()(x)
    m = VIT(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=64, depth=1, num_heads=2, pos_drop_rate=0.1)
    m.tensor_par_size, m.tensor_par_group = 2, "my_tp_group"
    with pytest.raises(NotImplementedError, match="pos_drop_rate=0.1 under a tensor-parallel group.*my_tp_group.*same seed"):
        m.train()._pos_embed(torch.zeros(2, 16, 64), None)
    # the autograd Functions refuse a dropout site under a tensor-parallel handle themselves
    from UCF_VIT._hip import functional as HF
    with pytest.raises(NotImplementedError, match="tensor-parallel group.*my_tp_group.*same seed"):
        HF._site((0.1, 5), HF.TP("my_tp_group", 2))
    assert HF._site((0.0, 5)) is None and HF._site(None) is None and HF._site((0.1, 5)) == (0.1, 5, 1)


def test_config_keys_reach_the_model_arguments():
    import os
    import sys
    import yaml
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd", "training_scripts"))
    try:
        import _common
    finally:
        sys.path.pop(0)
    conf = yaml.safe_load(open(os.path.join(ROOT, "ucf-vit_amd", "configs", "catsdogs_vit_tiny_smoke.yaml")))
    margs, _, _ = _common.model_args(conf)
    assert margs["pos_drop_rate"] == 0.0 and margs["proj_drop_rate"] == 0.0
    conf["model"]["net"]["init_args"].update(pos_drop_rate=0.05, proj_drop_rate=0.15)
    margs, _, _ = _common.model_args(conf)
    assert margs["pos_drop_rate"] == 0.05 and margs["proj_drop_rate"] == 0.15
    # seed_dropout: one CPU generator per active module, different per rank and per module
    from UCF_VIT.simple.arch import VIT
    kw = dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=64, depth=1, num_heads=2)
    m = VIT(drop_rate=0.1, proj_drop_rate=0.1, **kw)
    seeds = {}
    for rank in (0, 1):
        assert _common.seed_dropout(m, "cpu", rank) == 4
        seeds[rank] = [m.head_drop.draw(), m.blocks[0].attn.proj_drop.draw(), m.blocks[0].mlp.drop1.draw(), m.blocks[0].mlp.drop2.draw()]
        assert m.pos_drop.generator is None and m.blocks[0].attn.attn_drop.generator is None
    assert len(set(seeds[0] + seeds[1])) == 8
    assert _common.seed_dropout(m, "cpu", 0) == 4 and m.head_drop.draw() == seeds[0][0]
