"""Stochastic depth without a GPU: the binding of the three entry points of csrc/drop_path.hip, their argument validation (which happens
before any HIP call), the host function that sizes the column-sum partials, and what the DropPath / Block modules do off the device."""
import ctypes
import re
import subprocess

import pytest
import torch

NEW = ("ucfvit_drop_path_add", "ucfvit_drop_path_scale", "ucfvit_drop_path_colsum_rows")


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
    assert lib.ABI_VERSION == L.ucfvit_abi_version() == 24


def test_argument_validation_needs_no_gpu():
    lib, L = _lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    add = lambda res, ldr, br, s, out, rows, D, rps: L.ucfvit_drop_path_add(res, ldr, br, s, out, rows, D, rps, lib.F32, None)
    scale = lambda x, s, out, rows, D, rps: L.ucfvit_drop_path_scale(x, s, out, None, rows, D, rps, lib.F32, None)
    err = lambda: L.ucfvit_last_error().decode()
    assert add(None, 8, p, p, p, 4, 8, 2) == -1 and "ucfvit_drop_path_add" in err() and "null pointer" in err()
    assert add(p, 8, p, None, p, 4, 8, 2) == -1 and "null pointer" in err()
    assert add(p, 0, p, p, p, 4, 0, 2) == -1 and "D=0" in err()
    assert add(p, 8, p, p, p, 4, 8, 0) == -1 and "rows_per_sample=0" in err()
    assert add(p, 8, p, p, p, 5, 8, 2) == -1 and "not a multiple" in err() and "rows=5" in err()
    assert add(p, 7, p, p, p, 4, 8, 2) == -1 and "ldr=7" in err()
    assert L.ucfvit_drop_path_add(p, 8, p, p, p, 4, 8, 2, 7, None) == -1 and "dtype" in err()
    assert scale(None, p, p, 4, 8, 2) == -1 and "ucfvit_drop_path_scale" in err() and "null pointer" in err()
    assert scale(p, p, None, 4, 8, 2) == -1 and "null pointer" in err()
    assert scale(p, p, p, 4, 0, 2) == -1 and "D=0" in err()
    assert scale(p, p, p, 4, 8, -1) == -1 and "rows_per_sample=-1" in err()
    assert scale(p, p, p, 7, 8, 2) == -1 and "not a multiple" in err()


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("rps", [1, 5, 197])
@pytest.mark.parametrize("D", [64, 100, 192, 1024])
def test_colsum_rows_is_a_host_function(B, rps, D):
    _, L = _lib()
    R = L.ucfvit_drop_path_colsum_rows(B * rps, rps, D)
    assert 0 < R <= max(1, -(-B * rps // 16))                      # at least 16 rows to a chunk
    assert L.ucfvit_drop_path_colsum_rows(665 * 197, 197, 1024) == 512
    assert L.ucfvit_drop_path_colsum_rows(0, rps, D) == 0


def test_module_off_the_device():
    from UCF_VIT.simple import building_blocks as S
    from UCF_VIT.fsdp import building_blocks as F
    x = torch.randn(4, 5, 8)
    assert S.DropPath(0.0)(x) is x
    assert S.DropPath(0.3).eval()(x) is x
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        S.DropPath(0.3).train()(x)
    assert F.DropPath is S.DropPath
    d = S.DropPath(0.25)
    s = d.draw(64, "cpu")                                            # the draw itself is host plumbing: B floats
    assert s.dtype == torch.float32 and tuple(s.shape) == (64,) and d.last_scale is s
    assert set(s.tolist()) <= {0.0, (torch.ones(1) / 0.75).item()}
    assert set(S.DropPath(0.25, scale_by_keep=False).draw(64, "cpu").tolist()) <= {0.0, 1.0}
    assert set(S.DropPath(1.0).draw(8, "cpu").tolist()) == {0.0}     # keep == 0: no division


def test_block_under_a_parallel_group_is_refused(monkeypatch):
    from UCF_VIT.fsdp import building_blocks as F
    from UCF_VIT.fsdp import seq_parallel as SP
    with pytest.raises(NotImplementedError, match="tensor-parallel group.*my_tp_group"):
        F.Block(64, 2, drop_path=0.2, tensor_par_size=2, tensor_par_group="my_tp_group")
    F.Block(64, 2, drop_path=0.0, tensor_par_size=2, tensor_par_group="my_tp_group")

    class Group:                                                    # stands in for a SeqParallelGroups: only its size is read
        size, rank = 2, 0
    monkeypatch.setattr(SP, "SeqParallelGroups", Group)
    with pytest.raises(NotImplementedError, match="sequence-parallel group of 2 ranks"):
        SP.SeqParallelBlock(F.Block(64, 2, drop_path=0.2), Group())
    SP.SeqParallelBlock(F.Block(64, 2), Group())
