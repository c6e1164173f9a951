"""ucfvit_ddim_step on the MI355X: bit for bit against the fp32 restatement of the header's operation order (csrc/diffusion.hip is compiled
without fma contraction, so every product and sum is rounded on its own), and element by element against float64 with the first-order bound
that tests/ddim_ref.py derives from the restatement's rounding count (ddim_step64).  pred in fp32 and bf16, with and without noise, without a
clamp and with clip = 1 and 0.25, out = x and out apart, 2-D and 3-D patch geometry."""
import numpy as np
import pytest
import torch

import ddim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [((2, 3, 8, 8), 4), ((1, 1, 8, 12), 4), ((2, 2, 4, 4, 8), 2)]
# s_ab^2 + s_1mab^2 = 1 as for a real step (abar = 0.36), c_x0 and c_eps of abar_prev = 0.64 with sigma = 0.3
COEF = tuple(float(np.float32(v)) for v in (0.6, 0.8, 1 / 0.6, 1 / 0.8, 0.8, np.sqrt(0.36 - 0.09), 0.3))
_REF = {}


def rnd(shape, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal(tuple(shape)).astype(np.float32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def case(shape, p, dtype):
    """inputs and references of one (shape, pred dtype), computed once: x, z, pred (torch, host), e = unpatchify(pred) as the kernel reads it"""
    key = (shape, p, dtype)
    if key not in _REF:
        x, z = rnd(shape, 1), rnd(shape, 2)
        pred = torch.from_numpy(R.patchify(rnd(shape, 3), p)).contiguous().to(dtype)
        e = R.unpatchify(pred.float().numpy(), shape[1], shape[2:], p)
        _REF[key] = (x, z, pred, np.ascontiguousarray(e))
    return _REF[key]


def coef_for(has_z):
    return COEF if has_z else COEF[:6] + (0.0,)


@pytest.mark.parametrize("clip", [0.0, 1.0, 0.25])
@pytest.mark.parametrize("has_z", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,p", SHAPES)
def test_ddim_step(shape, p, dtype, has_z, clip):
    from UCF_VIT._hip import ops
    x, z, pred, e = case(shape, p, dtype)
    coef = coef_for(has_z)
    zz = z if has_z else None
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    out = ops.ddim_step(dev(x), pred.to(DEV), dev(zz), p, *coef, clip=clip)
    assert out.shape == tuple(shape) and out.dtype == torch.float32
    got = out.cpu().numpy()
    want32, hit = R.ddim_step32(x, e, zz, coef, clip)
    if clip == 0.25:
        assert hit.mean() >= 1 / 3                                          # the clamp branch is really exercised
    elif clip == 0.0:
        assert not hit.any()
    assert same_bits(got, want32)
    want64, bound = R.ddim_step64(x, e, zz, coef, clip)
    err = np.abs(got.astype(np.float64) - want64)
    print(f"ddim_step {shape} p={p} {dtype} z={has_z} clip={clip}: worst err/bound {np.max(err / bound):.3f} clamped {hit.mean():.2f}")
    assert (err <= bound).all()
    xin = dev(x)
    assert ops.ddim_step(xin, pred.to(DEV), dev(zz), p, *coef, clip=clip, out=xin) is xin                   # out may be x
    assert same_bits(xin.cpu().numpy(), got)
    if clip == 0.0:
        assert same_bits(ops.ddim_step(dev(x), pred.to(DEV), dev(zz), p, *coef, clip=None).cpu().numpy(), got)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_nan_stays_nan_under_the_clamp(dtype):
    from UCF_VIT._hip import ops
    shape, p = SHAPES[0]
    x, z, pred, e = case(shape, p, dtype)
    x = x.copy()
    x[0, 1, 2, 3] = np.nan
    x[1, 0, 7, 7] = np.inf                                                  # x0 = +Inf clamps to clip; e' = (Inf - ..) = Inf
    out = ops.ddim_step(torch.from_numpy(x).to(DEV), pred.to(DEV), torch.from_numpy(z).to(DEV), p, *COEF, clip=1.0).cpu().numpy()
    assert np.isnan(out[0, 1, 2, 3])
    mask = np.ones(shape, dtype=bool)
    mask[0, 1, 2, 3] = mask[1, 0, 7, 7] = False
    assert np.isfinite(out[mask]).all()
    want32, _ = R.ddim_step32(x, e, z, COEF, 1.0)
    assert same_bits(out[mask], want32[mask]) and not np.isfinite(out[1, 0, 7, 7])


def test_python_checks_on_the_device():
    from UCF_VIT._hip import ops
    shape, p = SHAPES[0]
    x, z, pred, _ = case(shape, p, torch.float32)
    xd, zd, pd = torch.from_numpy(x).to(DEV), torch.from_numpy(z).to(DEV), pred.to(DEV)
    with pytest.raises(ValueError, match="pred"):
        ops.ddim_step(xd, pd[:, :-1].contiguous(), None, p, *coef_for(False))
    with pytest.raises(ValueError, match="z must have x's shape"):
        ops.ddim_step(xd, pd, zd[:1], p, *COEF)
    with pytest.raises(Exception, match="without noise"):
        ops.ddim_step(xd, pd, None, p, *COEF)                               # sigma != 0 without z
    with pytest.raises(ValueError, match="clip"):
        ops.ddim_step(xd, pd, zd, p, *COEF, clip=-0.5)
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x)
