"""float64 references and derived bounds for gradient clipping by global norm (csrc/grad_clip.hip).

What the kernels compute.  x_i = fl32(g_i * k) is the value AdamW consumes: k = mult without a loss scaler, k = fl32(mult * inv_scale) with
one.  NORM = fl32(sqrt(S)), S the sum of x_i^2 accumulated in double.  COEF = min(1, MAX_NORM / (NORM + 1e-6)) in fp32, NaN kept.

Bound of NORM (norm_bound).  The square of an fp32 value has 48 significant bits and is exact in double, so the only roundings of S are its
additions, at most one per term however the terms are grouped: n of them inside the segments and `partials` more in the final fold.  All
terms are non-negative, so each addition perturbs the running sum by at most u64 = 2^-53 relative and the sum by at most
(n + partials) u64 relative to first order, independent of the order.  The double square root adds u64 and halves the relative error of its
argument; the rounding to fp32 adds u32 = 2^-24.  Together

    |NORM - norm64| <= norm64 * (u32 + ((n + partials) / 2 + 2) * u64) * (1 + 2^-20),

the last factor covering the products of these terms.  At the sizes used here the u64 part is below 2^-30: the bound is the half ulp of the
final rounding, as it should be for a sum carried in double.

Bound of COEF (coef_bound), where it is below 1: COEF = fl32(M / fl32(NORM + 1e-6)).  The reference divides M by norm64 + 1e-6 in double.
NORM carries norm_bound, the constant 1e-6f differs from 1e-6 by less than 2^-25 relative of itself, the sum and the quotient round once each:
the relative error is at most rel(NORM) + 3 u32 to first order."""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53


def f32(x):
    return np.float32(x)


def products(g, mult=1.0, inv_scale=None):
    """fl32(g * k) as float64 values; g an array of float32 (bf16 gradients are passed widened, which is exact)"""
    g = np.asarray(g, dtype=np.float32)
    k = f32(mult) if inv_scale is None else f32(f32(mult) * f32(inv_scale))
    with np.errstate(over="ignore", invalid="ignore"):
        return (g * k).astype(np.float32).astype(np.float64)


def norm64(segments, mult=1.0, inv_scale=None):
    """float64 global L2 norm of the fp32 products over a list of segments"""
    s = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for g in segments:
            x = products(g, mult, inv_scale)
            s += float(np.sum(x * x))
    return float(np.sqrt(s))


def coef64(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient in float64: an Inf norm gives 0, a NaN norm NaN"""
    c = float(f32(max_norm)) / (norm + 1e-6)
    return c if c != c else min(c, 1.0)


def norm_rel_bound(n, partials):
    return (U32 + ((n + partials) / 2.0 + 2.0) * U64) * (1.0 + 2.0 ** -20)


def norm_bound(norm, n, partials):
    return abs(norm) * norm_rel_bound(n, partials)


def coef_bound(coef, n, partials):
    return abs(coef) * (norm_rel_bound(n, partials) + 3.0 * U32) * (1.0 + 2.0 ** -20)
