"""numpy restatements for tests/test_ema_*.py and tests/test_ddim_*.py, written from the header's contracts (include/ucfvit_hip.h) and the
DDIM paper's formulas, not from the kernels: the strided schedule, the step coefficients in float64, the generalised reverse step in float64
and as an fp32 restatement in the kernel's stated operation order, and the weights' moving average in float64 with its roundoff bound."""
import numpy as np

import diffusion_ref as DRF

U = 2.0 ** -24                      # fp32 unit roundoff
F = np.float32


# ------------------------------------------------------------------------------------------------ schedule and coefficients
def ddim_timesteps(T, S):
    if S == 1:
        return [T - 1]
    return [(k * (T - 1) + (S - 1) // 2) // (S - 1) for k in range(S)]


def pairs(T, S):
    """(i, i_prev) in the order a sampler walks them; i_prev = -1 on the last step"""
    tau = ddim_timesteps(T, S)
    return [(tau[k], tau[k - 1] if k else -1) for k in range(len(tau) - 1, -1, -1)]


def ddim_coefficients64(alpha, i, i_prev, eta):
    """alpha: the fp32 table abar as float64.  -> dict of float64 values"""
    ab = float(alpha[i])
    abp = float(alpha[i_prev]) if i_prev >= 0 else 1.0
    sigma = eta * np.sqrt((1.0 - abp) / (1.0 - ab)) * np.sqrt(1.0 - ab / abp)
    return dict(s_ab=np.sqrt(ab), s_1mab=np.sqrt(1.0 - ab), r_ab=1.0 / np.sqrt(ab), r_1mab=1.0 / np.sqrt(1.0 - ab), c_x0=np.sqrt(abp),
                c_eps=np.sqrt(max(1.0 - abp - sigma * sigma, 0.0)), sigma=sigma, ab=ab, ab_prev=abp)


ORDER = ("s_ab", "s_1mab", "r_ab", "r_1mab", "c_x0", "c_eps", "sigma")


def coef32(alpha, i, i_prev, eta):
    """the seven values the kernel receives: float64 formulas rounded once to fp32"""
    c = ddim_coefficients64(alpha, i, i_prev, eta)
    return tuple(float(F(c[k])) for k in ORDER)


# ------------------------------------------------------------------------------------------------ the step
def ddim_step32(x, e, z, coef, clip):
    """the step in fp32, one rounding per product and sum, in the order the header states.  x, e (already in the image layout), z fp32 arrays;
    coef the seven fp32 values; clip 0 / None: no clamp.  -> (out fp32, clamped mask)"""
    s_ab, s_1mab, r_ab, r_1mab, c_x0, c_eps, sigma = (F(v) for v in coef)
    x, e = x.astype(F), e.astype(F)
    with np.errstate(invalid="ignore"):
        x0 = (x - s_1mab * e) * r_ab
        hit = np.zeros(x.shape, dtype=bool)
        if clip:
            c = F(clip)
            hit = (x0 < -c) | (x0 > c)
            x0 = np.where(x0 < -c, -c, np.where(x0 > c, c, x0)).astype(F)
            e = (x - s_ab * x0) * r_1mab
        o = c_x0 * x0 + c_eps * e
        if z is not None:
            o = o + sigma * z.astype(F)
    assert o.dtype == F
    return o, hit


def ddim_step64(x, e, z, coef, clip):
    """float64 result of the same formulas with the fp32 coefficients, and a first-order roundoff bound for the fp32 evaluation.
    Rounding count, every operation of the fp32 chain adding a relative u of its own result and passing on what its inputs carry:
      a = s_1mab e (1), d = x - a (1), x0 = d r_ab (1): |err x0| <= u r_ab (3 |x| + 3 |a|)   [each term passes at most 3 roundings]
      clamped: x0 is exactly +-clip where the clamp acts, otherwise carries err x0 (a value within err x0 of the bound may fall on either
        side: both results are then within err x0 of each other, so the same bound holds);
        b = s_ab x0 (1), f = x - b (1), e' = f r_1mab (1): |err e'| <= r_1mab (s_ab err x0 (1 + 3u) + 3u (|x| + |b|))
      o = c_x0 x0 (1) + c_eps e' (1), sum (1): <= c_x0 (err x0 + 2u |x0|) + c_eps (err e' + 2u |e'|)
      + sigma z (1) and the last sum (1): every earlier term passes one more rounding, sigma z two.
    The bound below charges one u more per term than counted (4, 4, 3 instead of 3, 3, 2) to cover the second-order terms."""
    s_ab, s_1mab, r_ab, r_1mab, c_x0, c_eps, sigma = (float(F(v)) for v in coef)
    x, e = x.astype(np.float64), e.astype(np.float64)
    a = s_1mab * e
    x0 = (x - a) * r_ab
    err_x0 = 4 * U * abs(r_ab) * (np.abs(x) + np.abs(a))
    ee, err_e = e, np.zeros_like(x)
    if clip:
        x0 = np.clip(x0, -clip, clip)
        b = s_ab * x0
        ee = (x - b) * r_1mab
        err_e = abs(r_1mab) * (abs(s_ab) * err_x0 * (1 + 4 * U) + 4 * U * (np.abs(x) + np.abs(b)))
    o = c_x0 * x0 + c_eps * ee
    bound = abs(c_x0) * (err_x0 + 3 * U * np.abs(x0)) + abs(c_eps) * (err_e + 3 * U * np.abs(ee))
    if z is not None:
        n = sigma * z.astype(np.float64)
        o = o + n
        bound = bound * (1 + 2 * U) + U * (np.abs(c_x0 * x0) + np.abs(c_eps * ee)) + 3 * U * np.abs(n)
    return o, bound


def unpatchify(pred, C, dims, p):
    return DRF.unpatchify(pred, C, dims, p)


def patchify(img, p):
    """the inverse of unpatchify for [B, C, *dims]: -> [B, L, p^nd C]"""
    B, C = img.shape[:2]
    dims = img.shape[2:]
    if len(dims) == 2:
        h, w = dims[0] // p, dims[1] // p
        return np.einsum("nchpwq->nhwpqc", img.reshape(B, C, h, p, w, p)).reshape(B, h * w, p * p * C)
    h, w, d = dims[0] // p, dims[1] // p, dims[2] // p
    return np.einsum("nchpwqdr->nhwdpqrc", img.reshape(B, C, h, p, w, p, d, p)).reshape(B, h * w * d, p ** 3 * C)


def point_mass_sampler32(alpha, c, x_T, S, eta, clip, noise):
    """the whole sampler on the fp32 restatement with the oracle of a point mass at c: eps_hat = (x - sqrt(abar) c) / sqrt(1 - abar), formed in
    float64 from the fp32 x and rounded once.  noise(k) -> fp32 array of step k.  -> x_0 fp32"""
    x = x_T.astype(F)
    T = len(alpha)
    for k, (i, ip) in enumerate(pairs(T, S)):
        ab = float(alpha[i])
        e = ((x.astype(np.float64) - np.sqrt(ab) * c.astype(np.float64)) / np.sqrt(1.0 - ab)).astype(F)
        coef = coef32(alpha, i, ip, eta)
        x, _ = ddim_step32(x, e, noise(k) if coef[6] != 0.0 else None, coef, clip)
    return x


# ------------------------------------------------------------------------------------------------ the moving average
def ema64(e, p_new, rate):
    """e + r (p_new - e) in float64; rate: the fp32 value the kernel receives"""
    r = float(F(rate))
    e, p_new = e.astype(np.float64), p_new.astype(np.float64)
    return e + r * (p_new - e)


def ema_bound(e, p_new, rate):
    """|fp32 result - ema64| <= u (2 r |p_new - e| + |e'|) (1 + 2u) for fp32 inputs e, p_new: the difference d = fl(p_new - e) carries u |d|,
    the product fl(r d) that and u of its own, the sum u |e'| (to first order; the factor 1 + 2u covers the products of two roundings).
    A fused multiply-add skips the product's rounding and stays inside.  Where p_new == e the difference is an exact 0 and the result is e."""
    r = float(F(rate))
    e64 = ema64(e, p_new, rate)
    return U * (2 * r * np.abs(p_new.astype(np.float64) - e.astype(np.float64)) + np.abs(e64)) * (1 + 2 * U)


def ema_trajectory64(ps, rate):
    """ps: the parameter after 0, 1, .. K steps (fp32 arrays).  -> (float64 average after K steps, bound on an fp32 evaluation's distance
    from it): per step the bound of ema_bound at the float64 average, widened by what the previous steps left: an input error b enters
    e' as (1 - r) b, and |p - e| is known only to b."""
    r = float(F(rate))
    e = ps[0].astype(np.float64)
    b = np.zeros_like(e)
    for p in ps[1:]:
        p = p.astype(np.float64)
        e_new = e + r * (p - e)
        b = (1 - r) * b + U * (2 * r * (np.abs(p - e) + b) + np.abs(e_new) + b) * (1 + 2 * U)
        e = e_new
    return e, b
