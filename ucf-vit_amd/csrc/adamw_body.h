// The AdamW update of one flat segment (torch.optim.AdamW update order) + optional bf16 shadow write: the one body behind
// adamw_kernel (elementwise.hip: bias corrections from the host) and adamw_scaled_kernel (grad_scaler.hip: bias corrections
// and gradient multiplier from the loss scaler's device state).
// EMA = true (ucfvit_adamw_ema / ucfvit_adamw_scaled_ema): the same pass also moves an exponential moving average of the weights towards the
// value just stored to p, ema += rate * (p_new - ema) with rate = 1 - decay; with EMA = false neither `ema` nor `rate` is read and the
// instantiation is the one the entry points without an average have always launched.
#pragma once
#include "common.h"

template <typename G, bool EMA>
__device__ __forceinline__ void adamw_update(float* __restrict__ p, const G* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, bf16* __restrict__ shadow, float* __restrict__ ema, int64_t n, float lr,
                                             float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale, float rate) {
    const int64_t nv = n >> 2;
    const float step_size = lr / bc1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
        f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
        f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
        const Vec4<G> gv = reinterpret_cast<const Vec4<G>*>(g)[i];
        f32x4 av;
        if (EMA) av = reinterpret_cast<f32x4*>(ema)[i];
        bf16x4 sh;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gr = gv.get(e) * gscale;
            float pe = pv[e] * (1.f - lr * wd);
            const float me = b1 * mv[e] + (1.f - b1) * gr;
            const float ve = b2 * vv[e] + (1.f - b2) * gr * gr;
            const float denom = sqrtf(ve) / bc2_sqrt + eps;
            pe -= step_size * (me / denom);
            pv[e] = pe;
            mv[e] = me;
            vv[e] = ve;
            sh[e] = (bf16)pe;
            if (EMA) av[e] = av[e] + rate * (pe - av[e]);
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
        reinterpret_cast<f32x4*>(m)[i] = mv;
        reinterpret_cast<f32x4*>(v)[i] = vv;
        if (shadow) reinterpret_cast<bf16x4*>(shadow)[i] = sh;
        if (EMA) reinterpret_cast<f32x4*>(ema)[i] = av;
    }
    // tail (n % 4)
    const int64_t t = (nv << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) {
        const float gr = to_f32<G>(g[t]) * gscale;
        float pe = p[t] * (1.f - lr * wd);
        const float me = b1 * m[t] + (1.f - b1) * gr;
        const float ve = b2 * v[t] + (1.f - b2) * gr * gr;
        pe -= step_size * (me / (sqrtf(ve) / bc2_sqrt + eps));
        p[t] = pe;
        m[t] = me;
        v[t] = ve;
        if (shadow) shadow[t] = (bf16)pe;
        if (EMA) ema[t] = ema[t] + rate * (pe - ema[t]);
    }
}
