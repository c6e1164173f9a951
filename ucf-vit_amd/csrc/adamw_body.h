// The AdamW update of one flat segment (torch.optim.AdamW update order) + optional bf16 shadow write: the one body behind
// adamw_kernel (elementwise.hip: bias corrections from the host) and adamw_scaled_kernel (grad_scaler.hip: bias corrections
// and gradient multiplier from the loss scaler's device state).
#pragma once
#include "common.h"

template <typename G>
__device__ __forceinline__ void adamw_update(float* __restrict__ p, const G* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, bf16* __restrict__ shadow, int64_t n, float lr, float b1, float b2,
                                             float eps, float wd, float bc1, float bc2_sqrt, float gscale) {
    const int64_t nv = n >> 2;
    const float step_size = lr / bc1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
        f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
        f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
        const Vec4<G> gv = reinterpret_cast<const Vec4<G>*>(g)[i];
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
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
        reinterpret_cast<f32x4*>(m)[i] = mv;
        reinterpret_cast<f32x4*>(v)[i] = vv;
        if (shadow) reinterpret_cast<bf16x4*>(shadow)[i] = sh;
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
    }
}
