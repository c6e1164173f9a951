// Dynamic loss scaling on the device (the reference's bf16 policy: ShardedGradScaler(init_scale=8192, growth_interval=100) and the floor
// of 128, training_scripts/train_masked_fsdp.py:417-419,601-606).  Three kernels around one small fp32 state block (layout UCFVIT_GS_* in
// include/ucfvit_hip.h): a read-only non-finite check of the gradients, AdamW that skips itself when the check fired, and the scale
// update.  Nothing here needs the host to look at the flag, so a training step stays free of synchronisation.
#include "common.h"
#include "adamw_body.h"

namespace {

#define DTYPE_OK(d) ((d) == UCFVIT_F32 || (d) == UCFVIT_BF16)

constexpr int NF_BLOCK = 256;
constexpr int NF_MAX_GRID = 1024;   // 4 workgroups per CU, each thread with 4 independent 16-byte loads in flight (16 MiB in all)
constexpr int NF_UNROLL = 4;

// |x| <= FLT_MAX is false exactly for +-Inf and NaN
__device__ __forceinline__ bool non_finite(float x) { return !(fabsf(x) <= 3.402823466e+38f); }

template <typename G>
__device__ __forceinline__ bool vec_non_finite(const Vec16<G>& a, float k) {
    bool bad = false;
#pragma unroll
    for (int e = 0; e < Vec16<G>::N; ++e) bad |= non_finite(a.get(e) * k);
    return bad;
}

// state[FOUND_INF] = 1 if any g[i] * mult * inv_scale is not finite (the value adamw_scaled_kernel consumes); never cleared here.
// Every writer stores the same 1.0f, so plain stores from different waves need no atomic.
template <typename G>
__global__ __launch_bounds__(NF_BLOCK) void grad_nonfinite_kernel(const G* __restrict__ g, int64_t n, float mult,
                                                                  float* __restrict__ state) {
    constexpr int EPV = Vec16<G>::N;
    const float k = mult * state[UCFVIT_GS_INV_SCALE];
    const int64_t nv = n / EPV;
    const int64_t stride = (int64_t)gridDim.x * NF_BLOCK;
    const Vec16<G>* gv = reinterpret_cast<const Vec16<G>*>(g);
    int64_t i = (int64_t)blockIdx.x * NF_BLOCK + threadIdx.x;
    bool bad = false;
    for (; i + (NF_UNROLL - 1) * stride < nv; i += NF_UNROLL * stride) {
        Vec16<G> a[NF_UNROLL];
#pragma unroll
        for (int u = 0; u < NF_UNROLL; ++u) a[u] = gv[i + u * stride];
#pragma unroll
        for (int u = 0; u < NF_UNROLL; ++u) bad |= vec_non_finite<G>(a[u], k);
    }
    for (; i < nv; i += stride) bad |= vec_non_finite<G>(gv[i], k);
    // tail (n % EPV)
    const int64_t t = nv * EPV + (int64_t)blockIdx.x * NF_BLOCK + threadIdx.x;
    if (t < n) bad |= non_finite(to_f32<G>(g[t]) * k);
    const unsigned long long hit = __ballot(bad);
    if (hit != 0ull && (threadIdx.x & 63) == 0) state[UCFVIT_GS_FOUND_INF] = 1.0f;
}

// AdamW with the loss scaler's state: nothing is touched when the check fired; otherwise gradients are multiplied by
// gscale * inv_scale and the bias corrections come from the number of APPLIED steps, which a skipped step does not advance.
template <typename G>
__global__ void adamw_scaled_kernel(float* __restrict__ p, const G* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                    bf16* __restrict__ shadow, int64_t n, float lr, double b1, double b2, float eps, float wd,
                                    float gscale, const float* __restrict__ state) {
    if (state[UCFVIT_GS_FOUND_INF] != 0.f) return;
    const double t = (double)state[UCFVIT_GS_APPLIED_STEPS] + 1.0;
    const float bc1 = (float)(1.0 - pow(b1, t));                      // formed in double, rounded once: as ops.adamw does on the host
    const float bc2 = (float)(1.0 - pow(b2, t));
    adamw_update<G, false>(p, g, m, v, shadow, nullptr, n, lr, (float)b1, (float)b2, eps, wd, bc1, sqrtf(bc2),
                           gscale * state[UCFVIT_GS_INV_SCALE], 0.f);
}

// the same with the weights' exponential moving average, which a skipped step leaves alone as it leaves p, m, v and the shadow
template <typename G>
__global__ void adamw_scaled_ema_kernel(float* __restrict__ p, const G* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                        bf16* __restrict__ shadow, float* __restrict__ ema, int64_t n, float lr, double b1, double b2,
                                        float eps, float wd, float gscale, float rate, const float* __restrict__ state) {
    if (state[UCFVIT_GS_FOUND_INF] != 0.f) return;
    const double t = (double)state[UCFVIT_GS_APPLIED_STEPS] + 1.0;
    const float bc1 = (float)(1.0 - pow(b1, t));
    const float bc2 = (float)(1.0 - pow(b2, t));
    adamw_update<G, true>(p, g, m, v, shadow, ema, n, lr, (float)b1, (float)b2, eps, wd, bc1, sqrtf(bc2),
                          gscale * state[UCFVIT_GS_INV_SCALE], rate);
}

// torch's _amp_update_scale_ + the reference's floor; one thread
__global__ void grad_scaler_update_kernel(float* __restrict__ state) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float scale = state[UCFVIT_GS_SCALE];
    if (state[UCFVIT_GS_FOUND_INF] != 0.f) {
        scale *= state[UCFVIT_GS_BACKOFF_FACTOR];
        state[UCFVIT_GS_GROWTH_TRACKER] = 0.f;
        state[UCFVIT_GS_SKIPPED_STEPS] += 1.f;
    } else {
        state[UCFVIT_GS_APPLIED_STEPS] += 1.f;
        const float successful = state[UCFVIT_GS_GROWTH_TRACKER] + 1.f;
        if (successful == state[UCFVIT_GS_GROWTH_INTERVAL]) {
            const float grown = scale * state[UCFVIT_GS_GROWTH_FACTOR];
            if (!non_finite(grown)) scale = grown;
            state[UCFVIT_GS_GROWTH_TRACKER] = 0.f;
        } else {
            state[UCFVIT_GS_GROWTH_TRACKER] = successful;
        }
    }
    scale = fmaxf(scale, state[UCFVIT_GS_MIN_SCALE]);
    state[UCFVIT_GS_SCALE] = scale;
    state[UCFVIT_GS_INV_SCALE] = (float)(1.0 / (double)scale);
    state[UCFVIT_GS_FOUND_INF] = 0.f;
}

inline unsigned grid_for(int64_t work_items, int block, int cap) {
    int64_t g = (work_items + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

}  // namespace

extern "C" int ucfvit_grad_nonfinite(const void* g, int64_t n, int dtype, float mult, float* state, void* stream) {
    UCF_CHECK_ARG(n >= 0, "ucfvit_grad_nonfinite: negative size");
    UCF_CHECK_ARG(DTYPE_OK(dtype), "ucfvit_grad_nonfinite: bad dtype %d", dtype);
    UCF_CHECK_ARG(state, "ucfvit_grad_nonfinite: null state");
    UCF_CHECK_ARG((((uintptr_t)state) & 3) == 0, "ucfvit_grad_nonfinite: misaligned state");
    if (n == 0) return UCFVIT_OK;                      // empty segment (g may be NULL)
    UCF_CHECK_ARG(g, "ucfvit_grad_nonfinite: null pointer");
    UCF_CHECK_ARG(ucf_is_aligned16(g), "ucfvit_grad_nonfinite: gradients must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == UCFVIT_F32) {
        const unsigned grid = grid_for((n + 3) / 4, NF_BLOCK, NF_MAX_GRID);
        hipLaunchKernelGGL(grad_nonfinite_kernel<float>, dim3(grid), dim3(NF_BLOCK), 0, s, (const float*)g, n, mult, state);
    } else {
        const unsigned grid = grid_for((n + 7) / 8, NF_BLOCK, NF_MAX_GRID);
        hipLaunchKernelGGL(grad_nonfinite_kernel<bf16>, dim3(grid), dim3(NF_BLOCK), 0, s, (const bf16*)g, n, mult, state);
    }
    UCF_LAUNCH_CHECK("ucfvit_grad_nonfinite");
    return UCFVIT_OK;
}

extern "C" int ucfvit_adamw_scaled(float* p, const void* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr, double beta1,
                                   double beta2, float eps, float weight_decay, float grad_scale, int grad_dtype, const float* state,
                                   void* stream) {
    UCF_CHECK_ARG(p && g && m && v, "ucfvit_adamw_scaled: null pointer");
    UCF_CHECK_ARG(state, "ucfvit_adamw_scaled: null state");
    UCF_CHECK_ARG(n >= 0, "ucfvit_adamw_scaled: negative size");
    UCF_CHECK_ARG(DTYPE_OK(grad_dtype), "ucfvit_adamw_scaled: bad grad dtype %d", grad_dtype);
    UCF_CHECK_ARG(ucf_is_aligned16(p) && ucf_is_aligned16(m) && ucf_is_aligned16(v) && (((uintptr_t)g) % 8 == 0) &&
                      (((uintptr_t)shadow_bf16) % 8 == 0) && (((uintptr_t)state) % 4 == 0),
                  "ucfvit_adamw_scaled: pointers must be 16-byte aligned (grad/shadow 8, state 4)");
    if (n == 0) return UCFVIT_OK;
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = grid_for((n + 3) / 4, 256, 256 * 8);       // ucfvit_adamw's grid
    if (grad_dtype == UCFVIT_F32) {
        UCF_CHECK_ARG(ucf_is_aligned16(g), "ucfvit_adamw_scaled: fp32 grads must be 16-byte aligned");
        hipLaunchKernelGGL(adamw_scaled_kernel<float>, dim3(grid), dim3(256), 0, s, p, (const float*)g, m, v, (bf16*)shadow_bf16, n, lr,
                           beta1, beta2, eps, weight_decay, grad_scale, state);
    } else {
        hipLaunchKernelGGL(adamw_scaled_kernel<bf16>, dim3(grid), dim3(256), 0, s, p, (const bf16*)g, m, v, (bf16*)shadow_bf16, n, lr,
                           beta1, beta2, eps, weight_decay, grad_scale, state);
    }
    UCF_LAUNCH_CHECK("ucfvit_adamw_scaled");
    return UCFVIT_OK;
}

extern "C" int ucfvit_adamw_scaled_ema(float* p, const void* g, float* m, float* v, void* shadow_bf16, float* ema, int64_t n, float lr,
                                       double beta1, double beta2, float eps, float weight_decay, float grad_scale, float ema_rate,
                                       int grad_dtype, const float* state, void* stream) {
    UCF_CHECK_ARG(p && g && m && v && ema, "ucfvit_adamw_scaled_ema: null pointer");
    UCF_CHECK_ARG(state, "ucfvit_adamw_scaled_ema: null state");
    UCF_CHECK_ARG(n >= 0, "ucfvit_adamw_scaled_ema: negative size");
    UCF_CHECK_ARG(DTYPE_OK(grad_dtype), "ucfvit_adamw_scaled_ema: bad grad dtype %d", grad_dtype);
    UCF_CHECK_ARG(ema_rate > 0.f && ema_rate <= 1.f, "ucfvit_adamw_scaled_ema: ema_rate %g outside (0, 1]", (double)ema_rate);   // false for NaN
    UCF_CHECK_ARG(ucf_is_aligned16(p) && ucf_is_aligned16(m) && ucf_is_aligned16(v) && ucf_is_aligned16(ema) && (((uintptr_t)g) % 8 == 0) &&
                      (((uintptr_t)shadow_bf16) % 8 == 0) && (((uintptr_t)state) % 4 == 0),
                  "ucfvit_adamw_scaled_ema: pointers must be 16-byte aligned (grad/shadow 8, state 4)");
    if (n == 0) return UCFVIT_OK;
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = grid_for((n + 3) / 4, 256, 256 * 8);       // ucfvit_adamw's grid
    if (grad_dtype == UCFVIT_F32) {
        UCF_CHECK_ARG(ucf_is_aligned16(g), "ucfvit_adamw_scaled_ema: fp32 grads must be 16-byte aligned");
        hipLaunchKernelGGL(adamw_scaled_ema_kernel<float>, dim3(grid), dim3(256), 0, s, p, (const float*)g, m, v, (bf16*)shadow_bf16, ema, n,
                           lr, beta1, beta2, eps, weight_decay, grad_scale, ema_rate, state);
    } else {
        hipLaunchKernelGGL(adamw_scaled_ema_kernel<bf16>, dim3(grid), dim3(256), 0, s, p, (const bf16*)g, m, v, (bf16*)shadow_bf16, ema, n,
                           lr, beta1, beta2, eps, weight_decay, grad_scale, ema_rate, state);
    }
    UCF_LAUNCH_CHECK("ucfvit_adamw_scaled_ema");
    return UCFVIT_OK;
}

extern "C" int ucfvit_grad_scaler_update(float* state, void* stream) {
    UCF_CHECK_ARG(state, "ucfvit_grad_scaler_update: null state");
    UCF_CHECK_ARG((((uintptr_t)state) & 3) == 0, "ucfvit_grad_scaler_update: misaligned state");
    hipLaunchKernelGGL(grad_scaler_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state);
    UCF_LAUNCH_CHECK("ucfvit_grad_scaler_update");
    return UCFVIT_OK;
}
