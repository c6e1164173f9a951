// Gradient clipping by global L2 norm on the device (torch.nn.utils.clip_grad_norm_'s rule) without rewriting a gradient and without the host
// looking at the norm.  Three kernels around one small fp32 state block (layout UCFVIT_GC_* in include/ucfvit_hip.h):
//   grad_sqnorm    one read-only pass over a gradient segment: one partial sum of squares per workgroup, and under a loss scaler the
//                  non-finite check of grad_nonfinite_kernel (grad_scaler.hip) in the same pass;
//   grad_clip_coef one workgroup folds the partials of all segments, writes the norm and the coefficient min(1, max_norm / (norm + 1e-6));
//   adamw_clipped  the AdamW body of adamw_body.h with the coefficient multiplied into the factor it already applies to every gradient.
// The sum is a pure function of the inputs and the segment layout: squares are accumulated in double from the first add, every fold runs in a
// fixed order, and no atomic or cross-workgroup handshake is involved.  Data-parallel ranks therefore get the same coefficient from the same
// all-reduced buffer without a collective.
#include "common.h"
#include "adamw_body.h"

namespace {

#define DTYPE_OK(d) ((d) == UCFVIT_F32 || (d) == UCFVIT_BF16)

constexpr int GC_BLOCK = 256;
constexpr int GC_WAVES = GC_BLOCK / 64;
constexpr int GC_MAX_GRID = 1024;   // grad_nonfinite's shape: 4 workgroups per CU, 4 independent 16-byte loads per thread in flight
constexpr int GC_UNROLL = 4;

// acc += x^2 over one 16-byte vector, x = g * k rounded to fp32 as adamw_update forms it; the square of an fp32 value is exact in double
template <typename G>
__device__ __forceinline__ void vec_sq(const Vec16<G>& a, float k, double& acc) {
#pragma unroll
    for (int e = 0; e < Vec16<G>::N; ++e) {
        const float x = a.get(e) * k;
        acc = fma((double)x, (double)x, acc);
    }
}

// grad_nonfinite's predicate read off the sum: a finite x has x^2 <= 1.2e77, and no int64 count of those reaches DBL_MAX, so a thread's sum is
// Inf or NaN exactly when one of its x was (Inf^2 = Inf, NaN^2 = NaN, and neither leaves a sum again).  The check costs nothing per element.
__device__ __forceinline__ bool non_finite(double s) { return !(fabs(s) <= 1.7976931348623157e+308); }

// the workgroup's sum, the same bits in every run: xor-butterfly inside each wave, then the waves in index order by thread 0
__device__ __forceinline__ double block_sum_fixed(double acc, double* lds) {
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < GC_WAVES; ++w) s += lds[w];
    }
    return s;      // valid in thread 0
}

// partials[blockIdx.x] = sum over this workgroup's elements of (g[i] * k)^2, k = mult (SCALED = false) or mult * state[INV_SCALE];
// SCALED: state[FOUND_INF] = 1 if any g[i] * k is not finite, never cleared here (every writer stores the same 1.0f: no atomic needed)
template <typename G, bool SCALED>
__global__ __launch_bounds__(GC_BLOCK) void grad_sqnorm_kernel(const G* __restrict__ g, int64_t n, float mult, float* __restrict__ state,
                                                               double* __restrict__ partials) {
    __shared__ double lds[GC_WAVES];
    constexpr int EPV = Vec16<G>::N;
    const float k = SCALED ? mult * state[UCFVIT_GS_INV_SCALE] : mult;
    const int64_t nv = n / EPV;
    const int64_t stride = (int64_t)gridDim.x * GC_BLOCK;
    const Vec16<G>* gv = reinterpret_cast<const Vec16<G>*>(g);
    int64_t i = (int64_t)blockIdx.x * GC_BLOCK + threadIdx.x;
    double acc = 0.0;
    for (; i + (GC_UNROLL - 1) * stride < nv; i += GC_UNROLL * stride) {
        Vec16<G> a[GC_UNROLL];
#pragma unroll
        for (int u = 0; u < GC_UNROLL; ++u) a[u] = gv[i + u * stride];
#pragma unroll
        for (int u = 0; u < GC_UNROLL; ++u) vec_sq<G>(a[u], k, acc);
    }
    for (; i < nv; i += stride) vec_sq<G>(gv[i], k, acc);
    // tail (n % EPV)
    const int64_t t = nv * EPV + (int64_t)blockIdx.x * GC_BLOCK + threadIdx.x;
    if (t < n) {
        const float x = to_f32<G>(g[t]) * k;
        acc = fma((double)x, (double)x, acc);
    }
    if (SCALED) {
        const unsigned long long hit = __ballot(non_finite(acc));
        if (hit != 0ull && (threadIdx.x & 63) == 0) state[UCFVIT_GS_FOUND_INF] = 1.0f;
    }
    const double s = block_sum_fixed(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// one workgroup: thread t takes partials t, t + 256, ... in order, then the fixed fold.  Reads exactly `count` partials.
// An Inf sum gives norm Inf and coefficient 0; a NaN sum gives NaN in both (torch's clamp(max=1) keeps a NaN; fminf would not).
__global__ __launch_bounds__(GC_BLOCK) void grad_clip_coef_kernel(const double* __restrict__ partials, int64_t count,
                                                                  float* __restrict__ clip) {
    __shared__ double lds[GC_WAVES];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += GC_BLOCK) acc += partials[i];
    const double s = block_sum_fixed(acc, lds);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        const float c = clip[UCFVIT_GC_MAX_NORM] / (norm + 1e-6f);
        clip[UCFVIT_GC_NORM] = norm;
        clip[UCFVIT_GC_COEF] = c > 1.0f ? 1.0f : c;
    }
}

// AdamW with the clip coefficient in the gradient factor.  SCALED = false: ucfvit_adamw(_ema) with gscale * coef.  SCALED = true:
// ucfvit_adamw_scaled(_ema) with (gscale * inv_scale) * coef, skipped when the check fired, bias corrections from the applied-step count.
template <typename G, bool EMA, bool SCALED>
__global__ void adamw_clipped_kernel(float* __restrict__ p, const G* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                     bf16* __restrict__ shadow, float* __restrict__ ema, int64_t n, float lr, double b1, double b2, float eps,
                                     float wd, float bc1, float bc2_sqrt, float gscale, float rate, const float* __restrict__ state,
                                     const float* __restrict__ clip) {
    if (SCALED) {
        if (state[UCFVIT_GS_FOUND_INF] != 0.f) return;
        const double t = (double)state[UCFVIT_GS_APPLIED_STEPS] + 1.0;
        bc1 = (float)(1.0 - pow(b1, t));                              // as adamw_scaled_kernel: formed in double, rounded once
        bc2_sqrt = sqrtf((float)(1.0 - pow(b2, t)));
        gscale = gscale * state[UCFVIT_GS_INV_SCALE];
    }
    adamw_update<G, EMA>(p, g, m, v, shadow, ema, n, lr, (float)b1, (float)b2, eps, wd, bc1, bc2_sqrt, gscale * clip[UCFVIT_GC_COEF], rate);
}

inline unsigned grid_for(int64_t work_items, int block, int cap) {
    int64_t g = (work_items + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

inline unsigned sqnorm_grid(int64_t n, int dtype) {
    const int epv = dtype == UCFVIT_F32 ? 4 : 8;
    return grid_for((n + epv - 1) / epv, GC_BLOCK, GC_MAX_GRID);
}

template <typename G, bool EMA, bool SCALED>
void launch_adamw_clipped(unsigned grid, hipStream_t s, float* p, const void* g, float* m, float* v, void* shadow, float* ema, int64_t n,
                          float lr, double b1, double b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale, float rate,
                          const float* state, const float* clip) {
    hipLaunchKernelGGL((adamw_clipped_kernel<G, EMA, SCALED>), dim3(grid), dim3(256), 0, s, p, (const G*)g, m, v, (bf16*)shadow, ema, n, lr, b1,
                       b2, eps, wd, bc1, bc2_sqrt, gscale, rate, state, clip);
}

}  // namespace

extern "C" int64_t ucfvit_grad_sqnorm_partials(int64_t n, int dtype) {
    if (n < 0 || !DTYPE_OK(dtype)) {
        ucfvit_set_error("ucfvit_grad_sqnorm_partials: negative size or bad dtype %d", dtype);
        return -1;
    }
    return n == 0 ? 0 : (int64_t)sqnorm_grid(n, dtype);
}

extern "C" int ucfvit_grad_sqnorm(const void* g, int64_t n, int dtype, float mult, float* gs_state, double* partials, void* stream) {
    UCF_CHECK_ARG(n >= 0, "ucfvit_grad_sqnorm: negative size");
    UCF_CHECK_ARG(DTYPE_OK(dtype), "ucfvit_grad_sqnorm: bad dtype %d", dtype);
    UCF_CHECK_ARG((((uintptr_t)gs_state) & 3) == 0, "ucfvit_grad_sqnorm: misaligned state");
    if (n == 0) return UCFVIT_OK;                      // empty segment: no partial is written (g and partials may be NULL)
    UCF_CHECK_ARG(g, "ucfvit_grad_sqnorm: null pointer");
    UCF_CHECK_ARG(partials, "ucfvit_grad_sqnorm: null partials");
    UCF_CHECK_ARG(ucf_is_aligned16(g), "ucfvit_grad_sqnorm: gradients must be 16-byte aligned");
    UCF_CHECK_ARG((((uintptr_t)partials) & 7) == 0, "ucfvit_grad_sqnorm: partials must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = sqnorm_grid(n, dtype);
#define SQNORM(G, SCALED) \
    hipLaunchKernelGGL((grad_sqnorm_kernel<G, SCALED>), dim3(grid), dim3(GC_BLOCK), 0, s, (const G*)g, n, mult, gs_state, partials)
    if (dtype == UCFVIT_F32) {
        if (gs_state) SQNORM(float, true);
        else SQNORM(float, false);
    } else {
        if (gs_state) SQNORM(bf16, true);
        else SQNORM(bf16, false);
    }
#undef SQNORM
    UCF_LAUNCH_CHECK("ucfvit_grad_sqnorm");
    return UCFVIT_OK;
}

extern "C" int ucfvit_grad_clip_coef(const double* partials, int64_t count, float* clip_state, void* stream) {
    UCF_CHECK_ARG(count >= 0, "ucfvit_grad_clip_coef: negative count");
    UCF_CHECK_ARG(clip_state, "ucfvit_grad_clip_coef: null state");
    UCF_CHECK_ARG((((uintptr_t)clip_state) & 3) == 0, "ucfvit_grad_clip_coef: misaligned state");
    UCF_CHECK_ARG(partials || count == 0, "ucfvit_grad_clip_coef: null partials");      // count 0 (no gradient anywhere): norm 0
    UCF_CHECK_ARG((((uintptr_t)partials) & 7) == 0, "ucfvit_grad_clip_coef: partials must be 8-byte aligned");
    hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(GC_BLOCK), 0, (hipStream_t)stream, partials, count, clip_state);
    UCF_LAUNCH_CHECK("ucfvit_grad_clip_coef");
    return UCFVIT_OK;
}

extern "C" int ucfvit_adamw_clipped(float* p, const void* g, float* m, float* v, void* shadow_bf16, float* ema, int64_t n, float lr,
                                    double beta1, double beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2,
                                    float grad_scale, float ema_rate, int grad_dtype, const float* gs_state, const float* clip_state,
                                    void* stream) {
    UCF_CHECK_ARG(p && g && m && v, "ucfvit_adamw_clipped: null pointer");
    UCF_CHECK_ARG(clip_state, "ucfvit_adamw_clipped: null clip state");
    UCF_CHECK_ARG(n >= 0, "ucfvit_adamw_clipped: negative size");
    UCF_CHECK_ARG(DTYPE_OK(grad_dtype), "ucfvit_adamw_clipped: bad grad dtype %d", grad_dtype);
    UCF_CHECK_ARG(!ema || (ema_rate > 0.f && ema_rate <= 1.f), "ucfvit_adamw_clipped: ema_rate %g outside (0, 1]", (double)ema_rate);   // false for NaN
    UCF_CHECK_ARG(ucf_is_aligned16(p) && ucf_is_aligned16(m) && ucf_is_aligned16(v) && ucf_is_aligned16(ema) && (((uintptr_t)g) % 8 == 0) &&
                      (((uintptr_t)shadow_bf16) % 8 == 0) && (((uintptr_t)gs_state) % 4 == 0) && (((uintptr_t)clip_state) % 4 == 0),
                  "ucfvit_adamw_clipped: pointers must be 16-byte aligned (grad/shadow 8, states 4)");
    UCF_CHECK_ARG(grad_dtype != UCFVIT_F32 || ucf_is_aligned16(g), "ucfvit_adamw_clipped: fp32 grads must be 16-byte aligned");
    if (n == 0) return UCFVIT_OK;
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = grid_for((n + 3) / 4, 256, 256 * 8);       // ucfvit_adamw's grid
    const float bc2s = gs_state ? 0.f : sqrtf(bias_corr2);           // under the scaler both corrections are formed on the device
#define CLIPPED(G, EMA, SCALED)                                                                                                        \
    launch_adamw_clipped<G, EMA, SCALED>(grid, s, p, g, m, v, shadow_bf16, ema, n, lr, beta1, beta2, eps, weight_decay, bias_corr1, bc2s, \
                                         grad_scale, ema_rate, gs_state, clip_state)
#define CLIPPED_G(G)                         \
    do {                                     \
        if (ema && gs_state) CLIPPED(G, true, true);       \
        else if (ema) CLIPPED(G, true, false);             \
        else if (gs_state) CLIPPED(G, false, true);        \
        else CLIPPED(G, false, false);                     \
    } while (0)
    if (grad_dtype == UCFVIT_F32) CLIPPED_G(float);
    else CLIPPED_G(bf16);
#undef CLIPPED_G
#undef CLIPPED
    UCF_LAUNCH_CHECK("ucfvit_adamw_clipped");
    return UCFVIT_OK;
}
