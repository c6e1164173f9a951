// The streaming passes of DDPM training and sampling around the DiffusionVIT (reference: train_diffusion_simple.py, ddpm/ddpm.py):
//   ucfvit_ddpm_q_sample      forward noising            out[b][i] = sqrt_ab[t[b]] x0[b][i] + sqrt_1mab[t[b]] eps[b][i]
//   ucfvit_relu_dropout[_bwd] hidden layer of the time MLP   y = f m max(x, 0),   dx = f m [x > 0] dy    (mask of csrc/dropout_mask.h)
//   ucfvit_ddpm_step          one ancestral reverse step     out = c1 (x - c2 eps_hat) + sigma z, eps_hat read in the patch layout of pred
//   ucfvit_ddim_step          one generalised reverse step   out = c_x0 x0_hat + c_eps eps_hat + sigma z, x0_hat optionally clamped
// (the token assembly with the time row, ucfvit_time_tokens_fwd / _bwd, lives with the token kernels in csrc/elementwise.hip).
// All are bound by memory: fp32 arithmetic, one rounding to the output type, 16-byte accesses where sizes and pointers allow and an element
// path with the same results otherwise, no atomics.  The file is compiled without fma contraction (Makefile): every product and sum below
// is rounded on its own, in the order written, so the vector and the element path cannot differ.
#include "common.h"
#include "row_pass.h"
#include "dropout_mask.h"
#include "patch_geom.h"

namespace {

#define DTYPE_OK(d) ((d) == UCFVIT_F32 || (d) == UCFVIT_BF16)

constexpr int DF_BLOCK = 256;

inline unsigned df_grid(int64_t work_items) {
    int64_t g = (work_items + DF_BLOCK - 1) / DF_BLOCK;
    if (g > 256 * 8) g = 256 * 8;  // ~8 workgroups per CU, grid-stride the rest
    if (g < 1) g = 1;
    return (unsigned)g;
}

// ---------------------------------------------------------------------------------------------------
// q_sample.  W = 4: n % 4 == 0 and 16-byte aligned pointers, so a pack never straddles two samples.  t is clamped into [0, T-1]: the
// kernel cannot refuse a step it only sees on the device, and must not read outside the tables.
// out may be x0 (or eps): a lane reads its elements before it writes them and no other lane touches them.
// ---------------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(DF_BLOCK) void q_sample_kernel(const float* x0, const float* eps, const int64_t* __restrict__ t,
                                                            const float* __restrict__ sqrt_ab, const float* __restrict__ sqrt_1mab,
                                                            float* out, int64_t B, int64_t n, int T) {
    const int64_t npk = n / W, total = B * npk;
    for (int64_t i = (int64_t)blockIdx.x * DF_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * DF_BLOCK) {
        const int64_t b = i / npk;
        int64_t tb = t[b];
        tb = tb < 0 ? 0 : tb > T - 1 ? T - 1 : tb;
        const float a = sqrt_ab[tb], s = sqrt_1mab[tb];
        const Pack<float, W> x = Pack<float, W>::load(x0 + i * W), e = Pack<float, W>::load(eps + i * W);
        Pack<float, W> o;
#pragma unroll
        for (int k = 0; k < W; ++k) o.set(k, a * x.get(k) + s * e.get(k));
        o.store(out + i * W);
    }
}

// ---------------------------------------------------------------------------------------------------
// ReLU + dropout.  With row_step = 1 the mask index (r * row_step) * D + c of element (r, c) is the flat index, so the pass is flat; a pack
// of the vector path starts at a multiple of W (D % W == 0).  MASK = false (p == 0, eval): plain ReLU, no Philox code.
// BWD: out = f m [x > 0] dy, the mask recomputed.  A dropped element and x <= 0 are selects: NaN / Inf there do not pass.  x = NaN is not
// > 0 and gives 0 in both directions.  out may be x (forward) or dy (backward).
// ---------------------------------------------------------------------------------------------------
template <typename T, int W, bool MASK, bool BWD>
__global__ __launch_bounds__(DF_BLOCK) void relu_dropout_kernel(const T* x, const T* dy, T* out, int64_t n, DoParams P) {
    const int64_t npk = n / W;
    for (int64_t i = (int64_t)blockIdx.x * DF_BLOCK + threadIdx.x; i < npk; i += (int64_t)gridDim.x * DF_BLOCK) {
        const Pack<T, W> a = Pack<T, W>::load(x + i * W);
        Pack<T, W> g, o;
        if (BWD) g = Pack<T, W>::load(dy + i * W);
        const uint32_t keep = MASK ? keep_bits<W>(i * W, P) : ~0u;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float xv = a.get(k);
            const float v = BWD ? g.get(k) : xv;
            const bool on = xv > 0.f && ((keep >> k) & 1u);
            o.set(k, on ? (MASK ? P.inv_keep * v : v) : 0.f);
        }
        o.store(out + i * W);
    }
}

template <typename T, bool BWD>
int rd_launch(const void* x, const void* dy, void* out, int64_t rows, int64_t D, bool mask, const DoParams& P, hipStream_t st,
              const char* name) {
    constexpr int EPV = Vec16<T>::N;
    const int64_t n = rows * D;
    const bool vec = D % EPV == 0 && ucf_is_aligned16(x) && ucf_is_aligned16(out) && (!BWD || ucf_is_aligned16(dy));
#define RD_GO(W, M)                                                                                                                  \
    hipLaunchKernelGGL((relu_dropout_kernel<T, W, M, BWD>), dim3(df_grid(n / W)), dim3(DF_BLOCK), 0, st, (const T*)x, (const T*)dy, \
                       (T*)out, n, P)
    if (vec) {
        if (mask) RD_GO(EPV, true); else RD_GO(EPV, false);
    } else {
        if (mask) RD_GO(1, true); else RD_GO(1, false);
    }
#undef RD_GO
    UCF_LAUNCH_CHECK(name);
    return UCFVIT_OK;
}

int rd_check(const char* name, int64_t rows, int64_t D, double p, uint64_t seed, int dtype, DoParams* P) {
    UCF_CHECK_ARG(D > 0 && D < (1ll << 30), "%s: bad row width D=%lld", name, (long long)D);
    UCF_CHECK_ARG(rows >= 0 && rows < (1ll << 30), "%s: bad row count %lld", name, (long long)rows);
    const int rc = do_mask_check(name, rows, 1, p, seed, true, P);
    if (rc != UCFVIT_OK) return rc;
    UCF_CHECK_ARG(DTYPE_OK(dtype), "%s: bad dtype %d", name, dtype);
    return UCFVIT_OK;
}

// ---------------------------------------------------------------------------------------------------
// reverse step: one work item per element of pred (coalesced reads of the prediction; the image accesses are the scatter that
// patch_pixel_index defines, every pixel exactly once, so out may be x).  HAS_Z = false: step 0, no noise is read.
// ---------------------------------------------------------------------------------------------------
template <typename T, bool HAS_Z>
__global__ __launch_bounds__(DF_BLOCK) void ddpm_step_kernel(const float* x, const T* __restrict__ pred, const float* __restrict__ z,
                                                             float* out, PatchGeom g, int64_t B, float c1, float c2, float sigma) {
    const int64_t total = B * g.L * g.P;
    for (int64_t i = (int64_t)blockIdx.x * DF_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * DF_BLOCK) {
        const int e = i % g.P;
        const int64_t bl = i / g.P;
        const int l = bl % g.L;
        const int64_t b = bl / g.L;
        const int64_t q = patch_pixel_index(g, b, l, e);
        const float m = c1 * (x[q] - c2 * to_f32<T>(pred[i]));
        out[q] = HAS_Z ? m + sigma * z[q] : m;
    }
}

// ---------------------------------------------------------------------------------------------------
// generalised reverse step (DDIM, and DDPM through its x0 form): the predicted x0 from eps_hat, optionally clamped to [-clip, clip] with
// eps_hat then re-derived from the clamped x0, and out = c_x0 x0 + c_eps eps_hat (+ sigma z).  Same work split and scatter as
// ddpm_step_kernel, so out may be x.  The clamp is two selects: a NaN x0 fails both comparisons and stays a NaN.
// ---------------------------------------------------------------------------------------------------
struct DdimCoef {
    float s_ab, s_1mab, r_ab, r_1mab, c_x0, c_eps, sigma, clip;
};

template <typename T, bool HAS_Z, bool CLIP>
__global__ __launch_bounds__(DF_BLOCK) void ddim_step_kernel(const float* x, const T* __restrict__ pred, const float* __restrict__ z,
                                                             float* out, PatchGeom g, int64_t B, DdimCoef k) {
    const int64_t total = B * g.L * g.P;
    for (int64_t i = (int64_t)blockIdx.x * DF_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * DF_BLOCK) {
        const int e = i % g.P;
        const int64_t bl = i / g.P;
        const int l = bl % g.L;
        const int64_t b = bl / g.L;
        const int64_t q = patch_pixel_index(g, b, l, e);
        const float xv = x[q];
        float eh = to_f32<T>(pred[i]);
        float x0 = (xv - k.s_1mab * eh) * k.r_ab;
        if (CLIP) {
            x0 = x0 < -k.clip ? -k.clip : (x0 > k.clip ? k.clip : x0);
            eh = (xv - k.s_ab * x0) * k.r_1mab;
        }
        const float o = k.c_x0 * x0 + k.c_eps * eh;
        out[q] = HAS_Z ? o + k.sigma * z[q] : o;
    }
}

// the checks ucfvit_ddpm_step and ucfvit_ddim_step share; *pg is filled when B > 0
int step_check(const char* name, const float* x, const void* pred, const float* z, float* out, int64_t B, int64_t C, const int64_t* dims,
               int nd, int64_t p, float sigma, int dtype, PatchGeom* pg) {
    UCF_CHECK_ARG(x && pred && out && dims, "%s: null pointer", name);
    UCF_CHECK_ARG(nd == 2 || nd == 3, "%s: nd must be 2 or 3", name);
    UCF_CHECK_ARG(DTYPE_OK(dtype), "%s: bad dtype %d", name, dtype);
    UCF_CHECK_ARG(B >= 0 && C > 0 && p > 0 && B < (1ll << 31) && C < (1ll << 16) && p < (1ll << 16), "%s: bad sizes", name);
    int64_t pixels = 1;
    for (int i = 0; i < nd; ++i) {
        UCF_CHECK_ARG(dims[i] > 0 && dims[i] < (1ll << 31) && dims[i] % p == 0, "%s: image dim %d (%lld) not a multiple of p=%lld", name, i,
                      (long long)dims[i], (long long)p);
        pixels *= dims[i];
        UCF_CHECK_ARG(pixels * C < (1ll << 31), "%s: a sample has 2^31 elements or more", name);   // L, P and the products inside
    }                                                                                                // patch_pixel_index are ints
    UCF_CHECK_ARG(z || sigma == 0.f, "%s: sigma=%g without noise (z == NULL needs sigma == 0)", name, (double)sigma);
    UCF_CHECK_ARG((((uintptr_t)x | (uintptr_t)z | (uintptr_t)out) & 3) == 0 && (((uintptr_t)pred) & (dtype == UCFVIT_F32 ? 3 : 1)) == 0,
                  "%s: misaligned pointer", name);
    if (B > 0) *pg = patch_geom_make(C, dims, nd, p);
    return UCFVIT_OK;
}

}  // namespace

extern "C" int ucfvit_ddpm_q_sample(const float* x0, const float* eps, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab,
                                    float* out, int64_t B, int64_t n_per_sample, int64_t T, void* stream) {
    UCF_CHECK_ARG(x0 && eps && t && sqrt_ab && sqrt_1mab && out, "ucfvit_ddpm_q_sample: null pointer");
    UCF_CHECK_ARG(B >= 0 && n_per_sample > 0 && B < (1ll << 31) && B * n_per_sample < (1ll << 40), "ucfvit_ddpm_q_sample: bad sizes B=%lld n=%lld",
                  (long long)B, (long long)n_per_sample);
    UCF_CHECK_ARG(T > 0 && T < (1ll << 31), "ucfvit_ddpm_q_sample: bad table length T=%lld", (long long)T);
    UCF_CHECK_ARG((((uintptr_t)x0 | (uintptr_t)eps | (uintptr_t)out | (uintptr_t)sqrt_ab | (uintptr_t)sqrt_1mab) & 3) == 0 && (((uintptr_t)t) & 7) == 0,
                  "ucfvit_ddpm_q_sample: misaligned pointer");
    if (B == 0) return UCFVIT_OK;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = n_per_sample % 4 == 0 && ucf_is_aligned16(x0) && ucf_is_aligned16(eps) && ucf_is_aligned16(out);
    if (vec)
        hipLaunchKernelGGL(q_sample_kernel<4>, dim3(df_grid(B * n_per_sample / 4)), dim3(DF_BLOCK), 0, s, x0, eps, t, sqrt_ab, sqrt_1mab, out, B,
                           n_per_sample, (int)T);
    else
        hipLaunchKernelGGL(q_sample_kernel<1>, dim3(df_grid(B * n_per_sample)), dim3(DF_BLOCK), 0, s, x0, eps, t, sqrt_ab, sqrt_1mab, out, B,
                           n_per_sample, (int)T);
    UCF_LAUNCH_CHECK("ucfvit_ddpm_q_sample");
    return UCFVIT_OK;
}

extern "C" int ucfvit_relu_dropout(const void* x, void* out, int64_t rows, int64_t D, double p, uint64_t seed, int dtype, void* stream) {
    UCF_CHECK_ARG(x && out, "ucfvit_relu_dropout: null pointer");
    DoParams P;
    const int rc = rd_check("ucfvit_relu_dropout", rows, D, p, seed, dtype, &P);
    if (rc != UCFVIT_OK) return rc;
    if (rows == 0) return UCFVIT_OK;
    if (dtype == UCFVIT_F32) return rd_launch<float, false>(x, nullptr, out, rows, D, p > 0.0, P, (hipStream_t)stream, "ucfvit_relu_dropout");
    return rd_launch<bf16, false>(x, nullptr, out, rows, D, p > 0.0, P, (hipStream_t)stream, "ucfvit_relu_dropout");
}

extern "C" int ucfvit_relu_dropout_bwd(const void* x, const void* dy, void* dx, int64_t rows, int64_t D, double p, uint64_t seed, int dtype,
                                       void* stream) {
    UCF_CHECK_ARG(x && dy && dx, "ucfvit_relu_dropout_bwd: null pointer");
    DoParams P;
    const int rc = rd_check("ucfvit_relu_dropout_bwd", rows, D, p, seed, dtype, &P);
    if (rc != UCFVIT_OK) return rc;
    if (rows == 0) return UCFVIT_OK;
    if (dtype == UCFVIT_F32) return rd_launch<float, true>(x, dy, dx, rows, D, p > 0.0, P, (hipStream_t)stream, "ucfvit_relu_dropout_bwd");
    return rd_launch<bf16, true>(x, dy, dx, rows, D, p > 0.0, P, (hipStream_t)stream, "ucfvit_relu_dropout_bwd");
}

extern "C" int ucfvit_ddpm_step(const float* x, const void* pred, const float* z, float* out, int64_t B, int64_t C, const int64_t* dims, int nd,
                                int64_t p, float c1, float c2, float sigma, int dtype, void* stream) {
    PatchGeom g;
    const int rc = step_check("ucfvit_ddpm_step", x, pred, z, out, B, C, dims, nd, p, sigma, dtype, &g);
    if (rc != UCFVIT_OK) return rc;
    if (B == 0) return UCFVIT_OK;
    const int64_t total = B * g.L * g.P;
    hipStream_t s = (hipStream_t)stream;
#define ST_GO(T, HZ)                                                                                                                          \
    hipLaunchKernelGGL((ddpm_step_kernel<T, HZ>), dim3(df_grid(total)), dim3(DF_BLOCK), 0, s, x, (const T*)pred, z, out, g, B, c1, c2, sigma)
    if (dtype == UCFVIT_F32) {
        if (z) ST_GO(float, true); else ST_GO(float, false);
    } else {
        if (z) ST_GO(bf16, true); else ST_GO(bf16, false);
    }
#undef ST_GO
    UCF_LAUNCH_CHECK("ucfvit_ddpm_step");
    return UCFVIT_OK;
}

extern "C" int ucfvit_ddim_step(const float* x, const void* pred, const float* z, float* out, int64_t B, int64_t C, const int64_t* dims, int nd,
                                int64_t p, float s_ab, float s_1mab, float r_ab, float r_1mab, float c_x0, float c_eps, float sigma, float clip,
                                int dtype, void* stream) {
    PatchGeom g;
    const int rc = step_check("ucfvit_ddim_step", x, pred, z, out, B, C, dims, nd, p, sigma, dtype, &g);
    if (rc != UCFVIT_OK) return rc;
    UCF_CHECK_ARG(clip >= 0.f, "ucfvit_ddim_step: clip %g must be 0 (no clamp) or positive", (double)clip);   // false for NaN
    if (B == 0) return UCFVIT_OK;
    const int64_t total = B * g.L * g.P;
    const DdimCoef k{s_ab, s_1mab, r_ab, r_1mab, c_x0, c_eps, sigma, clip};
    hipStream_t s = (hipStream_t)stream;
#define DI_GO(T, HZ, CL)                                                                                                                       \
    hipLaunchKernelGGL((ddim_step_kernel<T, HZ, CL>), dim3(df_grid(total)), dim3(DF_BLOCK), 0, s, x, (const T*)pred, z, out, g, B, k)
#define DI_Z(T, CL)                                                                                                                            \
    do {                                                                                                                                       \
        if (z) DI_GO(T, true, CL); else DI_GO(T, false, CL);                                                                                  \
    } while (0)
    if (dtype == UCFVIT_F32) {
        if (clip > 0.f) DI_Z(float, true); else DI_Z(float, false);
    } else {
        if (clip > 0.f) DI_Z(bf16, true); else DI_Z(bf16, false);
    }
#undef DI_Z
#undef DI_GO
    UCF_LAUNCH_CHECK("ucfvit_ddim_step");
    return UCFVIT_OK;
}
