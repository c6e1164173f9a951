// Attention of ONE query row per (batch element, head) against all N keys / values: what the last Block of a model whose head
// reads only the class token needs of its attention.  HBM-bound: K and V are read once (forward), K and V read and dqkv written
// once (backward); the arithmetic is plain fp32 VALU dot products, no MFMA.
//
// One workgroup of 4 waves per (batch element, head).  A key / value row of the head (DH elements) is covered by LPR = DH / EPV
// neighbouring lanes with one 16-byte vector each, so a wave reads whole contiguous head rows and 256 / LPR rows are in flight per
// step.  Everything that touches qkv / dqkv goes through a buffer descriptor over exactly the batch element's N rows.
#include "attn_tile.h"

namespace {

constexpr int AR_THREADS = 256;
constexpr int AR_U = 4;          // key rows a thread requests before it consumes the first
constexpr int AR_MAX_N = 8192;   // scores of one head live in LDS

template <typename T> __device__ __forceinline__ Vec16<T> ar_load(__amdgpu_buffer_rsrc_t r, int byte_off) {
    Vec16<T> v;
    v.v = __builtin_bit_cast(decltype(v.v), __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
    return v;
}
template <typename T> __device__ __forceinline__ void ar_store(__amdgpu_buffer_rsrc_t r, int byte_off, const Vec16<T>& v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v.v), r, byte_off, 0, 0);
}
template <int LPR> __device__ __forceinline__ float ar_row_sum(float v) {   // over the LPR lanes that share a row
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// block-wide reductions over the 4 waves; `slot`: 4 floats of LDS that nobody else uses until the next barrier pair
__device__ __forceinline__ float ar_block_max(float v, float* slot) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(slot[0], slot[1]), fmaxf(slot[2], slot[3]));
}
__device__ __forceinline__ float ar_block_sum(float v, float* slot) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}

// dynamic LDS: sc[N rounded up to 4] scores / probabilities, then red[AR_THREADS * EPV] cross-row-group partials
template <typename T, int DH>
__global__ __launch_bounds__(AR_THREADS) void attn_rows_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ out, float* __restrict__ lse,
                                                                   int N, int H, int qrow, float scale_log2e) {
    constexpr int EPV = Vec16<T>::N, LPR = DH / EPV, RPP = AR_THREADS / LPR, ES = (int)sizeof(T);
    extern __shared__ __attribute__((aligned(16))) float ar_smem[];
    __shared__ float wred[2][4];
    float* sc = ar_smem;
    float* red = ar_smem + ((N + 3) & ~3);
    const int tid = threadIdx.x, c = tid % LPR, g = tid / LPR;
    const int h = blockIdx.x % H;
    const int64_t b = blockIdx.x / H;
    const int D = H * DH, rs_bytes = 3 * D * ES;
    const __amdgpu_buffer_rsrc_t rQ = buffer_rsrc(qkv + b * N * 3 * (int64_t)D, N * rs_bytes);
    const int colb = (h * DH + c * EPV) * ES;
    const Vec16<T> qv = ar_load<T>(rQ, qrow * rs_bytes + colb);
    // scores s_j = q . K_j (unscaled)
    for (int j0 = 0; j0 < N; j0 += RPP * AR_U) {
        Vec16<T> kv[AR_U];
#pragma unroll
        for (int u = 0; u < AR_U; ++u) {
            const int j = j0 + u * RPP + g;
            if (j < N) kv[u] = ar_load<T>(rQ, j * rs_bytes + D * ES + colb);
        }
#pragma unroll
        for (int u = 0; u < AR_U; ++u) {
            const int j = j0 + u * RPP + g;
            float s = 0.f;
            if (j < N) {
#pragma unroll
                for (int e = 0; e < EPV; ++e) s = fmaf(qv.get(e), kv[u].get(e), s);
            }
            s = ar_row_sum<LPR>(s);
            if (c == 0 && j < N) sc[j] = s;
        }
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int j = tid; j < N; j += AR_THREADS) mx = fmaxf(mx, sc[j]);
    const float m = ar_block_max(mx, wred[0]) * scale_log2e;
    float l = 0.f;
    for (int j = tid; j < N; j += AR_THREADS) {
        const float p = __builtin_amdgcn_exp2f(fmaf(sc[j], scale_log2e, -m));
        sc[j] = p;
        l += p;
    }
    const float lt = ar_block_sum(l, wred[1]);        // (its barrier also publishes the probabilities)
    // o = sum_j p_j V_j
    float acc[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[e] = 0.f;
    for (int j0 = 0; j0 < N; j0 += RPP * AR_U) {
        Vec16<T> vv[AR_U];
#pragma unroll
        for (int u = 0; u < AR_U; ++u) {
            const int j = j0 + u * RPP + g;
            if (j < N) vv[u] = ar_load<T>(rQ, j * rs_bytes + 2 * D * ES + colb);
        }
#pragma unroll
        for (int u = 0; u < AR_U; ++u) {
            const int j = j0 + u * RPP + g;
            if (j < N) {
                const float p = sc[j];
#pragma unroll
                for (int e = 0; e < EPV; ++e) acc[e] = fmaf(p, vv[u].get(e), acc[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < EPV; ++e) red[tid * EPV + e] = acc[e];      // = red[g][c * EPV + e], rows of DH floats
    __syncthreads();
    if (tid < LPR) {
        const float inv = 1.f / lt;
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
            float t = 0.f;
            for (int r = 0; r < RPP; ++r) t += red[r * DH + tid * EPV + e];
            o.set(e, t * inv);
        }
        *reinterpret_cast<Vec16<T>*>(out + b * D + h * DH + tid * EPV) = o;
        if (tid == 0) lse[b * H + h] = m + log2f(lt);
    }
}

// dynamic LDS: red[AR_THREADS * EPV]
template <typename T, int DH>
__global__ __launch_bounds__(AR_THREADS) void attn_rows_bwd_kernel(const T* __restrict__ qkv, const T* __restrict__ out, const T* __restrict__ dout,
                                                                   const float* __restrict__ lse, T* __restrict__ dqkv,
                                                                   float* __restrict__ cs_partial, int N, int H, int qrow, float scale,
                                                                   float scale_log2e) {
    constexpr int EPV = Vec16<T>::N, LPR = DH / EPV, RPP = AR_THREADS / LPR, ES = (int)sizeof(T);
    extern __shared__ __attribute__((aligned(16))) float ar_smem[];
    float* red = ar_smem;
    const int tid = threadIdx.x, c = tid % LPR, g = tid / LPR;
    const int h = blockIdx.x % H;
    const int64_t b = blockIdx.x / H;
    const int D = H * DH, rs_bytes = 3 * D * ES;
    const __amdgpu_buffer_rsrc_t rQ = buffer_rsrc(qkv + b * N * 3 * (int64_t)D, N * rs_bytes);
    const __amdgpu_buffer_rsrc_t rDQ = buffer_rsrc(dqkv + b * N * 3 * (int64_t)D, N * rs_bytes);
    const int colb = (h * DH + c * EPV) * ES;
    const Vec16<T> qv = ar_load<T>(rQ, qrow * rs_bytes + colb);
    const Vec16<T> dov = *reinterpret_cast<const Vec16<T>*>(dout + b * D + h * DH + c * EPV);
    const Vec16<T> ov = *reinterpret_cast<const Vec16<T>*>(out + b * D + h * DH + c * EPV);
    float dl = 0.f;
#pragma unroll
    for (int e = 0; e < EPV; ++e) dl = fmaf(dov.get(e), ov.get(e), dl);
    const float delta = ar_row_sum<LPR>(dl);
    const float L = lse[b * H + h];
    Vec16<T> zero;
#pragma unroll
    for (int e = 0; e < EPV; ++e) zero.set(e, 0.f);
    float dqa[EPV], qs[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
        dqa[e] = 0.f;
        qs[e] = scale * qv.get(e);
    }
    for (int j0 = 0; j0 < N; j0 += RPP * AR_U) {
        Vec16<T> kv[AR_U], vv[AR_U];
#pragma unroll
        for (int u = 0; u < AR_U; ++u) {
            const int j = j0 + u * RPP + g;
            if (j < N) {
                kv[u] = ar_load<T>(rQ, j * rs_bytes + D * ES + colb);
                vv[u] = ar_load<T>(rQ, j * rs_bytes + 2 * D * ES + colb);
            }
        }
#pragma unroll
        for (int u = 0; u < AR_U; ++u) {
            const int j = j0 + u * RPP + g;
            float s = 0.f, dp = 0.f;
            if (j < N) {
#pragma unroll
                for (int e = 0; e < EPV; ++e) {
                    s = fmaf(qv.get(e), kv[u].get(e), s);
                    dp = fmaf(dov.get(e), vv[u].get(e), dp);
                }
            }
            s = ar_row_sum<LPR>(s);
            dp = ar_row_sum<LPR>(dp);
            if (j < N) {
                // p = ph * ph, applied one factor at a time: a single query's dK / dV rows ARE the products p * (...), with p far below
                // 2^-126 on the keys the row ignores while the other factor reaches 2^10 — v_exp_f32 would flush such a p to 0, and an
                // fp32 product must only underflow where its final value does
                const float ph = __builtin_amdgcn_exp2f(0.5f * fmaf(s, scale_log2e, -L));
                const float w = dp - delta;
                const float ds = ph * (ph * w);
                Vec16<T> dk, dv;
#pragma unroll
                for (int e = 0; e < EPV; ++e) {
                    dqa[e] = fmaf(ds, kv[u].get(e), dqa[e]);
                    dk.set(e, ph * (ph * (w * qs[e])));
                    dv.set(e, ph * (ph * dov.get(e)));
                }
                if (j != qrow) ar_store<T>(rDQ, j * rs_bytes + colb, zero);      // (the query's own row: below)
                ar_store<T>(rDQ, j * rs_bytes + D * ES + colb, dk);
                ar_store<T>(rDQ, j * rs_bytes + 2 * D * ES + colb, dv);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < EPV; ++e) red[tid * EPV + e] = dqa[e];
    __syncthreads();
    if (tid < LPR) {
        Vec16<T> dq;
        float dqf[EPV];
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
            float t = 0.f;
            for (int r = 0; r < RPP; ++r) t += red[r * DH + tid * EPV + e];
            dqf[e] = t * scale;
            dq.set(e, dqf[e]);
        }
        ar_store<T>(rDQ, qrow * rs_bytes + (h * DH + tid * EPV) * ES, dq);
        if (cs_partial) {
            float* cq = cs_partial + b * 2 * D + h * DH + tid * EPV;
#pragma unroll
            for (int e = 0; e < EPV; e += 4) {
                *reinterpret_cast<f32x4*>(cq + e) = f32x4{dqf[e], dqf[e + 1], dqf[e + 2], dqf[e + 3]};
                *reinterpret_cast<f32x4*>(cq + D + e) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
}

int ar_check(const char* who, int64_t B, int64_t N, int64_t H, int64_t dh, int64_t qrow, int dtype) {
    UCF_CHECK_ARG(B > 0 && N > 0 && H > 0 && B * H < (1ll << 31), "%s: bad shape B=%lld N=%lld H=%lld", who, (long long)B, (long long)N, (long long)H);
    UCF_CHECK_ARG(dh == 32 || dh == 64 || dh == 128, "%s: head dim %lld not in {32, 64, 128}", who, (long long)dh);
    UCF_CHECK_ARG(dtype == UCFVIT_F32 || dtype == UCFVIT_BF16, "%s: bad dtype %d", who, dtype);
    UCF_CHECK_ARG(qrow >= 0 && qrow < N, "%s: query row %lld outside [0, N=%lld)", who, (long long)qrow, (long long)N);
    const int64_t es = dtype == UCFVIT_F32 ? 4 : 2;
    if (N > AR_MAX_N || N * 3 * H * dh * es >= (1ll << 31)) {
        ucfvit_set_error("%s: N=%lld is outside the one-query kernels (N <= %d, one batch element's qkv below 2 GiB)", who, (long long)N, AR_MAX_N);
        return UCFVIT_ERR_UNSUPPORTED;
    }
    return UCFVIT_OK;
}

template <typename T, int DH>
int ar_fwd_launch(const void* qkv, void* out, float* lse, int64_t B, int64_t N, int64_t H, int64_t qrow, float scale, hipStream_t s) {
    constexpr int EPV = Vec16<T>::N;
    const size_t smem = (size_t)(((N + 3) & ~(int64_t)3) + AR_THREADS * EPV) * sizeof(float);
    hipLaunchKernelGGL((attn_rows_fwd_kernel<T, DH>), dim3((unsigned)(B * H)), dim3(AR_THREADS), smem, s, (const T*)qkv, (T*)out, lse, (int)N, (int)H,
                       (int)qrow, scale * LOG2E_F);
    UCF_LAUNCH_CHECK("ucfvit_attention_rows_fwd");
    return UCFVIT_OK;
}

template <typename T, int DH>
int ar_bwd_launch(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* cs_partial, int64_t B, int64_t N, int64_t H,
                  int64_t qrow, float scale, hipStream_t s) {
    constexpr int EPV = Vec16<T>::N;
    const size_t smem = (size_t)AR_THREADS * EPV * sizeof(float);
    hipLaunchKernelGGL((attn_rows_bwd_kernel<T, DH>), dim3((unsigned)(B * H)), dim3(AR_THREADS), smem, s, (const T*)qkv, (const T*)out, (const T*)dout, lse,
                       (T*)dqkv, cs_partial, (int)N, (int)H, (int)qrow, scale, scale * LOG2E_F);
    UCF_LAUNCH_CHECK("ucfvit_attention_rows_bwd");
    return UCFVIT_OK;
}

#define AR_DISPATCH(FN, ...)                                                      \
    do {                                                                          \
        if (dtype == UCFVIT_BF16) {                                               \
            if (dh == 32) return FN<bf16, 32>(__VA_ARGS__);                       \
            if (dh == 64) return FN<bf16, 64>(__VA_ARGS__);                       \
            return FN<bf16, 128>(__VA_ARGS__);                                    \
        }                                                                         \
        if (dh == 32) return FN<float, 32>(__VA_ARGS__);                          \
        if (dh == 64) return FN<float, 64>(__VA_ARGS__);                          \
        return FN<float, 128>(__VA_ARGS__);                                       \
    } while (0)

}  // namespace

extern "C" int ucfvit_attention_rows_fwd(const void* qkv, void* out, float* lse, int64_t B, int64_t N, int64_t H, int64_t dh, int64_t qrow,
                                         float scale, int dtype, void* stream) {
    if (B == 0) return UCFVIT_OK;                      // empty batch (pointers may be NULL)
    UCF_CHECK_ARG(qkv && out && lse, "ucfvit_attention_rows_fwd: null pointer");
    if (int rc = ar_check("ucfvit_attention_rows_fwd", B, N, H, dh, qrow, dtype)) return rc;
    UCF_CHECK_ARG(ucf_is_aligned16(qkv) && ucf_is_aligned16(out), "ucfvit_attention_rows_fwd: pointers must be 16-byte aligned");
    AR_DISPATCH(ar_fwd_launch, qkv, out, lse, B, N, H, qrow, scale, (hipStream_t)stream);
}

extern "C" int ucfvit_attention_rows_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* colsum_partial,
                                         int64_t B, int64_t N, int64_t H, int64_t dh, int64_t qrow, float scale, int dtype, void* stream) {
    if (B == 0) return UCFVIT_OK;                      // empty batch (pointers may be NULL)
    UCF_CHECK_ARG(qkv && out && dout && lse && dqkv, "ucfvit_attention_rows_bwd: null pointer");
    if (int rc = ar_check("ucfvit_attention_rows_bwd", B, N, H, dh, qrow, dtype)) return rc;
    UCF_CHECK_ARG(ucf_is_aligned16(qkv) && ucf_is_aligned16(out) && ucf_is_aligned16(dout) && ucf_is_aligned16(dqkv) && ucf_is_aligned16(colsum_partial),
                  "ucfvit_attention_rows_bwd: pointers must be 16-byte aligned");
    AR_DISPATCH(ar_bwd_launch, qkv, out, dout, lse, dqkv, colsum_partial, B, N, H, qrow, scale, (hipStream_t)stream);
}
