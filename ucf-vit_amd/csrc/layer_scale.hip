// LayerScale (timm's LayerScale(dim, init_values), which the reference's Block builds as ls1 / ls2): a learned fp32 factor gamma[c] per
// column on a residual branch.  Two row passes in the geometry of csrc/drop_path.hip (row_pass.h); the per-sample drop-path scale s and
// the dropout mask of csrc/dropout_mask.h ride along, so a branch with all three still costs one pass per direction:
//   layer_scale_add : out[r][c] = res[r ldr + c] + f_r * m(r, c) * (gamma[c] * branch[r][c])      (res == NULL: without the residual)
//   layer_scale_grad: g = f_r * m(r, c) * dy[r][c];  dbranch[r][c] = gamma[c] * g;
//                     colsum[c] = sum_r gamma[c] * g (the exit Linear's bias gradient), gsum[c] = sum_r g * branch[r][c] (gamma's gradient)
// f_r = s[r / rows_per_sample] * (1 / keep), a missing factor being 1; with neither, no product by f_r is made.  gamma is the fp32 master
// parameter, read directly: a lane loads the W gammas of its columns once, before the row loop.  fp32 arithmetic, one rounding to the
// output type.  p == 0 selects kernels without any Philox code (MASK = false).
// A dropped element is a select, not a product, and a row with f_r == 0 is never read: forward copies res bit for bit (or writes zeros),
// backward writes zeros and adds exact zeros to both sums.
// Both sums are handed out per row chunk in the fixed order of drop_path_scale (per wave in row order, four rows folded pairwise per step,
// then the 4 waves pairwise); ucfvit_reduce_rows folds the chunks; no atomics.
#include "common.h"
#include "row_pass.h"
#include "dropout_mask.h"

namespace {

#define DTYPE_OK(d) ((d) == UCFVIT_F32 || (d) == UCFVIT_BF16)

template <bool MASK> __device__ __forceinline__ float ls_row_factor(const float* __restrict__ s, int r, int rows_per_sample, const DoParams& P) {
    if (MASK) return s ? s[(unsigned)r / (unsigned)rows_per_sample] * P.inv_keep : P.inv_keep;
    return s ? s[(unsigned)r / (unsigned)rows_per_sample] : 1.f;
}

// v where element e is live, else an exact +0 whatever v holds (NaN, Inf, an unread register).  keep is 0 for a row with f_r == 0.  With the
// mask the select is a bitwise AND with bit e of keep sign-extended to 0 or ~0 (v_bfe_i32).  Written as a comparison, hipcc holds one
// 64-bit scalar condition per element and row across both sums of the backward kernel and spills SGPRs (41 for bf16, 7 for fp32)
template <bool MASK> __device__ __forceinline__ float ls_live(float v, uint32_t keep, int e, bool row_live) {
    if (MASK) return __uint_as_float(__float_as_uint(v) & (uint32_t)__builtin_amdgcn_sbfe((int)keep, e, 1));      // bit e, sign-extended
    return row_live ? v : 0.f;
}

// out may alias x (the branch): every lane reads its elements of a row before it writes them, and no other lane touches them.
template <typename T, int W, bool MASK>
__global__ __launch_bounds__(DP_BLOCK) void layer_scale_add_kernel(const T* res, int64_t ldr, const T* x, const float* __restrict__ gamma,
                                                                   const float* __restrict__ s, T* out, int rows, int D, int rows_per_sample,
                                                                   int rows_per_chunk, DoParams P) {
    // the wave index as a scalar: rows, and with them the row factors, are uniform over a wave, so s is read with scalar loads (which do
    // not queue behind the 16-byte row loads in flight) and the tests on f_r are scalar branches
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = (blockIdx.x * 64 + lane) * W;
    const int r_begin = blockIdx.y * rows_per_chunk;                      // chunks * rows_per_chunk < rows + chunks: no overflow, rows < 2^30
    const int r_end = min(rows, r_begin + rows_per_chunk);
    if (col >= D) return;
    const bool scaled = MASK || s != nullptr;                              // uniform: is there a row factor at all
    float gm[W];
#pragma unroll
    for (int e = 0; e < W; ++e) gm[e] = gamma[col + e];                    // W > 1: D % W == 0, so col + e < D
    int r = r_begin + wave;
    for (; r + (DP_UNROLL - 1) * DP_WAVES < r_end; r += DP_UNROLL * DP_WAVES) {
        float f[DP_UNROLL];
        uint32_t keep[DP_UNROLL];
        Pack<T, W> a[DP_UNROLL], b[DP_UNROLL];
#pragma unroll
        for (int u = 0; u < DP_UNROLL; ++u) f[u] = ls_row_factor<MASK>(s, r + u * DP_WAVES, rows_per_sample, P);     // all factors first
#pragma unroll
        for (int u = 0; u < DP_UNROLL; ++u) {
            const int ru = r + u * DP_WAVES;
            if (res) a[u] = Pack<T, W>::load(res + (int64_t)ru * ldr + col);
            if (f[u] != 0.f) b[u] = Pack<T, W>::load(x + (int64_t)ru * D + col);
        }
#pragma unroll
        for (int u = 0; u < DP_UNROLL; ++u)
            keep[u] = !MASK ? ~0u : f[u] != 0.f ? keep_bits<W>((int64_t)(r + u * DP_WAVES) * P.row_step * D + col, P) : 0u;
#pragma unroll
        for (int u = 0; u < DP_UNROLL; ++u) {
            Pack<T, W> o;
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const float v = gm[e] * b[u].get(e);
                const float t = ls_live<MASK>(scaled ? f[u] * v : v, keep[u], e, f[u] != 0.f);              // a select: what is not live is 0
                o.set(e, res ? a[u].get(e) + t : t);
            }
            if (res && f[u] == 0.f) o = a[u];                              // the residual's own bits
            o.store(out + (int64_t)(r + u * DP_WAVES) * D + col);
        }
    }
    for (; r < r_end; r += DP_WAVES) {
        const float f = ls_row_factor<MASK>(s, r, rows_per_sample, P);
        Pack<T, W> a, b, o;
        if (res) a = Pack<T, W>::load(res + (int64_t)r * ldr + col);
        if (f != 0.f) b = Pack<T, W>::load(x + (int64_t)r * D + col);
        const uint32_t keep = !MASK ? ~0u : f != 0.f ? keep_bits<W>((int64_t)r * P.row_step * D + col, P) : 0u;
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const float v = gm[e] * b.get(e);
            const float t = ls_live<MASK>(scaled ? f * v : v, keep, e, f != 0.f);
            o.set(e, res ? a.get(e) + t : t);
        }
        if (res && f == 0.f) o = a;
        o.store(out + (int64_t)r * D + col);
    }
}

// dbranch may alias dy.  x (the branch output) is read only when the gamma sums are wanted.  Two sets of W accumulators: acc_c the column
// sums of gamma g, acc_g those of g x.
template <typename T, int W, bool MASK>
__global__ __launch_bounds__(DP_BLOCK) void layer_scale_grad_kernel(const T* dy, const T* x, const float* __restrict__ gamma,
                                                                    const float* __restrict__ s, T* dx, float* __restrict__ part_c,
                                                                    float* __restrict__ part_g, int rows, int D, int rows_per_sample,
                                                                    int rows_per_chunk, DoParams P) {
    __shared__ float red[2][DP_WAVES][64 * W];
    // the wave index as a scalar: rows, and with them the row factors, are uniform over a wave, so s is read with scalar loads (which do
    // not queue behind the 16-byte row loads in flight) and the tests on f_r are scalar branches
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = (blockIdx.x * 64 + lane) * W;
    const int r_begin = blockIdx.y * rows_per_chunk;
    const int r_end = min(rows, r_begin + rows_per_chunk);
    const bool scaled = MASK || s != nullptr;
    float acc_c[W], acc_g[W];
#pragma unroll
    for (int e = 0; e < W; ++e) acc_c[e] = 0.f, acc_g[e] = 0.f;
    if (col < D) {
        float gm[W];
#pragma unroll
        for (int e = 0; e < W; ++e) gm[e] = gamma[col + e];
        int r = r_begin + wave;
        for (; r + (DP_UNROLL - 1) * DP_WAVES < r_end; r += DP_UNROLL * DP_WAVES) {
            float f[DP_UNROLL];
            uint32_t keep[DP_UNROLL];
            Pack<T, W> a[DP_UNROLL], b[DP_UNROLL];
#pragma unroll
            for (int u = 0; u < DP_UNROLL; ++u) f[u] = ls_row_factor<MASK>(s, r + u * DP_WAVES, rows_per_sample, P); // all factors first
#pragma unroll
            for (int u = 0; u < DP_UNROLL; ++u) {
                const int ru = r + u * DP_WAVES;
                if (f[u] != 0.f) {
                    a[u] = Pack<T, W>::load(dy + (int64_t)ru * D + col);
                    if (part_g) b[u] = Pack<T, W>::load(x + (int64_t)ru * D + col);
                }
            }
#pragma unroll
            for (int u = 0; u < DP_UNROLL; ++u)
                keep[u] = !MASK ? ~0u : f[u] != 0.f ? keep_bits<W>((int64_t)(r + u * DP_WAVES) * P.row_step * D + col, P) : 0u;
            float tc[DP_UNROLL][W], tg[DP_UNROLL][W];
#pragma unroll
            for (int u = 0; u < DP_UNROLL; ++u) {
                Pack<T, W> o;
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    const float g = scaled ? f[u] * a[u].get(e) : a[u].get(e);
                    tc[u][e] = ls_live<MASK>(gm[e] * g, keep[u], e, f[u] != 0.f);         // selects: what is not live is an exact 0
                    tg[u][e] = part_g ? ls_live<MASK>(g * b[u].get(e), keep[u], e, f[u] != 0.f) : 0.f;
                    o.set(e, tc[u][e]);
                }
                o.store(dx + (int64_t)(r + u * DP_WAVES) * D + col);
            }
            if (part_c) {
#pragma unroll
                for (int e = 0; e < W; ++e) acc_c[e] += (tc[0][e] + tc[1][e]) + (tc[2][e] + tc[3][e]);
            }
            if (part_g) {
#pragma unroll
                for (int e = 0; e < W; ++e) acc_g[e] += (tg[0][e] + tg[1][e]) + (tg[2][e] + tg[3][e]);
            }
        }
        for (; r < r_end; r += DP_WAVES) {
            const float f = ls_row_factor<MASK>(s, r, rows_per_sample, P);
            Pack<T, W> a, b, o;
            if (f != 0.f) {
                a = Pack<T, W>::load(dy + (int64_t)r * D + col);
                if (part_g) b = Pack<T, W>::load(x + (int64_t)r * D + col);
            }
            const uint32_t keep = !MASK ? ~0u : f != 0.f ? keep_bits<W>((int64_t)r * P.row_step * D + col, P) : 0u;
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const float g = scaled ? f * a.get(e) : a.get(e);
                const float tc = ls_live<MASK>(gm[e] * g, keep, e, f != 0.f), tg = part_g ? ls_live<MASK>(g * b.get(e), keep, e, f != 0.f) : 0.f;
                o.set(e, tc);
                acc_c[e] += tc;
                acc_g[e] += tg;
            }
            o.store(dx + (int64_t)r * D + col);
        }
    }
    if (!part_c && !part_g) return;                                        // uniform over the workgroup
#pragma unroll
    for (int e = 0; e < W; ++e) red[0][wave][lane * W + e] = acc_c[e], red[1][wave][lane * W + e] = acc_g[e];
    __syncthreads();
    if (wave == 0 && col < D) {
#pragma unroll
        for (int e = 0; e < W; ++e) {
            if (part_c)
                part_c[(int64_t)blockIdx.y * D + col + e] =
                    (red[0][0][lane * W + e] + red[0][1][lane * W + e]) + (red[0][2][lane * W + e] + red[0][3][lane * W + e]);
            if (part_g)
                part_g[(int64_t)blockIdx.y * D + col + e] =
                    (red[1][0][lane * W + e] + red[1][1][lane * W + e]) + (red[1][2][lane * W + e] + red[1][3][lane * W + e]);
        }
    }
}

template <typename T, bool MASK>
int ls_add_launch(const void* res, int64_t ldr, const void* x, const float* gamma, const float* s, void* out, int64_t rows, int64_t D,
                  int64_t rows_per_sample, const DoParams& P, hipStream_t st) {
    constexpr int EPV = Vec16<T>::N;
    const bool vec = D % EPV == 0 && ucf_is_aligned16(x) && ucf_is_aligned16(out) && (!res || (ldr % EPV == 0 && ucf_is_aligned16(res)));
    const int chunks = dp_chunks(rows, D);
    const int rpc = (int)((rows + chunks - 1) / chunks);
    if (vec) {
        const dim3 grid((unsigned)((D / EPV + 63) / 64), chunks);
        hipLaunchKernelGGL((layer_scale_add_kernel<T, EPV, MASK>), grid, dim3(DP_BLOCK), 0, st, (const T*)res, ldr, (const T*)x, gamma, s, (T*)out,
                           (int)rows, (int)D, (int)rows_per_sample, rpc, P);
    } else {
        const dim3 grid((unsigned)((D + 63) / 64), chunks);
        hipLaunchKernelGGL((layer_scale_add_kernel<T, 1, MASK>), grid, dim3(DP_BLOCK), 0, st, (const T*)res, ldr, (const T*)x, gamma, s, (T*)out,
                           (int)rows, (int)D, (int)rows_per_sample, rpc, P);
    }
    UCF_LAUNCH_CHECK("ucfvit_layer_scale_add");
    return UCFVIT_OK;
}

template <typename T, bool MASK>
int ls_grad_launch(const void* dy, const void* x, const float* gamma, const float* s, void* dx, float* part_c, float* part_g, int64_t rows,
                   int64_t D, int64_t rows_per_sample, const DoParams& P, hipStream_t st) {
    constexpr int EPV = Vec16<T>::N;
    const bool vec = D % EPV == 0 && ucf_is_aligned16(dy) && ucf_is_aligned16(dx) && (!x || ucf_is_aligned16(x));
    const int chunks = dp_chunks(rows, D);
    const int rpc = (int)((rows + chunks - 1) / chunks);
    if (vec) {
        const dim3 grid((unsigned)((D / EPV + 63) / 64), chunks);
        hipLaunchKernelGGL((layer_scale_grad_kernel<T, EPV, MASK>), grid, dim3(DP_BLOCK), 0, st, (const T*)dy, (const T*)x, gamma, s, (T*)dx,
                           part_c, part_g, (int)rows, (int)D, (int)rows_per_sample, rpc, P);
    } else {
        const dim3 grid((unsigned)((D + 63) / 64), chunks);
        hipLaunchKernelGGL((layer_scale_grad_kernel<T, 1, MASK>), grid, dim3(DP_BLOCK), 0, st, (const T*)dy, (const T*)x, gamma, s, (T*)dx,
                           part_c, part_g, (int)rows, (int)D, (int)rows_per_sample, rpc, P);
    }
    UCF_LAUNCH_CHECK("ucfvit_layer_scale_grad");
    return UCFVIT_OK;
}

// shared argument checks and the mask parameters (dropout_mask.h, p == 0 allowed: no mask); before any HIP call
int ls_check(const char* name, int64_t rows, int64_t D, int64_t rows_per_sample, int64_t row_step, double p, uint64_t seed, int dtype,
             DoParams* P) {
    UCF_CHECK_ARG(D > 0 && D < (1ll << 30), "%s: bad row width D=%lld", name, (long long)D);
    UCF_CHECK_ARG(rows_per_sample > 0, "%s: bad rows_per_sample=%lld", name, (long long)rows_per_sample);
    UCF_CHECK_ARG(rows >= 0 && rows < (1ll << 30), "%s: bad row count %lld", name, (long long)rows);
    UCF_CHECK_ARG(rows % rows_per_sample == 0, "%s: rows=%lld is not a multiple of rows_per_sample=%lld", name, (long long)rows,
                  (long long)rows_per_sample);
    const int rc = do_mask_check(name, rows, row_step, p, seed, true, P);
    if (rc != UCFVIT_OK) return rc;
    UCF_CHECK_ARG(DTYPE_OK(dtype), "%s: bad dtype %d", name, dtype);
    return UCFVIT_OK;
}

}  // namespace

extern "C" int ucfvit_layer_scale_add(const void* res, int64_t ldr, const void* branch, const float* gamma, const float* s, void* out,
                                      int64_t rows, int64_t D, int64_t rows_per_sample, int64_t row_step, double p, uint64_t seed, int dtype,
                                      void* stream) {
    UCF_CHECK_ARG(branch && out, "ucfvit_layer_scale_add: null pointer");
    UCF_CHECK_ARG(gamma, "ucfvit_layer_scale_add: null gamma");
    DoParams P;
    const int rc = ls_check("ucfvit_layer_scale_add", rows, D, rows_per_sample, row_step, p, seed, dtype, &P);
    if (rc != UCFVIT_OK) return rc;
    UCF_CHECK_ARG(!res || ldr >= D, "ucfvit_layer_scale_add: residual row stride ldr=%lld < D=%lld", (long long)ldr, (long long)D);
    if (rows == 0) return UCFVIT_OK;
    const hipStream_t st = (hipStream_t)stream;
    if (p > 0.0) {
        if (dtype == UCFVIT_F32) return ls_add_launch<float, true>(res, ldr, branch, gamma, s, out, rows, D, rows_per_sample, P, st);
        return ls_add_launch<bf16, true>(res, ldr, branch, gamma, s, out, rows, D, rows_per_sample, P, st);
    }
    if (dtype == UCFVIT_F32) return ls_add_launch<float, false>(res, ldr, branch, gamma, s, out, rows, D, rows_per_sample, P, st);
    return ls_add_launch<bf16, false>(res, ldr, branch, gamma, s, out, rows, D, rows_per_sample, P, st);
}

extern "C" int ucfvit_layer_scale_grad(const void* dy, const void* branch, const float* gamma, const float* s, void* dbranch,
                                       float* colsum_partial, float* gamma_partial, int64_t rows, int64_t D, int64_t rows_per_sample,
                                       int64_t row_step, double p, uint64_t seed, int dtype, void* stream) {
    UCF_CHECK_ARG(dy && dbranch, "ucfvit_layer_scale_grad: null pointer");
    UCF_CHECK_ARG(gamma, "ucfvit_layer_scale_grad: null gamma");
    UCF_CHECK_ARG(branch || !gamma_partial, "ucfvit_layer_scale_grad: the gamma sums need the branch output (branch is null)");
    DoParams P;
    const int rc = ls_check("ucfvit_layer_scale_grad", rows, D, rows_per_sample, row_step, p, seed, dtype, &P);
    if (rc != UCFVIT_OK) return rc;
    UCF_CHECK_ARG(rows > 0 || (!colsum_partial && !gamma_partial), "ucfvit_layer_scale_grad: no column sums of an empty input");
    if (rows == 0) return UCFVIT_OK;
    const hipStream_t st = (hipStream_t)stream;
    if (p > 0.0) {
        if (dtype == UCFVIT_F32)
            return ls_grad_launch<float, true>(dy, branch, gamma, s, dbranch, colsum_partial, gamma_partial, rows, D, rows_per_sample, P, st);
        return ls_grad_launch<bf16, true>(dy, branch, gamma, s, dbranch, colsum_partial, gamma_partial, rows, D, rows_per_sample, P, st);
    }
    if (dtype == UCFVIT_F32)
        return ls_grad_launch<float, false>(dy, branch, gamma, s, dbranch, colsum_partial, gamma_partial, rows, D, rows_per_sample, P, st);
    return ls_grad_launch<bf16, false>(dy, branch, gamma, s, dbranch, colsum_partial, gamma_partial, rows, D, rows_per_sample, P, st);
}
