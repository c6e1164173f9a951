// Element-wise dropout on the token stream (nn.Dropout in training: head_drop, pos_drop, proj_drop, Mlp.drop1 / drop2 of the reference).
// The mask is never stored: it is a pure function of (seed, element index), defined in include/ucfvit_hip.h, and forward, backward and
// an activation-checkpoint recompute regenerate it.  With the 64-bit index i = (r * row_step) * D + c of element (r, c):
//   w = Philox4x32-10(counter = (lo32(i >> 2), hi32(i >> 2), 0, 0), key = (lo32(seed), hi32(seed)))[i & 3],   dropped iff w < T
// Two row passes in the geometry of csrc/drop_path.hip (row_pass.h), with the optional per-sample drop-path scale s riding along:
//   dropout     : out[r][c] = f_r * m * x[r][c]                  f_r = s[r / rows_per_sample] * (1 / keep) in fp32 (s == NULL: 1 / keep)
//   dropout_add : out[r][c] = res[r][c] + f_r * m * branch[r][c]
// A lane of the vector path owns 4 (fp32) or 8 (bf16) consecutive elements whose index starts at a multiple of 4: one or two Philox
// blocks, every word used.  The scalar path (odd D, unaligned base) evaluates one block per element and takes word i & 3: same mask.
// A dropped element is a select, not a product: NaN or Inf under the mask does not reach the output.  A row with s == 0 is never read
// and costs no Philox: dropout writes zeros, dropout_add copies res bit for bit.
// dropout can hand out fp32 column sums of the values it writes (before rounding), per row chunk in the fixed order of
// drop_path_scale; ucfvit_reduce_rows folds the chunks; no atomics.
#include "common.h"
#include "row_pass.h"
#include "dropout_mask.h"

namespace {

#define DTYPE_OK(d) ((d) == UCFVIT_F32 || (d) == UCFVIT_BF16)

// ADD: out = res + f m branch (x = branch, res with row stride ldr); else out = f m x.  out may alias x: every lane reads its elements of
// a row before it writes them, and no other lane touches them.
template <typename T, int W, bool ADD>
__global__ __launch_bounds__(DP_BLOCK) void dropout_kernel(const T* res, int64_t ldr, const T* x, const float* __restrict__ s, T* out,
                                                           float* __restrict__ partial, int rows, int D, int rows_per_sample,
                                                           int rows_per_chunk, DoParams P) {
    __shared__ float red[DP_WAVES][64 * W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + lane) * W;
    const int r_begin = blockIdx.y * rows_per_chunk;                      // chunks * rows_per_chunk < rows + chunks: no overflow, rows < 2^30
    const int r_end = min(rows, r_begin + rows_per_chunk);
    float acc[W];
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = 0.f;
    if (col < D) {
        int r = r_begin + wave;
        for (; r + (DP_UNROLL - 1) * DP_WAVES < r_end; r += DP_UNROLL * DP_WAVES) {
            float f[DP_UNROLL];
            uint32_t keep[DP_UNROLL];
            Pack<T, W> a[DP_UNROLL], b[DP_UNROLL];
#pragma unroll
            for (int u = 0; u < DP_UNROLL; ++u) {
                const int ru = r + u * DP_WAVES;
                f[u] = s ? s[(unsigned)ru / (unsigned)rows_per_sample] * P.inv_keep : P.inv_keep;
                if (ADD) a[u] = Pack<T, W>::load(res + (int64_t)ru * ldr + col);
                if (f[u] != 0.f) b[u] = Pack<T, W>::load(x + (int64_t)ru * D + col);
            }
#pragma unroll
            for (int u = 0; u < DP_UNROLL; ++u)
                keep[u] = f[u] != 0.f ? keep_bits<W>((int64_t)(r + u * DP_WAVES) * P.row_step * D + col, P) : 0u;
            float t[DP_UNROLL][W];
#pragma unroll
            for (int u = 0; u < DP_UNROLL; ++u) {
                Pack<T, W> o;
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    t[u][e] = (keep[u] >> e) & 1u ? f[u] * b[u].get(e) : 0.f;
                    o.set(e, ADD ? a[u].get(e) + t[u][e] : t[u][e]);
                }
                if (ADD && f[u] == 0.f) o = a[u];                          // the residual's own bits
                o.store(out + (int64_t)(r + u * DP_WAVES) * D + col);
            }
            if (partial) {
#pragma unroll
                for (int e = 0; e < W; ++e) acc[e] += (t[0][e] + t[1][e]) + (t[2][e] + t[3][e]);
            }
        }
        for (; r < r_end; r += DP_WAVES) {
            const float f = s ? s[(unsigned)r / (unsigned)rows_per_sample] * P.inv_keep : P.inv_keep;
            Pack<T, W> a, b, o;
            if (ADD) a = Pack<T, W>::load(res + (int64_t)r * ldr + col);
            if (f != 0.f) b = Pack<T, W>::load(x + (int64_t)r * D + col);
            const uint32_t keep = f != 0.f ? keep_bits<W>((int64_t)r * P.row_step * D + col, P) : 0u;
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const float t = (keep >> e) & 1u ? f * b.get(e) : 0.f;
                o.set(e, ADD ? a.get(e) + t : t);
                acc[e] += t;
            }
            if (ADD && f == 0.f) o = a;
            o.store(out + (int64_t)r * D + col);
        }
    }
    if (!partial) return;                                                  // uniform over the workgroup
#pragma unroll
    for (int e = 0; e < W; ++e) red[wave][lane * W + e] = acc[e];
    __syncthreads();
    if (wave == 0 && col < D) {
#pragma unroll
        for (int e = 0; e < W; ++e)
            partial[(int64_t)blockIdx.y * D + col + e] =
                (red[0][lane * W + e] + red[1][lane * W + e]) + (red[2][lane * W + e] + red[3][lane * W + e]);
    }
}

template <typename T, bool ADD>
int do_launch(const void* res, int64_t ldr, const void* x, const float* s, void* out, float* partial, int64_t rows, int64_t D,
              int64_t rows_per_sample, const DoParams& P, hipStream_t st, const char* name) {
    constexpr int EPV = Vec16<T>::N;
    const bool vec = D % EPV == 0 && ucf_is_aligned16(x) && ucf_is_aligned16(out) && (!ADD || (ldr % EPV == 0 && ucf_is_aligned16(res)));
    const int chunks = dp_chunks(rows, D);
    const int rpc = (int)((rows + chunks - 1) / chunks);
    if (vec) {
        const dim3 grid((unsigned)((D / EPV + 63) / 64), chunks);
        hipLaunchKernelGGL((dropout_kernel<T, EPV, ADD>), grid, dim3(DP_BLOCK), 0, st, (const T*)res, ldr, (const T*)x, s, (T*)out, partial,
                           (int)rows, (int)D, (int)rows_per_sample, rpc, P);
    } else {
        const dim3 grid((unsigned)((D + 63) / 64), chunks);
        hipLaunchKernelGGL((dropout_kernel<T, 1, ADD>), grid, dim3(DP_BLOCK), 0, st, (const T*)res, ldr, (const T*)x, s, (T*)out, partial,
                           (int)rows, (int)D, (int)rows_per_sample, rpc, P);
    }
    UCF_LAUNCH_CHECK(name);
    return UCFVIT_OK;
}

// shared argument checks and the mask parameters (dropout_mask.h); before any HIP call
int do_check(const char* name, int64_t rows, int64_t D, int64_t rows_per_sample, int64_t row_step, double p, uint64_t seed, int dtype,
             DoParams* P) {
    UCF_CHECK_ARG(D > 0 && D < (1ll << 30), "%s: bad row width D=%lld", name, (long long)D);
    UCF_CHECK_ARG(rows_per_sample > 0, "%s: bad rows_per_sample=%lld", name, (long long)rows_per_sample);
    UCF_CHECK_ARG(rows >= 0 && rows < (1ll << 30), "%s: bad row count %lld", name, (long long)rows);
    UCF_CHECK_ARG(rows % rows_per_sample == 0, "%s: rows=%lld is not a multiple of rows_per_sample=%lld", name, (long long)rows,
                  (long long)rows_per_sample);
    const int rc = do_mask_check(name, rows, row_step, p, seed, false, P);
    if (rc != UCFVIT_OK) return rc;
    UCF_CHECK_ARG(DTYPE_OK(dtype), "%s: bad dtype %d", name, dtype);
    return UCFVIT_OK;
}

}  // namespace

extern "C" int ucfvit_dropout_add(const void* res, int64_t ldr, const void* branch, const float* s, void* out, int64_t rows, int64_t D,
                                  int64_t rows_per_sample, int64_t row_step, double p, uint64_t seed, int dtype, void* stream) {
    UCF_CHECK_ARG(res && branch && out, "ucfvit_dropout_add: null pointer");
    DoParams P;
    const int rc = do_check("ucfvit_dropout_add", rows, D, rows_per_sample, row_step, p, seed, dtype, &P);
    if (rc != UCFVIT_OK) return rc;
    UCF_CHECK_ARG(ldr >= D, "ucfvit_dropout_add: residual row stride ldr=%lld < D=%lld", (long long)ldr, (long long)D);
    if (rows == 0) return UCFVIT_OK;
    if (dtype == UCFVIT_F32)
        return do_launch<float, true>(res, ldr, branch, s, out, nullptr, rows, D, rows_per_sample, P, (hipStream_t)stream, "ucfvit_dropout_add");
    return do_launch<bf16, true>(res, ldr, branch, s, out, nullptr, rows, D, rows_per_sample, P, (hipStream_t)stream, "ucfvit_dropout_add");
}

extern "C" int ucfvit_dropout(const void* x, const float* s, void* out, float* colsum_partial, int64_t rows, int64_t D,
                              int64_t rows_per_sample, int64_t row_step, double p, uint64_t seed, int dtype, void* stream) {
    UCF_CHECK_ARG(x && out, "ucfvit_dropout: null pointer");
    DoParams P;
    const int rc = do_check("ucfvit_dropout", rows, D, rows_per_sample, row_step, p, seed, dtype, &P);
    if (rc != UCFVIT_OK) return rc;
    UCF_CHECK_ARG(rows > 0 || !colsum_partial, "ucfvit_dropout: no column sums of an empty input");
    if (rows == 0) return UCFVIT_OK;
    if (dtype == UCFVIT_F32)
        return do_launch<float, false>(nullptr, 0, x, s, out, colsum_partial, rows, D, rows_per_sample, P, (hipStream_t)stream, "ucfvit_dropout");
    return do_launch<bf16, false>(nullptr, 0, x, s, out, colsum_partial, rows, D, rows_per_sample, P, (hipStream_t)stream, "ucfvit_dropout");
}
