// Stochastic depth (timm's DropPath(drop_prob, scale_by_keep=True), which the reference imports): every sample b of the batch carries
// one fp32 scale s[b] = mask_b / keep, drawn on the host side (B floats, no kernel); the two row-wise kernels here apply it.
//   drop_path_add  : out[r] = res[r] + s[r / rows_per_sample] * branch[r]     (forward of a residual branch)
//   drop_path_scale: out[r] = s[r / rows_per_sample] * x[r]                   (gradient of the branch; the stand-alone module)
// Both are bound by memory.  Geometry (that of colsum_kernel, csrc/norm.hip): lanes along D, a wave covers 64 x 16 B = 1 KiB of contiguous
// columns of one row, the 4 waves of a workgroup take rows r, r+1, r+2, r+3 of their row chunk and step by 4, four rows in flight per
// lane; grid = (column blocks, row chunks), the chunk count capped so that the bf16 ViT widths launch about 1024 workgroups and loop over
// the rest.  A row narrower than 1 KiB leaves lanes idle: the widths this runs at in earnest (768, 1024, 1280) fill one or two waves.
// A sample with s == 0 is never read: add copies res bit for bit, scale writes zeros (so a non-finite value in a dropped branch does not
// reach the stream, unlike timm's 0 * inf).
// The scale kernel can hand out fp32 column sums of the values it writes, taken before rounding: partial[chunk][D], one row per row
// chunk, each the fixed-order sum over the chunk's rows (per wave in row order, four rows folded pairwise per step, then the 4 waves
// pairwise).  ucfvit_reduce_rows folds the chunks; no atomics, the order depends on the shape alone.
#include "common.h"
#include "row_pass.h"

namespace {

#define DTYPE_OK(d) ((d) == UCFVIT_F32 || (d) == UCFVIT_BF16)

// ADD: out = res + s * branch (x = branch, res with row stride ldr); else out = s * x.  out may alias x: every lane reads its elements
// of a row before it writes them, and no other lane touches them.
template <typename T, int W, bool ADD>
__global__ __launch_bounds__(DP_BLOCK) void drop_path_kernel(const T* res, int64_t ldr, const T* x, const float* __restrict__ s, T* out,
                                                             float* __restrict__ partial, int rows, int D, int rows_per_sample,
                                                             int rows_per_chunk) {
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
            float sc[DP_UNROLL];
            Pack<T, W> a[DP_UNROLL], b[DP_UNROLL];
#pragma unroll
            for (int u = 0; u < DP_UNROLL; ++u) {
                const int ru = r + u * DP_WAVES;
                sc[u] = s[(unsigned)ru / (unsigned)rows_per_sample];
                if (ADD) a[u] = Pack<T, W>::load(res + (int64_t)ru * ldr + col);
                if (sc[u] != 0.f) b[u] = Pack<T, W>::load(x + (int64_t)ru * D + col);
            }
            float t[DP_UNROLL][W];
#pragma unroll
            for (int u = 0; u < DP_UNROLL; ++u) {
                Pack<T, W> o;
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    t[u][e] = sc[u] != 0.f ? sc[u] * b[u].get(e) : 0.f;
                    o.set(e, ADD ? a[u].get(e) + t[u][e] : t[u][e]);
                }
                if (ADD && sc[u] == 0.f) o = a[u];                         // the residual's own bits
                o.store(out + (int64_t)(r + u * DP_WAVES) * D + col);
            }
            if (partial) {
#pragma unroll
                for (int e = 0; e < W; ++e) acc[e] += (t[0][e] + t[1][e]) + (t[2][e] + t[3][e]);
            }
        }
        for (; r < r_end; r += DP_WAVES) {
            const float sc = s[(unsigned)r / (unsigned)rows_per_sample];
            Pack<T, W> a, b, o;
            if (ADD) a = Pack<T, W>::load(res + (int64_t)r * ldr + col);
            if (sc != 0.f) b = Pack<T, W>::load(x + (int64_t)r * D + col);
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const float t = sc != 0.f ? sc * b.get(e) : 0.f;
                o.set(e, ADD ? a.get(e) + t : t);
                acc[e] += t;
            }
            if (ADD && sc == 0.f) o = a;
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
int dp_launch(const void* res, int64_t ldr, const void* x, const float* s, void* out, float* partial, int64_t rows, int64_t D,
              int64_t rows_per_sample, hipStream_t st, const char* name) {
    constexpr int EPV = Vec16<T>::N;
    const bool vec = D % EPV == 0 && ucf_is_aligned16(x) && ucf_is_aligned16(out) && (!ADD || (ldr % EPV == 0 && ucf_is_aligned16(res)));
    const int chunks = dp_chunks(rows, D);
    const int rpc = (int)((rows + chunks - 1) / chunks);
    if (vec) {
        const dim3 grid((unsigned)((D / EPV + 63) / 64), chunks);
        hipLaunchKernelGGL((drop_path_kernel<T, EPV, ADD>), grid, dim3(DP_BLOCK), 0, st, (const T*)res, ldr, (const T*)x, s, (T*)out, partial,
                           (int)rows, (int)D, (int)rows_per_sample, rpc);
    } else {
        const dim3 grid((unsigned)((D + 63) / 64), chunks);
        hipLaunchKernelGGL((drop_path_kernel<T, 1, ADD>), grid, dim3(DP_BLOCK), 0, st, (const T*)res, ldr, (const T*)x, s, (T*)out, partial,
                           (int)rows, (int)D, (int)rows_per_sample, rpc);
    }
    UCF_LAUNCH_CHECK(name);
    return UCFVIT_OK;
}

// shared argument checks; before any HIP call
int dp_check(const char* name, int64_t rows, int64_t D, int64_t rows_per_sample, int dtype) {
    UCF_CHECK_ARG(D > 0 && D < (1ll << 30), "%s: bad row width D=%lld", name, (long long)D);
    UCF_CHECK_ARG(rows_per_sample > 0, "%s: bad rows_per_sample=%lld", name, (long long)rows_per_sample);
    UCF_CHECK_ARG(rows >= 0 && rows < (1ll << 30), "%s: bad row count %lld", name, (long long)rows);
    UCF_CHECK_ARG(rows % rows_per_sample == 0, "%s: rows=%lld is not a multiple of rows_per_sample=%lld", name, (long long)rows,
                  (long long)rows_per_sample);
    UCF_CHECK_ARG(DTYPE_OK(dtype), "%s: bad dtype %d", name, dtype);
    return UCFVIT_OK;
}

}  // namespace

extern "C" int64_t ucfvit_drop_path_colsum_rows(int64_t rows, int64_t rows_per_sample, int64_t D) {
    if (rows <= 0 || rows_per_sample <= 0 || D <= 0 || rows >= (1ll << 30) || D >= (1ll << 30)) return 0;    // what the kernels refuse
    return dp_chunks(rows, D);
}

extern "C" int ucfvit_drop_path_add(const void* res, int64_t ldr, const void* branch, const float* s, void* out, int64_t rows, int64_t D,
                                    int64_t rows_per_sample, int dtype, void* stream) {
    UCF_CHECK_ARG(res && branch && s && out, "ucfvit_drop_path_add: null pointer");
    const int rc = dp_check("ucfvit_drop_path_add", rows, D, rows_per_sample, dtype);
    if (rc != UCFVIT_OK) return rc;
    UCF_CHECK_ARG(ldr >= D, "ucfvit_drop_path_add: residual row stride ldr=%lld < D=%lld", (long long)ldr, (long long)D);
    if (rows == 0) return UCFVIT_OK;
    if (dtype == UCFVIT_F32)
        return dp_launch<float, true>(res, ldr, branch, s, out, nullptr, rows, D, rows_per_sample, (hipStream_t)stream, "ucfvit_drop_path_add");
    return dp_launch<bf16, true>(res, ldr, branch, s, out, nullptr, rows, D, rows_per_sample, (hipStream_t)stream, "ucfvit_drop_path_add");
}

extern "C" int ucfvit_drop_path_scale(const void* x, const float* s, void* out, float* colsum_partial, int64_t rows, int64_t D,
                                      int64_t rows_per_sample, int dtype, void* stream) {
    UCF_CHECK_ARG(x && s && out, "ucfvit_drop_path_scale: null pointer");
    const int rc = dp_check("ucfvit_drop_path_scale", rows, D, rows_per_sample, dtype);
    if (rc != UCFVIT_OK) return rc;
    UCF_CHECK_ARG(rows > 0 || !colsum_partial, "ucfvit_drop_path_scale: no column sums of an empty input");
    if (rows == 0) return UCFVIT_OK;
    if (dtype == UCFVIT_F32)
        return dp_launch<float, false>(nullptr, 0, x, s, out, colsum_partial, rows, D, rows_per_sample, (hipStream_t)stream,
                                       "ucfvit_drop_path_scale");
    return dp_launch<bf16, false>(nullptr, 0, x, s, out, colsum_partial, rows, D, rows_per_sample, (hipStream_t)stream,
                                  "ucfvit_drop_path_scale");
}
