// QK-norm (the reference Attention's q_norm / k_norm, building_blocks.py:161): a LayerNorm over the dh elements of every (row, head) segment
// of the Q third and of the K third of the packed qkv buffer [rows][3][H][dh], between the qkv Linear and the attention core.  Two row passes:
//   qk_norm_fwd: y = (x - mean) * rstd * gamma + beta in place over the 2 H dh columns of Q and K (the V third is neither read nor written);
//                for training also a bit copy of the un-normalised Q and K [rows][2][H][dh] and the fp32 statistics [rows][2][H]
//   qk_norm_bwd: the LayerNorm backward per segment, in place over the Q and K thirds of dqkv, xhat = (saved - mean) * rstd recomputed
//                (the same bits whichever sums are asked for);
//                per row chunk the sums over rows and heads for dgamma_q, dbeta_q, dgamma_k, dbeta_k and the column sums of the values
//                written (the Q and K thirds of the qkv bias gradient), both folded by ucfvit_reduce_rows
// Geometry: lanes along the 2 H dh columns, 16 bytes per lane, so a segment lies in G = dh / W adjacent lanes (W = 8 bf16 or 4 fp32; G = 4 ...
// 32 divides 64, segments never straddle a wave) and its sums are xor butterflies over those lanes: every lane of a segment ends with the same
// bits.  The 4 waves of a workgroup take rows r, r+1, r+2, r+3 of their row chunk and step by 4, four rows in flight per lane (row_pass.h).
// gamma / beta are the fp32 master parameters [dh], shared by all heads: a lane loads the W of its columns once per column tile.  fp32
// arithmetic, biased variance from the centred values, one rounding to the output type.  No atomics: the backward sums are per lane in row
// order, then the 4 waves pairwise, then the heads of a column tile in ascending order, the tiles in ascending order.
#include "common.h"
#include "row_pass.h"

namespace {

#define DTYPE_OK(d) ((d) == UCFVIT_F32 || (d) == UCFVIT_BF16)

constexpr int64_t QKN_MAX_ROWS = (1ll << 31) - 4096;          // row indices are ints: chunk starts and the unrolled steps stay below 2^31

// rows in flight per lane in the backward kernel: two packs, two statistics and three sets of W accumulators per row; with four rows hipcc
// takes 180-256 VGPRs for the bf16 kernels with both sums (1-2 waves per SIMD), with two 111-115 (4 waves; profiles/qk_norm.md)
constexpr int QKN_BWD_UNROLL = 2;

// row chunks of the backward kernel (one workgroup each, all column tiles): 16 rows at least, at most 1024 workgroups
inline int qkn_chunks(int64_t rows) {
    int64_t c = (rows + 15) / 16;
    if (c > DP_MAX_CHUNKS) c = DP_MAX_CHUNKS;
    if (c < 1) c = 1;
    return (int)c;
}

template <int G> __device__ __forceinline__ float seg_sum(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one segment slice of one row: -> normalised pack, the segment's statistics
template <typename T, int DH>
__device__ __forceinline__ Pack<T, Vec16<T>::N> qkn_fwd_row(const Pack<T, Vec16<T>::N>& a, const float* gm, const float* bt, float eps, float& mu,
                                                            float& rs) {
    constexpr int W = Vec16<T>::N, G = DH / W;
    float x[W], s = 0.f, q = 0.f;
#pragma unroll
    for (int e = 0; e < W; ++e) x[e] = a.get(e), s += x[e];
    mu = seg_sum<G>(s) * (1.f / DH);
#pragma unroll
    for (int e = 0; e < W; ++e) x[e] -= mu, q = __builtin_fmaf(x[e], x[e], q);
    rs = rsqrtf(seg_sum<G>(q) * (1.f / DH) + eps);
    Pack<T, W> o;
#pragma unroll
    for (int e = 0; e < W; ++e) o.set(e, __builtin_fmaf(x[e] * rs, gm[e], bt[e]));
    return o;
}

template <typename T, int DH>
__global__ __launch_bounds__(DP_BLOCK) void qk_norm_fwd_kernel(T* qkv, const float* __restrict__ gq, const float* __restrict__ bq,
                                                               const float* __restrict__ gk, const float* __restrict__ bk, T* __restrict__ saved,
                                                               float* __restrict__ mean, float* __restrict__ rstd, int rows, int H, float eps,
                                                               int rows_per_chunk) {
    constexpr int W = Vec16<T>::N, G = DH / W;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int HD = H * DH, C2 = 2 * HD;
    const int64_t ld = 3 * (int64_t)HD;
    const int col = (blockIdx.x * 64 + lane) * W;
    const int r_begin = blockIdx.y * rows_per_chunk;
    const int r_end = min(rows, r_begin + rows_per_chunk);
    if (col >= C2) return;                                                 // whole segments leave: C2 % DH == 0 and G divides 64
    const bool isk = col >= HD;
    const int pos = col & (DH - 1), seg = col / DH;
    const float* __restrict__ gp = (isk ? gk : gq) + pos;
    const float* __restrict__ bp = (isk ? bk : bq) + pos;
    float gm[W], bt[W];
#pragma unroll
    for (int e = 0; e < W; ++e) gm[e] = gp[e], bt[e] = bp[e];
    const bool first = (lane & (G - 1)) == 0;                              // the lane that writes its segment's statistics
    int r = r_begin + wave;
    for (; r + (DP_UNROLL - 1) * DP_WAVES < r_end; r += DP_UNROLL * DP_WAVES) {
        Pack<T, W> a[DP_UNROLL];
#pragma unroll
        for (int u = 0; u < DP_UNROLL; ++u) a[u] = Pack<T, W>::load(qkv + (int64_t)(r + u * DP_WAVES) * ld + col);
#pragma unroll
        for (int u = 0; u < DP_UNROLL; ++u) {
            const int ru = r + u * DP_WAVES;
            float mu, rs;
            const Pack<T, W> o = qkn_fwd_row<T, DH>(a[u], gm, bt, eps, mu, rs);
            if (saved) {
                a[u].store(saved + (int64_t)ru * C2 + col);
                if (first) mean[(int64_t)ru * 2 * H + seg] = mu, rstd[(int64_t)ru * 2 * H + seg] = rs;
            }
            o.store(qkv + (int64_t)ru * ld + col);
        }
    }
    for (; r < r_end; r += DP_WAVES) {
        const Pack<T, W> a = Pack<T, W>::load(qkv + (int64_t)r * ld + col);
        float mu, rs;
        const Pack<T, W> o = qkn_fwd_row<T, DH>(a, gm, bt, eps, mu, rs);
        if (saved) {
            a.store(saved + (int64_t)r * C2 + col);
            if (first) mean[(int64_t)r * 2 * H + seg] = mu, rstd[(int64_t)r * 2 * H + seg] = rs;
        }
        o.store(qkv + (int64_t)r * ld + col);
    }
}

// one segment slice of one row of the backward pass; adds this row's terms to the lane's accumulators
template <typename T, int DH, bool PSUM, bool CSUM>
__device__ __forceinline__ Pack<T, Vec16<T>::N> qkn_bwd_row(const Pack<T, Vec16<T>::N>& dy, const Pack<T, Vec16<T>::N>& xs, const float* gm, float mu,
                                                            float rs, float* acc_g, float* acc_b, float* acc_c) {
    // The four instantiations (with / without each set of sums) must give dx the same bits.  Under -ffp-contract=fast hipcc fuses a product
    // into whichever additions use it, differently per instantiation (measured: dx off by one ulp where the column sums are taken, the
    // product rs * t fused into acc_c += dx).  So this file is compiled with -ffp-contract=off (Makefile, FLAGS_qk_norm) and the fmas
    // that are wanted are spelled out.  The two empty asm statements below are not part of that: they pin the two values that several
    // expressions share to a register where they are formed, which keeps hipcc from carrying both rows' products along (bf16 with both
    // sums: 162 -> 113 VGPRs, 3 -> 4 waves per SIMD; 0.104 -> 0.093 ms at the ViT-B stream).  Without them the bits are the same.
    constexpr int W = Vec16<T>::N, G = DH / W;
    float xh[W], g[W], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < W; ++e) {
        const float d = dy.get(e);
        xh[e] = (xs.get(e) - mu) * rs;
        g[e] = d * gm[e];
        asm("" : "+v"(g[e]));                                              // (register pressure only, see above)
        s1 += g[e];
        s2 = __builtin_fmaf(g[e], xh[e], s2);
        if (PSUM) acc_g[e] = __builtin_fmaf(d, xh[e], acc_g[e]), acc_b[e] += d;
    }
    const float c1 = seg_sum<G>(s1) * (1.f / DH), c2 = seg_sum<G>(s2) * (1.f / DH);
    Pack<T, W> o;
#pragma unroll
    for (int e = 0; e < W; ++e) {
        float dx = rs * __builtin_fmaf(-xh[e], c2, g[e] - c1);
        asm("" : "+v"(dx));                                                // (register pressure only, see above)
        if (CSUM) acc_c[e] += dx;
        o.set(e, dx);
    }
    return o;
}

// grid = row chunks; a workgroup walks the column tiles (64 lanes x 16 bytes) of its rows one after the other, so that the sums over the
// heads, which lie in different tiles, meet in one workgroup: one row of each partial per row chunk
template <typename T, int DH, bool PSUM, bool CSUM>
__global__ __launch_bounds__(DP_BLOCK) void qk_norm_bwd_kernel(T* dqkv, const T* __restrict__ saved, const float* __restrict__ gq,
                                                               const float* __restrict__ gk, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, float* __restrict__ ppart, float* __restrict__ cpart,
                                                               int rows, int H, int rows_per_chunk) {
    constexpr int W = Vec16<T>::N, G = DH / W, TILE = 64 * W;
    __shared__ float red[(PSUM ? 2 : 0) + (CSUM ? 1 : 0) + (PSUM || CSUM ? 0 : 1)][DP_WAVES][TILE];       // [dgamma, dbeta,] [colsum]
    __shared__ float ptot[4][DH];                                          // dgamma_q, dbeta_q, dgamma_k, dbeta_k of this row chunk
    constexpr int RC = PSUM ? 2 : 0;                                       // where the column sums lie in red
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int HD = H * DH, C2 = 2 * HD;
    const int64_t ld = 3 * (int64_t)HD;
    const int r_begin = blockIdx.x * rows_per_chunk;
    const int r_end = min(rows, r_begin + rows_per_chunk);
    if (PSUM)
        for (int i = tid; i < 4 * DH; i += DP_BLOCK) (&ptot[0][0])[i] = 0.f;
    for (int c0 = 0; c0 < C2; c0 += TILE) {
        const int col = c0 + lane * W;
        float acc_g[W], acc_b[W], acc_c[W];
#pragma unroll
        for (int e = 0; e < W; ++e) acc_g[e] = 0.f, acc_b[e] = 0.f, acc_c[e] = 0.f;
        if (col < C2) {
            const float* __restrict__ gp = (col >= HD ? gk : gq) + (col & (DH - 1));
            const int seg = col / DH;
            float gm[W];
#pragma unroll
            for (int e = 0; e < W; ++e) gm[e] = gp[e];
            int r = r_begin + wave;
            for (; r + (QKN_BWD_UNROLL - 1) * DP_WAVES < r_end; r += QKN_BWD_UNROLL * DP_WAVES) {
                Pack<T, W> a[QKN_BWD_UNROLL], b[QKN_BWD_UNROLL];
                float mu[QKN_BWD_UNROLL], rs[QKN_BWD_UNROLL];
#pragma unroll
                for (int u = 0; u < QKN_BWD_UNROLL; ++u) {
                    const int ru = r + u * DP_WAVES;
                    a[u] = Pack<T, W>::load(dqkv + (int64_t)ru * ld + col);
                    b[u] = Pack<T, W>::load(saved + (int64_t)ru * C2 + col);
                    mu[u] = mean[(int64_t)ru * 2 * H + seg];
                    rs[u] = rstd[(int64_t)ru * 2 * H + seg];
                }
#pragma unroll
                for (int u = 0; u < QKN_BWD_UNROLL; ++u)
                    qkn_bwd_row<T, DH, PSUM, CSUM>(a[u], b[u], gm, mu[u], rs[u], acc_g, acc_b, acc_c)
                        .store(dqkv + (int64_t)(r + u * DP_WAVES) * ld + col);
            }
            for (; r < r_end; r += DP_WAVES) {
                const Pack<T, W> a = Pack<T, W>::load(dqkv + (int64_t)r * ld + col), b = Pack<T, W>::load(saved + (int64_t)r * C2 + col);
                const float mu = mean[(int64_t)r * 2 * H + seg], rs = rstd[(int64_t)r * 2 * H + seg];
                qkn_bwd_row<T, DH, PSUM, CSUM>(a, b, gm, mu, rs, acc_g, acc_b, acc_c).store(dqkv + (int64_t)r * ld + col);
            }
        }
        if constexpr (!PSUM && !CSUM) continue;
#pragma unroll
        for (int e = 0; e < W; ++e) {
            if constexpr (PSUM) red[0][wave][lane * W + e] = acc_g[e], red[1][wave][lane * W + e] = acc_b[e];
            if constexpr (CSUM) red[RC][wave][lane * W + e] = acc_c[e];
        }
        __syncthreads();
        // the 4 waves pairwise; column j of the tile belongs to one thread, which leaves the sum in wave 0's place
        for (int j = tid; j < TILE; j += DP_BLOCK) {
            if constexpr (PSUM) {
                red[0][0][j] = (red[0][0][j] + red[0][1][j]) + (red[0][2][j] + red[0][3][j]);
                red[1][0][j] = (red[1][0][j] + red[1][1][j]) + (red[1][2][j] + red[1][3][j]);
            }
            if constexpr (CSUM)
                if (c0 + j < C2) cpart[(int64_t)blockIdx.x * C2 + c0 + j] = (red[RC][0][j] + red[RC][1][j]) + (red[RC][2][j] + red[RC][3][j]);
        }
        if constexpr (PSUM) {
            __syncthreads();
            // the heads of this tile in ascending order, on top of the tiles before it; entry i belongs to one thread
            for (int i = tid; i < 4 * DH; i += DP_BLOCK) {
                const int kind = i / DH, pos = i & (DH - 1);
                float t = ptot[kind][pos];
#pragma unroll
                for (int sg = 0; sg < TILE / DH; ++sg) {
                    const int c = c0 + sg * DH + pos;
                    if (c < C2 && (c >= HD) == (kind >= 2)) t += red[kind & 1][0][sg * DH + pos];
                }
                ptot[kind][pos] = t;
            }
        }
        __syncthreads();                                                   // before the next tile's accumulators overwrite red
    }
    if (PSUM)
        for (int i = tid; i < 4 * DH; i += DP_BLOCK) ppart[(int64_t)blockIdx.x * 4 * DH + i] = (&ptot[0][0])[i];
}

template <typename T, int DH>
int qkn_fwd_launch(void* qkv, const float* gq, const float* bq, const float* gk, const float* bk, void* saved, float* mean, float* rstd,
                   int64_t rows, int64_t H, float eps, hipStream_t st) {
    const int64_t C2 = 2 * H * DH;
    const int chunks = dp_chunks(rows, C2);
    const int rpc = (int)((rows + chunks - 1) / chunks);
    const dim3 grid((unsigned)((C2 / Vec16<T>::N + 63) / 64), chunks);
    hipLaunchKernelGGL((qk_norm_fwd_kernel<T, DH>), grid, dim3(DP_BLOCK), 0, st, (T*)qkv, gq, bq, gk, bk, (T*)saved, mean, rstd, (int)rows, (int)H,
                       eps, rpc);
    UCF_LAUNCH_CHECK("ucfvit_qk_norm_fwd");
    return UCFVIT_OK;
}

template <typename T, int DH, bool PSUM, bool CSUM>
int qkn_bwd_launch2(void* dqkv, const void* saved, const float* gq, const float* gk, const float* mean, const float* rstd, float* ppart,
                    float* cpart, int64_t rows, int64_t H, hipStream_t st) {
    const int chunks = qkn_chunks(rows);
    const int rpc = (int)((rows + chunks - 1) / chunks);
    hipLaunchKernelGGL((qk_norm_bwd_kernel<T, DH, PSUM, CSUM>), dim3(chunks), dim3(DP_BLOCK), 0, st, (T*)dqkv, (const T*)saved, gq, gk, mean, rstd,
                       ppart, cpart, (int)rows, (int)H, rpc);
    UCF_LAUNCH_CHECK("ucfvit_qk_norm_bwd");
    return UCFVIT_OK;
}

template <typename T, int DH>
int qkn_bwd_launch(void* dqkv, const void* saved, const float* gq, const float* gk, const float* mean, const float* rstd, float* ppart,
                   float* cpart, int64_t rows, int64_t H, hipStream_t st) {
    if (ppart && cpart) return qkn_bwd_launch2<T, DH, true, true>(dqkv, saved, gq, gk, mean, rstd, ppart, cpart, rows, H, st);
    if (ppart) return qkn_bwd_launch2<T, DH, true, false>(dqkv, saved, gq, gk, mean, rstd, ppart, cpart, rows, H, st);
    if (cpart) return qkn_bwd_launch2<T, DH, false, true>(dqkv, saved, gq, gk, mean, rstd, ppart, cpart, rows, H, st);
    return qkn_bwd_launch2<T, DH, false, false>(dqkv, saved, gq, gk, mean, rstd, ppart, cpart, rows, H, st);
}

// shared argument checks; before any HIP call
int qkn_check(const char* name, int64_t rows, int64_t H, int64_t dh, int dtype) {
    UCF_CHECK_ARG(dh == 32 || dh == 64 || dh == 128, "%s: bad head width dh=%lld (32, 64 or 128)", name, (long long)dh);
    UCF_CHECK_ARG(H >= 1 && 2 * H * dh < (1ll << 30), "%s: bad head count H=%lld", name, (long long)H);
    UCF_CHECK_ARG(rows >= 0 && rows < QKN_MAX_ROWS, "%s: bad row count %lld", name, (long long)rows);
    UCF_CHECK_ARG(DTYPE_OK(dtype), "%s: bad dtype %d", name, dtype);
    return UCFVIT_OK;
}

}  // namespace

extern "C" int64_t ucfvit_qk_norm_partial_rows(int64_t rows, int64_t H, int64_t dh) {
    if (rows <= 0 || rows >= QKN_MAX_ROWS || H < 1 || !(dh == 32 || dh == 64 || dh == 128) || 2 * H * dh >= (1ll << 30)) return 0;   // refused
    return qkn_chunks(rows);
}

extern "C" int ucfvit_qk_norm_fwd(void* qkv, const float* gamma_q, const float* beta_q, const float* gamma_k, const float* beta_k, void* saved_qk,
                                  float* mean, float* rstd, int64_t rows, int64_t H, int64_t dh, float eps, int dtype, void* stream) {
    UCF_CHECK_ARG(qkv, "ucfvit_qk_norm_fwd: null pointer");
    UCF_CHECK_ARG(gamma_q && beta_q && gamma_k && beta_k, "ucfvit_qk_norm_fwd: null parameter");
    UCF_CHECK_ARG((saved_qk != nullptr) == (mean != nullptr) && (mean != nullptr) == (rstd != nullptr),
                  "ucfvit_qk_norm_fwd: saved_qk, mean and rstd go together (all three or none)");
    const int rc = qkn_check("ucfvit_qk_norm_fwd", rows, H, dh, dtype);
    if (rc != UCFVIT_OK) return rc;
    UCF_CHECK_ARG(eps >= 0.f, "ucfvit_qk_norm_fwd: bad eps=%g", (double)eps);          // refuses NaN too
    UCF_CHECK_ARG(ucf_is_aligned16(qkv) && ucf_is_aligned16(saved_qk), "ucfvit_qk_norm_fwd: qkv and saved_qk must be 16-byte aligned");
    if (rows == 0) return UCFVIT_OK;
    const hipStream_t st = (hipStream_t)stream;
#define QKN_FWD(T, DH) return qkn_fwd_launch<T, DH>(qkv, gamma_q, beta_q, gamma_k, beta_k, saved_qk, mean, rstd, rows, H, eps, st)
    if (dtype == UCFVIT_F32) {
        if (dh == 32) QKN_FWD(float, 32);
        if (dh == 64) QKN_FWD(float, 64);
        QKN_FWD(float, 128);
    }
    if (dh == 32) QKN_FWD(bf16, 32);
    if (dh == 64) QKN_FWD(bf16, 64);
    QKN_FWD(bf16, 128);
#undef QKN_FWD
}

extern "C" int ucfvit_qk_norm_bwd(void* dqkv, const void* saved_qk, const float* gamma_q, const float* gamma_k, const float* mean,
                                  const float* rstd, float* param_partial, float* colsum_partial, int64_t rows, int64_t H, int64_t dh, int dtype,
                                  void* stream) {
    UCF_CHECK_ARG(dqkv && saved_qk && mean && rstd, "ucfvit_qk_norm_bwd: null pointer");
    UCF_CHECK_ARG(gamma_q && gamma_k, "ucfvit_qk_norm_bwd: null parameter");
    const int rc = qkn_check("ucfvit_qk_norm_bwd", rows, H, dh, dtype);
    if (rc != UCFVIT_OK) return rc;
    UCF_CHECK_ARG(ucf_is_aligned16(dqkv) && ucf_is_aligned16(saved_qk), "ucfvit_qk_norm_bwd: dqkv and saved_qk must be 16-byte aligned");
    UCF_CHECK_ARG(rows > 0 || (!param_partial && !colsum_partial), "ucfvit_qk_norm_bwd: no sums of an empty input");
    if (rows == 0) return UCFVIT_OK;
    const hipStream_t st = (hipStream_t)stream;
#define QKN_BWD(T, DH) return qkn_bwd_launch<T, DH>(dqkv, saved_qk, gamma_q, gamma_k, mean, rstd, param_partial, colsum_partial, rows, H, st)
    if (dtype == UCFVIT_F32) {
        if (dh == 32) QKN_BWD(float, 32);
        if (dh == 64) QKN_BWD(float, 64);
        QKN_BWD(float, 128);
    }
    if (dh == 32) QKN_BWD(bf16, 32);
    if (dh == 64) QKN_BWD(bf16, 64);
    QKN_BWD(bf16, 128);
#undef QKN_BWD
}
