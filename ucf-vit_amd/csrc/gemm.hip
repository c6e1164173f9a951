// GEMM with fused epilogue for gfx950: C[M,N] = epi(alpha * op(A)·op(B)).
//
// v1 structure ("register-staged, one LDS image per operand"):
//   128x128 output tile per 256-thread workgroup (4 waves as 2x2, 64x64 per wave = 4x4 MFMA 16x16 fragments),
//   K-tile = 128 bytes of the contraction index (64 bf16 / 32 fp32).  Global->VGPR loads of K-tile t+1 are issued
//   before the MFMA phase of tile t and written to LDS after the barrier (issue-early / write-late).
//   MFMA: v_mfma_f32_16x16x32_bf16 (bf16) or v_mfma_f32_16x16x4_f32 (exact fp32).
//   Operands are staged in their natural memory layout with 16-byte coalesced loads:
//     KC (contraction contiguous): LDS image [128 rows][128 B], 16-B slots XOR-swizzled by (row&7); fragments by ds_read_b128
//     KS (contraction strided)   : LDS image [k][128 rows], 32-B groups XOR-swizzled; fragments by ds_read_b64_tr_b16
//                                  (bf16, hardware transpose) or 4 ds_read_b32 (fp32)
//   The MFMA is issued with the operand roles swapped (D = Btile·Atileᵀ) so each lane ends up holding 4 CONSECUTIVE
//   output columns of one output row: bias/residual/aux are read and C is written with 8/16-byte vectors.
//
// Requirements of the MFMA path (checked on the host; anything else goes to the scalar fallback kernel):
//   16-byte aligned base pointers, leading dimensions and the contiguous extent of each operand multiples of 16 bytes.
#include <stdlib.h>

#include "gemm_epi.h"
#include "gemm_route.h"
#include "gemm_tile.h"

namespace {

constexpr int BM = 128, BN = 128, NTHREADS = 256;
constexpr int TILE_BYTES = 16384;  // one operand K-tile: 128 rows x 128 B (KC) or BK k-rows x (128 elems) (KS)

template <typename T> struct MmaT;
template <> struct MmaT<bf16> {
    static constexpr int BK = 64;      // contraction elements per K-tile
    static constexpr int EPV = 8;      // elements per 16 bytes
    static constexpr int KCHUNK = 32;  // contraction elements consumed per fragment pair
    typedef bf16x8 frag_t;
    static __device__ __forceinline__ void mma(f32x4& acc, const frag_t& a, const frag_t& b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    }
};
template <> struct MmaT<float> {
    static constexpr int BK = 32;
    static constexpr int EPV = 4;
    static constexpr int KCHUNK = 16;
    typedef f32x4 frag_t;
    static __device__ __forceinline__ void mma(f32x4& acc, const frag_t& a, const frag_t& b) {
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
    }
};

// ---- LDS image addressing (KC image and the bf16 KS swizzle: gemm_tile.h) ---------------------------
// KS image, bf16: k-row = 128 elems = 256 B
__device__ __forceinline__ int ks_off_bf16(int krow, int colbyte) { return krow * 256 + (colbyte ^ ks_swz(krow)); }
// KS image, fp32: k-row = 128 elems = 512 B
__device__ __forceinline__ int ks_off_f32(int krow, int colbyte) { return krow * 512 + (colbyte ^ (((krow >> 2) & 1) << 6)); }

template <typename T> struct Stage {  // 4 x 16 B per thread per operand K-tile
    u32x4 v[4];
};

// Global -> registers for one operand K-tile.  R = extent of the operand's row/col index, K = contraction extent.
template <typename T, int LAYOUT>
__device__ __forceinline__ void stage_load(Stage<T>& st, const T* __restrict__ base, int64_t ld, int r0, int k0, int R, int K,
                                           int tid) {
    constexpr int EPV = MmaT<T>::EPV;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = tid + i * NTHREADS;
        int64_t off;
        bool ok;
        if (LAYOUT == UCFVIT_LAYOUT_KC) {
            const int row = p >> 3, slot = p & 7;
            const int k = k0 + slot * EPV;
            ok = (r0 + row < R) && (k < K);
            off = (int64_t)(r0 + row) * ld + k;
        } else {
            constexpr int PPR = 128 / EPV;  // 16-B pieces per k-row
            const int krow = p / PPR, piece = p % PPR;
            const int r = r0 + piece * EPV;
            ok = (k0 + krow < K) && (r < R);
            off = (int64_t)(k0 + krow) * ld + r;
        }
        u32x4 z = {0u, 0u, 0u, 0u};
        st.v[i] = ok ? *reinterpret_cast<const u32x4*>(base + off) : z;
    }
}

template <typename T, int LAYOUT>
__device__ __forceinline__ void stage_store(const Stage<T>& st, char* lds, int tid) {
    constexpr int EPV = MmaT<T>::EPV;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = tid + i * NTHREADS;
        int off;
        if (LAYOUT == UCFVIT_LAYOUT_KC) {
            off = kc_off(p >> 3, p & 7);
        } else {
            constexpr int PPR = 128 / EPV;
            const int krow = p / PPR, piece = p % PPR;
            off = (sizeof(T) == 2) ? ks_off_bf16(krow, piece * 16) : ks_off_f32(krow, piece * 16);
        }
        *reinterpret_cast<u32x4*>(lds + off) = st.v[i];
    }
}

// Fragment of the 16 rows [rbase, rbase+16) for k-chunk `c` of the K-tile.
template <typename T, int LAYOUT>
__device__ __forceinline__ typename MmaT<T>::frag_t load_frag(const char* lds, int rbase, int c, int lane) {
    typedef typename MmaT<T>::frag_t frag_t;
    const int g = lane >> 4, i = lane & 15;
    if constexpr (LAYOUT == UCFVIT_LAYOUT_KC) {
        return kc_frag<frag_t>(lds, rbase, c, lane);
    } else if constexpr (sizeof(T) == 2) {
        // two hardware-transposed reads: k-rows kb+{0..3} and kb+4+{0..3}, columns rbase..rbase+15;
        // lane 4q+p of each 16-lane group supplies the address of k-row q, columns 4p..4p+3.
        const int kb = 32 * c + 8 * g, q = i >> 2, p = i & 3;
        const int colbyte = (rbase + 4 * p) * 2;
        short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(short4v, lds + ks_off_bf16(kb + q, colbyte)));
        short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(short4v, lds + ks_off_bf16(kb + 4 + q, colbyte)));
        short8v r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(frag_t, r);
    } else {
        const int kb = 16 * c + 4 * g;
        const int colbyte = (rbase + i) * 4;
        f32x4 r;
#pragma unroll
        for (int s = 0; s < 4; ++s) r[s] = *reinterpret_cast<const float*>(lds + ks_off_f32(kb + s, colbyte));
        return __builtin_bit_cast(frag_t, r);
    }
}

struct EpiArgs {
    const void* bias;
    const void* residual;
    const void* aux_in;
    void* aux_out;
    int64_t ldc, ldr, ldaux;
    int act, accumulate;
    float alpha;
};

template <typename T, typename OutT, int LA, int LB>
__global__ __launch_bounds__(NTHREADS) void gemm_mfma_kernel(const T* __restrict__ A, const T* __restrict__ B,
                                                              OutT* __restrict__ C, int M, int N, int K, int64_t lda,
                                                              int64_t ldb, EpiArgs ep, int tiles_m, int tiles_n) {
    typedef MmaT<T> MM;
    typedef typename MM::frag_t frag_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ldsA = smem;
    char* ldsB = smem + TILE_BYTES;

    // XCD-aware tile order: each XCD label gets a contiguous run of tiles; inside a run, tiles walk down M within a
    // band of 8 N-tiles so neighbouring workgroups share the B panel and successive ones reuse the A panel from L2.
    const int nwg = tiles_m * tiles_n;
    const int t = xcd_remap(blockIdx.x, nwg);
    constexpr int BAND = 8;
    const int band_tiles = BAND * tiles_m;
    const int band = t / band_tiles;
    const int band_w = min(BAND, tiles_n - band * BAND);
    const int in_band = t - band * band_tiles;
    const int tm = in_band / band_w;
    const int tn = band * BAND + in_band % band_w;
    const int m0 = tm * BM, n0 = tn * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = (K + MM::BK - 1) / MM::BK;
    Stage<T> sa, sb;
    stage_load<T, LA>(sa, A, lda, m0, 0, M, K, tid);
    stage_load<T, LB>(sb, B, ldb, n0, 0, N, K, tid);

    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();  // everyone finished reading the previous tile's LDS image
        stage_store<T, LA>(sa, ldsA, tid);
        stage_store<T, LB>(sb, ldsB, tid);
        __syncthreads();
        if (kt + 1 < nk) {  // next tile's loads fly under this tile's MFMAs
            stage_load<T, LA>(sa, A, lda, m0, (kt + 1) * MM::BK, M, K, tid);
            stage_load<T, LB>(sb, B, ldb, n0, (kt + 1) * MM::BK, N, K, tid);
        }
#pragma unroll
        for (int c = 0; c < MM::BK / MM::KCHUNK; ++c) {
            frag_t fa[4], fb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) fa[i] = load_frag<T, LA>(ldsA, wm + 16 * i, c, lane);
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[j] = load_frag<T, LB>(ldsB, wn + 16 * j, c, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) MM::mma(acc[i][j], fb[j], fa[i]);  // roles swapped: D[n][m]
        }
    }

    // Epilogue.  acc[i][j][r] = C[m0+wm+16i+(lane&15)][n0+wn+16j+4*(lane>>4)+r]
    const int g = lane >> 4, li = lane & 15;
    const T* bias = (const T*)ep.bias;
    const T* res = (const T*)ep.residual;
    const T* auxi = (const T*)ep.aux_in;
    T* auxo = (T*)ep.aux_out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm + 16 * i + li;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn + 16 * j + 4 * g;
            if (n >= N) continue;  // N % 4 == 0 on this path, so the 4 columns are all in range
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = ep.alpha * acc[i][j][r];
            if (bias) {
                Vec4<T> b = *reinterpret_cast<const Vec4<T>*>(bias + n);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += b.get(r);
            }
            EPI_V1_ACT(4, Vec4<T>, ep.act, v, auxi, auxo, ep.ldaux, m, n);
            if (res) {
                Vec4<T> rr = *reinterpret_cast<const Vec4<T>*>(res + (int64_t)m * ep.ldr + n);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += rr.get(r);
            }
            OutT* cp = C + (int64_t)m * ep.ldc + n;
            if (ep.accumulate) {
                Vec4<OutT> old = *reinterpret_cast<const Vec4<OutT>*>(cp);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += old.get(r);
            }
            Vec4<OutT> o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o.set(r, v[r]);
            *reinterpret_cast<Vec4<OutT>*>(cp) = o;
        }
    }
}

// Scalar fallback for tiny / unaligned shapes (e.g. a 2-class head): one thread per output element.
template <typename T, typename OutT>
__global__ void gemm_scalar_kernel(const T* __restrict__ A, const T* __restrict__ B, OutT* __restrict__ C, int64_t M,
                                   int64_t N, int64_t K, int64_t lda, int64_t ldb, int la, int lb, EpiArgs ep) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * N) return;
    const int64_t m = idx / N, n = idx % N;
    float acc = 0.f;
    for (int64_t k = 0; k < K; ++k) {
        const float a = to_f32<T>(la == UCFVIT_LAYOUT_KC ? A[m * lda + k] : A[k * lda + m]);
        const float b = to_f32<T>(lb == UCFVIT_LAYOUT_KC ? B[n * ldb + k] : B[k * ldb + n]);
        acc = fmaf(a, b, acc);
    }
    float v = ep.alpha * acc;
    if (ep.bias) v += to_f32<T>(((const T*)ep.bias)[n]);
    EPI_V1_ACT(1, Vec1<T>, ep.act, (&v), (const T*)ep.aux_in, (T*)ep.aux_out, ep.ldaux, m, n);
    if (ep.residual) v += to_f32<T>(((const T*)ep.residual)[m * ep.ldr + n]);
    OutT* cp = C + m * ep.ldc + n;
    if (ep.accumulate) v += to_f32<OutT>(*cp);
    *cp = from_f32<OutT>(v);
}

template <typename T, typename OutT, int LA, int LB>
int launch_mfma(const ucfvit_gemm_desc* d, const EpiArgs& ep, hipStream_t s) {
    const int tiles_m = (int)((d->M + BM - 1) / BM), tiles_n = (int)((d->N + BN - 1) / BN);
    const int nwg = tiles_m * tiles_n;
    hipLaunchKernelGGL((gemm_mfma_kernel<T, OutT, LA, LB>), dim3(nwg), dim3(NTHREADS), 2 * TILE_BYTES, s, (const T*)d->A,
                       (const T*)d->B, (OutT*)d->C, (int)d->M, (int)d->N, (int)d->K, d->lda, d->ldb, ep, tiles_m, tiles_n);
    UCF_LAUNCH_CHECK("ucfvit_gemm(mfma)");
    return UCFVIT_OK;
}

template <typename T, typename OutT>
int launch_v1(const ucfvit_gemm_desc* d, bool mfma, hipStream_t s) {
    const EpiArgs ep = {d->bias, d->residual, d->aux_in, d->aux_out, d->ldc, d->ldr, d->ldaux, d->act, d->accumulate, d->alpha};
    const int la = d->a_layout, lb = d->b_layout;
    if (mfma) {
        return gemm_with_layouts(la, lb, [&](auto la_c, auto lb_c) {
            return launch_mfma<T, OutT, decltype(la_c)::value, decltype(lb_c)::value>(d, ep, s);
        });
    }
    const int64_t total = d->M * d->N;
    const int64_t blocks = (total + 255) / 256;
    UCF_CHECK_ARG(blocks < (1ll << 31), "ucfvit_gemm: scalar fallback grid too large (M=%lld N=%lld)", (long long)d->M,
                  (long long)d->N);
    hipLaunchKernelGGL((gemm_scalar_kernel<T, OutT>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)d->A, (const T*)d->B,
                       (OutT*)d->C, d->M, d->N, d->K, d->lda, d->ldb, la, lb, ep);
    UCF_LAUNCH_CHECK("ucfvit_gemm(scalar)");
    return UCFVIT_OK;
}

// UCFVIT_GEMM_STAGGER — a TEST / measurement hook: 0 keeps every launch on gemm3_kernel (tests/test_hip_ops.py compares the dynamic tile
// schedule with the static order of the SAME kernel; tools/block_gemm_bench.py A/B), 1 / 2 / 4 / 8 force the number of epilogue steps
// (tests/test_gemm_stagger.py runs every variant).  Read once (thread-safe static).
int stagger_override() {
    static const int v = [] {
        const char* e = getenv("UCFVIT_GEMM_STAGGER");
        return e ? atoi(e) : -1;
    }();
    return v;
}

}  // namespace

int ucfvit_gemm_launch_v1(const ucfvit_gemm_desc* d, const GemmRoute& r, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const bool mfma = r.kernel == GK_V1_MFMA;
    if (d->dtype == UCFVIT_F32) {
        UCF_CHECK_ARG(d->out_dtype == UCFVIT_F32, "ucfvit_gemm: f32 inputs require f32 output");
        return launch_v1<float, float>(d, mfma, s);
    } else if (d->dtype == UCFVIT_BF16) {
        if (d->out_dtype == UCFVIT_BF16) return launch_v1<bf16, bf16>(d, mfma, s);
        if (d->out_dtype == UCFVIT_F32) return launch_v1<bf16, float>(d, mfma, s);
    }
    ucfvit_set_error("ucfvit_gemm: unsupported dtype combination (%d -> %d)", d->dtype, d->out_dtype);
    return UCFVIT_ERR_UNSUPPORTED;
}

extern "C" int ucfvit_gemm(const ucfvit_gemm_desc* d, void* stream) {
    UCF_CHECK_ARG(d != nullptr, "ucfvit_gemm: null descriptor");
    if (d->M == 0 || d->N == 0) return UCFVIT_OK;      // empty batch / empty output: nothing to write (pointers may be NULL)
    UCF_CHECK_ARG(d->A && d->B && d->C, "ucfvit_gemm: null operand pointer");
    UCF_CHECK_ARG(d->M >= 0 && d->N >= 0 && d->K >= 0, "ucfvit_gemm: negative size");
    UCF_CHECK_ARG(d->a_layout == 0 || d->a_layout == 1, "ucfvit_gemm: bad a_layout %d", d->a_layout);
    UCF_CHECK_ARG(d->b_layout == 0 || d->b_layout == 1, "ucfvit_gemm: bad b_layout %d", d->b_layout);
    UCF_CHECK_ARG(d->act >= 0 && d->act <= 4, "ucfvit_gemm: bad act %d", d->act);
    UCF_CHECK_ARG((d->act != UCFVIT_ACT_GELU_GRAD && d->act != UCFVIT_ACT_MUL_AUX) || d->aux_in, "ucfvit_gemm: act %d needs aux_in", d->act);
    UCF_CHECK_ARG(d->act != UCFVIT_ACT_GELU_SAVE_DERIV || d->aux_out, "ucfvit_gemm: ACT_GELU_SAVE_DERIV needs aux_out");
    UCF_CHECK_ARG(d->lda >= ((d->a_layout == 0) ? d->K : d->M), "ucfvit_gemm: lda too small");
    UCF_CHECK_ARG(d->ldb >= ((d->b_layout == 0) ? d->K : d->N), "ucfvit_gemm: ldb too small");
    UCF_CHECK_ARG(d->ldc >= d->N, "ucfvit_gemm: ldc too small");
    const GemmRoute r = gemm_route(d, stagger_override());
    if (d->c_colsum_partial && (r.colsum_rows == 0 || !ucf_is_aligned16(d->c_colsum_partial))) {
        ucfvit_set_error("ucfvit_gemm: c_colsum_partial is not available for this problem (ask ucfvit_gemm_colsum_rows first)");
        return UCFVIT_ERR_UNSUPPORTED;
    }
    switch (r.kernel) {
        case GK_V1_SCALAR:
        case GK_V1_MFMA: return ucfvit_gemm_launch_v1(d, r, stream);
        case GK_STAGGER: return ucfvit_gemm_launch_stagger(d, r, stream);
        default: return ucfvit_gemm_launch_dma(d, r, stream);
    }
}

// The three route queries: host only, no HIP call; all of them answer from the route ucfvit_gemm itself would take.
extern "C" int64_t ucfvit_gemm_workspace(const ucfvit_gemm_desc* d) { return d ? gemm_route(d, stagger_override()).workspace_bytes : 0; }

extern "C" int64_t ucfvit_gemm_colsum_rows(const ucfvit_gemm_desc* d) { return d ? gemm_route(d, stagger_override()).colsum_rows : 0; }

extern "C" int ucfvit_gemm_route(const ucfvit_gemm_desc* d, char* out, int64_t cap) {
    UCF_CHECK_ARG(d && out && cap > 0, "ucfvit_gemm_route: null descriptor or no room for the text");
    return gemm_route_name(gemm_route(d, stagger_override()), out, cap);
}
