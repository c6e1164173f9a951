// The epilogue steps the GEMM translation units share (gemm.hip, gemm2.hip, gemm_stagger.hip), one definition each: the order that
// include/ucfvit_hip.h fixes (alpha * acc, + bias, activation, + residual, + C_old, one rounding) is written here.
//   EPI_STAGE_STRIP + epi_finish8 : the generic LDS-staged epilogue of the bf16 DMA kernels (gemm2_kernel, gemm3_kernel<EPI_GENERIC>);
//                                   epi_finish8 holds the run-time activation step of that path (fast GELU forms), 8 columns per lane
//   EPI_V1_ACT                    : the activation step of gemm_mfma_kernel and gemm_scalar_kernel (erf-based GELU), 4 or 1 columns
//   EPI_COLSUM_FOLD               : the column sums gemm3_kernel and gemm5_kernel hand to ucfvit_reduce_rows
// and the two launch helpers every GEMM launcher uses (gemm_with_layouts, gemm_raise_lds).
// Three of them are macros in the idiom of PP_READ: a function is optimised on its own before it is inlined, and every function form
// of these three changed register counts, scratch sizes or opcode counts of the kernels (profiles/gemm_epilogue_refactor.md).
#pragma once
#include <type_traits>

#include "common.h"

// C / aux tiles are written once and not read again by this kernel: stored with the non-temporal hint, the dirty lines leave L2 as the
// K loop's fills need the ways instead of in one write-back burst one L2 turnover later (4 MB of C per XCD and tile round).
#ifndef UCFVIT_GEMM_STORE_TEMPORAL
__device__ __forceinline__ void store_out16(bf16* p, const Vec16<bf16>& o) { __builtin_nontemporal_store(o.v, reinterpret_cast<bf16x8*>(p)); }
#else
__device__ __forceinline__ void store_out16(bf16* p, const Vec16<bf16>& o) { *reinterpret_cast<Vec16<bf16>*>(p) = o; }
#endif

namespace {      // (a kernel-argument type: kept file-local, as the kernels that take it are)
struct Epi2 {
    const bf16* bias;
    const bf16* residual;
    const bf16* aux_in;
    bf16* aux_out;
    int64_t ldc, ldr, ldaux;
    int act, accumulate;
    float alpha;
    float* slab;       // split-K: fp32 partial matrices [splits][M][N] (ld = N); NULL when gridDim.y == 1
    float* cs_partial; // column sums of the output per 128-row block: [2 * tiles_m][N] (CS instantiations only), or NULL
    unsigned* sched;   // dynamic tile schedule of the persistent 256x256 kernel (desc->sched_state), or NULL: static round-robin
};
}  // namespace

// ---- the generic epilogue of the DMA kernels (gemm2_kernel, gemm3_kernel<EPI_GENERIC>) -----------------------------------------------
// Per-lane finish of 8 columns (lo, hi: by value, an array handed over by reference is optimised as memory before it is inlined):
// split-K slab store, or activation / aux / residual / accumulate and one 16-byte (bf16) or two 16-byte (fp32) stores.
template <typename OutT>
__device__ __forceinline__ void epi_finish8(const f32x4 lo, const f32x4 hi, const Epi2& ep, OutT* C, int64_t ldc, int accum, float* slab,
                                            int m, int n, int N) {
    if (slab) {
        *reinterpret_cast<f32x4*>(slab + (int64_t)m * N + n) = lo;
        *reinterpret_cast<f32x4*>(slab + (int64_t)m * N + n + 4) = hi;
        return;
    }
    float v[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        v[r] = lo[r];
        v[4 + r] = hi[r];
    }
    if (ep.act == UCFVIT_ACT_GELU) {
        if (ep.aux_out) {
            Vec16<bf16> o;
#pragma unroll
            for (int r = 0; r < 8; ++r) o.set(r, v[r]);
            store_out16(ep.aux_out + (int64_t)m * ep.ldaux + n, o);
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = o.get(r);   // activation sees the stored (rounded) pre-activation
        }
        gelu_fast8(v);
    } else if (ep.act == UCFVIT_ACT_GELU_GRAD) {
        const Vec16<bf16> h = *reinterpret_cast<const Vec16<bf16>*>(ep.aux_in + (int64_t)m * ep.ldaux + n);
        float hf[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) hf[r] = h.get(r);
        gelu_grad_fast8(v, hf);
    } else if (ep.act == UCFVIT_ACT_GELU_SAVE_DERIV) {
        float df[8];
        gelu_and_grad_fast8(v, df);
        Vec16<bf16> o;
#pragma unroll
        for (int r = 0; r < 8; ++r) o.set(r, df[r]);
        store_out16(ep.aux_out + (int64_t)m * ep.ldaux + n, o);
    } else if (ep.act == UCFVIT_ACT_MUL_AUX) {
        const Vec16<bf16> h = *reinterpret_cast<const Vec16<bf16>*>(ep.aux_in + (int64_t)m * ep.ldaux + n);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] *= h.get(r);
    }
    if (ep.residual) {
        const Vec16<bf16> rv = *reinterpret_cast<const Vec16<bf16>*>(ep.residual + (int64_t)m * ep.ldr + n);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] += rv.get(r);
    }
    OutT* cp = C + (int64_t)m * ldc + n;
    if constexpr (sizeof(OutT) == 2) {
        if (accum) {
            const Vec16<bf16> old = *reinterpret_cast<const Vec16<bf16>*>(cp);
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] += old.get(r);
        }
        Vec16<bf16> o;
#pragma unroll
        for (int r = 0; r < 8; ++r) o.set(r, v[r]);
        store_out16(cp, o);
    } else {
        f32x4 o0, o1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o0[r] = v[r];
            o1[r] = v[4 + r];
        }
        if (accum) {
            o0 += *reinterpret_cast<const f32x4*>(cp);
            o1 += *reinterpret_cast<const f32x4*>(cp + 4);
        }
        *reinterpret_cast<f32x4*>(cp) = o0;
        *reinterpret_cast<f32x4*>(cp + 4) = o1;
    }
}

// Phase A of that epilogue: v = alpha*acc + bias (fp32) of one 16-row x 16 FN-col strip (acc_ = acc[i]) -> the wave-private LDS rows
// `stage` (PADW words per row); split-K partial sums (slab) are staged as they are.  nw_ = first column of the wave's sub-tile; FN, PADW,
// g = lane >> 4, li = lane & 15 and N are the kernel's.  (As a function, strip by reference or the whole epilogue with the accumulators
// by reference, the kernels came out with other register and scratch sizes.)
#define EPI_STAGE_STRIP(acc_, stage_, ep_, slab_, nw_)                                             \
    do {                                                                                           \
        _Pragma("unroll") for (int j = 0; j < FN; ++j) {                                           \
            f32x4 v = (acc_)[j];                                                                   \
            if (!(slab_)) {                                                                        \
                const int n = (nw_) + 16 * j + 4 * g;                                              \
                _Pragma("unroll") for (int r = 0; r < 4; ++r) v[r] *= (ep_).alpha;                 \
                if ((ep_).bias && n < N) {                                                         \
                    const Vec4<bf16> b = *reinterpret_cast<const Vec4<bf16>*>((ep_).bias + n);     \
                    _Pragma("unroll") for (int r = 0; r < 4; ++r) v[r] += b.get(r);                \
                }                                                                                  \
            }                                                                                      \
            *reinterpret_cast<f32x4*>((stage_) + li * PADW + 16 * j + 4 * g) = v;                  \
        }                                                                                          \
    } while (0)

// ---- column sums of the output (gemm3_kernel and gemm5_kernel, CS) ---------------------------------------------------------------------
// csum_[8] = this lane's 8 columns summed over its rows of the wave's 128 x 64 sub-tile.  Lanes l, l+8, ..., l+56 hold the same 8
// columns for different rows: xor-shuffle over lane bits 3..5, then lanes 0-7 (prow_ == 0) write the 64 column sums of the sub-tile
// to row `row_block_` (128-row blocks of the output) of cs_partial_: every [row block][column] entry is written exactly once.
// (Every function form moved instructions in gemm5_kernel, whose epilogue is scheduled by hand.)
#define EPI_COLSUM_FOLD(csum_, cs_partial_, row_block_, n_, N_, prow_)                             \
    do {                                                                                           \
        _Pragma("unroll") for (int r = 0; r < 8; ++r) {                                            \
            float t = (csum_)[r];                                                                  \
            t += __shfl_xor(t, 8, 64);                                                             \
            t += __shfl_xor(t, 16, 64);                                                            \
            t += __shfl_xor(t, 32, 64);                                                            \
            (csum_)[r] = t;                                                                        \
        }                                                                                          \
        const int n = (n_);                                                                        \
        if ((prow_) == 0 && n < (N_)) {                                                            \
            float* cp = (cs_partial_) + (int64_t)(row_block_) * (N_) + n;                          \
            *reinterpret_cast<f32x4*>(cp) = f32x4{(csum_)[0], (csum_)[1], (csum_)[2], (csum_)[3]}; \
            *reinterpret_cast<f32x4*>(cp + 4) = f32x4{(csum_)[4], (csum_)[5], (csum_)[6], (csum_)[7]}; \
        }                                                                                          \
    } while (0)

// ---- the activation step of the v1 kernels (erf-based gelu_f / gelu_grad_f) ---------------------------------------------------------------
// W consecutive elements of row m: gemm_mfma_kernel 4 (V = Vec4<T>), gemm_scalar_kernel 1 (V = Vec1<T>).  aux_in / aux_out are the
// arrays' base pointers ([..][ldaux]), (m, n) the position of v[0].  ACT_GELU sees the stored, rounded pre-activation only when aux_out
// is given.
template <typename T> struct Vec1 {
    T v;
    __device__ __forceinline__ float get(int) const { return to_f32<T>(v); }
    __device__ __forceinline__ void set(int, float x) { v = from_f32<T>(x); }
};
// (As a function, element-wise or W wide, by pointer or by value, it moved a register count or a v_cndmask / v_mul count in both kernels.)
#define EPI_V1_ACT(W_, V_, act_, v_, aux_in_, aux_out_, ldaux_, m_, n_)                                                \
    do {                                                                                                               \
        if ((act_) == UCFVIT_ACT_GELU) {                                                                               \
            if (aux_out_) {                                                                                            \
                V_ o;                                                                                                  \
                _Pragma("unroll") for (int r = 0; r < W_; ++r) o.set(r, (v_)[r]);                                      \
                *reinterpret_cast<V_*>((aux_out_) + (int64_t)(m_) * (ldaux_) + (n_)) = o;                              \
                _Pragma("unroll") for (int r = 0; r < W_; ++r) (v_)[r] = o.get(r);  /* sees the stored (rounded) pre-activation */ \
            }                                                                                                          \
            _Pragma("unroll") for (int r = 0; r < W_; ++r) (v_)[r] = gelu_f((v_)[r]);                                  \
        } else if ((act_) == UCFVIT_ACT_GELU_GRAD) {                                                                   \
            V_ h = *reinterpret_cast<const V_*>((aux_in_) + (int64_t)(m_) * (ldaux_) + (n_));                          \
            _Pragma("unroll") for (int r = 0; r < W_; ++r) (v_)[r] *= gelu_grad_f(h.get(r));                           \
        } else if ((act_) == UCFVIT_ACT_GELU_SAVE_DERIV) {                                                             \
            V_ o;                                                                                                      \
            _Pragma("unroll") for (int r = 0; r < W_; ++r) {                                                           \
                o.set(r, gelu_grad_f((v_)[r]));                                                                        \
                (v_)[r] = gelu_f((v_)[r]);                                                                             \
            }                                                                                                          \
            *reinterpret_cast<V_*>((aux_out_) + (int64_t)(m_) * (ldaux_) + (n_)) = o;                                  \
        } else if ((act_) == UCFVIT_ACT_MUL_AUX) {                                                                     \
            V_ h = *reinterpret_cast<const V_*>((aux_in_) + (int64_t)(m_) * (ldaux_) + (n_));                          \
            _Pragma("unroll") for (int r = 0; r < W_; ++r) (v_)[r] *= h.get(r);                                        \
        }                                                                                                              \
    } while (0)

// ---- host: what every GEMM launcher does ---------------------------------------------------------------------------------------------
// f(LA, LB) with the two operand layouts as integral constants (decltype(LA)::value is UCFVIT_LAYOUT_KC or UCFVIT_LAYOUT_KS)
template <typename F> int gemm_with_layouts(int la, int lb, F&& f) {
    typedef std::integral_constant<int, UCFVIT_LAYOUT_KC> KC;
    typedef std::integral_constant<int, UCFVIT_LAYOUT_KS> KS;
    if (la == UCFVIT_LAYOUT_KC && lb == UCFVIT_LAYOUT_KC) return f(KC{}, KC{});
    if (la == UCFVIT_LAYOUT_KC && lb == UCFVIT_LAYOUT_KS) return f(KC{}, KS{});
    if (la == UCFVIT_LAYOUT_KS && lb == UCFVIT_LAYOUT_KS) return f(KS{}, KS{});
    return f(KS{}, KC{});
}

// Raise the dynamic-LDS limit of kernel KERN to `bytes`, once per kernel: the function-local static is initialised by the first thread
// that gets here and the others wait for it (forward and autograd threads both launch GEMMs).
template <auto KERN> int gemm_raise_lds(size_t bytes) {
    static const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        ucfvit_set_error("ucfvit_gemm: cannot raise dynamic LDS to %zu bytes: %s", bytes, hipGetErrorString(e));
        return UCFVIT_ERR_HIP;
    }
    return UCFVIT_OK;
}
