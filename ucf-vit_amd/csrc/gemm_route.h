// Which kernel runs a GEMM descriptor, with which epilogue and which split: decided once, on the host, in plain C++ (no HIP).
// ucfvit_gemm switches on the result; ucfvit_gemm_workspace, ucfvit_gemm_colsum_rows and ucfvit_gemm_route return fields of it;
// ucfvit_gemm_grouped uses the same operand rules.  Every rule of the dispatch is written here once.
#pragma once
#include <stdint.h>

#include "../../include/ucfvit_hip.h"

enum GemmKernel {
    GK_V1_SCALAR,  // gemm_scalar_kernel: tiny / unaligned shapes
    GK_V1_MFMA,    // gemm_mfma_kernel: fp32, and bf16 below the DMA path's sizes
    GK_G2_128,     // gemm2_kernel 128x128 (+ splitk_reduce_kernel when splits > 1)
    GK_G2_256,     // gemm2_kernel 256x256: an operand spanning 4 GiB or more
    GK_G3,         // gemm3_kernel: 256x256 ping-pong
    GK_STAGGER     // gemm5_kernel: 256x256 ping-pong with the epilogue under the partner group's K loop
};

// Epilogue specialisations of gemm3_kernel (see gemm2.hip); gemm5_kernel has PLAIN, RESIDUAL, GELU_SAVE_DERIV and MUL_AUX
enum { EPI_GENERIC = 0, EPI_PLAIN = 1, EPI_RESIDUAL = 2, EPI_GELU = 3, EPI_GELU_GRAD = 4, EPI_GELU_SAVE_DERIV = 5, EPI_MUL_AUX = 6 };

struct GemmRoute {
    GemmKernel kernel;
    int epi;                  // EPI_* (GK_G3, GK_STAGGER)
    bool cs;                  // the launch writes desc->c_colsum_partial
    int splits, k_per_split;  // K slices (GK_G2_*, GK_G3); splits > 1 only with a sufficient desc->workspace
    int stagger_steps;        // epilogue steps E of gemm5_kernel (GK_STAGGER)
    int64_t colsum_rows;      // rows of c_colsum_partial this problem can write; reads neither c_colsum_partial nor sched_state
    int64_t workspace_bytes;  // split-K scratch the plan wants; does not read desc->workspace
};

// ---- operand rules --------------------------------------------------------------------------------------------------------------
static inline bool gemm_ptr_aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p) % bytes == 0; }

// Every kernel but the scalar one moves its operands in vectors: 16-byte pieces of A and B along their contiguous index (`in_vec`
// elements), `out_vec` consecutive columns of C and of the C-shaped epilogue operands per lane.
struct GemmVectorRule {
    int64_t in_vec, out_vec;
    uintptr_t c_align, bias_align, cshape_align;  // bytes
};
static inline bool gemm_vectors_ok(const ucfvit_gemm_desc* d, const GemmVectorRule& v) {
    const int64_t a_contig = (d->a_layout == UCFVIT_LAYOUT_KC) ? d->K : d->M;
    const int64_t b_contig = (d->b_layout == UCFVIT_LAYOUT_KC) ? d->K : d->N;
    bool ok = gemm_ptr_aligned(d->A, 16) && gemm_ptr_aligned(d->B, 16) && d->lda % v.in_vec == 0 && d->ldb % v.in_vec == 0 &&
              a_contig % v.in_vec == 0 && b_contig % v.in_vec == 0 && d->N % v.out_vec == 0 && d->ldc % v.out_vec == 0 &&
              gemm_ptr_aligned(d->C, v.c_align) && d->M < (1ll << 31) && d->N < (1ll << 31) && d->K < (1ll << 31);
    if (d->bias) ok = ok && gemm_ptr_aligned(d->bias, v.bias_align);
    if (d->residual) ok = ok && gemm_ptr_aligned(d->residual, v.cshape_align) && d->ldr % v.out_vec == 0;
    if (d->aux_in) ok = ok && gemm_ptr_aligned(d->aux_in, v.cshape_align) && d->ldaux % v.out_vec == 0;
    if (d->aux_out) ok = ok && gemm_ptr_aligned(d->aux_out, v.cshape_align) && d->ldaux % v.out_vec == 0;
    return ok;
}
// the DMA kernels (bf16): 8 elements per 16-byte DMA lane, 8 output columns per lane
static inline bool gemm_dma_operands_ok(const ucfvit_gemm_desc* d) { return gemm_vectors_ok(d, {8, 8, 16, 8, 16}); }
// gemm_mfma_kernel: 16 bytes of A / B per load, 4 output columns per lane
static inline bool gemm_v1_vectors_ok(const ucfvit_gemm_desc* d) {
    const uintptr_t in = d->dtype == UCFVIT_F32 ? 4 : 2, out = d->out_dtype == UCFVIT_F32 ? 4 : 2;
    return gemm_vectors_ok(d, {(int64_t)(16 / in), 4, 4 * out, 4 * in, 4 * in});
}

// bytes between the first element of a [rows][ld] array and the end of its last row
static inline int64_t gemm_extent_bytes(int64_t rows, int64_t ld, int64_t elem_bytes) { return rows * ld * elem_bytes; }
// gemm3_kernel / gemm5_kernel address A and B with 32-bit byte offsets from the base pointer
static inline bool gemm_fits_u32(int64_t bytes) { return bytes < (1ll << 32); }
// gemm5_kernel's epilogue goes through buffer descriptors whose byte count is a positive int
static inline bool gemm_fits_i31(int64_t bytes) { return bytes <= (1ll << 31) - 1; }
static inline bool gemm_ab_fit_u32(const ucfvit_gemm_desc* d) {
    return gemm_fits_u32(gemm_extent_bytes(d->a_layout == UCFVIT_LAYOUT_KC ? d->M : d->K, d->lda, 2)) &&
           gemm_fits_u32(gemm_extent_bytes(d->b_layout == UCFVIT_LAYOUT_KC ? d->N : d->K, d->ldb, 2));
}

// sizes the DMA kernels take at all (anything else: gemm_mfma_kernel / gemm_scalar_kernel)
static inline bool gemm_dma_shape_ok(const ucfvit_gemm_desc* d) {
    if (d->dtype != UCFVIT_BF16) return false;
    if (d->K < 128) return false;
    // ragged last K-tile is zero-filled by the DMA issue; 16-byte vectors along K need K % 8 == 0 only for KC operands
    if ((d->a_layout == UCFVIT_LAYOUT_KC || d->b_layout == UCFVIT_LAYOUT_KC) && d->K % 8 != 0) return false;
    return d->M >= 128 && d->N >= 128;
}

// ---- tile size and split-K ------------------------------------------------------------------------------------------------------
// p->splits, p->k_per_split and *big (1: 256x256 tile, 0: 128x128) of the DMA kernels; false: the problem is none of theirs
static inline bool gemm_plan(const ucfvit_gemm_desc* d, GemmRoute* p, int* big) {
    constexpr int BK = 64;
    if (!gemm_dma_shape_ok(d)) return false;
    const int64_t t256 = ((d->M + 255) / 256) * ((d->N + 255) / 256);
    const int64_t t128 = ((d->M + 127) / 128) * ((d->N + 127) / 128);
    const int64_t ktiles = (d->K + BK - 1) / BK;
    const bool plain_epi = !d->bias && !d->residual && !d->aux_in && !d->aux_out && d->act == UCFVIT_ACT_NONE;
    p->splits = 1;
    *big = t256 >= 192;
    if (!*big) {
        if (plain_epi && t128 < 384) {
            constexpr int target = 384;
            // split-K so that every XCD owns whole 8 x 8-tile blocks (64 resident workgroups = 2 per CU) of ONE K-slice and
            // all 8 XCDs are busy in every round: nb64 * s block-slices must be a multiple of 8 (see Sched2 in gemm2.hip)
            const int64_t tm = (d->M + 127) / 128, tn = (d->N + 127) / 128;
            const int nb64 = (int)(((tm + 7) / 8) * ((tn + 7) / 8));
            int g8 = 8;
            while (nb64 % g8) g8 >>= 1;                     // gcd(nb64, 8)
            int s = 8 / g8;
            if (nb64 * s > target / 8) s = 1;                // too many rounds of slab traffic: plain persistent walk
            const int kmax = (int)(ktiles / 8);              // at least 8 K-tiles per slice
            if (s > kmax) s = kmax;
            if (s < 1) s = 1;
            p->splits = s;
        }
    }
    p->k_per_split = (int)(((ktiles + p->splits - 1) / p->splits) * BK);
    p->splits = (int)((d->K + p->k_per_split - 1) / p->k_per_split);
    return true;
}

// ---- epilogues ------------------------------------------------------------------------------------------------------------------
// the straight-line epilogue of gemm3_kernel for this descriptor ((KC, KC), bf16 out, no accumulate), or EPI_GENERIC
static inline int gemm_epilogue(const ucfvit_gemm_desc* d) {
    const bool res = d->residual != nullptr, aux_out = d->aux_out != nullptr;
    switch (d->act) {
        case UCFVIT_ACT_NONE: return aux_out ? EPI_GENERIC : (res ? EPI_RESIDUAL : EPI_PLAIN);
        case UCFVIT_ACT_GELU: return res ? EPI_GENERIC : EPI_GELU;
        case UCFVIT_ACT_GELU_GRAD: return (res || aux_out) ? EPI_GENERIC : EPI_GELU_GRAD;
        case UCFVIT_ACT_GELU_SAVE_DERIV: return res ? EPI_GENERIC : EPI_GELU_SAVE_DERIV;
        case UCFVIT_ACT_MUL_AUX: return (res || aux_out) ? EPI_GENERIC : EPI_MUL_AUX;
    }
    return EPI_GENERIC;
}

// Epilogue steps E of gemm5_kernel for a launch that gemm3_kernel would run with the specialised epilogue `epi`; 0: stay on
// gemm3_kernel.  `override_` is UCFVIT_GEMM_STAGGER (< 0: unset, 0: never, 1 / 2 / 4 / 8: force that E wherever the kernel can run).
// Measured (tools/block_gemm_bench.py, ViT-L shapes at M = 131005; profiles/r03_a_*): a K-step with only ONE group computing costs
// about what a paired K-step costs (the step is paced by the DMA round trip, not by the MFMAs), so the fewer such steps the better:
// E = 1 wins everywhere it applies, larger E loses.  The residual epilogue only pays for itself behind a long K loop, and the
// column-sum variant of the multiply epilogue does not fit the register budget at E = 1: both stay on gemm3_kernel.
// Which launches: per-shape A/B at the shapes of all five workloads (profiles/r03_c_stagger_shapes.txt): the staggered kernel wins
// 3-7 % at K >= 1536, 0-6 % at K = 1024 and LOSES 4-10 % at K = 768 / 512 (the cyclic re-read of a B K-tile and the two unpaired
// steps per tile weigh 1 / nk): K >= 1024 only.
static inline int gemm_stagger_steps(const ucfvit_gemm_desc* d, int epi, bool cs, int override_) {
    if (override_ == 0 || d->sched_state || d->K % 64 != 0) return 0;
    if (epi != EPI_PLAIN && epi != EPI_RESIDUAL && epi != EPI_GELU_SAVE_DERIV && epi != EPI_MUL_AUX) return 0;
    if ((epi == EPI_PLAIN || epi == EPI_RESIDUAL) && d->aux_in) return 0;
    if (epi == EPI_MUL_AUX && d->bias) return 0;             // (data gradients carry no bias: that epilogue has no bias registers)
    const int64_t ldin = epi == EPI_PLAIN ? 0 : (epi == EPI_RESIDUAL ? d->ldr : d->ldaux);   // the epilogue's C-shaped operand
    if (!gemm_fits_i31(gemm_extent_bytes(d->M, d->ldc, 2)) || !gemm_fits_i31(gemm_extent_bytes(d->M, ldin, 2))) return 0;
    if (cs && epi != EPI_MUL_AUX) return 0;
    const int nk = (int)(d->K / 64);
    int E = 1;                                       // (fc1 forward with the GELU epilogue, E = 1 / 2 / 4 / 8: 1251 / 1262 / 1317 / 1652 us)
    if (override_ > 0) E = override_;
    else if (nk < 16) return 0;
    else if (epi == EPI_RESIDUAL && nk < 32) return 0;
    else if (cs) return 0;
    if (nk < 2 * E) E = nk >= 8 ? 4 : (nk >= 4 ? 2 : (nk >= 2 ? 1 : 0));
    if (cs && E == 1) return 0;
    return E;
}

// ---- the route ------------------------------------------------------------------------------------------------------------------
static inline GemmRoute gemm_route(const ucfvit_gemm_desc* d, int stagger_override) {
    GemmRoute r = {};
    int big = 0;
    const bool planned = gemm_plan(d, &r, &big);
    if (planned && r.splits > 1) r.workspace_bytes = (int64_t)r.splits * d->M * d->N * (int64_t)sizeof(float);
    if (!planned || !gemm_dma_operands_ok(d) || (d->out_dtype != UCFVIT_BF16 && d->out_dtype != UCFVIT_F32)) {
        r.kernel = (gemm_v1_vectors_ok(d) && d->M * d->N >= 256) ? GK_V1_MFMA : GK_V1_SCALAR;
        r.splits = 1;
        return r;
    }
    if (r.splits > 1 && !(d->workspace && d->workspace_bytes >= r.workspace_bytes && gemm_ptr_aligned(d->workspace, 16))) {
        r.splits = 1;                                        // no (or too small a) workspace: run un-split
        r.k_per_split = (int)d->K;
    }
    r.kernel = !big ? GK_G2_128 : (gemm_ab_fit_u32(d) ? GK_G3 : GK_G2_256);      // (a 256x256 plan is never split)
    r.epi = EPI_GENERIC;
    if (r.kernel != GK_G3 || d->a_layout != UCFVIT_LAYOUT_KC || d->b_layout != UCFVIT_LAYOUT_KC || d->out_dtype != UCFVIT_BF16 || d->accumulate)
        return r;
    r.epi = gemm_epilogue(d);
    // the output column sums exist in the specialised MUL_AUX and plain epilogues: the data-gradient GEMM through the activation
    // (C = dh of the MLP) and the plain data gradients (C = dO of the attention projection: the V third of the qkv bias gradient),
    // two 128-row blocks per output tile row
    if (r.epi == EPI_MUL_AUX || (r.epi == EPI_PLAIN && !d->aux_in)) r.colsum_rows = 2 * ((d->M + 255) / 256);
    r.cs = d->c_colsum_partial && r.colsum_rows > 0;
    r.stagger_steps = gemm_stagger_steps(d, r.epi, r.cs, stagger_override);
    if (r.stagger_steps > 0) r.kernel = GK_STAGGER;
    return r;
}

// the route as text, in the vocabulary of tests/test_gemm_ops.py; returns the length (the text is cut to cap - 1 characters)
static inline int gemm_route_name(const GemmRoute& r, char* out, int64_t cap) {
    static const char* const epi[] = {"GENERIC", "PLAIN", "RESIDUAL", "GELU", "GELU_GRAD", "GELU_SAVE_DERIV", "MUL_AUX"};
    const char* head = "";
    const char* tail = "";
    switch (r.kernel) {
        case GK_V1_SCALAR: head = "v1-scalar"; break;
        case GK_V1_MFMA: head = "v1-mfma"; break;
        case GK_G2_128: head = r.splits > 1 ? "g2-128-splitk" : "g2-128"; break;
        case GK_G2_256: head = "g2-256"; break;
        case GK_G3: head = "g3-"; tail = epi[r.epi]; break;
        case GK_STAGGER: head = "stagger-"; tail = epi[r.epi]; break;
    }
    const char* parts[3] = {head, tail, r.cs ? "+CS" : ""};
    int n = 0;
    for (const char* s : parts)
        for (; *s; ++s, ++n)
            if (n < cap - 1) out[n] = *s;
    if (cap > 0) out[n < cap - 1 ? n : cap - 1] = 0;
    return n;
}

// ---- launchers, one per translation unit: they launch what the route names and do not decline --------------------------------
int ucfvit_gemm_launch_v1(const ucfvit_gemm_desc* d, const GemmRoute& r, void* stream);       // gemm.hip
int ucfvit_gemm_launch_dma(const ucfvit_gemm_desc* d, const GemmRoute& r, void* stream);      // gemm2.hip
int ucfvit_gemm_launch_stagger(const ucfvit_gemm_desc* d, const GemmRoute& r, void* stream);  // gemm_stagger.hip
