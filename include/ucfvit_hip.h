/*
 * ucfvit_hip.h — C ABI of libucfvit_hip.so: the MI355X (gfx950) kernels behind the UCF-VIT operator layer.
 *
 * The reference (irlyngaas/UCF-VIT) has no FFI: its drop-in boundary is the Python nn.Module operator layer
 * (src/UCF_VIT/simple/building_blocks.py: PatchEmbed:30, Mlp:94, Attention:131, Block:194; MAE gathers in
 * src/UCF_VIT/simple/arch.py:663,683).  Every entry point below replaces the torch/ATen call sites of one of
 * those operators; the replaced reference lines are cited per function.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *  - plain pointers and sizes only, no torch types.  All pointers are DEVICE pointers unless stated otherwise.
 *  - `dtype` selects the arithmetic/storage type of activations and (shadow) weights:
 *       UCFVIT_F32  : fp32 storage, exact-fp32 MFMA (v_mfma_f32_16x16x4_f32)  — the reference's `simple/` mode
 *       UCFVIT_BF16 : bf16 storage, bf16 MFMA with fp32 accumulation          — the reference's fsdp MixedPrecision mode
 *    statistics (LayerNorm mean/rstd, softmax log-sum-exp), losses, parameter gradients and optimizer state
 *    are always fp32.
 *  - `stream` is a hipStream_t passed as void*; every function only enqueues work on it (no synchronisation,
 *    no allocation) so callers may capture the calls into a hipGraph.
 *  - the caller owns every buffer (inputs, outputs, workspaces).  The library keeps no tensor memory.
 *  - return value: 0 on success, <0 on error (see codes); ucfvit_last_error() returns a thread-local message.
 *    Nothing throws across the ABI and nothing calls exit().
 *  - re-entrant: may be called concurrently from the Python main thread and autograd worker threads.
 */
#ifndef UCFVIT_HIP_H
#define UCFVIT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UCFVIT_ABI_VERSION 24 /* still 24 with the dropout, LayerScale, QK-norm, DDPM, EMA and DDIM entry points (ucfvit_dropout*, ucfvit_layer_scale_*, ucfvit_qk_norm_*, ucfvit_ddpm_*, ucfvit_time_tokens_*, ucfvit_relu_dropout*, ucfvit_adamw_ema, ucfvit_adamw_scaled_ema, ucfvit_ddim_step, ucfvit_grad_sqnorm*, ucfvit_grad_clip_coef, ucfvit_adamw_clipped): symbols were only added */

#define UCFVIT_OK 0
#define UCFVIT_ERR_INVALID_ARGUMENT (-1)
#define UCFVIT_ERR_UNSUPPORTED (-2)
#define UCFVIT_ERR_HIP (-3)

#define UCFVIT_F32 0
#define UCFVIT_BF16 1

int ucfvit_abi_version(void);
const char* ucfvit_last_error(void);

/* Diagnostic (no reference counterpart): launches a pure bf16 MFMA stream (operands in registers, 2 waves per SIMD on every CU,
 * `iters` x 16 v_mfma_f32_16x16x32_bf16 per wave on 16 independent accumulators) and returns the FLOPs it executes (< 0: error).  Timed with HIP events by
 * bench.py: the rate is the ceiling the chip's clock / power management leaves to any bf16 MFMA kernel on that device.
 * sink: >= 256 floats of device memory (never written in practice). */
int64_t ucfvit_mfma_probe(float* sink, int iters, void* stream);

/* Diagnostic (no reference counterpart): `workgroups` workgroups that each hold one CU (512 threads, 96 KiB LDS) for about `microseconds`,
 * doing nothing — a stand-in for a collective's kernel next to the persistent GEMM grids on a one-GPU box (tools/gemm_contention.py).
 * sink: >= 512 floats of device memory (never written). */
int ucfvit_occupy(int workgroups, int microseconds, float* sink, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * GEMM with fused epilogue:  C[M,N] = epilogue( alpha * op(A)[M,K] · op(B)[K,N] )
 *
 * Replaces nn.Linear forward/backward on the hot path: qkv / proj (building_blocks.py:150,154,159,190),
 * fc1 / fc2 (:115,119,123,127), the patch-embedding projection (conv k=s=p ≡ im2col + GEMM, :58-60,89),
 * head (arch.py:268-271,484), MAE decoder_embed / decoder_pred (arch.py:552-559,685,700).
 *
 * Operand storage ("KC" = contraction index contiguous, "KS" = contraction index strided):
 *   a_layout KC: A stored [M][K] row-major, lda = row stride      a_layout KS: A stored [K][M], lda = stride of k
 *   b_layout KC: B stored [N][K] row-major (nn.Linear weight)     b_layout KS: B stored [K][N], ldb = stride of k
 *   forward  y = x·Wᵀ      : (KC, KC)   A=x[M,K]   B=W[N,K]
 *   dgrad    dx = dy·W     : (KC, KS)   A=dy[M,N'] B=W[N',K']   (contraction over W's rows)
 *   wgrad    dW = dyᵀ·x    : (KS, KS)   A=dy[M',N] (as [K][M]), B=x[M',K'] (as [K][N])
 *
 * Epilogue, in order:  v = alpha*acc ; v += bias[n] ; act ; v += residual[m][n] ; v += C_old (accumulate) ; store.
 *   act = UCFVIT_ACT_GELU      : if aux_out, aux_out[m][n] = v (pre-activation, saved for backward); v = gelu_erf(v)
 *   act = UCFVIT_ACT_GELU_GRAD : v *= gelu_erf'(aux_in[m][n])   (dgrad through the activation; aux_in = saved pre-activation)
 *   act = UCFVIT_ACT_GELU_SAVE_DERIV / UCFVIT_ACT_MUL_AUX : the same pair with the derivative evaluated once, in the forward
 *         epilogue where gelu shares its erfc, and saved in place of the pre-activation; the backward epilogue is a multiply.
 *         The bf16 training path uses this pair (one bf16 rounding of gelu' instead of one of its argument); fp32 keeps the first.
 * `dtype` = type of A and B (and bias/residual/aux); `out_dtype` = type of C (UCFVIT_F32 for parameter gradients).
 * ------------------------------------------------------------------------------------------------------ */
#define UCFVIT_LAYOUT_KC 0
#define UCFVIT_LAYOUT_KS 1
#define UCFVIT_ACT_NONE 0
#define UCFVIT_ACT_GELU 1
#define UCFVIT_ACT_GELU_GRAD 2
#define UCFVIT_ACT_GELU_SAVE_DERIV 3 /* forward:  aux_out[m][n] = gelu_erf'(v) (required); v = gelu_erf(v) */
#define UCFVIT_ACT_MUL_AUX 4         /* backward: v *= aux_in[m][n]   (aux_in = the derivative saved by ACT_GELU_SAVE_DERIV) */

typedef struct ucfvit_gemm_desc {
    const void* A;
    const void* B;
    void* C;
    const void* bias;     /* [N] dtype, or NULL */
    const void* residual; /* [M][ldr] dtype, or NULL */
    const void* aux_in;   /* [M][ldaux] dtype, or NULL (ACT_GELU_GRAD) */
    void* aux_out;        /* [M][ldaux] dtype, or NULL (ACT_GELU) */
    int64_t M, N, K;
    int64_t lda, ldb, ldc, ldr, ldaux;
    int32_t a_layout, b_layout;
    int32_t dtype, out_dtype;
    int32_t act;
    int32_t accumulate; /* 1: C += result (gradient accumulation) */
    float alpha;
    void* workspace;         /* optional fp32 scratch for split-K partial sums (see ucfvit_gemm_workspace), or NULL */
    int64_t workspace_bytes;
    float* c_colsum_partial; /* optional by-product of the epilogue: per block of output rows, the column sums of the values written to
                              * C (taken in fp32 before the rounding to dtype): fp32 [ucfvit_gemm_colsum_rows(desc)][N], every entry
                              * written.  Summed over its rows (ucfvit_reduce_rows) it is the bias gradient of the Linear layer whose
                              * output gradient this GEMM produces (fc1: C = dh), so dh is not read again by ucfvit_colsum.  NULL: off. */
    void* sched_state;       /* optional: UCFVIT_GEMM_SCHED_BYTES of device memory, 16-byte aligned, zeroed ONCE by the caller and then
                              * used by every launch of ONE stream.  With it the persistent 256x256 kernel hands its output tiles out through
                              * device-scope atomic counters (work-conserving when another kernel — an RCCL collective overlapping backward —
                              * holds some of the CUs: workgroups that start late find the list empty instead of owning a share of it) and
                              * leaves the state zeroed.  Results do not depend on the tile order (every tile is computed by one workgroup either way); a launch
                              * with sched_state always takes the ping-pong kernel, a launch without it may take the staggered kernel (csrc/gemm_stagger.hip),
                              * whose rows 128-255 of a tile accumulate over K in a rotated — equally fixed — order: the same values up to fp32 summation order.
                              * NULL: static tile order. */
} ucfvit_gemm_desc;
#define UCFVIT_GEMM_SCHED_BYTES 1024

/* bytes of workspace the split-K path would use for this problem (0: none).  Without it the GEMM still runs, un-split. */
int64_t ucfvit_gemm_workspace(const ucfvit_gemm_desc* desc);
int ucfvit_gemm(const ucfvit_gemm_desc* desc, void* stream);
/* rows of desc->c_colsum_partial this problem would write (desc->c_colsum_partial itself is not read); 0: the kernel that runs this
 * problem has no such by-product and ucfvit_gemm rejects a non-NULL c_colsum_partial with UCFVIT_ERR_UNSUPPORTED. */
int64_t ucfvit_gemm_colsum_rows(const ucfvit_gemm_desc* desc);
/* which kernel ucfvit_gemm would run for this descriptor, as text ("v1-scalar", "v1-mfma", "g2-128", "g2-128-splitk", "g2-256",
 * "g3-PLAIN+CS", "g3-GENERIC", "stagger-RESIDUAL", ...); reads workspace / workspace_bytes (split-K only with a sufficient workspace),
 * c_colsum_partial ("+CS") and sched_state (keeps a launch off the staggered kernel) as ucfvit_gemm does, the descriptor's other pointers
 * for their alignment only; host only, no HIP call; returns the length (the text is cut to cap - 1 characters), or < 0 */
int ucfvit_gemm_route(const ucfvit_gemm_desc* desc, char* out, int64_t cap);
/* out[n] (+)= sum_r partial[r][n]  (fp32, fixed order) — the second stage of every two-stage column sum of this library */
int ucfvit_reduce_rows(const float* partial, float* out, int64_t rows, int64_t N, int accumulate, void* stream);

/* n <= 32 epilogue-free GEMMs with the same K, layouts and dtypes (the weight gradients dW_qkv, dW_proj, dW_fc1, dW_fc2 of one
 * or several transformer Blocks all contract over the B*N tokens) as ONE persistent launch over the union of their output tiles:
 * fills the 256 CUs without split-K partial sums (ViT-L: 192 tiles per Block, so four Blocks = 768 tiles = 3 whole rounds).
 * Falls back to n ucfvit_gemm calls when the set is not groupable. */
int ucfvit_gemm_grouped(const ucfvit_gemm_desc* descs, int64_t n, void* stream);

/* column sums  out[n] (fp32) (+)= sum_m x[m][n]   — bias gradients of every nn.Linear (autograd of :159,190,123,127) */
int64_t ucfvit_colsum_workspace(int64_t M, int64_t N); /* bytes of fp32 scratch for the deterministic two-stage sum */
int ucfvit_colsum(const void* x, float* out, int64_t M, int64_t N, int64_t ldx, int accumulate, void* workspace, int dtype,
                  void* stream);

/* ------------------------------------------------------------------------------------------------------
 * LayerNorm over the last dimension (biased variance, affine): nn.LayerNorm(D, eps) at building_blocks.py:212,226,
 * arch.py:170,266 (eps 1e-6) and arch.py:560 (decoder_norm, eps 1e-5).
 * x,y,dy,dx: [rows][D] dtype ; gamma,beta: [D] dtype ; mean,rstd: [rows] fp32 (saved for backward).
 * bwd: dx = LN-grad(dy) + dres (dres: optional [rows][D] dtype, the residual branch's gradient, fused; NULL = none);
 *      dgamma/dbeta are fp32 [D]; `accumulate` adds into them.  workspace: fp32, >= ucfvit_layernorm_bwd_workspace() bytes.
 *      dx_colsum: optional fp32 [D] (+)= column sums of dx (taken in fp32 before rounding): dx is the gradient of the residual
 *      stream, i.e. the output gradient of the proj / fc2 Linear before this norm, so this IS that layer's bias gradient and the
 *      separate ucfvit_colsum pass over dx is not needed.  NULL = off.
 * ------------------------------------------------------------------------------------------------------ */
int ucfvit_layernorm_fwd(const void* x, const void* gamma, const void* beta, void* y, float* mean, float* rstd,
                         int64_t rows, int64_t D, float eps, int dtype, void* stream);
int64_t ucfvit_layernorm_bwd_workspace(int64_t rows, int64_t D);
int ucfvit_layernorm_bwd(const void* dy, const void* x, const void* gamma, const float* mean, const float* rstd,
                         const void* dres, void* dx, float* dgamma, float* dbeta, int64_t rows, int64_t D, int accumulate,
                         float* dx_colsum, int dx_colsum_accumulate, void* workspace, int dtype, void* stream);
/* The same backward with a residual-branch gradient that exists for one row in every `dres_period` only: row r receives
 * dres[r / dres_period] (dres: [ceil(rows / dres_period)][D] dtype) when r % dres_period == 0 and +0 otherwise, i.e. exactly what
 * ucfvit_layernorm_bwd computes for that dres expanded to [rows][D] with zeros, bit for bit, without the expanded array existing.
 * (The class-token rows of a [B][N][D] residual stream: dres_period = N.)  dres_period = 1 is ucfvit_layernorm_bwd; rows < 2^31. */
int ucfvit_layernorm_bwd_rows(const void* dy, const void* x, const void* gamma, const float* mean, const float* rstd,
                              const void* dres, int64_t dres_period, void* dx, float* dgamma, float* dbeta, int64_t rows, int64_t D,
                              int accumulate, float* dx_colsum, int dx_colsum_accumulate, void* workspace, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Fused multi-head self-attention core, softmax(q·kᵀ·scale)·v, non-causal, no mask, dropout 0:
 * building_blocks.py:159-189 (reshape [B,N,3,H,dh] → permute(2,0,3,1,4) → SDPA / explicit math → transpose → reshape).
 * qkv : [B][N][3][H][dh] dtype — exactly the output of the qkv Linear (no permute copy is made)
 * out : [B][N][H*dh] dtype     — already in the layout `proj` consumes
 * lse : [B][H][N] fp32, log2-domain log-sum-exp of the scaled scores (saved for backward)
 * bwd : dqkv has qkv's layout; delta_ws is fp32 [B][H][N] scratch.  dh ∈ {32, 64, 128}.
 * Dispatch: attn_route() in csrc/attn_route.h decides once per call between the kernels that keep a head's whole sequence in LDS
 * (csrc/attention_short.hip: bf16, dh 32 / 64, N <= 256) and the streaming kernels (csrc/attention.hip: everything else); both families
 * take their MFMA fragments through csrc/attn_tile.h.  ucfvit_attention_route names the decision.
 * ------------------------------------------------------------------------------------------------------ */
int ucfvit_attention_fwd(const void* qkv, void* out, float* lse, int64_t B, int64_t N, int64_t H, int64_t dh,
                         float scale, int dtype, void* stream);
int ucfvit_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                         float* delta_ws, int64_t B, int64_t N, int64_t H, int64_t dh, float scale, int dtype,
                         void* stream);
/* The same backward, also handing out what the qkv bias gradient needs (building_blocks.py:154 qkv = nn.Linear(dim, 3 dim, bias=qkv_bias): its
 * bias gradient is dqkv summed over all B N token rows) so that dqkv is not read a second time for it:
 *   colsum_partial fp32 [B][2][H][dh]: row b holds the column sums of dQ over batch element b's N tokens (from the fp32 gradients before they
 *   are rounded), then H dh zeros for dK; the caller sums the B rows (ucfvit_reduce_rows) into the first two thirds of the bias gradient.
 *   The K third of the bias gradient is identically zero — sum_key dS[q][key] = sum_key P (dP - delta) = delta - delta: a key bias shifts
 *   every score of a row alike and the softmax does not see it (the reference's value there is rounding noise around 0) — and the V third
 *   is the column sum of `dout` (sum_key P = 1), which the projection's data-gradient GEMM can produce in its epilogue
 *   (ucfvit_gemm c_colsum_partial): neither needs this kernel.
 * Only where the fused short-sequence kernel runs: ucfvit_attention_bwd_colsum_supported returns 1 (bf16, head dim 32 / 64, N <= 256),
 * else 0 and ucfvit_attention_bwd_colsum fails with UCFVIT_ERR_UNSUPPORTED. */
int ucfvit_attention_bwd_colsum_supported(int64_t B, int64_t N, int64_t H, int64_t dh, int dtype);
int ucfvit_attention_bwd_colsum(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                                float* delta_ws, float* colsum_partial, int64_t B, int64_t N, int64_t H, int64_t dh, float scale,
                                int dtype, void* stream);
/* which kernels ucfvit_attention_fwd (backward = 0) or ucfvit_attention_bwd / _bwd_colsum (backward = 1) would run for this shape, as
 * text: "short-nb4", "short-nb8", "s3-nb13", "short-nb16" (forward) or "fused-nb4" .. "fused-nb16" (backward), NB being the 16-row blocks
 * the kernel is built for, followed by "-exact" (N fills them: only the last key block is masked) or "-masked"; otherwise "stream-bf16" /
 * "stream-fp32".  ucfvit_attention_bwd_colsum_supported is 1 exactly for the "fused-" names.  Host only, no HIP call; returns the length
 * (the text is cut to cap - 1 characters), or < 0 for a shape the attention entry points refuse */
int ucfvit_attention_route(int64_t B, int64_t N, int64_t H, int64_t dh, int dtype, int backward, char* out, int64_t cap);

/* The same attention for ONE query row per batch element (a model whose head reads only the class token needs nothing else of its
 * last Block's attention output).  qkv as above, all N keys / values are read; the query is token `qrow` of every batch element.
 *   fwd: out [B][H*dh] dtype (compact: one row per batch element), lse fp32 [B][H], log2 domain.
 *   bwd: dout / out are the compact [B][H*dh] rows; dqkv (qkv's layout) is written whole: the K and V thirds of every token, the Q
 *        third of token `qrow`, zeros in the Q third of every other token.
 *        colsum_partial (optional) fp32 [B][2][H][dh]: row b = dq of batch element b (fp32, before rounding), then H dh zeros — the
 *        same contract as ucfvit_attention_bwd_colsum (the V third of the bias gradient is the column sum of the compact dout).
 * fp32 and bf16, dh in {32, 64, 128}, N <= 8192; one pass over K and V, plain VALU arithmetic (HBM-bound). */
int ucfvit_attention_rows_fwd(const void* qkv, void* out, float* lse, int64_t B, int64_t N, int64_t H, int64_t dh, int64_t qrow,
                              float scale, int dtype, void* stream);
int ucfvit_attention_rows_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                              float* colsum_partial, int64_t B, int64_t N, int64_t H, int64_t dh, int64_t qrow, float scale,
                              int dtype, void* stream);

/* Attention of a QUERY block against ANOTHER token block's keys / values: the building block of ring sequence parallelism (no reference
 * counterpart: the reference constructs seq_par_group and asserts seq_par_size == 1, training_scripts/train_masked_fsdp.py:220).
 *   q [B][Nq][ldq], k / v [B][Nk][ldkv] with head h at columns [h*dh, (h+1)*dh);  out [B][Nq][H*dh] (dtype), lse [B][H][Nq] in log2 units.
 * Backward of one (query block, key block) pair of a softmax that spans several key blocks: `lse` is the log-sum-exp over ALL key blocks and
 * `out` the final merged output (delta = rowsum(dO * O) is taken from them), so dq / dk / dv (fp32 [B][Nq|Nk][H*dh], += when accumulate)
 * receive exactly this pair's terms.  delta_ws: B*H*Nq floats of scratch. */
int ucfvit_attention_cross_fwd(const void* q, const void* k, const void* v, void* out, float* lse, int64_t B, int64_t Nq, int64_t Nk, int64_t H,
                               int64_t dh, int64_t ldq, int64_t ldkv, float scale, int dtype, void* stream);
int ucfvit_attention_cross_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse, float* dq,
                               float* dk, float* dv, float* delta_ws, int64_t B, int64_t Nq, int64_t Nk, int64_t H, int64_t dh, int64_t ldq,
                               int64_t ldkv, float scale, int accumulate, int dtype, void* stream);
/* online merge of partial results over disjoint key blocks: lse' = log2(2^lse_acc + 2^lse_part), o' = o_acc 2^(lse_acc - lse') +
 * o_part 2^(lse_part - lse'); o_acc fp32 [B][Nq][H*dh], o_part dtype; first != 0: o_acc = o_part, lse_acc = lse_part */
int ucfvit_attention_merge(float* o_acc, float* lse_acc, const void* o_part, const float* lse_part, int64_t B, int64_t Nq, int64_t H, int64_t dh,
                           int first, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Patch embedding front end (PatchEmbed.forward, building_blocks.py:78-92): non-overlapping p×p(×p) patches of an
 * NCHW / NCHWD fp32 image are laid out as GEMM rows [B·L][C·p^nd] with K-order (c, ph, pw[, pd]) = the flattening of
 * the conv weight [D,C,p,p(,p)], token order row-major over the patch grid.  Coalesced reads of image rows through
 * LDS tiles; output in `dtype`.  nd = 2 or 3; dims = {H, W} or {H, W, Dz}.
 * ------------------------------------------------------------------------------------------------------ */
int ucfvit_im2col(const float* img, void* cols, int64_t B, int64_t C, const int64_t* dims, int nd, int64_t p,
                  int dtype, void* stream);

/* Token assembly (VIT._pos_embed, arch.py:367-393): out[b][0] = cls + pos[0] (if cls), out[b][t+pre] = patches[b][t] + pos[t+pre].
 * pos may be NULL (pos_embed='none').  bwd: dpatches = dout[:,pre:], dpos (fp32,[N][D]) (+)= sum_b dout, dcls (fp32,[D]) (+)= sum_b dout[:,0]. */
int ucfvit_tokens_fwd(const void* patches, const void* cls, const void* pos, void* out, int64_t B, int64_t L, int64_t D,
                      int has_cls, int dtype, void* stream);
int ucfvit_tokens_bwd(const void* dout, void* dpatches, float* dpos, float* dcls, int64_t B, int64_t L, int64_t D,
                      int has_cls, int accumulate, int dtype, void* stream);

/* Adaptive-patching front end (VIT.forward_features / _pos_embed with adaptive_patching=True, arch.py:465-467, :366-393).
 * The data loader delivers the token sequence already cut and resized: x fp32 [B][C][S][P] (S tokens of P = p^nd pixels per
 * channel) and seq_ps fp32 [B][S][kin] (kin = 3 for 2-D, 4 for 3-D input: position and size of each token).
 * ucfvit_seq_patches: rows_out[b*S+s][p*C+c] = x[b][c][s][p]  (einops 'b c s p -> b s (p c)'), in `dtype`; C*P <= 16384.
 * ucfvit_adaptive_pos_fwd: out[b][0] = cls (if has_cls; its position embedding is zero, arch.py:381-385),
 *     out[b][t+pre] = x[b][t] + GELU(seq_ps[b][t] . w^T + bias)     (adaptive_pos_dep_emb = Linear(kin, D) + erf-GELU, arch.py:311-321)
 *     x [B*S][D], w [D][kin], bias [D], cls [D], out [B][S+pre][D], all `dtype`; the pre-activation is recomputed in backward.
 * ucfvit_adaptive_pos_bwd: dx [B*S][D] = dout[:,pre:] (or NULL), dw fp32 [D][kin], dbias fp32 [D], dcls fp32 [D] (each may be NULL);
 *     accumulate is a bit mask (1: dw +=, 2: dbias +=, 4: dcls +=).  workspace: ucfvit_adaptive_pos_bwd_workspace bytes.
 *     Deterministic: per-chunk partial sums in the workspace, then one ordered pass. */
int ucfvit_seq_patches(const float* x, void* rows_out, int64_t B, int64_t C, int64_t S, int64_t P, int dtype, void* stream);
int ucfvit_adaptive_pos_fwd(const void* x, const float* seq_ps, const void* w, const void* bias, const void* cls, void* out,
                            int64_t B, int64_t S, int64_t D, int kin, int has_cls, int dtype, void* stream);
int64_t ucfvit_adaptive_pos_bwd_workspace(int64_t B, int64_t S, int64_t D, int kin, int has_cls, int dtype);
int ucfvit_adaptive_pos_bwd(const void* dout, const float* seq_ps, const void* w, const void* bias, void* dx, float* dw, float* dbias,
                            float* dcls, int64_t B, int64_t S, int64_t D, int kin, int has_cls, int accumulate, void* workspace,
                            int dtype, void* stream);

/* GPU-side fixed-length quadtree patcher (the adaptive-patching data transform: dataloaders/quadtree.py:84-174 FixedQuadTree,
 * dataloaders/transform.py:9-55 Patchify), a whole batch per call.  Edge detection is not included: `edges` is its result.
 * ucfvit_quadtree_build: edges uint8 [B][H][W] (cv2.Canny output: 0 / 255).  Per image the reference's greedy refinement: replace
 *     the FIRST node of maximum value (value = sum(region) / 255) by its quadrants lt, rt, lb, rb in place until fixed_length = L
 *     nodes exist (L must be 3n+1, train_unetr_simple.py:214) or that node is 2 pixels wide.  Bit-exact integer logic.
 *     nodes int32 [B][L][4] = (x1, x2, y1, y2) in list order, values int32 [B][L], count int32 [B] (valid nodes; the rest is padding),
 *     seq_ps fp32 [B][L][3] = (size = x2-x1, centre x, centre y); padding: size 0, centre (-1, -1) like FixedQuadTree.serialize.
 *     workspace: ucfvit_quadtree_workspace bytes (summed-area tables).  H, W < 32768, H*W*255 < 2^32.
 * ucfvit_quadtree_serialize: img fp32 [B][H][W][C] (channels last, as the reference's numpy images); every node's region resampled
 *     to p x p with the cv2.INTER_CUBIC kernel (A = -0.75, aligned pixel centres, replicated border) into seq fp32 [B][L][p][p][C];
 *     Patchify's plain reshape of that memory to [C][L][p*p] per image is the model input x[B][C][S][P].  Padding nodes: zeros. */
int64_t ucfvit_quadtree_workspace(int64_t B, int64_t H, int64_t W);
int ucfvit_quadtree_build(const uint8_t* edges, int32_t* nodes, int32_t* values, int32_t* count, float* seq_ps, int64_t B, int64_t H,
                          int64_t W, int64_t L, void* workspace, void* stream);
int ucfvit_quadtree_serialize(const float* img, const int32_t* nodes, const int32_t* count, float* seq, int64_t B, int64_t H, int64_t W,
                              int64_t C, int64_t L, int64_t p, void* stream);

/* Octree patcher for 3-D volumes (dataloaders/octree.py:66-151 FixedOctTree, transform.py:57-132 Patchify_3D's tree + serialize part).
 * domain uint8 [B][N][N][N] indexed [z][y][x] (cubic, N <= 256); value = sum(region) / norm_factor (norm_factor = int(255 / channels),
 * transform.py:120); children in the reference's order (x fastest, then y, then z); fixed_length L must be 7n+1; stop when the first
 * maximum node is 2 wide.  nodes int32 [B][L][6] = (x1, x2, y1, y2, z1, z2), values, count as for the quadtree; seq_ps fp32 [B][L][4] =
 * (size, centre x, y, z), padding size 0 / centre -1.  workspace: ucfvit_octree_workspace bytes.  N^3 * 255 / norm_factor < 2^31 (values
 * are int32): refused otherwise, e.g. N >= 204 with norm_factor 1.
 * ucfvit_octree_serialize: img fp32 [B][N][N][N][C]; leaf img[z1:z2, y1:y2, x1:x2, :] -> p^3 by linear interpolation with aligned corners
 * (the reference's scipy RegularGridInterpolator on linspace(0, n, n) -> linspace(0, n, p)), seq fp32 [B][L][p][p][p][C]. */
int64_t ucfvit_octree_workspace(int64_t B, int64_t N);
int ucfvit_octree_build(const uint8_t* domain, int32_t* nodes, int32_t* values, int32_t* count, float* seq_ps, int64_t B, int64_t N, int64_t L,
                        int norm_factor, void* workspace, void* stream);
int ucfvit_octree_serialize(const float* img, const int32_t* nodes, const int32_t* count, float* seq, int64_t B, int64_t N, int64_t C,
                            int64_t L, int64_t p, void* stream);

/* Label serializers and tree deserializers: the two tree operations between the patcher and a segmentation loss / metric (reference
 * quadtree.py:176-221 + Rect.set_area, octree.py:152-213 + Cube.set_area; one image and one Python loop per call there).  nodes / count as the
 * builders above leave them.  Padding rows (s >= count[b]), empty leaves (any extent <= 0) and nodes whose box leaves the image read nothing:
 * the serializers give them class 0 (the reference's zero patch followed by F.one_hot), the deserializers write nothing for them.
 * Limits as above: H, W < 32768; N <= 256; 1 <= num_classes <= 255; 1 <= C <= 255; a request outside them returns an error and launches nothing.
 *
 * ucfvit_quadtree_serialize_labels: labels [B][H][W], uint8 or int64 by `label_dtype`; every leaf's region resampled to p x p by the
 *     cv2.resize(INTER_NEAREST) rule: source column = min((px * w) / p, w - 1) in integer arithmetic, rows alike.
 *     idx int64 [B][L][p][p] (class indices) and / or onehot fp32 [B][num_classes][L * p * p] (the memory order of the reference's collate
 *     output, datamodule.py:40-51, that training_step_adaptive reshapes plainly); a null pointer skips one of them.  A label >= num_classes or
 *     < 0 is written unchanged to idx and gives an all-zero one-hot column.
 * ucfvit_octree_serialize_labels: labels [B][N][N][N] ([z][y][x]), nodes [B][L][6], idx [B][L][p][p][p], onehot [B][num_classes][L * p^3].
 *     Rule per axis: scipy RegularGridInterpolator(method='nearest') on linspace(0, n, n) queried at linspace(0, n, p): position
 *     f = j (n-1) / (p-1), cell i = min(floor(f), n-2), take i if the fraction is <= 1/2, else i+1, evaluated in exact integer arithmetic
 *     (2 (j (n-1) - i (p-1)) <= p-1); p = 1 and n = 1 take voxel 0.  TIES GO TO THE LOWER INDEX: an even p has no ties and equals scipy on
 *     every sample; for an odd p scipy's double arithmetic sends some exact midpoints up (n = 4, p = 3: scipy [0, 2, 3], this rule [0, 1, 3]).
 * ucfvit_quadtree_deserialize: seq fp32 read in place, element (b, c, s, e = py * p + px) at b stride_b + c stride_c + s stride_s + e stride_e
 *     (the reference's patch list [B][L][p][p][C] and the model's [B][C][L][p*p] both without a copy); out fp32, element (b, c, pixel = y W + x)
 *     at b out_b + c out_c + pixel out_pixel, which must be dense [B][C][H][W] or dense [B][H][W][C].  The output is zero-filled first; then
 *     every valid leaf region is its p x p patch resized to (w, h): mode UCFVIT_RESAMPLE_SMOOTH by the rule of ucfvit_quadtree_serialize
 *     (A = -0.75, half-pixel centres, taps clamped to the patch, no anti-aliasing), with `trunc` != 0 after truncf of every tap (the
 *     reference's seq.astype(int), quadtree.py:213); mode UCFVIT_RESAMPLE_NEAREST by patch column = min((x * p) / w, p - 1), which keeps class
 *     maps and one-hot planes exact.  Overlapping leaves are outside the contract (a tree never produces them).
 * ucfvit_octree_deserialize: the same for [p][p][p] patches (e = (pz * p + py) * p + px) into [B][C][N][N][N] or [B][N][N][N][C]:
 *     UCFVIT_RESAMPLE_SMOOTH is aligned-corner trilinear (Cube.set_area: linspace(0, p, p) onto linspace(0, p, n)), UCFVIT_RESAMPLE_NEAREST the
 *     integer grid rule above with patch and leaf exchanged.  No trunc (the reference commented it out in 3-D).
 * ucfvit_quadtree_deserialize_bwd / ucfvit_octree_deserialize_bwd: the adjoints (the gradient of a loss taken in the image plane).  With the
 *     forward's weights, out[c][x] = sum_k w(x, k) seq[c][k] per leaf, they give dseq[c][k] = sum over the leaf's pixels of w(x, k) dout[c][x].
 *     dout fp32 is read through (out_b, out_c, out_pixel), which must be one of the two dense layouts the forward writes; dseq fp32 is written
 *     through (stride_b, stride_c, stride_s, stride_e) as the forward reads seq (stride_b > 0 unless B = 1), so the gradient lands in
 *     [B][C][L][p^d] or in the patch list [B][L][p]..[C] without a copy.  EVERY element of every row is written: padding rows, empty leaves and
 *     leaves whose box leaves the image get 0; pixels no leaf covers contribute nothing.  No trunc: truncation has no gradient.
 *     Deterministic, no atomics: a leaf is cut along its slowest axis into at most 16 slices of at least 1024 pixels, a rule of the leaf's
 *     extents alone; a leaf of one slice is summed by one thread per element, the slices of a larger leaf leave partial tiles in the workspace
 *     ([B * L][16][C * p^d] fp32, *_bwd_workspace bytes; 0 for images of at most 1024 pixels, then NULL is accepted; -1 with
 *     ucfvit_last_error for arguments the op refuses) and a second kernel adds them in slice order.  The same bits on every call and for
 *     either layout of dout.
 * Parity: the 3-D rules are pinned against the reference with scipy (tests/golden/tree_labels.npz); the 2-D rules are parity UNPINNED, like
 *     ucfvit_quadtree_serialize (no cv2 to record from); the nearest rules coincide with any implementation whenever w / p or p / w is whole. */
#define UCFVIT_LABEL_U8 0
#define UCFVIT_LABEL_I64 1
#define UCFVIT_RESAMPLE_SMOOTH 0
#define UCFVIT_RESAMPLE_NEAREST 1
int ucfvit_quadtree_serialize_labels(const void* labels, const int32_t* nodes, const int32_t* count, int64_t* idx, float* onehot, int64_t B,
                                     int64_t H, int64_t W, int64_t L, int64_t p, int64_t num_classes, int label_dtype, void* stream);
int ucfvit_octree_serialize_labels(const void* labels, const int32_t* nodes, const int32_t* count, int64_t* idx, float* onehot, int64_t B,
                                   int64_t N, int64_t L, int64_t p, int64_t num_classes, int label_dtype, void* stream);
int ucfvit_quadtree_deserialize(const float* seq, const int32_t* nodes, const int32_t* count, float* out, int64_t B, int64_t H, int64_t W,
                                int64_t C, int64_t L, int64_t p, int64_t stride_b, int64_t stride_c, int64_t stride_s, int64_t stride_e,
                                int64_t out_b, int64_t out_c, int64_t out_pixel, int mode, int trunc, void* stream);
int ucfvit_octree_deserialize(const float* seq, const int32_t* nodes, const int32_t* count, float* out, int64_t B, int64_t N, int64_t C,
                              int64_t L, int64_t p, int64_t stride_b, int64_t stride_c, int64_t stride_s, int64_t stride_e, int64_t out_b,
                              int64_t out_c, int64_t out_pixel, int mode, void* stream);
int64_t ucfvit_quadtree_deserialize_bwd_workspace(int64_t B, int64_t H, int64_t W, int64_t C, int64_t L, int64_t p);
int64_t ucfvit_octree_deserialize_bwd_workspace(int64_t B, int64_t N, int64_t C, int64_t L, int64_t p);
int ucfvit_quadtree_deserialize_bwd(const float* dout, const int32_t* nodes, const int32_t* count, float* dseq, int64_t B, int64_t H, int64_t W,
                                    int64_t C, int64_t L, int64_t p, int64_t stride_b, int64_t stride_c, int64_t stride_s, int64_t stride_e,
                                    int64_t out_b, int64_t out_c, int64_t out_pixel, int mode, void* workspace, void* stream);
int ucfvit_octree_deserialize_bwd(const float* dout, const int32_t* nodes, const int32_t* count, float* dseq, int64_t B, int64_t N, int64_t C,
                                  int64_t L, int64_t p, int64_t stride_b, int64_t stride_c, int64_t stride_s, int64_t stride_e, int64_t out_b,
                                  int64_t out_c, int64_t out_pixel, int mode, void* workspace, void* stream);

/* Variable aggregation (VariableMapping_Attention, simple/building_blocks.py:301-373, called by VIT.aggregate_variables,
 * simple/arch.py:414-432) with one aggregated variable: for every token row r and head h,
 *     p_v = softmax_v(scale * q_h . k[v][r][h]),  out[r][h] = sum_v p_v * v[v][r][h].
 * kv [V][R][2D] `dtype` (the kv Linear applied to the V per-variable token embeddings: k = columns [0, D), v = [D, 2D)), q fp32 [D]
 * (the q Linear applied to the learnt query), out [R][D] `dtype`, lse fp32 [R][H] (saved for backward).
 * bwd: dkv [V][R][2D], dq_rows fp32 [R][D] (its column sums = the gradient of q; ucfvit_colsum).  head_dim | D, both multiples of
 * 8 (bf16) / 4 (fp32), D <= 2048 (bf16) / 1024 (fp32), head_dim / 8 (4) a power of two. */
int ucfvit_varagg_fwd(const void* kv, const float* q, void* out, float* lse, int64_t R, int64_t V, int64_t D, int64_t head_dim, float scale,
                      int dtype, void* stream);
int ucfvit_varagg_bwd(const void* kv, const float* q, const void* out, const float* lse, const void* dout, void* dkv, float* dq_rows, int64_t R,
                      int64_t V, int64_t D, int64_t head_dim, float scale, int dtype, void* stream);

/* Softmax cross-entropy, mean over the batch (nn.CrossEntropyLoss, training_scripts/train_class_simple.py:24-30).
 * logits [B][C] dtype, labels int64 [B]; loss: fp32 scalar (device); row_loss: fp32 [B] per-sample losses (also scratch);
 * dlogits [B][C] dtype = grad_scale*(softmax - onehot)/B, or NULL. */
int ucfvit_cross_entropy(const void* logits, const int64_t* labels, float* loss, float* row_loss, void* dlogits, int64_t B,
                         int64_t C, float grad_scale, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * MAE random masking index math (MAE.random_masking, arch.py:663-681), bit-exact for distinct noise values:
 * ids_restore[b][i] = rank of noise[b][i] in its row (= argsort(argsort(noise))), ids_shuffle[b][r] = argsort(noise)[r]
 * (ids_keep = ids_shuffle[:, :len_keep]), mask[b][i] = (ids_restore[b][i] >= len_keep) ? 1 : 0.
 * int64 indices [B][L], fp32 mask [B][L], like torch.
 * ------------------------------------------------------------------------------------------------------ */
int ucfvit_mae_mask(const float* noise, int64_t* ids_shuffle, int64_t* ids_restore, float* mask, int64_t B, int64_t L,
                    int64_t len_keep, void* stream);

/* Row gather  out[b][r][:] = src[b][idx[b*idx_stride + r]][:]  (torch.gather(seq, 1, ids_keep[...,None].repeat), arch.py:675) —
 * bit-exact copy; src [B][L][D], out [B][R][D].  scatter is its adjoint for a duplicate-free idx:
 * dsrc = 0; dsrc[b][idx[b][r]][:] = dout[b][r][:]. */
int ucfvit_gather_rows(const void* src, const int64_t* idx, void* out, int64_t B, int64_t L, int64_t R, int64_t D,
                       int64_t idx_stride, int dtype, void* stream);
int ucfvit_scatter_rows(const void* dout, const int64_t* idx, void* dsrc, int64_t B, int64_t L, int64_t R, int64_t D,
                        int64_t idx_stride, int dtype, void* stream);

/* MAE un-shuffle (MAE.mask_head, arch.py:687-697): x_ = cat(x[B,R,D], mask_token repeated) ; out[b][i] = x_[b][ids_restore[b][i]] (+ pos[i]).
 * bwd: dx[b][r] = dout[b][i : ids_restore==r] ; dmask_token (fp32 [D]) (+)= sum over masked positions ; dpos (fp32 [L][D]) (+)= sum_b dout. */
int ucfvit_unshuffle_fwd(const void* x, const void* mask_token, const int64_t* ids_restore, const void* pos, void* out,
                         int64_t B, int64_t L, int64_t R, int64_t D, int dtype, void* stream);
int64_t ucfvit_unshuffle_bwd_workspace(int64_t B, int64_t D);
int ucfvit_unshuffle_bwd(const void* dout, const int64_t* ids_restore, void* dx, float* dmask_token, float* dpos,
                         int64_t B, int64_t L, int64_t R, int64_t D, int accumulate, void* workspace, int dtype, void* stream);

/* MAE reconstruction loss against patchify(img) without materialising the target (utils/misc.py:14-33 'nchpwq->nhwpqc',
 * training_scripts/train_masked_simple.py:43-47; masked variant utils/metrics.py:11-17).
 * pred [B][L][p^nd*C] dtype with per-patch order (ph,pw[,pd],c); img NCHW(D) fp32; mask fp32 [B][L] or NULL (plain MSE over all).
 * loss: fp32 scalar (device, overwritten); dpred = grad_scale * dloss/dpred (or NULL). workspace: >= 2049 floats.
 * nd = 1: the adaptive-patching target (train_masked_simple.py:24-32): img is the token sequence x fp32 [B][C][S][P], dims = {S},
 * p = P pixels per token and channel, pred [B][S][P*C] with per-token order (p, c) = rearrange 'b c s p -> b s (p c)'. */
int ucfvit_patch_mse(const void* pred, const float* img, const float* mask, float* loss, void* dpred, int64_t B, int64_t C,
                     const int64_t* dims, int nd, int64_t p, float grad_scale, float* workspace, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Fused AdamW over a flat fp32 parameter segment (torch.optim.AdamW semantics; utils/misc.py:58-84):
 *   p *= 1 - lr*wd ; m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g² ; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
 * grads are fp32 (grad_dtype F32) or bf16 (BF16), multiplied by grad_scale first.  If shadow != NULL the updated
 * parameter is also written as bf16 (the compute copy used by the bf16 kernels) in the same pass.
 * ------------------------------------------------------------------------------------------------------ */
int ucfvit_adamw(float* p, const void* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2, float grad_scale,
                 int grad_dtype, void* stream);
/* ucfvit_adamw_ema: ucfvit_adamw, and in the same pass an exponential moving average of the weights, fp32 [n]:
 *   ema[i] = ema[i] + ema_rate * (p_new[i] - ema[i]),  p_new the fp32 value just stored to p[i],  ema_rate = 1 - decay.
 * p, m, v and the shadow get the bits ucfvit_adamw gives them.  ema_rate is formed by the caller in double and rounded once (a float 0.9999
 * carries a relative error of 6e-4 in 1 - decay); it must be inside (0, 1] (1: ema = p_new; NaN is refused).  ema must be non-null and 16-byte
 * aligned.  ucfvit_adamw_scaled_ema (below) is the same for ucfvit_adamw_scaled: a skipped step leaves ema alone too. */
int ucfvit_adamw_ema(float* p, const void* g, float* m, float* v, void* shadow_bf16, float* ema, int64_t n, float lr, float beta1,
                     float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2, float grad_scale, float ema_rate,
                     int grad_dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Dynamic loss scaling with on-device skipping of non-finite steps (the reference's bf16 policy: ShardedGradScaler(init_scale=8192,
 * growth_interval=100) and its floor of 128, training_scripts/train_masked_fsdp.py:417-419,601-606; update rule = torch's
 * _amp_update_scale_, check = torch's _amp_foreach_non_finite_check_and_unscale_ without the in-place rewrite of the gradients).
 *
 * All scaler state is ONE device array of UCFVIT_GS_STATE_FLOATS fp32 owned by the caller; the host never has to read it during a step:
 *   [SCALE] loss scale   [INV_SCALE] (float)(1.0 / scale)   [FOUND_INF] 0 or 1, ORed by the check, cleared by the update
 *   [GROWTH_TRACKER] consecutive applied steps since the scale last changed   [APPLIED_STEPS] / [SKIPPED_STEPS] counts (fp32: exact to 2^24)
 *   [GROWTH_FACTOR] [BACKOFF_FACTOR] [GROWTH_INTERVAL] [MIN_SCALE] constants (MIN_SCALE 0: no floor); the rest is reserved (zero).
 *
 * grad_nonfinite:  one read-only pass; sets state[FOUND_INF] = 1 if any g[i] * mult * state[INV_SCALE] is +-Inf or NaN (the value
 *                  adamw_scaled consumes when mult is its grad_scale).  Never clears the flag: calls over several segments OR together.
 * adamw_scaled:    ucfvit_adamw, except that (1) every workgroup returns before touching p, m, v or the shadow when state[FOUND_INF] is set,
 *                  (2) gradients are multiplied by grad_scale * state[INV_SCALE], (3) the bias corrections 1 - beta^t are formed on the device, in
 *                  double from the double betas and rounded once to fp32, with t = state[APPLIED_STEPS] + 1: a skipped step does not advance t.
 * grad_scaler_update: after the adamw_scaled launches of a step.  FOUND_INF set: scale *= BACKOFF_FACTOR, tracker = 0, SKIPPED_STEPS += 1.
 *                  Otherwise APPLIED_STEPS += 1, tracker += 1, and when the tracker reaches GROWTH_INTERVAL it returns to 0 and scale becomes
 *                  scale * GROWTH_FACTOR unless that is not finite.  Then scale = max(scale, MIN_SCALE), INV_SCALE is recomputed, FOUND_INF cleared.
 * ------------------------------------------------------------------------------------------------------ */
#define UCFVIT_GS_SCALE 0
#define UCFVIT_GS_INV_SCALE 1
#define UCFVIT_GS_FOUND_INF 2
#define UCFVIT_GS_GROWTH_TRACKER 3
#define UCFVIT_GS_APPLIED_STEPS 4
#define UCFVIT_GS_SKIPPED_STEPS 5
#define UCFVIT_GS_GROWTH_FACTOR 6
#define UCFVIT_GS_BACKOFF_FACTOR 7
#define UCFVIT_GS_GROWTH_INTERVAL 8
#define UCFVIT_GS_MIN_SCALE 9
#define UCFVIT_GS_STATE_FLOATS 16
int ucfvit_grad_nonfinite(const void* g, int64_t n, int dtype, float mult, float* state, void* stream);
int ucfvit_adamw_scaled(float* p, const void* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr, double beta1,
                        double beta2, float eps, float weight_decay, float grad_scale, int grad_dtype, const float* state,
                        void* stream);
int ucfvit_adamw_scaled_ema(float* p, const void* g, float* m, float* v, void* shadow_bf16, float* ema, int64_t n, float lr, double beta1,
                            double beta2, float eps, float weight_decay, float grad_scale, float ema_rate, int grad_dtype,
                            const float* state, void* stream);
int ucfvit_grad_scaler_update(float* state, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Gradient clipping by global L2 norm (torch.nn.utils.clip_grad_norm_'s rule) folded into AdamW: gradients are never rewritten and the host
 * never reads the norm.  The clip state is ONE device array of UCFVIT_GC_STATE_FLOATS fp32 owned by the caller:
 *   [MAX_NORM] the threshold, written by the host   [NORM] the global norm of the last step before clipping, of the gradients as AdamW
 *   consumes them (after grad_scale and, under a loss scaler, after the division by the scale)   [COEF] min(1, MAX_NORM / (NORM + 1e-6));
 *   the rest is spare.
 *
 * grad_sqnorm:   one read-only pass over one gradient segment (fp32 or bf16).  Workgroup b writes partials[b] = the sum in double of x^2,
 *                x = g[i] * k rounded to fp32 as AdamW forms it, k = mult (gs_state NULL) or mult * gs_state[INV_SCALE].  With gs_state the
 *                same pass sets gs_state[FOUND_INF] under ucfvit_grad_nonfinite's rule and never clears it: it replaces that launch.
 *                ucfvit_grad_sqnorm_partials(n, dtype) (host only) is the number of partials such a call writes: 0 for n = 0, when g and
 *                partials may be NULL; -1 for a negative n or an unknown dtype.  Segments are laid side by side in one workspace with it.
 * grad_clip_coef: one workgroup sums `count` partials in a fixed order and writes NORM = (float)sqrt(sum) and COEF.  An Inf norm gives
 *                COEF = 0, a NaN norm a NaN COEF, as torch's clamp does.  count = 0: NORM = 0.
 *                No atomics anywhere: NORM's bits are a function of the gradients and the segment layout alone, so data-parallel ranks
 *                reach the same COEF from the same all-reduced buffer without a collective.
 * adamw_clipped: ema NULL, gs_state NULL: ucfvit_adamw with the gradient factor grad_scale * COEF.  ema given: ucfvit_adamw_ema likewise.
 *                gs_state given: ucfvit_adamw_scaled(_ema) with (grad_scale * INV_SCALE) * COEF; bias_corr1/2 are then ignored, the
 *                corrections come from APPLIED_STEPS, and a step whose check fired returns before touching anything.  With COEF = 1 every
 *                output has the bits of the respective entry point without clipping.
 * ------------------------------------------------------------------------------------------------------ */
#define UCFVIT_GC_MAX_NORM 0
#define UCFVIT_GC_NORM 1
#define UCFVIT_GC_COEF 2
#define UCFVIT_GC_STATE_FLOATS 8
int64_t ucfvit_grad_sqnorm_partials(int64_t n, int dtype);
int ucfvit_grad_sqnorm(const void* g, int64_t n, int dtype, float mult, float* gs_state, double* partials, void* stream);
int ucfvit_grad_clip_coef(const double* partials, int64_t count, float* clip_state, void* stream);
int ucfvit_adamw_clipped(float* p, const void* g, float* m, float* v, void* shadow_bf16, float* ema, int64_t n, float lr, double beta1,
                         double beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2, float grad_scale, float ema_rate,
                         int grad_dtype, const float* gs_state, const float* clip_state, void* stream);

/* dtype conversion / scaling helpers (fp32 master → bf16 shadow cast; bf16 gradient transport for the DP all-reduce) */
int ucfvit_cast(const void* src, void* dst, int64_t n, int src_dtype, int dst_dtype, float scale, void* stream);

/* Batched 2-D transposes of bf16 matrices inside one flat buffer: the transposed shadow of every nn.Linear weight, so the
 * data-gradient GEMMs (dx = dy·W, building_blocks.py:123,127,159,190 under autograd) read both operands contraction-contiguous.
 * table (device): int64 [n_mats][5] = {src_off, dst_off, rows, cols, first_tile} in elements; rows, cols multiples of 8;
 * a matrix uses ceil(rows/64)*ceil(cols/64) tiles; total_tiles = sum. */
int ucfvit_transpose_batched(const void* src, void* dst, const int64_t* table, int64_t n_mats, int64_t total_tiles, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * UNETR convolutional decoder, HBM-bound part.  Tensors in torch's N C (D) H W layout: `rows` = N*C contiguous rows
 * of S voxels.  Reference call sites: src/UCF_VIT/simple/arch.py:808-940 (monai UnetResBlock: conv -> instance norm -> LeakyReLU(0.01) ->
 * conv -> instance norm, + residual, LeakyReLU), training_scripts/train_unetr_simple.py:38 (monai DiceCELoss(to_onehot_y, softmax,
 * squared_pred)); monai is not vendored: parity is against the plain-torch restatement of these formulas.
 *
 * ucfvit_instnorm_fwd:  mean / rstd per row (biased variance, eps), y = lrelu((x - mean) rstd [+ res], slope)   (slope 1: no activation)
 * ucfvit_instnorm_bwd:  dn = dy (y > 0 ? 1 : slope); dres = dn (if dres); dx = rstd (dn - mean(dn) - n mean(dn n)), n = (x - mean) rstd
 * workspace: ucfvit_instnorm_workspace(rows, S) bytes (both directions).  S must be a multiple of 16 bytes / element size.
 * ------------------------------------------------------------------------------------------------------ */
int64_t ucfvit_instnorm_workspace(int64_t rows, int64_t S);
int ucfvit_instnorm_fwd(const void* x, const void* res, void* y, float* mean, float* rstd, int64_t rows, int64_t S, float eps, float slope,
                        void* workspace, int dtype, void* stream);
int ucfvit_instnorm_bwd(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, void* dx, void* dres, int64_t rows,
                        int64_t S, float slope, void* workspace, int dtype, void* stream);
/* Dice + cross-entropy of logits [B][n][S] (2 <= n <= 8) against int64 labels [B][S], fused forward + backward:
 *   p = softmax over the classes; dice_bc = 1 - (2 sum_v p onehot + smooth_nr) / (sum_v p^2 + sum_v onehot + smooth_dr);
 *   loss = mean_bc dice_bc + mean_bv -log p[label];  dlogits (dtype, may be NULL) = grad_scale * d loss / d logits.
 * Logits element (b, class c, voxel i) at logits[b stride_b + c stride_c + i stride_s] (dlogits alike): N C (D) H W is (n S, S, 1); a
 * channels-last tensor whose voxel rows are ld apart is (S ld, 1, ld). */
int64_t ucfvit_dice_ce_workspace(int64_t B, int64_t S);
int ucfvit_dice_ce(const void* logits, const int64_t* labels, float* loss, void* dlogits, int64_t B, int64_t n, int64_t S, int64_t stride_b,
                   int64_t stride_c, int64_t stride_s, float smooth_nr, float smooth_dr, float grad_scale, void* workspace, int dtype, void* stream);

/* Dice + CE over a volume SHARDED across the ranks of a sequence-parallel group (X-slabs of the UNETR decoder; no reference counterpart: the
 * reference asserts seq_par_size == 1, training_scripts/train_masked_fsdp.py:220 — the loss itself is train_unetr_simple.py:38).  Every term
 * is a function of per-(batch, class) sums over voxels: ucfvit_dice_ce_stats writes this rank's sums (stats: B x ucfvit_dice_ce_stats_floats()
 * floats; workspace: ucfvit_dice_ce_workspace bytes), the caller adds them over the group, ucfvit_dice_ce_from_stats evaluates the loss of the
 * WHOLE volume from the summed stats (rewritten in place) and the gradient of the LOCAL logits (S local voxels, S_total voxels of the whole
 * volume, both per batch element).  Unsharded: S_total = S gives ucfvit_dice_ce's loss up to rounding. */
int ucfvit_dice_ce_stats_floats(void);
int ucfvit_dice_ce_stats(const void* logits, const int64_t* labels, float* stats, int64_t B, int64_t n, int64_t S, int64_t stride_b, int64_t stride_c,
                         int64_t stride_s, void* workspace, int dtype, void* stream);
int ucfvit_dice_ce_from_stats(const void* logits, const int64_t* labels, float* stats, float* loss, void* dlogits, int64_t B, int64_t n, int64_t S,
                              int64_t S_total, int64_t stride_b, int64_t stride_c, int64_t stride_s, float smooth_nr, float smooth_dr,
                              float grad_scale, int dtype, void* stream);

/* Segmentation and Dice-accuracy counts of logits [B][n][S] (2 <= n <= 8) against int64 labels [B][S] in one pass (csrc/seg_metric.hip;
 * reference train_unetr_simple.py:399-401,453-460 and inference_unetr_simple.py: torch.argmax, one_hot, monai DiceMetric):
 *   pred   uint8 [B][S] dense (may be NULL): argmax over the classes as torch.argmax(dim = 1) takes it: the FIRST maximal class wins a
 *          tie, a NaN counts as maximal and the first NaN wins, +-inf are ordinary values;
 *   counts int64 [B][3][8]: per batch element and class c  TP[c] = #voxels with argmax == c and label == c, PRED[c] = #voxels with
 *          argmax == c, LAB[c] = #voxels with label == c; classes >= n hold exact zeros.
 * A label outside [0, n) adds to no LAB and no TP entry; its voxel still gets a prediction and a PRED count (the reference's one_hot
 * would raise, which needs a host synchronisation).  All counts are integers: no floating point, no atomics, the same bits on every call.
 * Addressing, dtype (fp32 or bf16) and limits (B in 1..65535) are ucfvit_dice_ce's: element (b, c, i) at logits[b stride_b + c stride_c +
 * i stride_s].  Channels-last (stride_c == 1, rows ld >= n apart) and N C (D) H W (stride_s == 1) have kernels that load and store whole
 * vectors where base and strides are aligned for them; everything else runs one voxel per lane.  ucfvit_seg_counts_route writes the name of
 * the kernel a call would take ("cl nv<2|4|8> ...", "ncs vpt8 ...", "scalar ...") and its constants to out (at most cap bytes with the
 * terminator) and returns the length of the whole name.  workspace: ucfvit_seg_counts_workspace(B, S) bytes. */
int64_t ucfvit_seg_counts_workspace(int64_t B, int64_t S);
int ucfvit_seg_counts(const void* logits, const int64_t* labels, uint8_t* pred, int64_t* counts, int64_t B, int64_t n, int64_t S, int64_t stride_b,
                      int64_t stride_c, int64_t stride_s, void* workspace, int dtype, void* stream);
int ucfvit_seg_counts_route(const void* logits, const int64_t* labels, const uint8_t* pred, int64_t B, int64_t n, int64_t S, int64_t stride_b,
                            int64_t stride_c, int64_t stride_s, int dtype, char* out, int64_t cap);

/* ------------------------------------------------------------------------------------------------------
 * SAP segmentation head (reference simple/arch.py:491-536): ConvTranspose{2,3}d(D -> K, kernel = stride = p, no bias) followed by a 1x1
 * convolution (K -> C, bias) with no nonlinearity between them, run as ONE Linear layer on the tokens:
 *   W_eff[(delta, c)][d] = sum_k W_neck[d][k][delta] W_head[c][k]        delta = the P = p^nd offsets inside a patch, (kx p + ky) p + kz
 *   rows[B S][P C] = tokens[B S][D] · W_effᵀ  (ucfvit_gemm, fp32 output),  map[b][c][voxel] = rows[b, token][(delta, c)] + bias[c]
 * token t = (tx s + ty) s + tz of the s^nd grid, voxel (tx p + kx, ty p + ky, tz p + kz) of the (s p)^nd map; nd = 2 or 3, any p, s, C >= 1.
 * Nothing here uses a floating-point atomic; every sum has a fixed order (results are bitwise reproducible).
 *
 * ucfvit_sap_fold:    w_neck fp32 [D][K][P], w_head fp32 [C][K] -> w_eff [P C][D] in `dtype` (summed in fp32 over k ascending, rounded once)
 * ucfvit_sap_unfold:  dw_eff fp32 [P C][D] -> dw_neck fp32 [D][K][P] = sum_c dw_eff[(delta, c)][d] w_head[c][k] and
 *                     dw_head fp32 [C][K] = sum_{d, delta} dw_eff[(delta, c)][d] w_neck[d][k][delta] (per d, then over d: ucfvit_reduce_rows);
 *                     workspace: ucfvit_sap_unfold_workspace bytes.  P C <= 16384.
 * ucfvit_sap_scatter_fwd: rows fp32 -> map fp32, one add per element.
 * ucfvit_sap_scatter_bwd: dmap fp32 -> drows in `dtype` (the inverse permutation) and, unless dbias is NULL, dbias fp32 [C] = sum over b
 *                     and voxels (two stages; workspace: ucfvit_sap_scatter_bwd_workspace bytes). */
int ucfvit_sap_fold(const float* w_neck, const float* w_head, void* w_eff, int64_t D, int64_t K, int64_t P, int64_t C, int dtype, void* stream);
int64_t ucfvit_sap_unfold_workspace(int64_t D, int64_t K, int64_t C);
int ucfvit_sap_unfold(const float* dw_eff, const float* w_neck, const float* w_head, float* dw_neck, float* dw_head, int64_t D, int64_t K,
                      int64_t P, int64_t C, void* workspace, void* stream);
int ucfvit_sap_scatter_fwd(const float* rows, const float* bias, float* map, int64_t B, int64_t s, int64_t p, int64_t C, int nd, void* stream);
int64_t ucfvit_sap_scatter_bwd_workspace(int64_t B, int64_t s, int64_t p, int64_t C, int nd);
int ucfvit_sap_scatter_bwd(const float* dmap, void* drows, float* dbias, int64_t B, int64_t s, int64_t p, int64_t C, int nd, void* workspace,
                           int dtype, void* stream);

/* Dice + binary cross-entropy over channels 1..C-1 of a segmentation map (reference utils/metrics.py:95-121, the loss of
 * train_sap_simple.py): p = sigmoid(z), I = sum p t, n = B (C - 1) S,
 *   loss = weight mean(BCE) + (1 - weight) (1 - (2 I + smooth) / (sum p + sum t + smooth))
 * logits [B][C][S] contiguous in `dtype`, targets fp32 [B][C][S] with values in [0, 1] (not necessarily one-hot).
 * BCE(z, t) = t min(softplus(-z), 100) + (1 - t) min(softplus(z), 100): binary_cross_entropy(sigmoid(z), t) with its clamp of the logarithms
 * at -100, evaluated without forming log(sigmoid) (so it stays exact where fp32 sigmoid has rounded to 0 or 1, |z| > ~17).
 * ucfvit_dice_bce_stats:      one pass; stats fp32 [ucfvit_dice_bce_stats_floats() = 4] = sum p t, sum p, sum t, sum BCE (per-workgroup partial
 *                             sums, then one fixed-order sum of the partials); workspace: ucfvit_dice_bce_workspace bytes.
 * ucfvit_dice_bce_from_stats: loss (unless NULL) and dlogits (unless NULL; fp32 whatever `dtype`, channel 0 exact zeros) =
 *                             g (weight (p - t) / n + (1 - weight) p (1 - p) ((2 I + smooth) / Dn^2 - 2 t / Dn)),  Dn = sum p + sum t + smooth,
 *                             g = grad_scale, times *grad_scale_dev when that device pointer is not NULL (the upstream gradient of autograd,
 *                             read on the device: no host synchronisation). */
int ucfvit_dice_bce_stats_floats(void);
int64_t ucfvit_dice_bce_workspace(int64_t B, int64_t C, int64_t S);
int ucfvit_dice_bce_stats(const void* logits, const float* targets, float* stats, int64_t B, int64_t C, int64_t S, void* workspace, int dtype,
                          void* stream);
int ucfvit_dice_bce_from_stats(const void* logits, const float* targets, const float* stats, float* loss, float* dlogits, int64_t B, int64_t C,
                               int64_t S, float weight, float smooth, float grad_scale, const float* grad_scale_dev, int dtype, void* stream);

/* Channels-last instance norm (+ LeakyReLU, + residual) for the layout of the convolution kernels below: x, res, y [B][S][C] bf16,
 * mean / rstd [B][C] fp32; C a power of two in 8..2048.  Same formulas as ucfvit_instnorm_fwd / _bwd, one entry point per pass:
 *   forward:  ucfvit_instnorm_cl_stats (mean / rstd of x), then ucfvit_instnorm_cl_apply (y = lrelu((x - mean) rstd [+ res], slope)).
 *   backward: ucfvit_instnorm_cl_bwd_sums leaves the per-(batch, channel) MEANS over the voxels of dy' (the gradient behind the activation
 *             mask) and of dy' xhat in m1 / m2 [B][C], then ucfvit_instnorm_cl_bwd_apply writes dx (and dres).  A volume sharded across
 *             ranks averages m1 / m2 over the ranks in between (equal slabs: the mean over the whole volume).
 * had_res: the forward pass added a residual, so the activation mask is read from y; without one sign(y) = sign(x - mean) and y is not read
 * at all (dres requires had_res).  ld_dy: voxel-row stride of dy in elements (C for a dense tensor; larger when dy is a channel slice of a
 * concatenation's gradient).  workspace: ucfvit_instnorm_cl_workspace bytes, for _stats and _bwd_sums; its last 2 B C floats are not
 * touched by either, so a caller may keep m1 / m2 there.  (The forward statistics of a sharded volume combine from the ranks'
 * ucfvit_instnorm_cl_stats by the parallel-variance formula: mean = avg(mean_r), var = avg(var_r + (mean_r - mean)^2), in double.) */
int64_t ucfvit_instnorm_cl_workspace(int64_t B, int64_t S, int64_t C);
int ucfvit_instnorm_cl_bwd_sums(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, float* m1, float* m2, int64_t B,
                                int64_t S, int64_t C, int64_t ld_dy, float slope, int had_res, void* workspace, void* stream);
int ucfvit_instnorm_cl_bwd_apply(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, const float* m1, const float* m2,
                                 void* dx, void* dres, int64_t B, int64_t S, int64_t C, int64_t ld_dy, float slope, int had_res, void* stream);

/* The tail of a residual block whose residual branch is itself normalised (monai UnetResBlock with the 1x1x1 projection):
 *   ucfvit_instnorm_cl_stats:  mean / rstd of x, one per branch
 *   ucfvit_instnorm_cl_apply2: y = lrelu((x - mean) rstd + (x2 - mean2) rstd2, slope) — the normalised branch is never materialised
 *   ucfvit_instnorm_cl_bwd2:   dx, dx2 from dy, y (activation mask) and the raw inputs: one pair of passes for both normalisations
 *                              (workspace: ucfvit_instnorm_cl_bwd2_workspace bytes). */
int ucfvit_instnorm_cl_stats(const void* x, float* mean, float* rstd, int64_t B, int64_t S, int64_t C, float eps, void* workspace, void* stream);
int ucfvit_instnorm_cl_apply(const void* x, const void* res, void* y, const float* mean, const float* rstd, int64_t B, int64_t S, int64_t C,
                             float slope, void* stream); /* the apply pass alone, statistics given */
int ucfvit_instnorm_cl_apply2(const void* x, const float* mean, const float* rstd, const void* x2, const float* mean2, const float* rstd2, void* y,
                              int64_t B, int64_t S, int64_t C, float slope, void* stream);
int64_t ucfvit_instnorm_cl_bwd2_workspace(int64_t B, int64_t S, int64_t C);
int ucfvit_instnorm_cl_bwd2(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, const void* x2, const float* mean2,
                            const float* rstd2, void* dx, void* dx2, int64_t B, int64_t S, int64_t C, int64_t ld_dy, float slope, void* workspace,
                            void* stream);

/* ------------------------------------------------------------------------------------------------------
 * UNETR convolutional decoder, convolutions.  Reference call sites: src/UCF_VIT/simple/arch.py:808-940 — monai's
 * blocks are chains of Conv3d(kernel 3, stride 1, padding 1, no bias) and ConvTranspose3d(kernel 2, stride 2, no bias); these entry
 * points replace torch.nn.functional.conv3d / conv_transpose3d (MIOpen) under them, and the 1x1x1 layers (residual projections, the
 * UnetOutBlock head, the transposed convolutions' channel mixing at small channel counts).
 * Activations are channels-last bf16 [B][X][Y][Z][C] (= torch.channels_last_3d memory of an [B, C, X, Y, Z] tensor).
 *
 * ucfvit_conv3d_fwd: y[v ldy + co] = bias[co] + sum_{tap, ci} w[co][ci][tap] x[v + tap - pad][ci] for co < cout_store (zero outside the
 *   volume; ksize 3 with padding 1, or ksize 1 = a pointwise layer over tall-skinny voxel rows), fp32 accumulation on MFMA, output bf16 or
 *   fp32 (out_dtype).  Cin in {8, 16, 32 k}, Cout = 16 k = the rows of w_packed; cout_store <= Cout channels are written with row stride
 *   ldy (a 4-class head writes [V][4] from a 16-row weight block); bias fp32 [Cout] or NULL; accumulate: y += result (the second of two
 *   data gradients that flow into the same input, e.g. a residual block's 3x3x3 and 1x1x1 branches).
 *   stats_partial (may be NULL): the instance-norm statistics of the OUTPUT as a by-product — per channel the count, the mean and
 *   M2 = sum (q - mean)^2 of the rounded outputs each wave stored (accumulated relative to a per-wave shift, so a channel whose |mean| is far
 *   larger than its spread keeps its variance bits), [B][rows][3][Cout] fp32 with rows = ucfvit_conv3d_fwd_stats_rows(...) (0: the kernel
 *   serving this shape has no such epilogue); ucfvit_instnorm_cl_stats_fold combines the rows (parallel-variance formula, double) into
 *   mean / rstd, which saves the statistics pass over the output.
 *   w_packed (bf16) holds the weights per 32-wide contraction step: with CPC = min(Cin, 32), TPS = 32 / CPC taps per step and
 *   NTS = ceil(ksize^3 / TPS) steps per channel chunk, w_packed[cc][ts][co][kk] = w[co][cc CPC + kk % CPC][tap] for tap = ts TPS + kk / CPC
 *   (zero when tap >= ksize^3); tap = (dx 3 + dy) 3 + dz.  The data gradient is the same call on dy with the flipped, transposed weights.
 * ucfvit_conv3d_wgrad: dw[tap][co][ci] = sum_v dy[v][co] x[v + tap - pad][ci] in fp32, written as
 *   [Cout / (16 MB)][Cin / CPC][ksize^3][16 MB][max(CPC, 16)] with MB = 2 when Cout % 32 == 0, else 1 (ucfvit_conv3d_wgrad_size floats; for
 *   CPC = 8 columns 8..15 are scratch).  workspace: ucfvit_conv3d_wgrad_workspace bytes (per-workgroup partials, folded in a fixed order:
 *   deterministic).
 * Dispatch: conv_fwd_route() / conv_wgrad_route() in csrc/conv_route.h decide once per call which instantiation runs and with what
 *   geometry; the size queries return fields of the same route and ucfvit_conv3d_route names it.
 * ucfvit_depth_to_space2: the transposed convolution is the GEMM x[V][Cin] * w[Cin][8 Cout] followed by this shuffle of
 *   cols [B Xi Yi Zi][(dx, dy, dz)][C] into out [B][2 Xi][2 Yi][2 Zi][C] (to_space = 1) — or its inverse for the backward pass (0).  The
 *   space tensor may be a channel slice of a wider channels-last buffer (voxel-row stride ld_space elements): the up-sampled map is written
 *   straight into the concatenation the next block reads; with `skip` (dense [..][Cs], to_space = 1) the skip connection is copied behind it
 *   in the same pass, so the concatenation is written as whole rows.
 * ucfvit_pad_channels8: fp32 N C D H W input [B][C][S] with C <= 8 -> bf16 channels-last [B][S][8] (channels C..7 zero): the input volume as
 *   an operand of the kernels above.
 * ucfvit_pad_rows8: V rows of C <= 8 values (src_dtype UCFVIT_F32 or UCFVIT_BF16, row stride ld elements) -> dense bf16 [V][8], columns C..7
 *   zero: the gradient of the output head's logits (_hip/conv.py:Conv1x1x1Fn.backward) as an operand of the kernels above, in one pass.
 * ------------------------------------------------------------------------------------------------------ */
int ucfvit_conv3d_fwd(const void* x, const void* w_packed, const float* bias, void* y, int64_t B, int64_t X, int64_t Y, int64_t Z, int64_t Cin,
                      int64_t Cout, int ksize, int64_t ldy, int64_t cout_store, int out_dtype, int accumulate, float* stats_partial, void* stream);
int64_t ucfvit_conv3d_fwd_stats_rows(int64_t B, int64_t X, int64_t Y, int64_t Z, int64_t Cin, int64_t Cout, int ksize, int has_bias);
int ucfvit_instnorm_cl_stats_fold(const float* partial, float* mean, float* rstd, int64_t B, int64_t S, int64_t C, int64_t rows, float eps,
                                  void* workspace /* B * 256 * 2 C floats, or NULL */, void* stream);
int64_t ucfvit_conv3d_wgrad_size(int64_t Cin, int64_t Cout, int ksize);
int64_t ucfvit_conv3d_wgrad_workspace(int64_t B, int64_t X, int64_t Y, int64_t Z, int64_t Cin, int64_t Cout, int ksize);
int ucfvit_conv3d_wgrad(const void* x, const void* dy, float* dw_packed, void* workspace, int64_t B, int64_t X, int64_t Y, int64_t Z,
                        int64_t Cin, int64_t Cout, int ksize, void* stream);
/* which kernel ucfvit_conv3d_fwd (pass = 0; the data gradient is the same call) or ucfvit_conv3d_wgrad (pass = 1, which ignores has_bias,
 * out_dtype, ldy and cout_store) would run for these arguments, as text.  mode = the value of the test hook UCFVIT_CONV_STRIP to assume
 * (0 .. 3), or -1 for this process's own.  Forward: "tile", "strip-fast", "strip-branching" (the column kernel with its branch-free or its
 * branching memory operations; "-share" appended for 3x3x3 with 16 input channels) or "mc1" / "mc2" / "mc4" (the multi-chunk column kernel
 * and its z tiles), then the instantiation and the statistics rows per batch element (0: no statistics epilogue), e.g.
 * "strip-fast-share cpc16 ks3 nb1 4x8 depth2 rows8".  Weight gradient: "wgrad cpc32 ks3 mb2 n_wg24 tiles_per_wg2 slots1 n_out884736"
 * (n_wg workgroups, each walking tiles_per_wg tiles and writing `slots` partials of n_out floats).  Host only, no HIP call; returns the
 * length (the text is cut to cap - 1 characters), or < 0 for arguments the entry points refuse */
int ucfvit_conv3d_route(int pass, int64_t B, int64_t X, int64_t Y, int64_t Z, int64_t Cin, int64_t Cout, int ksize, int has_bias, int out_dtype,
                        int64_t ldy, int64_t cout_store, int mode, char* out, int64_t cap);
int ucfvit_depth_to_space2(const void* src, void* dst, int64_t B, int64_t Xi, int64_t Yi, int64_t Zi, int64_t C, int64_t ld_space, int to_space,
                           const void* skip, int64_t Cs, void* stream);
int ucfvit_pad_channels8(const float* src, void* dst, int64_t B, int64_t C, int64_t S, void* stream);
int ucfvit_pad_rows8(const void* src, int src_dtype, void* dst, int64_t V, int64_t C, int64_t ld, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * UNETR convolutional decoder in the plane (csrc/conv2d.hip).  Reference call sites: src/UCF_VIT/simple/arch.py:794-797 — with twoD the
 * monai blocks are built with spatial_dims = 2: chains of Conv2d(kernel 3, stride 1, padding 1, no bias) and ConvTranspose2d(kernel 2,
 * stride 2, no bias).  Activations are channels-last bf16 [B][X][Y][C] (= torch.channels_last memory of a [B, C, X, Y] tensor).  Only the
 * neighbourhood arithmetic is new: the pointwise layers (residual 1x1 projections, the output head, the transposed convolution's channel
 * mixing x[V][Cin] * w[Cin][4 Cout]) are geometry-free and go through ucfvit_conv3d_fwd / _wgrad with ksize 1 over a factorisation of
 * X Y; the instance-norm family, ucfvit_pad_channels8, ucfvit_pad_rows8 and ucfvit_dice_ce take [B][S][C] as they are.
 *
 * ucfvit_conv2d_fwd: y[p ldy + co] = bias[co] + sum_{tap, ci} w[co][ci][tap] x[p + tap - 1][ci] for co < cout_store: 3 x 3, stride 1,
 *   padding 1, zero outside the image, tap = dx 3 + dy; implicit GEMM on mfma_f32_16x16x32_bf16 with fp32 accumulation, the input halo
 *   staged in LDS.  Cin in {8, 16, 32 k}, Cout = 16 k = the rows of w_packed; the output contract is that of ucfvit_conv3d_fwd: out_dtype
 *   bf16 or fp32, row stride ldy, cout_store <= Cout channels written, accumulate (y += result), bias fp32 [Cout] or NULL.  No statistics
 *   epilogue: the norm statistics of the output come from ucfvit_instnorm_cl_stats.
 *   w_packed (bf16) is the 3-D definition with 9 taps: with CPC = min(Cin, 32), TPS = 32 / CPC taps per step and NTS = ceil(9 / TPS) steps
 *   per channel chunk, w_packed[cc][ts][co][kk] = w[co][cc CPC + kk % CPC][tap] for tap = ts TPS + kk / CPC (zero when tap >= 9).  The
 *   data gradient is the same call on dy with the flipped, transposed weights.
 * ucfvit_conv2d_wgrad: dw[tap][co][ci] = sum_p dy[p][co] x[p + tap - 1][ci] in fp32, written as
 *   [Cout / (16 MB)][Cin / CPC][9][16 MB][max(CPC, 16)] with MB = 2 when Cout % 32 == 0, else 1 (ucfvit_conv2d_wgrad_size floats; for
 *   CPC = 8 columns 8..15 are scratch).  workspace: ucfvit_conv2d_wgrad_workspace bytes (one partial per workgroup, folded in a fixed
 *   order by ucfvit_reduce_rows: no atomics, the same bits on every call).  Both size queries return 0 for a shape the kernels refuse.
 * Dispatch: conv2d_fwd_route() / conv2d_wgrad_route() in csrc/conv2d_route.h decide once per call which instantiation runs and with what
 *   geometry; the size queries return fields of the same route and ucfvit_conv2d_route names it.
 * ucfvit_conv2d_route: which kernel ucfvit_conv2d_fwd (pass = 0; the data gradient is the same call) or ucfvit_conv2d_wgrad (pass = 1,
 *   which ignores has_bias, out_dtype, ldy and cout_store) would run for these arguments, as text: "tile2d cpc32 nb4 8x16 bf16 grid64x2"
 *   (channels per chunk, 16-channel output blocks per workgroup, the tile in pixels, the output type, the grid) or
 *   "wgrad2d cpc16 mb1 n_wg8 tiles_per_wg1 n_out2304".  Host only, no HIP call; returns the length (the text is cut to cap - 1 characters),
 *   or < 0 for arguments the entry points refuse.
 * ucfvit_depth_to_space2_2d: the shuffle behind the 2 x 2 stride-2 transposed convolution, cols [B Xi Yi][(dx, dy)][C] into
 *   out [B][2 Xi][2 Yi][C] (to_space = 1) or its inverse (0), with the row stride ld_space and the fused skip copy of ucfvit_depth_to_space2.
 * ------------------------------------------------------------------------------------------------------ */
int ucfvit_conv2d_fwd(const void* x, const void* w_packed, const float* bias, void* y, int64_t B, int64_t X, int64_t Y, int64_t Cin, int64_t Cout,
                      int64_t ldy, int64_t cout_store, int out_dtype, int accumulate, void* stream);
int64_t ucfvit_conv2d_wgrad_size(int64_t Cin, int64_t Cout);
int64_t ucfvit_conv2d_wgrad_workspace(int64_t B, int64_t X, int64_t Y, int64_t Cin, int64_t Cout);
int ucfvit_conv2d_wgrad(const void* x, const void* dy, float* dw_packed, void* workspace, int64_t B, int64_t X, int64_t Y, int64_t Cin,
                        int64_t Cout, void* stream);
int ucfvit_conv2d_route(int pass, int64_t B, int64_t X, int64_t Y, int64_t Cin, int64_t Cout, int has_bias, int out_dtype, int64_t ldy,
                        int64_t cout_store, char* out, int64_t cap);
int ucfvit_depth_to_space2_2d(const void* src, void* dst, int64_t B, int64_t Xi, int64_t Yi, int64_t C, int64_t ld_space, int to_space,
                              const void* skip, int64_t Cs, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * UNETR decoder, align-corners trilinear resampling (csrc/resample.hip).  Reference call sites: src/UCF_VIT/simple/arch.py:887-906, 942-943,
 * 989-991 — when the token grid times 16 is not the tile size (patch 4 / adaptive patching), dec1 goes through
 * nn.Upsample(size=img_size, mode='trilinear', align_corners=True) before decoder2.  Channels-last bf16 [B][X][Y][Z][C], C % 8 == 0; every
 * axis is resampled on its own, up, down or not at all (Xi -> Xo, ...), with torch's index and weight formula in fp32:
 *   scale = (in - 1) / (out - 1) (0 when out == 1), src = scale * dst, i0 = (int) src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1.
 *
 * ucfvit_resample_trilinear_fwd: x dense [B][Xi][Yi][Zi][C] -> y[v ld_dst + c] over the [B][Xo][Yo][Zo] output voxels v, the 8 taps summed
 *   in fp32 and rounded once.  ld_dst >= C, a multiple of 8 (larger: y is a channel slice of a wider channels-last buffer, pointer at the
 *   slice's first channel).  skip (may be NULL): a dense [B][Xo][Yo][Zo][Cs] map copied behind the C channels of every row in the same pass
 *   (Cs % 8 == 0, ld_dst >= C + Cs): the concatenation (resampled, skip) of UnetrUpBlock written as whole rows, as ucfvit_depth_to_space2.
 * ucfvit_resample_trilinear_bwd: dx dense [B][Xi][Yi][Zi][C] = the transposed operator applied to dy[v ld_dy + c] (ld_dy >= C, a multiple
 *   of 8: the gradient may be a channel slice of the concatenation's gradient).  Gather form: each input voxel sums the output voxels whose
 *   stencil touches it in a fixed order, fp32, one rounding; no atomics, bitwise reproducible.
 * ------------------------------------------------------------------------------------------------------ */
int ucfvit_resample_trilinear_fwd(const void* x, void* y, int64_t B, int64_t Xi, int64_t Yi, int64_t Zi, int64_t Xo, int64_t Yo, int64_t Zo,
                                  int64_t C, int64_t ld_dst, const void* skip, int64_t Cs, void* stream);
int ucfvit_resample_trilinear_bwd(const void* dy, void* dx, int64_t B, int64_t Xi, int64_t Yi, int64_t Zi, int64_t Xo, int64_t Yo, int64_t Zo,
                                  int64_t C, int64_t ld_dy, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Stochastic depth (csrc/drop_path.hip): timm's DropPath(drop_prob, scale_by_keep=True), which the reference's Block imports.  Every sample
 * b of the batch has one scale s[b] (fp32, on the device): 0 for a dropped sample, 1 / keep (or 1) for a kept one.  Row r of a
 * [rows][D] token matrix belongs to sample r / rows_per_sample; rows must be a multiple of rows_per_sample and below 2^30, s holds
 * rows / rows_per_sample values.  fp32 arithmetic, one rounding to the output type.  16-byte accesses where D and the pointers allow
 * (D % 8 == 0 for bf16, D % 4 == 0 for fp32, 16-byte aligned pointers, ldr a multiple of the same), else an element-wise path.
 *
 * ucfvit_drop_path_add: out[r][:] = res[r ldr + :] + s[r / rows_per_sample] * branch[r][:].  branch and out are dense [rows][D]; res has
 *   the row stride ldr >= D (the last Block reads the class rows of the stream in place: ldr = N D, rows_per_sample = 1).  out may be
 *   branch itself.  A sample with s == 0 copies res bit for bit and does not read branch: a non-finite value in a dropped branch does not
 *   reach the stream, where timm's x + 0 * inf gives NaN.
 * ucfvit_drop_path_scale: out[r][:] = s[r / rows_per_sample] * x[r][:] (the gradient of a branch, and the module applied on its own);
 *   a sample with s == 0 writes zeros and does not read x.  out may be x itself.  colsum_partial (may be NULL): fp32 [R][D],
 *   R = ucfvit_drop_path_colsum_rows(rows, rows_per_sample, D) (a host function, no HIP call), receives per row chunk the column sums of
 *   the values written, taken in fp32 before they are rounded, in a fixed order; summed over its R rows (ucfvit_reduce_rows) they are
 *   the bias gradient of the Linear layer that ends the branch.  No atomics: the same bits on every call.
 * Arguments are checked before any HIP call.
 * ------------------------------------------------------------------------------------------------------ */
int64_t ucfvit_drop_path_colsum_rows(int64_t rows, int64_t rows_per_sample, int64_t D);
int ucfvit_drop_path_add(const void* res, int64_t ldr, const void* branch, const float* s, void* out, int64_t rows, int64_t D,
                         int64_t rows_per_sample, int dtype, void* stream);
int ucfvit_drop_path_scale(const void* x, const float* s, void* out, float* colsum_partial, int64_t rows, int64_t D, int64_t rows_per_sample,
                           int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Element-wise dropout (csrc/dropout.hip): nn.Dropout(p) in training on a [rows][D] token matrix, optionally together with the per-sample
 * drop-path scale s of the section above (s == NULL means 1), so that a residual branch with both costs one row pass.
 *
 * The mask is a pure function of (seed, element index) and is never stored; the backward pass and an activation-checkpoint recomputation
 * regenerate it from the same seed.  Definition (all integers unsigned, lo32 / hi32 the halves of a 64-bit value):
 *   - element (r, c) of the logical [rows][D] matrix has the 64-bit index i = (r * row_step) * D + c;
 *   - w = Philox4x32-10(counter = (lo32(i >> 2), hi32(i >> 2), 0, 0), key = (lo32(seed), hi32(seed)))[i & 3]
 *     (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; multipliers D2511F53 / CD9E8D57, key increments
 *     9E3779B9 / BB67AE85, ten rounds, the key bumped before every round but the first: Random123's philox4x32_R(10, ...));
 *   - the element is DROPPED iff w < T, T = min(2^32 - 1, floor(p * 2^32)), computed on the host in double;
 *   - a kept element is multiplied by 1.0f / (1.0f - (float)p), an fp32 division, in fp32: with the row factor
 *     f = s[r / rows_per_sample] * (1.0f / (1.0f - p)) (one fp32 product; without s just the quotient) the value is f * x;
 *     a dropped element contributes exactly 0 whatever x holds (a select, so NaN / Inf under the mask do not pass).
 *   The kernels take 0 < p < 1 (p == 0 and p == 1 need no mask: the caller returns the input / writes zeros).  row_step >= 1 is 1 for a
 *   dense matrix and N for the class-row tail of the last Block, so that row b of the tail draws the mask of dense row b * N;
 *   rows * row_step must stay below 2^32.  The mask depends on the index alone: the 16-byte and the element path (chosen as for drop
 *   path), any grid and any residual stride give the same mask.  Ten rounds were kept after measuring: see profiles/dropout.md.
 *
 * ucfvit_dropout: out[r][c] = f_r * m(r, c) * x[r][c].  out may be x itself.  A row with s == 0 writes zeros and is not read.
 *   colsum_partial (may be NULL): fp32 [R][D] with R = ucfvit_drop_path_colsum_rows(rows, rows_per_sample, D) -- the row-chunk geometry is
 *   that of ucfvit_drop_path_scale, so its host function sizes these partials too -- receives per row chunk the column sums of the values
 *   written, taken in fp32 before they are rounded, in a fixed order; ucfvit_reduce_rows folds the R rows (a bias gradient).
 * ucfvit_dropout_add: out[r][c] = res[r ldr + c] + f_r * m(r, c) * branch[r][c]; res has the row stride ldr >= D, out may be branch
 *   itself.  A row with s == 0 copies res bit for bit and does not read branch.
 * fp32 arithmetic, one rounding to the output type; no atomics, the same bits on every call.  Arguments (null pointers, D, rows,
 * rows % rows_per_sample, ldr < D, p outside (0, 1), row_step < 1, dtype) are checked before any HIP call.
 * ------------------------------------------------------------------------------------------------------ */
int ucfvit_dropout(const void* x, const float* s, void* out, float* colsum_partial, int64_t rows, int64_t D, int64_t rows_per_sample,
                   int64_t row_step, double p, uint64_t seed, int dtype, void* stream);
int ucfvit_dropout_add(const void* res, int64_t ldr, const void* branch, const float* s, void* out, int64_t rows, int64_t D,
                       int64_t rows_per_sample, int64_t row_step, double p, uint64_t seed, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * LayerScale (csrc/layer_scale.hip): timm's LayerScale(dim, init_values), the ls1 / ls2 of the reference's Block: a learned factor
 * gamma[c] per column on a residual branch.  gamma is always fp32 [D] (the master parameter, read directly).  The drop-path scale s (may
 * be NULL) and the dropout mask (p, seed, row_step) of the two sections above ride along, so that a branch with all three costs one row
 * pass per direction.  Here p == 0 is allowed and means "no mask": such a call runs a kernel without any Philox code.  0 < p < 1 uses
 * the mask definition above unchanged (index (r * row_step) * D + c, threshold T, factor 1.0f / (1.0f - (float)p)).  The row factor is
 * f_r = s[r / rows_per_sample] * (1 / keep) in fp32, a missing factor being 1; with neither s nor a mask no product by f_r is made.
 * fp32 arithmetic, one rounding to the output type; 16-byte accesses under the rule of the drop-path section (all of D, ldr and the
 * pointers of the token matrices), else the element path, with the same mask; no atomics, the same bits on every call.
 *
 * ucfvit_layer_scale_add: out[r][c] = res[r ldr + c] + f_r * m(r, c) * (gamma[c] * branch[r][c]), evaluated as u = fl(gamma * b),
 *   t = fl(f_r * u), then the add (which the compiler may contract with the product before it).  res == NULL gives
 *   out = f_r * m * gamma * branch, the LayerScale module applied on its own; ldr is then ignored.  res has the row stride ldr >= D, out
 *   may be branch itself.  A row with f_r == 0 copies res bit for bit (zeros without res) and does not read branch; a masked element is a
 *   select, so NaN / Inf under the mask or in a dropped sample do not pass.  Under a masked element of a kept row the result is
 *   res + (+0): the residual's value, a residual of -0 coming out as +0; only whole rows with f_r == 0 are copied bit for bit.
 * ucfvit_layer_scale_grad: with g = f_r * m(r, c) * dy[r][c] in fp32, dbranch[r][c] = round(gamma[c] * g); dbranch may be dy itself.
 *   colsum_partial (may be NULL) receives per row chunk the column sums of gamma[c] * g before rounding: folded, the bias gradient of the
 *   branch's exit Linear.  gamma_partial (may be NULL) receives per row chunk the column sums of g * branch[r][c]: folded, the gradient of
 *   gamma.  branch (the branch's unscaled output) may be NULL only when gamma_partial is.  Both partials are fp32 [R][D],
 *   R = ucfvit_drop_path_colsum_rows(rows, rows_per_sample, D), in the fixed summation order of ucfvit_drop_path_scale, folded by
 *   ucfvit_reduce_rows.  A row with f_r == 0 writes zeros, reads neither dy nor branch and adds exact zeros to both sums.
 * Arguments (null pointers, null gamma, branch == NULL with gamma_partial, D, rows, rows % rows_per_sample, ldr < D, p outside [0, 1),
 * row_step < 1, dtype, sums of an empty input) are checked before any HIP call.
 * ------------------------------------------------------------------------------------------------------ */
int ucfvit_layer_scale_add(const void* res, int64_t ldr, const void* branch, const float* gamma, const float* s, void* out, int64_t rows,
                           int64_t D, int64_t rows_per_sample, int64_t row_step, double p, uint64_t seed, int dtype, void* stream);
int ucfvit_layer_scale_grad(const void* dy, const void* branch, const float* gamma, const float* s, void* dbranch, float* colsum_partial,
                            float* gamma_partial, int64_t rows, int64_t D, int64_t rows_per_sample, int64_t row_step, double p, uint64_t seed,
                            int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * QK-norm (csrc/qk_norm.hip): the q_norm / k_norm of the reference's Attention, a LayerNorm over the dh elements of every (row, head)
 * segment of Q and of K, applied between the qkv Linear and the attention core.  The layout is the attention contract: qkv is
 * [rows = B N][3][H][dh], what the qkv GEMM writes and ucfvit_attention_fwd / ucfvit_attention_rows_fwd read.  dh is 32, 64 or 128, the
 * dtype fp32 or bf16.  gamma_q, beta_q, gamma_k, beta_k are fp32 [dh], shared by all heads: the master parameters, read directly.  fp32
 * arithmetic (mean, then the biased variance of the centred values, rstd = rsqrt(var + eps)), one rounding to the output type; 16-byte
 * accesses, so qkv / dqkv / saved_qk must be 16-byte aligned; no atomics, a fixed summation order, the same bits on every call.
 *
 * ucfvit_qk_norm_fwd: normalises the Q and K thirds of qkv in place, Q with (gamma_q, beta_q), K with (gamma_k, beta_k); the V third is
 *   neither read nor written.  saved_qk, mean, rstd go together: all three NULL (eval, no_grad) writes nothing but the in-place result;
 *   otherwise saved_qk [rows][2][H][dh] of the dtype receives the un-normalised Q and K bit for bit and mean / rstd fp32 [rows][2][H] the
 *   statistics.  The in-place result is the same bits either way.
 * ucfvit_qk_norm_bwd: rewrites the Q and K thirds of dqkv in place, from the gradient of the normalised values to the gradient of the
 *   Linear's output: dx = rstd * (g - mean_seg(g) - xhat * mean_seg(g * xhat)) with g = dy * gamma and xhat = (saved - mean) * rstd
 *   recomputed in fp32.  The V third is untouched.  param_partial (may be NULL) is fp32 [R][4][dh]: per row chunk the sums over rows and
 *   heads of dy * xhat and of dy for Q, then for K (dgamma_q, dbeta_q, dgamma_k, dbeta_k).  colsum_partial (may be NULL) is fp32
 *   [R][2][H][dh]: per row chunk the column sums of the values written to the Q and K thirds, taken before rounding: folded, the Q and K
 *   thirds of the qkv bias gradient (with a LayerNorm behind the bias the K third is no longer 0 and the Q third no longer the sum of
 *   dQ).  R = ucfvit_qk_norm_partial_rows(rows, H, dh) (0 for what the kernels refuse); ucfvit_reduce_rows folds both.
 * Arguments (null pointers, null parameters, dh outside {32, 64, 128}, H < 1, rows < 0 or >= 2^31 - 4096, eps < 0 or NaN, dtype,
 * alignment, saved_qk without the statistics or the reverse, sums of an empty input) are checked before any HIP call.
 * ------------------------------------------------------------------------------------------------------ */
int64_t ucfvit_qk_norm_partial_rows(int64_t rows, int64_t H, int64_t dh);
int ucfvit_qk_norm_fwd(void* qkv, const float* gamma_q, const float* beta_q, const float* gamma_k, const float* beta_k, void* saved_qk,
                       float* mean, float* rstd, int64_t rows, int64_t H, int64_t dh, float eps, int dtype, void* stream);
int ucfvit_qk_norm_bwd(void* dqkv, const void* saved_qk, const float* gamma_q, const float* gamma_k, const float* mean, const float* rstd,
                       float* param_partial, float* colsum_partial, int64_t rows, int64_t H, int64_t dh, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * DDPM training and sampling around the DiffusionVIT (csrc/diffusion.hip; the token kernels in csrc/elementwise.hip).  Streaming passes:
 * fp32 arithmetic with every product and sum rounded on its own in the order written below (no fma contraction), one rounding to the
 * output type; 16-byte accesses where the sizes and pointers allow, else an element path with the same bits; no atomics, the same bits on
 * every call.  Arguments are checked on the host before any HIP call.
 *
 * ucfvit_ddpm_q_sample: the forward noising out[b][i] = fl(fl(sqrt_ab[t[b]] * x0[b][i]) + fl(sqrt_1mab[t[b]] * eps[b][i])) of B samples of
 *   n_per_sample fp32 elements each (an NCHW(D) image flattened per sample).  t is int64 [B] ON THE DEVICE, the tables fp32 [T] on the
 *   device.  The host cannot see t, so the kernel clamps every t[b] into [0, T - 1]: an out-of-range step reads the first / last table
 *   entry and never outside the tables.  out may be x0 (or eps).  The 16-byte path needs n_per_sample % 4 == 0 and 16-byte aligned x0, eps,
 *   out.  Checked: null pointers, B < 0, n_per_sample < 1, B n_per_sample >= 2^40, T < 1, pointers not aligned to their element.
 *
 * ucfvit_time_tokens_fwd / _bwd: ucfvit_tokens_fwd / _bwd with one more operand, the time row temb [B][D] of the dtype, one per sample:
 *   out[b][0] = (cls + pos[0]) + temb[b] if has_cls, out[b][j + pre] = (patches[b][j] + pos[j + pre]) + temb[b]; the parentheses are the
 *   order of the fp32 adds; pos may be NULL (then one add).  With temb == 0 the result is ucfvit_tokens_fwd's bit for bit.
 *   bwd: dpatches = dout[:, pre:] (may be NULL), dpos / dcls (may be NULL) exactly as ucfvit_tokens_bwd writes them, `accumulate` included
 *   (it does not apply to dtemb), and dtemb fp32 [B][D] = sum_n dout[b][n][:] over all L + pre rows: the 8 rows of a chunk are added by a
 *   fixed butterfly (rows r and r ^ 1, then ^ 2, then ^ 4), the chunk sums go to `workspace` (ucfvit_time_tokens_bwd_workspace bytes, fp32 [chunks][B][D]) and ucfvit_reduce_rows folds
 *   them in chunk order.  dout is read once for all four results.  Same shape rules as the token kernels (D a multiple of 4 (fp32) / 8
 *   (bf16), 16-byte aligned token pointers), B D < 2^31.  The workspace query returns 0 for sizes the kernel refuses.
 *
 * ucfvit_relu_dropout / _bwd: the hidden layer of the time MLP on [rows][D]: y = f * m(r, c) * relu(x), dx = f * m(r, c) * [x > 0] * dy,
 *   with EXACTLY the mask m and the factor f = 1.0f / (1.0f - (float)p) of the dropout section above at row_step = 1 and without a
 *   drop-path scale (index r D + c, Philox4x32-10, dropped iff w < T).  p must be inside [0, 1); p == 0 is plain ReLU (eval): no mask is
 *   generated and no product by f is made.  relu(x) is x where x > 0 and +0 elsewhere, so x = NaN gives 0 in both directions; a dropped or
 *   inactive element is a select: NaN / Inf under it do not pass.  out may be x, dx may be dy.  The backward pass reads the pre-activation x
 *   and recomputes the mask from the seed.  Checked: null pointers, D, rows (rows < 2^30), p, dtype.
 *
 * ucfvit_ddpm_step: one reverse (ancestral) step on the image without materialising unpatchify(pred):
 *   out = fl(fl(c1 * fl(x - fl(c2 * e))) + fl(sigma * z)), e[b][c][pixel] read from pred [B][L][p^nd C] (`dtype`) in the patch order that
 *   ucfvit_patch_mse documents, (ph, pw[, pd], c): the reference's unpatchify.  x, z, out are fp32 NCHW(D); dims = {H, W[, Dz]}, nd = 2 | 3.
 *   z may be NULL (step 0; sigma must then be 0, and out = fl(c1 * fl(x - fl(c2 * e)))).  out may be x.  Checked: null pointers, nd, dtype,
 *   sizes (every dim a multiple of p, C pixels < 2^31 per sample), sigma != 0 without z, pointers not aligned to their element.
 *
 * ucfvit_ddim_step: one generalised reverse step (DDIM; eta = 1 on every step is the ancestral sampler in its x0 form), with the geometry,
 *   checks and aliasing rule (out may be x) of ucfvit_ddpm_step.  Per element, every product and sum rounded on its own, in this order:
 *     e  = (float)pred[i]
 *     x0 = (x - s_1mab * e) * r_ab
 *     if clip > 0:  x0 = x0 < -clip ? -clip : (x0 > clip ? clip : x0)      (two selects: a NaN stays a NaN)
 *                   e  = (x - s_ab * x0) * r_1mab
 *     o  = c_x0 * x0 + c_eps * e
 *     out = z ? o + sigma * z : o
 *   s_ab = sqrt(abar_i), s_1mab = sqrt(1 - abar_i), r_ab and r_1mab their reciprocals, c_x0 = sqrt(abar_prev), c_eps =
 *   sqrt(1 - abar_prev - sigma^2): DDPM_Scheduler.ddim_coefficients.  clip == 0: no clamp; a negative or NaN clip is refused.  z == NULL
 *   needs sigma == 0.
 * ------------------------------------------------------------------------------------------------------ */
int ucfvit_ddpm_q_sample(const float* x0, const float* eps, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab, float* out,
                         int64_t B, int64_t n_per_sample, int64_t T, void* stream);
int ucfvit_time_tokens_fwd(const void* patches, const void* cls, const void* pos, const void* temb, void* out, int64_t B, int64_t L, int64_t D,
                           int has_cls, int dtype, void* stream);
int64_t ucfvit_time_tokens_bwd_workspace(int64_t B, int64_t L, int64_t D, int has_cls);
int ucfvit_time_tokens_bwd(const void* dout, void* dpatches, float* dpos, float* dcls, float* dtemb, int64_t B, int64_t L, int64_t D,
                           int has_cls, int accumulate, float* workspace, int dtype, void* stream);
int ucfvit_relu_dropout(const void* x, void* out, int64_t rows, int64_t D, double p, uint64_t seed, int dtype, void* stream);
int ucfvit_relu_dropout_bwd(const void* x, const void* dy, void* dx, int64_t rows, int64_t D, double p, uint64_t seed, int dtype, void* stream);
int ucfvit_ddpm_step(const float* x, const void* pred, const float* z, float* out, int64_t B, int64_t C, const int64_t* dims, int nd, int64_t p,
                     float c1, float c2, float sigma, int dtype, void* stream);
int ucfvit_ddim_step(const float* x, const void* pred, const float* z, float* out, int64_t B, int64_t C, const int64_t* dims, int nd, int64_t p,
                     float s_ab, float s_1mab, float r_ab, float r_1mab, float c_x0, float c_eps, float sigma, float clip, int dtype,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UCFVIT_HIP_H */
