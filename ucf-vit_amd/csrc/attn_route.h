// Which kernels run a self-attention pass over the packed qkv matrix: decided once, on the host, in plain C++ (no HIP).
// ucfvit_attention_fwd, ucfvit_attention_bwd and ucfvit_attention_bwd_colsum switch on the result; ucfvit_attention_bwd_colsum_supported
// and ucfvit_attention_route return fields of it.  Every rule of the dispatch is written here once.
#pragma once
#include <stdint.h>

#include "../../include/ucfvit_hip.h"

enum AttnPass { ATTN_FWD = 0, ATTN_BWD = 1 };

enum AttnFamily {
    AK_STREAM,     // attention.hip: attn_fwd_kernel / attn_delta_kernel + attn_bwd_dq_kernel + attn_bwd_dkv_kernel, any N, bf16 and fp32
    AK_SHORT_FWD,  // attn_s_fwd_kernel: K and V of a head resident in LDS
    AK_S3_FWD,     // attn_s3_fwd_kernel: the same with three workgroups per CU (129 .. 208 tokens: N = 197)
    AK_FUSED_BWD   // attn_g_bwd_kernel: dQ, dK, dV and delta in one launch
};

struct AttnRoute {
    AttnFamily family;
    int dtype;    // UCFVIT_BF16 / UCFVIT_F32
    int nb;       // 16-row blocks the kernel is instantiated for: 4, 8, 13 or 16 (the resident families; 0: streaming)
    bool exact;   // the sequence fills all nb blocks: the instantiation that masks only the last key block
    bool colsum;  // the pass can hand out the column sums of dQ (ucfvit_attention_bwd_colsum)
};

static inline AttnRoute attn_route(AttnPass pass, int64_t B, int64_t N, int64_t H, int64_t dh, int dtype) {
    AttnRoute r = {AK_STREAM, dtype, 0, false, false};
    // The resident kernels: bf16 only (fp32 instantiations exceed the register file; the exact-fp32 parity mode streams), the whole
    // sequence in 16 blocks of LDS, one workgroup per (batch, head) in grid.x
    if (dtype != UCFVIT_BF16 || N > 256 || (dh != 32 && dh != 64) || B * H >= (1ll << 31)) return r;
    const int blocks = (int)((N + 15) / 16);
    r.nb = blocks <= 4 ? 4 : (blocks <= 8 ? 8 : (blocks <= 13 ? 13 : 16));
    r.exact = blocks == r.nb;
    r.family = pass == ATTN_BWD ? AK_FUSED_BWD : (r.nb == 13 ? AK_S3_FWD : AK_SHORT_FWD);
    r.colsum = pass == ATTN_BWD;
    return r;
}

// the route as text, in the vocabulary of tests/test_attention_ops.py; returns the length (the text is cut to cap - 1 characters)
static inline int attn_route_name(const AttnRoute& r, char* out, int64_t cap) {
    const char* head = "";
    switch (r.family) {
        case AK_STREAM: head = r.dtype == UCFVIT_BF16 ? "stream-bf16" : "stream-fp32"; break;
        case AK_SHORT_FWD: head = "short-nb"; break;
        case AK_S3_FWD: head = "s3-nb"; break;
        case AK_FUSED_BWD: head = "fused-nb"; break;
    }
    const char* const nb = r.nb == 4 ? "4" : (r.nb == 8 ? "8" : (r.nb == 13 ? "13" : (r.nb == 16 ? "16" : "")));
    const char* parts[3] = {head, nb, r.nb == 0 ? "" : (r.exact ? "-exact" : "-masked")};
    int n = 0;
    for (const char* s : parts)
        for (; *s; ++s, ++n)
            if (n < cap - 1) out[n] = *s;
    if (cap > 0) out[n < cap - 1 ? n : cap - 1] = 0;
    return n;
}

// ---- launchers of attention_short.hip: they launch what the route names and do not decline ------------------------------------------
int ucfvit_attn_launch_short_fwd(const AttnRoute& r, const void* qkv, void* out, float* lse, int64_t B, int64_t N, int64_t H, int64_t dh,
                                 float scale, void* stream);                                            // AK_SHORT_FWD, AK_S3_FWD
// cs_partial (may be null): fp32 [B][2][H][dh], row b = the column sums of dQ over batch element b's tokens, then zeros for dK (see
// ucfvit_attention_bwd_colsum); needs no delta workspace
int ucfvit_attn_launch_fused_bwd(const AttnRoute& r, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                                 float* cs_partial, int64_t B, int64_t N, int64_t H, int64_t dh, float scale, void* stream);   // AK_FUSED_BWD
