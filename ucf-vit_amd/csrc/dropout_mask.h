// The dropout mask of include/ucfvit_hip.h, shared by the row passes that apply it (csrc/dropout.hip, csrc/layer_scale.hip): the mask
// parameters of one call, one Philox4x32-10 block, the keep bits of a lane's pack, and the host-side check of (p, row_step, seed).
// With the 64-bit index i = (r * row_step) * D + c of element (r, c):
//   w = Philox4x32-10(counter = (lo32(i >> 2), hi32(i >> 2), 0, 0), key = (lo32(seed), hi32(seed)))[i & 3],   dropped iff w < T
#pragma once
#include "common.h"

struct DoParams {
    uint32_t k0, k1;      // lo32(seed), hi32(seed)
    uint32_t thr;         // T = min(2^32 - 1, floor(p 2^32))
    float inv_keep;       // 1.0f / (1.0f - p)
    int64_t row_step;
};

// one Philox4x32-10 block (Salmon et al., SC'11; the Random123 constants) of the counter (c0, c1, 0, 0)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t (&w)[4]) {
    uint32_t c2 = 0u, c3 = 0u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// bit e set: element e of the W elements from index i0 on is KEPT.  W = 4 | 8: i0 is a multiple of 4 (D % W == 0, col % W == 0)
template <int W> __device__ __forceinline__ uint32_t keep_bits(int64_t i0, const DoParams& P) {
    uint32_t bits = 0u;
    if (W == 1) {
        uint32_t w[4];
        const uint64_t q = (uint64_t)i0 >> 2;
        philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), P.k0, P.k1, w);
        const int j = (int)(i0 & 3);
        const uint32_t v = j == 0 ? w[0] : j == 1 ? w[1] : j == 2 ? w[2] : w[3];
        bits = v >= P.thr ? 1u : 0u;
    } else {
#pragma unroll
        for (int b = 0; b < W / 4; ++b) {
            uint32_t w[4];
            const uint64_t q = ((uint64_t)i0 >> 2) + b;
            philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), P.k0, P.k1, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) bits |= (w[j] >= P.thr ? 1u : 0u) << (4 * b + j);
        }
    }
    return bits;
}

// the mask half of the argument checks, and the mask parameters; before any HIP call.  p_zero_ok: the caller takes p == 0 as "no mask"
// (then T = 0 and the factor is 1: nothing is dropped, and the caller launches a kernel without Philox)
inline int do_mask_check(const char* name, int64_t rows, int64_t row_step, double p, uint64_t seed, bool p_zero_ok, DoParams* P) {
    if (p_zero_ok) {
        UCF_CHECK_ARG(p >= 0.0 && p < 1.0, "%s: drop probability p=%g is not inside [0, 1)", name, p);   // false for NaN too
    } else {
        UCF_CHECK_ARG(p > 0.0 && p < 1.0, "%s: drop probability p=%g is not inside (0, 1)", name, p);    // false for NaN too
    }
    UCF_CHECK_ARG(row_step >= 1 && row_step < (1ll << 30) && rows * row_step < (1ll << 32), "%s: bad row_step=%lld for %lld rows", name,
                  (long long)row_step, (long long)rows);                  // so that (r row_step) D + c stays below 2^62
    const double t = p * 4294967296.0;                                     // exact: a scaling by 2^32
    P->thr = t >= 4294967295.0 ? 4294967295u : (uint32_t)t;               // floor, capped
    P->k0 = (uint32_t)seed, P->k1 = (uint32_t)(seed >> 32);
    const float pf = (float)p;
    P->inv_keep = 1.0f / (1.0f - pf);
    P->row_step = row_step;
    return UCFVIT_OK;
}
