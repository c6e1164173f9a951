// Device helpers shared by the attention translation units (attention.hip, attention_short.hip; attention_rows.hip takes the buffer
// descriptor and the constant): the MFMA trait, the swizzled LDS image of a [rows][DH] operand and the four ways a wave takes an MFMA
// operand fragment (a row of the image, the image transposed, an accumulator, a global row).  The streaming and the resident kernels
// read the same images with the same fragments: one definition each, so a change cannot reach one family and miss the other.
#pragma once
#include "common.h"

constexpr float LOG2E_F = 1.44269504088896340736f;   // the kernels work in log2 units: scale_log2e = scale * LOG2E_F

template <typename T> struct Mma16;
template <> struct Mma16<bf16> {
    typedef bf16x8 frag_t;
    static __device__ __forceinline__ void mma(f32x4& acc, const frag_t& a, const frag_t& b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    }
    static __device__ __forceinline__ frag_t ones() {
        frag_t r;
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = (bf16)1.0f;
        return r;
    }
};
template <> struct Mma16<float> {
    typedef f32x4 frag_t;
    static __device__ __forceinline__ void mma(f32x4& acc, const frag_t& a, const frag_t& b) {
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
    }
    static __device__ __forceinline__ frag_t ones() { return f32x4{1.f, 1.f, 1.f, 1.f}; }
};

// ---- LDS image of a [rows][DH] operand: rows of RB = DH * sizeof(T) bytes, their SPR = RB / 16 slots XOR-swizzled by the row ---------
template <int SPR> __device__ __forceinline__ int slot_swz(int row) {
    if (SPR == 4) return (0x1230 >> (((row >> 2) & 3) * 4)) & 3;  // {0,3,2,1}[(row>>2)&3]
    if (SPR == 8) return row & 7;
    return row & 15;
}
template <typename T, int DH> __device__ __forceinline__ int tile_off(int row, int slot) {
    constexpr int RB = DH * sizeof(T), SPR = RB / 16;
    return row * RB + ((slot ^ slot_swz<SPR>(row)) << 4);
}

// ---- operand fragments ----------------------------------------------------------------------------------------------------------
// "row" fragment: 16 B of row (rb*16 + lane&15) at head-dim chunk c: elements d = (4c + g)*EPV .. +EPV
template <typename T, int DH>
__device__ __forceinline__ typename Mma16<T>::frag_t frag_row(const char* lds, int rb, int c, int lane) {
    const int row = rb * 16 + (lane & 15), g = lane >> 4;
    return *reinterpret_cast<const typename Mma16<T>::frag_t*>(lds + tile_off<T, DH>(row, 4 * c + g));
}
// "transposed" fragment for a contraction over image rows: lane (lane&15 = i) gets column d = db*16 + i of the rows
// of row-chunk rc in ACCUMULATOR order: bf16: rows 32rc + 16*(j>>2) + 4g + (j&3), j=0..7 ; fp32: rows 16rc + 4g + s.
template <typename T, int DH>
__device__ __forceinline__ typename Mma16<T>::frag_t frag_tr(const char* lds, int rc, int db, int lane) {
    typedef typename Mma16<T>::frag_t frag_t;
    const int g = lane >> 4, i = lane & 15;
    if constexpr (sizeof(T) == 2) {
        const int q = i >> 2, p = i & 3;
        const int slot = 2 * db + (p >> 1), sub = (p & 1) * 8;
        const int r_lo = 32 * rc + 4 * g + q, r_hi = r_lo + 16;
        const char* a_lo = lds + tile_off<T, DH>(r_lo, slot) + sub;
        const char* a_hi = lds + tile_off<T, DH>(r_hi, slot) + sub;
        short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(short4v, a_lo));
        short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(short4v, a_hi));
        short8v r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(frag_t, r);
    } else {
        const int slot = 4 * db + (i >> 2), sub = (i & 3) * 4;
        f32x4 r;
#pragma unroll
        for (int s = 0; s < 4; ++s) r[s] = *reinterpret_cast<const float*>(lds + tile_off<T, DH>(16 * rc + 4 * g + s, slot) + sub);
        return __builtin_bit_cast(frag_t, r);
    }
}
// accumulator blocks -> operand fragment for row-chunk rc (bf16: two 16-row blocks packed; fp32: one block as is).  NBLK: the blocks
// `acc` holds where that number may be odd (the second block of the last chunk then contributes zeros); 0: every chunk is whole
template <typename T, int NBLK = 0> __device__ __forceinline__ typename Mma16<T>::frag_t frag_from_acc(const f32x4* acc, int rc) {
    typedef typename Mma16<T>::frag_t frag_t;
    if constexpr (sizeof(T) == 2) {
        bf16x8 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[j] = (bf16)acc[2 * rc][j];
            r[4 + j] = (NBLK == 0 || 2 * rc + 1 < NBLK) ? (bf16)acc[2 * rc + 1][j] : (bf16)0.f;
        }
        return __builtin_bit_cast(frag_t, r);
    } else {
        return __builtin_bit_cast(frag_t, acc[rc]);
    }
}
// 16 B of a global row as an operand fragment (zero beyond R)
template <typename T, int DH>
__device__ __forceinline__ typename Mma16<T>::frag_t frag_global(const T* __restrict__ base, int64_t row_stride, int row, int R, int c, int lane) {
    typedef typename Mma16<T>::frag_t frag_t;
    const int g = lane >> 4;
    u32x4 z = {0u, 0u, 0u, 0u};
    u32x4 v = (row < R) ? *reinterpret_cast<const u32x4*>(base + (int64_t)row * row_stride + (4 * c + g) * (16 / (int)sizeof(T))) : z;
    return __builtin_bit_cast(frag_t, v);
}

// ---- reductions over the 4 lane groups that share lane & 15 ------------------------------------------------------------------------
__device__ __forceinline__ float group_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// Raw-buffer descriptor over `bytes` bytes from `base`: an access past the end is out of range for the hardware (loads return 0, stores
// are dropped), so the kernels that use it need no branch around a row >= N
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

// ---- host: a kernel that wants more than 64 KiB of dynamic LDS has to say so once; `who` names the caller in the error text ----------
template <typename K> int raise_lds_limit(K kernel, size_t bytes, const char* who) {
    if (bytes <= 64 * 1024) return UCFVIT_OK;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        ucfvit_set_error("%s: cannot raise dynamic LDS to %zu bytes: %s", who, bytes, hipGetErrorString(e));
        return UCFVIT_ERR_HIP;
    }
    return UCFVIT_OK;
}
