// Device helpers shared by the GEMM translation units (gemm.hip, gemm2.hip, gemm_stagger.hip): the LDS image of an operand K-tile, the
// order in which a launch walks its output tiles, and the DMA issue of half a 256-row K-tile.  gemm3_kernel and gemm5_kernel read the
// same LDS images in the same tile order: one definition each, so a change cannot reach one kernel and miss the other.
#pragma once
#include "common.h"

typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// ---- LDS image addressing -------------------------------------------------------------------------
// KC image [rows][128 B]: byte offset of 16-B slot `slot` (0..7) of row `row`, slots XOR-swizzled by (row & 7)
__device__ __forceinline__ int kc_off(int row, int slot) { return row * 128 + ((slot ^ (row & 7)) << 4); }

// KS image [k][rows], bf16: 32-B groups swizzled so the 8 k-rows a half-wave's transposed read touches land on 8 distinct 32-B
// bank groups
__device__ __forceinline__ int ks_swz(int krow) { return ((krow & 3) | (((krow >> 3) & 1) << 2)) << 5; }

// KC fragment of the 16 rows [rbase, rbase + 16) for k-chunk `c` of the K-tile: lane holds the 16 B of slot 4 c + (lane >> 4) of row
// rbase + (lane & 15) (both dtypes: chunk = 64 B = 4 slots)
template <typename F> __device__ __forceinline__ F kc_frag(const char* lds, int rbase, int c, int lane) {
    const int g = lane >> 4, i = lane & 15;
    return *reinterpret_cast<const F*>(lds + kc_off(rbase + i, 4 * c + g));
}

// logical tile index -> (m0, n0): bands of 8 N-tiles, walking down M inside a band (neighbouring tiles share operand panels)
__device__ __forceinline__ void tile_origin(int t, int tiles_m, int tiles_n, int BM, int BN, int& m0, int& n0) {
    // 12 N-tiles (the qkv projection: N = 3072) as three bands of 4 rather than 8 + 4: every XCD block is 8 x 4 tiles
    const int BAND = (tiles_n > 8 && tiles_n % 8 != 0 && tiles_n % 4 == 0) ? 4 : 8;
    const int band_tiles = BAND * tiles_m;
    const int band = t / band_tiles;
    const int band_w = min(BAND, tiles_n - band * BAND);
    const int in_band = t - band * band_tiles;
    m0 = (in_band / band_w) * BM;
    n0 = (band * BAND + in_band % band_w) * BN;
}

// ---- DMA of half a 256-row operand K-tile (the 8-wave kernels: wave group `grp`, wave `w4` of the group) --------------------------
// Per-lane 32-bit byte offsets (row clamp + source-side swizzle folded in) of this wave's 4 DMA pieces (1 KiB each) of an operand
// K-tile; the K position is a wave-uniform byte offset added to the (SGPR) base pointer at issue time.
template <int LAYOUT, int BR>
__device__ __forceinline__ void half_offsets(unsigned (&off)[4], int64_t ld, int r0, int R, int grp, int w4, int lane) {
    constexpr int NP = BR / 8, PER = NP / 8;
    static_assert(PER == 4, "256-wide operand tiles only");
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int idx = grp * (NP / 2) + w4 * PER + i;
        if (LAYOUT == UCFVIT_LAYOUT_KC) {
            const int row = idx * 8 + (lane >> 3);
            const int gslot = (lane & 7) ^ (row & 7);
            int gr = r0 + row;
            gr = gr < R ? gr : R - 1;
            off[i] = (unsigned)(((int64_t)gr * ld + gslot * 8) * 2);
        } else {
            constexpr int RB = BR * 2, KPP = 1024 / RB;
            const int krow = idx * KPP + (lane * 16) / RB;
            const int pbyte = (lane * 16) % RB;
            const int col = (pbyte ^ ks_swz(krow)) >> 1;
            int gc = r0 + col;
            gc = gc <= R - 8 ? gc : R - 8;
            off[i] = (unsigned)(((int64_t)krow * ld + gc) * 2);
        }
    }
}
template <int BR>
__device__ __forceinline__ void issue_half(const char* __restrict__ base_k, const unsigned (&off)[4], char* lds, int grp, int w4) {
    constexpr int NP = BR / 8, PER = NP / 8;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int idx = grp * (NP / 2) + w4 * PER + i;
        __builtin_amdgcn_global_load_lds((gptr_t)(base_k + off[i]), (lptr_t)(lds + idx * 1024), 16, 0, 0);
    }
}

// Workgroup barrier the compiler moves nothing across; `hook_` runs right behind it (a diagnostic time stamp, or nothing)
#define TILE_BARRIER(hook_)                   \
    do {                                      \
        __builtin_amdgcn_sched_barrier(0);    \
        asm volatile("" ::: "memory");        \
        __builtin_amdgcn_s_barrier();         \
        asm volatile("" ::: "memory");        \
        hook_;                                \
        __builtin_amdgcn_sched_barrier(0);    \
    } while (0)
