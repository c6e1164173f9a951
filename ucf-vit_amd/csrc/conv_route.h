// Which kernel runs a convolution launch, and with what geometry: decided once, on the host, in plain C++ (no HIP).  ucfvit_conv3d_fwd and
// ucfvit_conv3d_wgrad switch on the result; ucfvit_conv3d_fwd_stats_rows, ucfvit_conv3d_wgrad_size, ucfvit_conv3d_wgrad_workspace and
// ucfvit_conv3d_route return fields of it.  Every rule of the dispatch is written here once.
#pragma once
#include <stdint.h>

#include "../../include/ucfvit_hip.h"

// ---- the shapes the kernels are instantiated for --------------------------------------------------------------------------------------
static inline bool conv_ksize_ok(int ksize) { return ksize == 1 || ksize == 3; }
static inline bool conv_cin_ok(int64_t Cin) { return Cin == 8 || Cin == 16 || (Cin > 0 && Cin % 32 == 0); }
static inline bool conv_cout_ok(int64_t Cout) { return Cout > 0 && Cout % 16 == 0; }
static inline bool conv_shape_ok(int64_t Cin, int64_t Cout, int ksize) { return conv_ksize_ok(ksize) && conv_cin_ok(Cin) && conv_cout_ok(Cout); }

constexpr int conv_cpc(int64_t Cin) { return Cin < 32 ? (int)Cin : 32; }               // channels per contraction chunk: 8, 16 or 32
constexpr int conv_taps(int ks) { return ks * ks * ks; }
constexpr int conv_steps(int cpc, int ks) { return (conv_taps(ks) + 32 / cpc - 1) / (32 / cpc); }   // 32-wide MFMA steps per chunk: 27, 14, 7; KS 1: 1
constexpr int conv_halo_bytes(int cpc, int ks, int tx, int ty, int tz) { return (tx + 2 * (ks / 2)) * (ty + 2 * (ks / 2)) * (tz + 2 * (ks / 2)) * cpc * 2; }

// ---- forward / data gradient ----------------------------------------------------------------------------------------------------------
enum ConvKind {
    CK_TILE = 0,   // conv_fwd_kernel: one TX x TY x 16 tile per workgroup, any Cin; no statistics epilogue
    CK_STRIP = 1,  // conv_fwd_strip_kernel: a workgroup walks the z extent of its (x, y) column; single-chunk inputs (Cin <= 32)
    CK_MC = 2      // conv3_fwd_mc_kernel: the column walk for Cin = 64, 128, ..., 3x3x3, dense bf16, Z = 16 / 32 / 64
};

// UCFVIT_CONV_STRIP, the `mode` of conv_fwd_route: 0 never a column kernel, 1 (default) when the columns fill the chip, 2 whenever one
// applies, 3 as 2 with the branching (non-FAST) memory operations
constexpr int64_t CONV_FILL_WGS = 512;                  // mode 1: workgroups from which a column kernel is chosen
constexpr int64_t CONV_FAST_LIMIT = (1ll << 32) - 64;   // FAST: bytes of a batch element's input and of its output stay below this

struct ConvFwdRoute {
    ConvKind kind;
    int cpc, ks, nb, TX, TY;  // the instantiation: channels per chunk, kernel size, 16-channel output blocks per workgroup, tile
    bool fast, share;         // CK_STRIP: the branch-free raw-buffer memory operations; one B fragment feeds the three dy taps (3x3x3, CPC 16)
    int depth;                // CK_STRIP: halo tiles in flight (2 needs fast and CPC <= 16)
    int tzt;                  // CK_MC: z tiles of a column, all kept in registers
    int tx, ty, tz;           // tile counts
    int64_t gx, gy;           // grid: tiles (CK_TILE) or (x, y) columns, by Cout / (16 nb)
    bool grid_too_large;
    int smem;                 // dynamic LDS bytes: halo + weight slab
    int64_t stats_rows;       // rows per batch element of the statistics partials [B][rows][3][Cout] the kernel can write; 0: no such epilogue
};
constexpr int conv_fwd_smem(int cpc, int ks, int nb, int TX, int TY, bool share) {
    return conv_halo_bytes(cpc, ks, TX, TY, 16) + (share ? 15 : conv_steps(cpc, ks)) * 16 * nb * 64;
}
static inline ConvFwdRoute conv_fwd_route(int64_t B, int64_t X, int64_t Y, int64_t Z, int64_t Cin, int64_t Cout, int ksize, bool has_bias,
                                          int out_dtype, int64_t ldy, int64_t cout_store, int mode) {
    ConvFwdRoute r = {};
    const int64_t nb16 = Cout / 16, osize = out_dtype == UCFVIT_BF16 ? 2 : 4;
    r.cpc = conv_cpc(Cin);
    r.ks = ksize;
    r.nb = nb16 % 4 == 0 ? 4 : (nb16 % 2 == 0 ? 2 : 1);
    r.kind = CK_TILE;
    r.depth = 1;
    const int64_t cols28 = B * ((X + 1) / 2) * ((Y + 7) / 8);      // columns of the (2, 8) tile, the measure of both size thresholds
    if (Cin > 32 && ksize == 3 && out_dtype == UCFVIT_BF16 && !has_bias && Cout % 32 == 0 && cout_store == Cout && ldy == Cout && mode &&
        (Z == 16 || Z == 32 || Z == 64) && (mode >= 2 || cols28 * (Cout / 32) >= CONV_FILL_WGS)) {
        r.kind = CK_MC;
        r.nb = 2;
        r.tzt = (int)(Z / 16);
    } else if (Cin <= 32 && Z > 16 && mode && (mode >= 2 || cols28 * (nb16 / r.nb) >= CONV_FILL_WGS)) {
        r.kind = CK_STRIP;
        r.fast = ldy % 4 == 0 && cout_store % 4 == 0 && X * Y * Z * Cin * 2 < CONV_FAST_LIMIT && X * Y * Z * ldy * osize < CONV_FAST_LIMIT && mode != 3;
        r.depth = r.fast && r.cpc <= 16 ? 2 : 1;
        r.share = ksize == 3 && r.cpc == 16;
    }
    // the tile: (2, 4) for 64 output channels per workgroup, else (2, 8); the column kernel with 16 takes (4, 8) — except at CPC 32, where
    // that tile's prefetch would not fit in registers
    r.TX = r.kind == CK_STRIP && r.nb == 1 && r.cpc < 32 ? 4 : 2;
    r.TY = r.nb == 4 ? 4 : 8;
    r.tx = (int)((X + r.TX - 1) / r.TX);
    r.ty = (int)((Y + r.TY - 1) / r.TY);
    r.tz = (int)((Z + 15) / 16);
    r.gx = B * r.tx * r.ty * (r.kind == CK_TILE ? r.tz : 1);
    r.gy = nb16 / r.nb;
    r.grid_too_large = r.gx >= (1ll << 31) || r.gy >= 65536;
    r.smem = conv_fwd_smem(r.cpc, r.ks, r.nb, r.TX, r.TY, r.share);
    r.stats_rows = r.kind == CK_TILE ? 0 : (int64_t)r.tx * r.ty * 4;
    return r;
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------------------
constexpr int CONV_WGRAD_TX = 2, CONV_WGRAD_TY = 4, CONV_WGRAD_TZ = 32;   // the tile: one 32-deep contraction step per (x, y) row
constexpr int64_t CONV_WGRAD_PART_FLOATS = 32ll << 20;                   // cap of the partial-sum scratch (128 MiB)
constexpr int CONV_WGRAD_MAX_WGS = 1024;

struct ConvWgradRoute {
    int cpc, ks, mb, nbk;      // the instantiation; mb, nbk: 16-channel blocks of Cout and of the Cin chunk per workgroup
    int tx, ty, tz, tiles;     // tile counts, tiles = B tx ty tz
    int n_wg, tiles_per_wg;    // grid x and the tiles each workgroup walks
    int gy;                    // grid y: (Cin chunk, Cout block) pairs
    int64_t n_out;             // floats of the packed weight gradient = of one partial
    int slots;                 // partials per workgroup: 1, KS 1: 4 (one per wave)
    int smem;                  // dynamic LDS bytes: dy image + x halo
    int64_t workspace_bytes;
};
constexpr int conv_wgrad_smem(int cpc, int ks, int mb) {
    return CONV_WGRAD_TX * CONV_WGRAD_TY * CONV_WGRAD_TZ * 32 * mb + conv_halo_bytes(cpc, ks, CONV_WGRAD_TX, CONV_WGRAD_TY, CONV_WGRAD_TZ) + 64;
}
static inline ConvWgradRoute conv_wgrad_route(int64_t B, int64_t X, int64_t Y, int64_t Z, int64_t Cin, int64_t Cout, int ksize) {
    ConvWgradRoute r = {};
    r.cpc = conv_cpc(Cin);
    r.ks = ksize;
    r.mb = Cout % 32 == 0 ? 2 : 1;
    r.nbk = r.cpc >= 16 ? r.cpc / 16 : 1;
    r.tx = (int)((X + CONV_WGRAD_TX - 1) / CONV_WGRAD_TX);
    r.ty = (int)((Y + CONV_WGRAD_TY - 1) / CONV_WGRAD_TY);
    r.tz = (int)((Z + CONV_WGRAD_TZ - 1) / CONV_WGRAD_TZ);
    r.tiles = (int)(B * r.tx * r.ty * r.tz);
    r.gy = (int)((Cin / r.cpc) * (Cout / (16 * r.mb)));
    r.n_out = (int64_t)r.gy * conv_taps(ksize) * (16 * r.mb * 16 * r.nbk);
    r.slots = ksize == 3 ? 1 : 4;
    int64_t cap = CONV_WGRAD_PART_FLOATS / (r.n_out * r.slots);
    cap = cap < 1 ? 1 : (cap > CONV_WGRAD_MAX_WGS ? CONV_WGRAD_MAX_WGS : cap);
    r.n_wg = (int)(r.tiles < cap ? r.tiles : cap);
    r.tiles_per_wg = (r.tiles + r.n_wg - 1) / r.n_wg;
    r.n_wg = (r.tiles + r.tiles_per_wg - 1) / r.tiles_per_wg;
    r.smem = conv_wgrad_smem(r.cpc, r.ks, r.mb);
    r.workspace_bytes = (int64_t)r.n_wg * r.slots * r.n_out * (int64_t)sizeof(float);
    return r;
}
