// Which kernel runs a 2-D convolution launch (csrc/conv2d.hip), and with what geometry: decided once, on the host, in plain C++ (no HIP), as
// conv_route.h does for the volumes.  ucfvit_conv2d_fwd and ucfvit_conv2d_wgrad switch on the result; ucfvit_conv2d_wgrad_size,
// ucfvit_conv2d_wgrad_workspace and ucfvit_conv2d_route return fields of it.  The channel rules are those of the 3-D kernels (conv_cin_ok,
// conv_cout_ok, conv_cpc): the two decoders accept the same models.
#pragma once
#include <stdint.h>

#include "conv_route.h"

constexpr int CONV2D_TAPS = 9;                                                        // 3 x 3, tap = dx 3 + dy
constexpr int conv2d_steps(int cpc) { return (CONV2D_TAPS + 32 / cpc - 1) / (32 / cpc); }   // 32-wide MFMA steps per chunk: 9, 5, 3
constexpr int conv2d_halo_bytes(int cpc, int tx, int ty) { return (tx + 2) * (ty + 2) * cpc * 2; }
static inline bool conv2d_shape_ok(int64_t Cin, int64_t Cout) { return conv_cin_ok(Cin) && conv_cout_ok(Cout); }

// ---- forward / data gradient ----------------------------------------------------------------------------------------------------------
// One workgroup = TX rows x 16 pixels along y x 16 nb output channels; its 4 waves take TX / 4 rows each.
constexpr int CONV2D_TY = 16;

struct Conv2dFwdRoute {
    int cpc, nb, TX;          // the instantiation: channels per chunk, 16-channel output blocks per workgroup, rows of a tile
    int tx, ty;               // tile counts
    int64_t gx, gy;           // grid: tiles by Cout / (16 nb)
    bool grid_too_large;
    int smem;                 // dynamic LDS bytes: halo + weight slab
};
constexpr int conv2d_fwd_smem(int cpc, int nb, int TX) { return conv2d_halo_bytes(cpc, TX, CONV2D_TY) + conv2d_steps(cpc) * 16 * nb * 64; }
static inline Conv2dFwdRoute conv2d_fwd_route(int64_t B, int64_t X, int64_t Y, int64_t Cin, int64_t Cout) {
    Conv2dFwdRoute r = {};
    const int64_t nb16 = Cout / 16;
    r.cpc = conv_cpc(Cin);
    r.nb = nb16 % 4 == 0 ? 4 : (nb16 % 2 == 0 ? 2 : 1);
    r.TX = r.nb == 4 ? 8 : 16;      // 64 output channels: 2 rows per wave (8 accumulator blocks), else 4 rows per wave (4 or 8)
    r.tx = (int)((X + r.TX - 1) / r.TX);
    r.ty = (int)((Y + CONV2D_TY - 1) / CONV2D_TY);
    r.gx = B * r.tx * r.ty;
    r.gy = nb16 / r.nb;
    r.grid_too_large = r.gx >= (1ll << 31) || r.gy >= 65536;
    r.smem = conv2d_fwd_smem(r.cpc, r.nb, r.TX);
    return r;
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------------------
constexpr int CONV2D_WGRAD_TX = 8, CONV2D_WGRAD_TY = 32;   // the tile: one 32-deep contraction step (32 pixels along y) per row
constexpr int CONV2D_WGRAD_WTAPS = 3;                      // taps per wave: wave w owns taps w, w + 4, w + 8

struct Conv2dWgradRoute {
    int cpc, mb, nbk;          // the instantiation; mb, nbk: 16-channel blocks of Cout and of the Cin chunk per workgroup
    int tx, ty, tiles;         // tile counts, tiles = B tx ty
    int n_wg, tiles_per_wg;    // grid x and the tiles each workgroup walks
    int gy;                    // grid y: (Cin chunk, Cout block) pairs
    int64_t n_out;             // floats of the packed weight gradient = of one partial
    int smem;                  // dynamic LDS bytes: dy image + x halo
    int64_t workspace_bytes;
};
constexpr int conv2d_wgrad_smem(int cpc, int mb) {
    return CONV2D_WGRAD_TX * CONV2D_WGRAD_TY * 32 * mb + conv2d_halo_bytes(cpc, CONV2D_WGRAD_TX, CONV2D_WGRAD_TY) + 64;
}
static inline Conv2dWgradRoute conv2d_wgrad_route(int64_t B, int64_t X, int64_t Y, int64_t Cin, int64_t Cout) {
    Conv2dWgradRoute r = {};
    r.cpc = conv_cpc(Cin);
    r.mb = Cout % 32 == 0 ? 2 : 1;
    r.nbk = r.cpc >= 16 ? r.cpc / 16 : 1;
    r.tx = (int)((X + CONV2D_WGRAD_TX - 1) / CONV2D_WGRAD_TX);
    r.ty = (int)((Y + CONV2D_WGRAD_TY - 1) / CONV2D_WGRAD_TY);
    r.tiles = (int)(B * r.tx * r.ty);
    r.gy = (int)((Cin / r.cpc) * (Cout / (16 * r.mb)));
    r.n_out = (int64_t)r.gy * CONV2D_TAPS * (16 * r.mb * 16 * r.nbk);
    int64_t cap = CONV_WGRAD_PART_FLOATS / r.n_out;
    cap = cap < 1 ? 1 : (cap > CONV_WGRAD_MAX_WGS ? CONV_WGRAD_MAX_WGS : cap);
    r.n_wg = (int)(r.tiles < cap ? r.tiles : cap);
    r.tiles_per_wg = (r.tiles + r.n_wg - 1) / r.n_wg;
    r.n_wg = (r.tiles + r.tiles_per_wg - 1) / r.tiles_per_wg;
    r.smem = conv2d_wgrad_smem(r.cpc, r.mb);
    r.workspace_bytes = (int64_t)r.n_wg * r.n_out * (int64_t)sizeof(float);
    return r;
}
