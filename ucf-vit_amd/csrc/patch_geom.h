// The patch layout that the patchify-MSE loss (csrc/elementwise.hip) and the DDPM reverse step (csrc/diffusion.hip) share: element e of
// token l of a prediction pred[b][l][e] belongs to one pixel of an NCHW(D) image,
//   e = ((ph*p + pw)[*p + pd])*C + c ,  l = (h*gw + w)[*gz + z]  ->  img[b][c][h*p+ph][w*p+pw][z*p+pd]
// which is the reference's unpatchify (misc.py:14-33).  nd == 1 is the pre-cut token sequence x[B][C][S][P] of the adaptive models.
#pragma once
#include "common.h"

struct PatchGeom {
    int C, H, W, Z, p, nd, gh, gw, gz, L, P;
};

// index into the image of element e of token l of sample b
__device__ __forceinline__ int64_t patch_pixel_index(const PatchGeom& g, int64_t b, int l, int e) {
    const int c = e % g.C;
    int s = e / g.C;
    if (g.nd == 1) {  // pre-cut token sequence x[B][C][S][P]: target row l = 'b c s p -> b s (p c)' (train_masked_simple.py:29)
        return ((b * g.C + c) * (int64_t)g.L + l) * g.p + s;
    } else if (g.nd == 2) {
        const int pw = s % g.p, ph = s / g.p;
        const int w = l % g.gw, h = l / g.gw;
        return ((b * g.C + c) * g.H + (h * g.p + ph)) * (int64_t)g.W + (w * g.p + pw);
    } else {
        const int pd = s % g.p;
        s /= g.p;
        const int pw = s % g.p, ph = s / g.p;
        const int z = l % g.gz;
        int t = l / g.gz;
        const int w = t % g.gw, h = t / g.gw;
        return (((b * g.C + c) * g.H + (h * g.p + ph)) * (int64_t)g.W + (w * g.p + pw)) * g.Z + (z * g.p + pd);
    }
}

// the geometry of an image (nd = 2 | 3: dims = {H, W[, Z]}, p = patch edge) or of a token sequence (nd = 1: dims = {S}, p = pixels per
// token and channel); the caller has checked the sizes
inline PatchGeom patch_geom_make(int64_t C, const int64_t* dims, int nd, int64_t p) {
    PatchGeom g;
    g.C = (int)C;
    g.H = (int)dims[0];
    g.W = (int)dims[1];
    g.Z = nd == 3 ? (int)dims[2] : 1;
    g.p = (int)p;
    g.nd = nd;
    g.gh = g.H / g.p;
    g.gw = g.W / g.p;
    g.gz = nd == 3 ? g.Z / g.p : 1;
    g.L = g.gh * g.gw * g.gz;
    g.P = (int)(C * p * p * (nd == 3 ? p : 1));
    if (nd == 1) {  // dims = {S}, p = pixels per token and channel
        g.H = g.W = g.Z = g.gh = g.gw = g.gz = 1;
        g.L = (int)dims[0];
        g.P = (int)(C * p);
    }
    return g;
}
