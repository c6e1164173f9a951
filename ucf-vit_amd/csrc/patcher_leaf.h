// What the kernels that walk (nodes, count) leaf by leaf share (patcher_labels.hip, patcher_labels_bwd.hip): the leaf of a workgroup, the pixel
// number of a leaf-local position, and the host checks of an image, a patch size and a dense image-plane layout.
#pragma once
#include "common.h"
#include "patcher_tree.h"

namespace {

// the leaf of workgroup blockIdx.x = b * L + s; `live`: a row below count[b] whose box is not empty and lies in the image
template <int ND>
struct BlockLeaf {
    int b, s;
    Leaf<ND> leaf;
    bool live;
    __device__ __forceinline__ BlockLeaf(const int* __restrict__ nodes, const int* __restrict__ count, int L, const int (&dims)[ND])
        : b((int)(blockIdx.x / (unsigned)L)), s((int)(blockIdx.x - (unsigned)b * (unsigned)L)), leaf(nodes + (int64_t)blockIdx.x * (2 * ND)) {
        live = s < count[b] && !leaf.empty() && leaf.inside(dims);
    }
};

// pixel number of leaf-local position x in an image of dims[a] pixels along axis a (x fastest)
template <int ND>
__device__ __forceinline__ int64_t pixel_of(const Leaf<ND>& lf, const int (&x)[ND], const int (&dims)[ND]) {
    int64_t pix = lf.o[ND - 1] + x[ND - 1];
#pragma unroll
    for (int a = ND - 2; a >= 0; --a) pix = pix * dims[a] + (lf.o[a] + x[a]);
    return pix;
}

template <int ND> struct Dims { int n[ND]; };              // pixels per axis, x first: (W, H) or (N, N, N)

// the output must be one of the two dense layouts of B images of S pixels and C channels: planar [B][C][S] or channels-last [B][S][C]
int out_layout(int64_t S, int64_t C, int64_t ob, int64_t oc, int64_t op, int* c_fast) {
    if (ob != S * C) return 0;
    if (oc == S && op == 1) {
        *c_fast = 0;
        return 1;
    }
    if (oc == 1 && op == C) {
        *c_fast = 1;
        return 1;
    }
    return 0;
}

// the image of an op, dims x first: 2-D H x W with sides below 32768, 3-D cubic of side 1..256
template <int ND>
int check_image(const char* who, int64_t B, const int64_t (&dims)[ND]) {
    if (ND == 2)
        UCF_CHECK_ARG(B >= 0 && dims[1] > 0 && dims[0] > 0 && dims[1] < 32768 && dims[0] < 32768, "%s: image %lld x %lld out of range", who,
                      (long long)dims[1], (long long)dims[0]);
    else
        UCF_CHECK_ARG(B >= 0 && dims[0] > 0 && dims[0] <= 256, "%s: cubic volumes of side 1..256 (got %lld)", who, (long long)dims[0]);
    return UCFVIT_OK;
}
constexpr int64_t max_patch(int nd) { return nd == 2 ? 1024 : 256; }

// the argument checks of a deserializer and of its adjoint: mode, image, shape limits, positive sequence strides, a dense image-plane layout;
// *pixels: the pixels of one image, *c_fast: 1 for the channels-last layout
template <int ND>
int check_deserialize(const char* who, int64_t B, const int64_t (&dims)[ND], int64_t C, int64_t L, int64_t p, int64_t stride_b, int64_t stride_c,
                      int64_t stride_s, int64_t stride_e, int64_t out_b, int64_t out_c, int64_t out_pixel, int mode, int64_t* pixels, int* c_fast) {
    UCF_CHECK_ARG(mode == UCFVIT_RESAMPLE_SMOOTH || mode == UCFVIT_RESAMPLE_NEAREST, "%s: unknown mode %d", who, mode);
    if (int rc = check_image<ND>(who, B, dims)) return rc;
    UCF_CHECK_ARG(C > 0 && C <= 255 && L > 0 && p > 0 && p <= max_patch(ND) && B * L < (1ll << 31), "%s: bad shape (C=%lld, L=%lld, p=%lld)", who,
                  (long long)C, (long long)L, (long long)p);
    UCF_CHECK_ARG(stride_b >= 0 && stride_c > 0 && stride_s > 0 && stride_e > 0, "%s: sequence strides must be positive", who);
    int64_t S = 1;
    for (int a = 0; a < ND; ++a) S *= dims[a];
    const char* px = ND == 2 ? "[H][W]" : "[N][N][N]";
    UCF_CHECK_ARG(out_layout(S, C, out_b, out_c, out_pixel, c_fast), "%s: output strides (%lld, %lld, %lld) are neither dense [B][C]%s nor dense [B]%s[C]",
                  who, (long long)out_b, (long long)out_c, (long long)out_pixel, px, px);
    *pixels = S;
    return UCFVIT_OK;
}

}  // namespace
