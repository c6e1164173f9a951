// The adjoints of the tree deserializers of patcher_labels.hip for gfx950: the gradient of a loss taken in the image plane, carried back through
// the tree to the token sequence.  The forward paints, per leaf, out[c, x] = sum_k w(x, k) seq[c, k] with separable weights (bicubic A = -0.75 with
// clamped taps, aligned-corner trilinear, nearest_floor / nearest_grid); this is dseq[c, k] = sum_{x in leaf} w(x, k) dout[c, x].
//
// A gather without atomics.  One thread owns one element (c, k) of a leaf's C * p^d gradient tile.  Per axis it walks a conservative run of leaf
// positions around token index k (Axis::range: about 4 n / p positions for bicubic, 2 n / p for linear, n / p for nearest, one spare on each
// side), evaluates every candidate position with the forward's own per-axis rule (resample_rules.h) and adds the taps that land on k, innermost
// axis first: for every row the sum over x, times the row's weight, summed over the rows (and over the planes in 3-D).  So a weight is never
// inverted, only evaluated, and an element's summation order follows from the leaf's extents and k alone.
//
// Leaves range from 2 to N pixels wide and the host cannot see the node list, so a large leaf is cut along its slowest axis into slices of
// slices_of() rows: a function of the leaf's extents and of BWD_SLICES / BWD_SLICE_PIXELS only.  grid.y = BWD_SLICES always; a workgroup whose
// slice lies past its leaf returns at once.  A leaf of one slice (every leaf up to BWD_SLICE_PIXELS pixels) writes dseq directly.  The slices of a
// larger leaf write their partial tiles to the workspace [B * L][BWD_SLICES][C * p^d] and deserialize_bwd_sum_kernel adds them in slice order.
// Neither gridDim, nor the layout of dout, nor timing enters a sum: the result is the same bits on every call.  Padding rows, empty leaves and
// leaves whose box leaves the image get zeros from the workgroup of slice 0, so every element of dseq is written exactly once.
#include "common.h"
// Built with -ffp-contract=off like patcher_labels.hip (Makefile: FLAGS_patcher_labels_bwd): the weights are then exactly the forward's.
#include "patcher_tree.h"
#include "patcher_leaf.h"
#include "resample_rules.h"
#include "patcher_gather.h"           // Axis, Gather, slices_of, BWD_SLICES, BWD_SLICE_PIXELS

namespace {

constexpr int BWD_THREADS = 256;
// element number o of a leaf's C x P gradient tile -> channel and patch element; the faster of the two in dseq is the faster in o
__device__ __forceinline__ void tile_index(int64_t o, int C, int P, bool c_first, int& c, int& e) {
    if (c_first) {
        c = (int)(o % C);
        e = (int)(o / C);
    } else {
        e = (int)(o % P);
        c = (int)(o / P);
    }
}

template <int ND, int RULE>
__global__ __launch_bounds__(BWD_THREADS) void deserialize_bwd_kernel(const float* __restrict__ dout, const int* __restrict__ nodes,
                                                                      const int* __restrict__ count, float* __restrict__ dseq,
                                                                      float* __restrict__ ws, Dims<ND> dims, int C, int L, int p, int64_t sb,
                                                                      int64_t sc, int64_t ss, int64_t se, int64_t ob, int64_t oc, int64_t op) {
    const BlockLeaf<ND> bl(nodes, count, L, dims.n);
    int P = p;
#pragma unroll
    for (int a = 1; a < ND; ++a) P *= p;
    const int64_t CP = (int64_t)C * P;
    const bool c_first = sc < se;
    float* dst = dseq + (int64_t)bl.b * sb + (int64_t)bl.s * ss;
    const int64_t first = (int64_t)blockIdx.z * BWD_THREADS + threadIdx.x, step = (int64_t)gridDim.z * BWD_THREADS;
    if (!bl.live) {
        if (blockIdx.y == 0)
            for (int64_t o = first; o < CP; o += step) {
                int c, e;
                tile_index(o, C, P, c_first, c, e);
                dst[(int64_t)c * sc + (int64_t)e * se] = 0.f;
            }
        return;
    }
    int rows, nsl;
    slices_of<ND>(bl.leaf, rows, nsl);
    if ((int)blockIdx.y >= nsl) return;
    const int r0 = (int)blockIdx.y * rows, r1 = r0 + rows < bl.leaf.n[ND - 1] ? r0 + rows : bl.leaf.n[ND - 1];
    Axis<RULE> ax[ND];
    int64_t pstride[ND], pix0 = 0, ps = 1;
#pragma unroll
    for (int a = 0; a < ND; ++a) {
        ax[a].set(bl.leaf.n[a], p);
        pstride[a] = ps;
        pix0 += (int64_t)bl.leaf.o[a] * ps;
        ps *= dims.n[a];
    }
    const float* g_b = dout + (int64_t)bl.b * ob;
    float* part = nsl > 1 ? ws + ((int64_t)blockIdx.x * BWD_SLICES + blockIdx.y) * CP : nullptr;
    for (int64_t o = first; o < CP; o += step) {
        int c, e, k[ND], lo[ND], hi[ND];
        tile_index(o, C, P, c_first, c, e);
        int r = e;
#pragma unroll
        for (int a = 0; a < ND; ++a) {                                      // e = (kz * p + ky) * p + kx
            k[a] = a < ND - 1 ? r % p : r;
            r /= p;
            ax[a].range(k[a], lo[a], hi[a]);
        }
        lo[ND - 1] = lo[ND - 1] > r0 ? lo[ND - 1] : r0;                     // this slice's rows
        hi[ND - 1] = hi[ND - 1] < r1 - 1 ? hi[ND - 1] : r1 - 1;
        const float acc = Gather<RULE, ND, ND - 1>::run(ax, k, lo, hi, g_b + (int64_t)c * oc, op, pix0, pstride);
        if (part) part[(int64_t)c * P + e] = acc;
        else dst[(int64_t)c * sc + (int64_t)e * se] = acc;
    }
}

// the leaves of more than one slice: dseq = partial tile of slice 0 + slice 1 + ... in this order
template <int ND>
__global__ __launch_bounds__(BWD_THREADS) void deserialize_bwd_sum_kernel(const float* __restrict__ ws, const int* __restrict__ nodes,
                                                                          const int* __restrict__ count, float* __restrict__ dseq, Dims<ND> dims,
                                                                          int C, int L, int p, int64_t sb, int64_t sc, int64_t ss, int64_t se) {
    const BlockLeaf<ND> bl(nodes, count, L, dims.n);
    if (!bl.live) return;
    int rows, nsl;
    slices_of<ND>(bl.leaf, rows, nsl);
    if (nsl < 2) return;
    int P = p;
#pragma unroll
    for (int a = 1; a < ND; ++a) P *= p;
    const int64_t CP = (int64_t)C * P;
    const bool c_first = sc < se;
    const float* part = ws + (int64_t)blockIdx.x * BWD_SLICES * CP;
    float* dst = dseq + (int64_t)bl.b * sb + (int64_t)bl.s * ss;
    for (int64_t o = (int64_t)blockIdx.y * BWD_THREADS + threadIdx.x; o < CP; o += (int64_t)gridDim.y * BWD_THREADS) {
        int c, e;
        tile_index(o, C, P, c_first, c, e);
        const float* q = part + (int64_t)c * P + e;
        float acc = q[0];
        for (int i = 1; i < nsl; ++i) acc += q[(int64_t)i * CP];
        dst[(int64_t)c * sc + (int64_t)e * se] = acc;
    }
}

constexpr int64_t WS_LIMIT = 1ll << 40;              // bytes: a request beyond it is refused, not wrapped

// bytes of partial tiles: none where no leaf of the image can have two slices
int64_t workspace_bytes(int64_t pixels, int64_t B, int64_t C, int64_t L, int64_t P) {
    if (pixels <= BWD_SLICE_PIXELS || B == 0) return 0;
    const int64_t tiles = B * L * BWD_SLICES;                               // < 2^35
    const int64_t tile = C * P * (int64_t)sizeof(float);                    // < 2^34
    return tile > WS_LIMIT / tiles ? -1 : tiles * tile;
}

template <int ND>
int64_t workspace_query(const char* who, int64_t B, const int64_t (&dims)[ND], int64_t C, int64_t L, int64_t p) {
    if (check_image<ND>(who, B, dims)) return -1;
    if (!(C > 0 && C <= 255 && L > 0 && p > 0 && p <= max_patch(ND) && B * L < (1ll << 31))) {
        ucfvit_set_error("%s: bad shape (C=%lld, L=%lld, p=%lld)", who, (long long)C, (long long)L, (long long)p);
        return -1;
    }
    int64_t S = 1, P = 1;
    for (int a = 0; a < ND; ++a) S *= dims[a], P *= p;
    const int64_t n = workspace_bytes(S, B, C, L, P);
    if (n < 0) ucfvit_set_error("%s: the workspace would exceed 2^40 bytes", who);
    return n;
}

template <int ND, int SMOOTH_RULE, int NEAREST_RULE>
int deserialize_bwd(const char* who, const float* dout, const int32_t* nodes, const int32_t* count, float* dseq, int64_t B,
                    const int64_t (&dims)[ND], int64_t C, int64_t L, int64_t p, int64_t stride_b, int64_t stride_c, int64_t stride_s, int64_t stride_e,
                    int64_t out_b, int64_t out_c, int64_t out_pixel, int mode, void* workspace, void* stream) {
    int64_t S = 0;
    int c_fast = 0;
    if (int rc = check_deserialize<ND>(who, B, dims, C, L, p, stride_b, stride_c, stride_s, stride_e, out_b, out_c, out_pixel, mode, &S, &c_fast)) return rc;
    UCF_CHECK_ARG(stride_b > 0 || B <= 1, "%s: batch elements of dseq must not share memory (stride_b = 0)", who);
    int64_t P = 1;
    for (int a = 0; a < ND; ++a) P *= p;
    const int64_t ws_bytes = workspace_bytes(S, B, C, L, P);
    UCF_CHECK_ARG(ws_bytes >= 0, "%s: the workspace would exceed 2^40 bytes", who);
    if (B == 0) return UCFVIT_OK;
    UCF_CHECK_ARG(dout && nodes && count && dseq && (workspace || ws_bytes == 0), "%s: null pointer", who);
    Dims<ND> d;
    for (int a = 0; a < ND; ++a) d.n[a] = (int)dims[a];
    hipStream_t s = (hipStream_t)stream;
    const int64_t tiles = (C * P + BWD_THREADS - 1) / BWD_THREADS;
    const unsigned gz = (unsigned)(tiles < (int64_t)BWD_TILES ? tiles : (int64_t)BWD_TILES);
    const dim3 grid((unsigned)(B * L), BWD_SLICES, gz);
    auto kern = mode == UCFVIT_RESAMPLE_NEAREST ? deserialize_bwd_kernel<ND, NEAREST_RULE> : deserialize_bwd_kernel<ND, SMOOTH_RULE>;
    hipLaunchKernelGGL(kern, grid, dim3(BWD_THREADS), 0, s, dout, nodes, count, dseq, (float*)workspace, d, (int)C, (int)L, (int)p, stride_b, stride_c,
                       stride_s, stride_e, out_b, out_c, out_pixel);
    UCF_LAUNCH_CHECK(who);
    if (ws_bytes > 0) {
        hipLaunchKernelGGL((deserialize_bwd_sum_kernel<ND>), dim3((unsigned)(B * L), gz), dim3(BWD_THREADS), 0, s, (const float*)workspace, nodes, count,
                           dseq, d, (int)C, (int)L, (int)p, stride_b, stride_c, stride_s, stride_e);
        UCF_LAUNCH_CHECK(who);
    }
    return UCFVIT_OK;
}

}  // namespace

extern "C" int64_t ucfvit_quadtree_deserialize_bwd_workspace(int64_t B, int64_t H, int64_t W, int64_t C, int64_t L, int64_t p) {
    return workspace_query<2>("ucfvit_quadtree_deserialize_bwd_workspace", B, {W, H}, C, L, p);
}

extern "C" int64_t ucfvit_octree_deserialize_bwd_workspace(int64_t B, int64_t N, int64_t C, int64_t L, int64_t p) {
    return workspace_query<3>("ucfvit_octree_deserialize_bwd_workspace", B, {N, N, N}, C, L, p);
}

extern "C" int ucfvit_quadtree_deserialize_bwd(const float* dout, const int32_t* nodes, const int32_t* count, float* dseq, int64_t B, int64_t H,
                                               int64_t W, int64_t C, int64_t L, int64_t p, int64_t stride_b, int64_t stride_c, int64_t stride_s,
                                               int64_t stride_e, int64_t out_b, int64_t out_c, int64_t out_pixel, int mode, void* workspace,
                                               void* stream) {
    return deserialize_bwd<2, RULE_CUBIC, RULE_FLOOR>("ucfvit_quadtree_deserialize_bwd", dout, nodes, count, dseq, B, {W, H}, C, L, p, stride_b, stride_c,
                                                      stride_s, stride_e, out_b, out_c, out_pixel, mode, workspace, stream);
}

extern "C" int ucfvit_octree_deserialize_bwd(const float* dout, const int32_t* nodes, const int32_t* count, float* dseq, int64_t B, int64_t N, int64_t C,
                                             int64_t L, int64_t p, int64_t stride_b, int64_t stride_c, int64_t stride_s, int64_t stride_e, int64_t out_b,
                                             int64_t out_c, int64_t out_pixel, int mode, void* workspace, void* stream) {
    return deserialize_bwd<3, RULE_LINEAR, RULE_GRID>("ucfvit_octree_deserialize_bwd", dout, nodes, count, dseq, B, {N, N, N}, C, L, p, stride_b, stride_c,
                                                      stride_s, stride_e, out_b, out_c, out_pixel, mode, workspace, stream);
}
