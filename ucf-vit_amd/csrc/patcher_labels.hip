// Label serializers and tree deserializers of the adaptive patcher for gfx950: the two tree operations that turn a patched input into a
// segmentation workload (reference: dataloaders/quadtree.py:176-221 + Rect.set_area, octree.py:152-213 + Cube.set_area).
//   *_serialize_labels : every leaf's label region resampled to p^d with a nearest-neighbour rule through the image's own tree, written
//                        as class indices int64 [B][L][p^d] and / or one-hot fp32 [B][nc][L * p^d] (the reference's collate output in the
//                        memory order training_step_adaptive's plain reshape reads).
//   *_deserialize      : a token sequence painted back into the image plane leaf by leaf: every leaf region is its p^d patch resized to
//                        the leaf's extent (bicubic A = -0.75 in 2-D, aligned-corner trilinear in 3-D, or nearest), read in place through
//                        element strides and written planar or channels-last (either dense layout, given as element strides).
// Pure gathers over (nodes, count) as quadtree.hip's builders leave them; no atomics.  Serializers: one workgroup per (b, leaf), p^d
// outputs each.  Deserializers: leaves range from 2 to N pixels wide, so grid.y walks fixed-size chunks of a leaf's outputs and a
// workgroup whose first chunk lies past the leaf returns at once.  A node whose box leaves the image is treated as an empty leaf.
#include "common.h"
// Built with -ffp-contract=off (Makefile: FLAGS_patcher_labels): every product and sum is rounded on its own.  The compiler may duplicate a
// deserializer's loop per output layout and vectorise one copy; with contraction left to it the two layouts differed in the last bit.
// Without it a result depends on the source alone and equals a plain fp32 evaluation of the same expressions, so the sampling expressions
// below can move between functions without changing a bit (quadtree.hip's serializers, built with contraction, cannot: see there).
#include "patcher_tree.h"            // Leaf, leaf_index
#include "patcher_leaf.h"            // BlockLeaf, pixel_of, Dims, out_layout, check_image, max_patch
#include "resample_rules.h"

namespace {

constexpr int DES_THREADS = 256;
constexpr int DES_CHUNK = 1024;                      // outputs of one leaf per workgroup step
constexpr int64_t DES_WORKGROUPS = 131072;           // workgroup budget of one deserializer launch (see chunk_rows)
constexpr int64_t DES_ROWS = 16;                     // workgroups per leaf where leaves are many

template <typename T> __device__ __forceinline__ long long load_label(const T* p) { return (long long)*p; }

// one resampled label: its index value and its one-hot column (all-zero for a label outside [0, nc))
__device__ __forceinline__ void put_label(long long v, int64_t* idx_out, float* onehot, int64_t plane, int nc) {
    if (idx_out) *idx_out = (int64_t)v;
    if (onehot)
        for (int c = 0; c < nc; ++c) onehot[(int64_t)c * plane] = (v == (long long)c) ? 1.f : 0.f;
}

// labels [B][dims, x fastest] -> p^ND resampled labels per leaf, patch axis 0 the slowest image axis (octree.py: img[z1:z2, y1:y2, x1:x2]).
// Per axis the 2-D rule is cv2's nearest_floor, the 3-D rule scipy's nearest_grid.
template <int ND, typename T>
__global__ __launch_bounds__(256) void labels_kernel(const T* __restrict__ labels, const int* __restrict__ nodes, const int* __restrict__ count,
                                                     int64_t* __restrict__ idx, float* __restrict__ onehot, Dims<ND> dims, int L, int p, int nc) {
    const BlockLeaf<ND> bl(nodes, count, L, dims.n);
    int P = p;
    int64_t npix = dims.n[0];
#pragma unroll
    for (int a = 1; a < ND; ++a) P *= p, npix *= dims.n[a];
    const int64_t plane = (int64_t)L * P;                                  // one class plane of one image
    int64_t* io = idx ? idx + (int64_t)blockIdx.x * P : nullptr;
    float* oo = onehot ? onehot + (int64_t)bl.b * nc * plane + (int64_t)bl.s * P : nullptr;
    const T* src = labels + (int64_t)bl.b * npix;
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        long long v = 0;                                                   // padding rows and empty leaves: class 0
        if (bl.live) {
            int x[ND], r = i;
#pragma unroll
            for (int a = 0; a < ND; ++a) {
                const int j = a < ND - 1 ? r % p : r;
                r /= p;
                x[a] = ND == 2 ? nearest_floor(j, bl.leaf.n[a], p) : nearest_grid(j, bl.leaf.n[a], p);
            }
            v = load_label(src + pixel_of(bl.leaf, x, dims.n));
        }
        put_label(v, io ? io + i : nullptr, oo ? oo + i : nullptr, plane, nc);
    }
}

// A live leaf's outputs, walked by the workgroups of one blockIdx.x: grid.y strides over chunks of DES_CHUNK outputs; sample(c, x) is the value of
// channel c at leaf-local pixel x, read from the leaf's patch.  Output layout as leaf_index orders it.
template <int ND, typename Sample>
__device__ __forceinline__ void paint_leaf(const Leaf<ND>& lf, const int (&dims)[ND], int C, int c_fast, float* __restrict__ dst_b, int64_t oc,
                                           int64_t op, Sample sample) {
    int64_t n_leaf = C;
#pragma unroll
    for (int a = 0; a < ND; ++a) n_leaf *= lf.n[a];
    const bool small = n_leaf <= 0x7fffffffLL;                             // 32-bit index arithmetic: a 64-bit division costs several times as much
    for (int64_t base = (int64_t)blockIdx.y * DES_CHUNK; base < n_leaf; base += (int64_t)gridDim.y * DES_CHUNK) {
        for (int64_t i = base + threadIdx.x; i < base + DES_CHUNK && i < n_leaf; i += DES_THREADS) {
            int c, x[ND];
            if (small) leaf_index<ND, unsigned>((unsigned)i, C, lf.n, c_fast, c, x);
            else leaf_index<ND, int64_t>(i, C, lf.n, c_fast, c, x);
            dst_b[(int64_t)c * oc + pixel_of(lf, x, dims) * op] = sample(c, x);
        }
    }
}

// 2-D: leaf region (w x h) <- its p x p patch.
template <bool NEAREST, bool TRUNC>
__global__ __launch_bounds__(DES_THREADS) void quadtree_deserialize_kernel(const float* __restrict__ seq, const int* __restrict__ nodes,
                                                                          const int* __restrict__ count, float* __restrict__ out, int H, int W,
                                                                          int C, int L, int p, int64_t sb, int64_t sc, int64_t ss, int64_t se,
                                                                          int64_t ob, int64_t oc, int64_t op, int c_fast) {
    const int dims[2] = {W, H};
    const BlockLeaf<2> bl(nodes, count, L, dims);
    if (!bl.live) return;
    const int w = bl.leaf.n[0], h = bl.leaf.n[1];
    const float sx = (float)p / (float)w, sy = (float)p / (float)h;
    const float* src_s = seq + (int64_t)bl.b * sb + (int64_t)bl.s * ss;
    paint_leaf<2>(bl.leaf, dims, C, c_fast, out + (int64_t)bl.b * ob, oc, op, [&](int c, const int (&xy)[2]) {
        const int x = xy[0], y = xy[1];
        const float* src = src_s + (int64_t)c * sc;
        float acc;
        if (NEAREST) {
            acc = src[(int64_t)(nearest_floor(y, p, h) * p + nearest_floor(x, p, w)) * se];
        } else {
            // positions and coefficients are resample_rules.h's, as the adjoint (patcher_labels_bwd.hip) evaluates them; the integer clamps of the
            // taps stay written out here (tap_clamp there): calling them moved this kernel's register allocation
            const float fy = half_pixel_pos(y, sy), fx = half_pixel_pos(x, sx);
            const float fyf = floorf(fy), fxf = floorf(fx);
            const int iy = (int)fyf, ix = (int)fxf;
            float wy[4], wx[4];
            cubic_coeffs(fy - fyf, wy);
            cubic_coeffs(fx - fxf, wx);
            acc = 0.f;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                int yy = iy - 1 + a;
                yy = yy < 0 ? 0 : (yy > p - 1 ? p - 1 : yy);
                float r = 0.f;
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    int xx = ix - 1 + d;
                    xx = xx < 0 ? 0 : (xx > p - 1 ? p - 1 : xx);
                    float t = src[(int64_t)(yy * p + xx) * se];
                    if (TRUNC) t = truncf(t);
                    r += wx[d] * t;
                }
                acc += wy[a] * r;
            }
        }
        return acc;
    });
}

// 3-D: leaf region (nx x ny x nz) <- its p^3 patch (patch axis 0 is z, 1 is y, 2 is x)
template <bool NEAREST>
__global__ __launch_bounds__(DES_THREADS) void octree_deserialize_kernel(const float* __restrict__ seq, const int* __restrict__ nodes,
                                                                        const int* __restrict__ count, float* __restrict__ out, int N, int C, int L,
                                                                        int p, int64_t sb, int64_t sc, int64_t ss, int64_t se, int64_t ob,
                                                                        int64_t oc, int64_t op, int c_fast) {
    const int dims[3] = {N, N, N};
    const BlockLeaf<3> bl(nodes, count, L, dims);
    if (!bl.live) return;
    const int nx = bl.leaf.n[0], ny = bl.leaf.n[1], nz = bl.leaf.n[2];
    const float invx = linear_inv(nx), invy = linear_inv(ny), invz = linear_inv(nz);
    const float* src_s = seq + (int64_t)bl.b * sb + (int64_t)bl.s * ss;
    paint_leaf<3>(bl.leaf, dims, C, c_fast, out + (int64_t)bl.b * ob, oc, op, [&](int c, const int (&xyz)[3]) {
        const int x = xyz[0], y = xyz[1], z = xyz[2];
        const float* src = src_s + (int64_t)c * sc;
        auto at = [&](int zz, int yy, int xx) { return src[(int64_t)((zz * p + yy) * p + xx) * se]; };
        float acc;
        if (NEAREST) {
            acc = at(nearest_grid(z, p, nz), nearest_grid(y, p, ny), nearest_grid(x, p, nx));
        } else {
            // as above: linear_cell / linear_upper written out
            const float fz = corner_pos(z, p, invz), fy = corner_pos(y, p, invy), fx = corner_pos(x, p, invx);
            int z0 = (int)fz, y0 = (int)fy, x0 = (int)fx;
            z0 = z0 > p - 1 ? p - 1 : z0;
            y0 = y0 > p - 1 ? p - 1 : y0;
            x0 = x0 > p - 1 ? p - 1 : x0;
            const float tz = fz - (float)z0, ty = fy - (float)y0, tx = fx - (float)x0;
            const int z1i = z0 + 1 < p ? z0 + 1 : p - 1, y1i = y0 + 1 < p ? y0 + 1 : p - 1, x1i = x0 + 1 < p ? x0 + 1 : p - 1;
            const float c00 = at(z0, y0, x0) * (1.f - tx) + at(z0, y0, x1i) * tx;
            const float c01 = at(z0, y1i, x0) * (1.f - tx) + at(z0, y1i, x1i) * tx;
            const float c10 = at(z1i, y0, x0) * (1.f - tx) + at(z1i, y0, x1i) * tx;
            const float c11 = at(z1i, y1i, x0) * (1.f - tx) + at(z1i, y1i, x1i) * tx;
            const float c0 = c00 * (1.f - ty) + c01 * ty, c1 = c10 * (1.f - ty) + c11 * ty;
            acc = c0 * (1.f - tz) + c1 * tz;
        }
        return acc;
    });
}

// grid.y: the workgroups that share one leaf; a workgroup walks its leaf in steps of grid.y chunks.  The host cannot see the largest leaf, so
// the rows are a fixed number: 16 where leaves are many (a workgroup whose first chunk lies past its leaf returns at once, but 131072 of them
// still cost 45 us on an MI355X, measured: more rows lost at 1024 leaves of 64^3, fewer lost at 8192 leaves of 512^2, where the 256^2 leaf
// is the tail), more where leaves are few (4096 workgroups to fill the device), within the budget and never more than the largest possible
// leaf (the whole image) has chunks.
unsigned chunk_rows(int64_t leaves, int64_t max_leaf_outputs) {
    const int64_t max_chunks = (max_leaf_outputs + DES_CHUNK - 1) / DES_CHUNK;
    int64_t gy = 4096 / leaves > DES_ROWS ? 4096 / leaves : DES_ROWS;
    gy = gy > DES_WORKGROUPS / leaves ? DES_WORKGROUPS / leaves : gy;
    gy = gy < 1 ? 1 : gy;
    gy = gy > max_chunks ? max_chunks : gy;
    return (unsigned)(gy > 65535 ? 65535 : gy);
}

template <int ND>
int serialize_labels(const char* who, const void* labels, const int32_t* nodes, const int32_t* count, int64_t* idx, float* onehot, int64_t B,
                     const int64_t (&dims)[ND], int64_t L, int64_t p, int64_t num_classes, int label_dtype, void* stream) {
    UCF_CHECK_ARG(label_dtype == UCFVIT_LABEL_U8 || label_dtype == UCFVIT_LABEL_I64, "%s: label dtype %d is neither uint8 nor int64", who, label_dtype);
    if (int rc = check_image<ND>(who, B, dims)) return rc;
    UCF_CHECK_ARG(L > 0 && p > 0 && p <= max_patch(ND) && B * L < (1ll << 31), "%s: bad shape (L=%lld, p=%lld)", who, (long long)L, (long long)p);
    UCF_CHECK_ARG(num_classes >= 1 && num_classes <= 255, "%s: num_classes=%lld outside 1..255", who, (long long)num_classes);
    if (B == 0) return UCFVIT_OK;
    UCF_CHECK_ARG(labels && nodes && count && (idx || onehot), "%s: null pointer", who);
    Dims<ND> d;
    for (int a = 0; a < ND; ++a) d.n[a] = (int)dims[a];
    auto launch = [&](auto type) {
        using T = decltype(type);
        hipLaunchKernelGGL((labels_kernel<ND, T>), dim3((unsigned)(B * L)), dim3(256), 0, (hipStream_t)stream, (const T*)labels, nodes, count, idx, onehot,
                           d, (int)L, (int)p, (int)num_classes);
    };
    if (label_dtype == UCFVIT_LABEL_U8) launch(uint8_t{});
    else launch(int64_t{});
    UCF_LAUNCH_CHECK(who);
    return UCFVIT_OK;
}

// checks, the zero fill of the dense output (B * S * C floats in either layout) and the grid; launch(grid, c_fast) starts the kernel
template <int ND, typename Launch>
int deserialize(const char* who, const float* seq, const int32_t* nodes, const int32_t* count, float* out, int64_t B, const int64_t (&dims)[ND],
                int64_t C, int64_t L, int64_t p, int64_t stride_b, int64_t stride_c, int64_t stride_s, int64_t stride_e, int64_t out_b, int64_t out_c,
                int64_t out_pixel, int mode, hipStream_t s, Launch launch) {
    int64_t S = 0;
    int c_fast = 0;
    if (int rc = check_deserialize<ND>(who, B, dims, C, L, p, stride_b, stride_c, stride_s, stride_e, out_b, out_c, out_pixel, mode, &S, &c_fast)) return rc;
    if (B == 0) return UCFVIT_OK;
    UCF_CHECK_ARG(seq && nodes && count && out, "%s: null pointer", who);
    if (hipMemsetAsync(out, 0, (size_t)(B * S * C) * sizeof(float), s) != hipSuccess) {
        ucfvit_set_error("%s: hipMemsetAsync failed", who);
        return UCFVIT_ERR_HIP;
    }
    launch(dim3((unsigned)(B * L), chunk_rows(B * L, S * C)), c_fast);
    UCF_LAUNCH_CHECK(who);
    return UCFVIT_OK;
}

}  // namespace

extern "C" int ucfvit_quadtree_serialize_labels(const void* labels, const int32_t* nodes, const int32_t* count, int64_t* idx, float* onehot,
                                                int64_t B, int64_t H, int64_t W, int64_t L, int64_t p, int64_t num_classes, int label_dtype,
                                                void* stream) {
    return serialize_labels<2>("ucfvit_quadtree_serialize_labels", labels, nodes, count, idx, onehot, B, {W, H}, L, p, num_classes, label_dtype, stream);
}

extern "C" int ucfvit_octree_serialize_labels(const void* labels, const int32_t* nodes, const int32_t* count, int64_t* idx, float* onehot, int64_t B,
                                              int64_t N, int64_t L, int64_t p, int64_t num_classes, int label_dtype, void* stream) {
    return serialize_labels<3>("ucfvit_octree_serialize_labels", labels, nodes, count, idx, onehot, B, {N, N, N}, L, p, num_classes, label_dtype, stream);
}

extern "C" int ucfvit_quadtree_deserialize(const float* seq, const int32_t* nodes, const int32_t* count, float* out, int64_t B, int64_t H, int64_t W,
                                           int64_t C, int64_t L, int64_t p, int64_t stride_b, int64_t stride_c, int64_t stride_s, int64_t stride_e,
                                           int64_t out_b, int64_t out_c, int64_t out_pixel, int mode, int trunc, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    auto kern = mode == UCFVIT_RESAMPLE_NEAREST ? quadtree_deserialize_kernel<true, false>
                : trunc                         ? quadtree_deserialize_kernel<false, true>
                                                : quadtree_deserialize_kernel<false, false>;
    return deserialize<2>("ucfvit_quadtree_deserialize", seq, nodes, count, out, B, {W, H}, C, L, p, stride_b, stride_c, stride_s, stride_e, out_b, out_c,
                          out_pixel, mode, s, [&](dim3 grid, int c_fast) {
                              hipLaunchKernelGGL(kern, grid, dim3(DES_THREADS), 0, s, seq, nodes, count, out, (int)H, (int)W, (int)C, (int)L, (int)p,
                                                 stride_b, stride_c, stride_s, stride_e, out_b, out_c, out_pixel, c_fast);
                          });
}

extern "C" int ucfvit_octree_deserialize(const float* seq, const int32_t* nodes, const int32_t* count, float* out, int64_t B, int64_t N, int64_t C,
                                         int64_t L, int64_t p, int64_t stride_b, int64_t stride_c, int64_t stride_s, int64_t stride_e, int64_t out_b,
                                         int64_t out_c, int64_t out_pixel, int mode, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    auto kern = mode == UCFVIT_RESAMPLE_NEAREST ? octree_deserialize_kernel<true> : octree_deserialize_kernel<false>;
    return deserialize<3>("ucfvit_octree_deserialize", seq, nodes, count, out, B, {N, N, N}, C, L, p, stride_b, stride_c, stride_s, stride_e, out_b, out_c,
                          out_pixel, mode, s, [&](dim3 grid, int c_fast) {
                              hipLaunchKernelGGL(kern, grid, dim3(DES_THREADS), 0, s, seq, nodes, count, out, (int)N, (int)C, (int)L, (int)p, stride_b,
                                                 stride_c, stride_s, stride_e, out_b, out_c, out_pixel, c_fast);
                          });
}
