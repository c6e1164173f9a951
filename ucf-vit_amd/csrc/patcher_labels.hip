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
// Built with -ffp-contract=off (Makefile: FLAGS_patcher_labels): every product and sum is rounded on its own.  The compiler duplicates the
// deserializers' loops per output layout and vectorises one copy; with contraction left to it the two layouts differed in the last bit.
// Without it a result depends on the source alone and equals a plain fp32 evaluation of the same expressions.
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

template <typename T>
__global__ __launch_bounds__(256) void quadtree_labels_kernel(const T* __restrict__ labels, const int* __restrict__ nodes,
                                                              const int* __restrict__ count, int64_t* __restrict__ idx, float* __restrict__ onehot,
                                                              int H, int W, int L, int p, int nc) {
    const int64_t bs = blockIdx.x;
    const int b = (int)(bs / L), s = (int)(bs - (int64_t)b * L);
    const int P = p * p;
    const int64_t plane = (int64_t)L * P;                                  // one class plane of one image
    int64_t* io = idx ? idx + bs * P : nullptr;
    float* oo = onehot ? onehot + (int64_t)b * nc * plane + (int64_t)s * P : nullptr;
    const int* q = nodes + bs * 4;
    const int x1 = q[0], x2 = q[1], y1 = q[2], y2 = q[3];
    const int w = x2 - x1, h = y2 - y1;
    const bool valid = s < count[b] && w > 0 && h > 0 && x1 >= 0 && y1 >= 0 && x2 <= W && y2 <= H;
    const T* src = labels + (int64_t)b * H * W;
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        long long v = 0;                                                   // padding rows and empty leaves: class 0
        if (valid) {
            const int px = i % p, py = i / p;
            v = load_label(src + (int64_t)(y1 + nearest_floor(py, h, p)) * W + (x1 + nearest_floor(px, w, p)));
        }
        put_label(v, io ? io + i : nullptr, oo ? oo + i : nullptr, plane, nc);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void octree_labels_kernel(const T* __restrict__ labels, const int* __restrict__ nodes,
                                                            const int* __restrict__ count, int64_t* __restrict__ idx, float* __restrict__ onehot,
                                                            int N, int L, int p, int nc) {
    const int64_t bs = blockIdx.x;
    const int b = (int)(bs / L), s = (int)(bs - (int64_t)b * L);
    const int P = p * p * p;
    const int64_t plane = (int64_t)L * P;
    int64_t* io = idx ? idx + bs * P : nullptr;
    float* oo = onehot ? onehot + (int64_t)b * nc * plane + (int64_t)s * P : nullptr;
    const int* q = nodes + bs * 6;
    const int x1 = q[0], y1 = q[2], z1 = q[4];
    const int nx = q[1] - x1, ny = q[3] - y1, nz = q[5] - z1;
    const bool valid = s < count[b] && nx > 0 && ny > 0 && nz > 0 && x1 >= 0 && y1 >= 0 && z1 >= 0 && q[1] <= N && q[3] <= N && q[5] <= N;
    const T* src = labels + (int64_t)b * N * N * N;
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        long long v = 0;
        if (valid) {
            // axis 0 of the leaf is z, axis 1 is y, axis 2 is x (octree.py: img[z1:z2, y1:y2, x1:x2])
            const int k = i % p, j = (i / p) % p, ii = i / (p * p);
            const int z = z1 + nearest_grid(ii, nz, p), y = y1 + nearest_grid(j, ny, p), x = x1 + nearest_grid(k, nx, p);
            v = load_label(src + ((int64_t)z * N + y) * N + x);
        }
        put_label(v, io ? io + i : nullptr, oo ? oo + i : nullptr, plane, nc);
    }
}

// (c, x, y[, z]) of output number i of a leaf: x fastest, then y (, z), then c (planar outputs) or c fastest, then x, y (, z) (channels-last
// outputs), so that consecutive lanes write consecutive addresses.  I: unsigned where the leaf has fewer than 2^31 outputs, else int64_t.
template <typename I>
__device__ __forceinline__ void leaf_index2(I i, int C, int w, int h, int c_fast, int& c, int& x, int& y) {
    if (c_fast) {
        c = (int)(i % (I)C);
        const I r = i / (I)C;
        x = (int)(r % (I)w);
        y = (int)(r / (I)w);
    } else {
        x = (int)(i % (I)w);
        const I r = i / (I)w;
        y = (int)(r % (I)h);
        c = (int)(r / (I)h);
    }
}
template <typename I>
__device__ __forceinline__ void leaf_index3(I i, int C, int nx, int ny, int nz, int c_fast, int& c, int& x, int& y, int& z) {
    I r = i;
    if (c_fast) {
        c = (int)(r % (I)C);
        r /= (I)C;
    }
    x = (int)(r % (I)nx);
    r /= (I)nx;
    y = (int)(r % (I)ny);
    r /= (I)ny;
    z = (int)(r % (I)nz);
    if (!c_fast) c = (int)(r / (I)nz);
}

// 2-D: leaf region (w x h) <- its p x p patch.
template <bool NEAREST, bool TRUNC>
__global__ __launch_bounds__(DES_THREADS) void quadtree_deserialize_kernel(const float* __restrict__ seq, const int* __restrict__ nodes,
                                                                          const int* __restrict__ count, float* __restrict__ out, int H, int W,
                                                                          int C, int L, int p, int64_t sb, int64_t sc, int64_t ss, int64_t se,
                                                                          int64_t ob, int64_t oc, int64_t op, int c_fast) {
    const int64_t bs = blockIdx.x;
    const int b = (int)(bs / L), s = (int)(bs - (int64_t)b * L);
    const int* q = nodes + bs * 4;
    const int x1 = q[0], x2 = q[1], y1 = q[2], y2 = q[3];
    const int w = x2 - x1, h = y2 - y1;
    if (s >= count[b] || w <= 0 || h <= 0 || x1 < 0 || y1 < 0 || x2 > W || y2 > H) return;
    const int64_t n_leaf = (int64_t)w * h * C;
    const bool small = n_leaf <= 0x7fffffffLL;                             // 32-bit index arithmetic: a 64-bit division costs several times as much
    const float sx = (float)p / (float)w, sy = (float)p / (float)h;
    const float* src_s = seq + (int64_t)b * sb + (int64_t)s * ss;
    float* dst_b = out + (int64_t)b * ob;
    for (int64_t base = (int64_t)blockIdx.y * DES_CHUNK; base < n_leaf; base += (int64_t)gridDim.y * DES_CHUNK) {
        for (int64_t i = base + threadIdx.x; i < base + DES_CHUNK && i < n_leaf; i += DES_THREADS) {
            int c, x, y;
            if (small) leaf_index2<unsigned>((unsigned)i, C, w, h, c_fast, c, x, y);
            else leaf_index2<int64_t>(i, C, w, h, c_fast, c, x, y);
            const float* src = src_s + (int64_t)c * sc;
            float acc;
            if (NEAREST) {
                acc = src[(int64_t)(nearest_floor(y, p, h) * p + nearest_floor(x, p, w)) * se];
            } else {
                const float fy = ((float)y + 0.5f) * sy - 0.5f, fx = ((float)x + 0.5f) * sx - 0.5f;
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
            dst_b[(int64_t)c * oc + ((int64_t)(y1 + y) * W + (x1 + x)) * op] = acc;
        }
    }
}

// 3-D: leaf region (nx x ny x nz) <- its p^3 patch (patch axis 0 is z, 1 is y, 2 is x)
template <bool NEAREST>
__global__ __launch_bounds__(DES_THREADS) void octree_deserialize_kernel(const float* __restrict__ seq, const int* __restrict__ nodes,
                                                                        const int* __restrict__ count, float* __restrict__ out, int N, int C, int L,
                                                                        int p, int64_t sb, int64_t sc, int64_t ss, int64_t se, int64_t ob,
                                                                        int64_t oc, int64_t op, int c_fast) {
    const int64_t bs = blockIdx.x;
    const int b = (int)(bs / L), s = (int)(bs - (int64_t)b * L);
    const int* q = nodes + bs * 6;
    const int x1 = q[0], y1 = q[2], z1 = q[4];
    const int nx = q[1] - x1, ny = q[3] - y1, nz = q[5] - z1;
    if (s >= count[b] || nx <= 0 || ny <= 0 || nz <= 0 || x1 < 0 || y1 < 0 || z1 < 0 || q[1] > N || q[3] > N || q[5] > N) return;
    const int64_t n_leaf = (int64_t)nx * ny * nz * C;
    const bool small = n_leaf <= 0x7fffffffLL;
    const float invx = nx > 1 ? 1.f / (float)(nx - 1) : 0.f, invy = ny > 1 ? 1.f / (float)(ny - 1) : 0.f,
                invz = nz > 1 ? 1.f / (float)(nz - 1) : 0.f;
    const float* src_s = seq + (int64_t)b * sb + (int64_t)s * ss;
    float* dst_b = out + (int64_t)b * ob;
    for (int64_t base = (int64_t)blockIdx.y * DES_CHUNK; base < n_leaf; base += (int64_t)gridDim.y * DES_CHUNK) {
        for (int64_t i = base + threadIdx.x; i < base + DES_CHUNK && i < n_leaf; i += DES_THREADS) {
            int c, x, y, z;
            if (small) leaf_index3<unsigned>((unsigned)i, C, nx, ny, nz, c_fast, c, x, y, z);
            else leaf_index3<int64_t>(i, C, nx, ny, nz, c_fast, c, x, y, z);
            const float* src = src_s + (int64_t)c * sc;
            auto at = [&](int zz, int yy, int xx) { return src[(int64_t)((zz * p + yy) * p + xx) * se]; };
            float acc;
            if (NEAREST) {
                acc = at(nearest_grid(z, p, nz), nearest_grid(y, p, ny), nearest_grid(x, p, nx));
            } else {
                const float fz = (float)z * (float)(p - 1) * invz, fy = (float)y * (float)(p - 1) * invy, fx = (float)x * (float)(p - 1) * invx;
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
            dst_b[(int64_t)c * oc + (((int64_t)(z1 + z) * N + (y1 + y)) * N + (x1 + x)) * op] = acc;
        }
    }
}

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

}  // namespace

extern "C" int ucfvit_quadtree_serialize_labels(const void* labels, const int32_t* nodes, const int32_t* count, int64_t* idx, float* onehot,
                                                int64_t B, int64_t H, int64_t W, int64_t L, int64_t p, int64_t num_classes, int label_dtype,
                                                void* stream) {
    UCF_CHECK_ARG(label_dtype == UCFVIT_LABEL_U8 || label_dtype == UCFVIT_LABEL_I64, "ucfvit_quadtree_serialize_labels: label dtype %d is neither uint8 nor int64",
                  label_dtype);
    UCF_CHECK_ARG(B >= 0 && H > 0 && W > 0 && H < 32768 && W < 32768, "ucfvit_quadtree_serialize_labels: image %lld x %lld out of range", (long long)H,
                  (long long)W);
    UCF_CHECK_ARG(L > 0 && p > 0 && p <= 1024 && B * L < (1ll << 31), "ucfvit_quadtree_serialize_labels: bad shape (L=%lld, p=%lld)", (long long)L,
                  (long long)p);
    UCF_CHECK_ARG(num_classes >= 1 && num_classes <= 255, "ucfvit_quadtree_serialize_labels: num_classes=%lld outside 1..255", (long long)num_classes);
    if (B == 0) return UCFVIT_OK;
    UCF_CHECK_ARG(labels && nodes && count && (idx || onehot), "ucfvit_quadtree_serialize_labels: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (label_dtype == UCFVIT_LABEL_U8)
        hipLaunchKernelGGL(quadtree_labels_kernel<uint8_t>, dim3((unsigned)(B * L)), dim3(256), 0, s, (const uint8_t*)labels, nodes, count, idx, onehot,
                           (int)H, (int)W, (int)L, (int)p, (int)num_classes);
    else
        hipLaunchKernelGGL(quadtree_labels_kernel<int64_t>, dim3((unsigned)(B * L)), dim3(256), 0, s, (const int64_t*)labels, nodes, count, idx, onehot,
                           (int)H, (int)W, (int)L, (int)p, (int)num_classes);
    UCF_LAUNCH_CHECK("ucfvit_quadtree_serialize_labels");
    return UCFVIT_OK;
}

extern "C" int ucfvit_octree_serialize_labels(const void* labels, const int32_t* nodes, const int32_t* count, int64_t* idx, float* onehot, int64_t B,
                                              int64_t N, int64_t L, int64_t p, int64_t num_classes, int label_dtype, void* stream) {
    UCF_CHECK_ARG(label_dtype == UCFVIT_LABEL_U8 || label_dtype == UCFVIT_LABEL_I64, "ucfvit_octree_serialize_labels: label dtype %d is neither uint8 nor int64",
                  label_dtype);
    UCF_CHECK_ARG(B >= 0 && N > 0 && N <= 256, "ucfvit_octree_serialize_labels: cubic volumes of side 1..256 (got %lld)", (long long)N);
    UCF_CHECK_ARG(L > 0 && p > 0 && p <= 256 && B * L < (1ll << 31), "ucfvit_octree_serialize_labels: bad shape (L=%lld, p=%lld)", (long long)L,
                  (long long)p);
    UCF_CHECK_ARG(num_classes >= 1 && num_classes <= 255, "ucfvit_octree_serialize_labels: num_classes=%lld outside 1..255", (long long)num_classes);
    if (B == 0) return UCFVIT_OK;
    UCF_CHECK_ARG(labels && nodes && count && (idx || onehot), "ucfvit_octree_serialize_labels: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (label_dtype == UCFVIT_LABEL_U8)
        hipLaunchKernelGGL(octree_labels_kernel<uint8_t>, dim3((unsigned)(B * L)), dim3(256), 0, s, (const uint8_t*)labels, nodes, count, idx, onehot,
                           (int)N, (int)L, (int)p, (int)num_classes);
    else
        hipLaunchKernelGGL(octree_labels_kernel<int64_t>, dim3((unsigned)(B * L)), dim3(256), 0, s, (const int64_t*)labels, nodes, count, idx, onehot,
                           (int)N, (int)L, (int)p, (int)num_classes);
    UCF_LAUNCH_CHECK("ucfvit_octree_serialize_labels");
    return UCFVIT_OK;
}

// zero fill of a dense output in either layout: the whole block is B * S * C floats
static int zero_output(float* out, int64_t B, int64_t S, int64_t C, hipStream_t s, const char* who) {
    if (hipMemsetAsync(out, 0, (size_t)(B * S * C) * sizeof(float), s) != hipSuccess) {
        ucfvit_set_error("%s: hipMemsetAsync failed", who);
        return UCFVIT_ERR_HIP;
    }
    return UCFVIT_OK;
}

extern "C" int ucfvit_quadtree_deserialize(const float* seq, const int32_t* nodes, const int32_t* count, float* out, int64_t B, int64_t H, int64_t W,
                                           int64_t C, int64_t L, int64_t p, int64_t stride_b, int64_t stride_c, int64_t stride_s, int64_t stride_e,
                                           int64_t out_b, int64_t out_c, int64_t out_pixel, int mode, int trunc, void* stream) {
    UCF_CHECK_ARG(mode == UCFVIT_RESAMPLE_SMOOTH || mode == UCFVIT_RESAMPLE_NEAREST, "ucfvit_quadtree_deserialize: unknown mode %d", mode);
    UCF_CHECK_ARG(B >= 0 && H > 0 && W > 0 && H < 32768 && W < 32768, "ucfvit_quadtree_deserialize: image %lld x %lld out of range", (long long)H,
                  (long long)W);
    UCF_CHECK_ARG(C > 0 && C <= 255 && L > 0 && p > 0 && p <= 1024 && B * L < (1ll << 31), "ucfvit_quadtree_deserialize: bad shape (C=%lld, L=%lld, p=%lld)",
                  (long long)C, (long long)L, (long long)p);
    UCF_CHECK_ARG(stride_b >= 0 && stride_c > 0 && stride_s > 0 && stride_e > 0, "ucfvit_quadtree_deserialize: sequence strides must be positive");
    int c_fast = 0;
    UCF_CHECK_ARG(out_layout(H * W, C, out_b, out_c, out_pixel, &c_fast),
                  "ucfvit_quadtree_deserialize: output strides (%lld, %lld, %lld) are neither dense [B][C][H][W] nor dense [B][H][W][C]", (long long)out_b,
                  (long long)out_c, (long long)out_pixel);
    if (B == 0) return UCFVIT_OK;
    UCF_CHECK_ARG(seq && nodes && count && out, "ucfvit_quadtree_deserialize: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = zero_output(out, B, H * W, C, s, "ucfvit_quadtree_deserialize")) return rc;
    const dim3 grid((unsigned)(B * L), chunk_rows(B * L, H * W * C));
#define UCF_QD_LAUNCH(NEAR, TR)                                                                                                              \
    hipLaunchKernelGGL((quadtree_deserialize_kernel<NEAR, TR>), grid, dim3(DES_THREADS), 0, s, seq, nodes, count, out, (int)H, (int)W, (int)C, \
                       (int)L, (int)p, stride_b, stride_c, stride_s, stride_e, out_b, out_c, out_pixel, c_fast)
    if (mode == UCFVIT_RESAMPLE_NEAREST) UCF_QD_LAUNCH(true, false);
    else if (trunc) UCF_QD_LAUNCH(false, true);
    else UCF_QD_LAUNCH(false, false);
#undef UCF_QD_LAUNCH
    UCF_LAUNCH_CHECK("ucfvit_quadtree_deserialize");
    return UCFVIT_OK;
}

extern "C" int ucfvit_octree_deserialize(const float* seq, const int32_t* nodes, const int32_t* count, float* out, int64_t B, int64_t N, int64_t C,
                                         int64_t L, int64_t p, int64_t stride_b, int64_t stride_c, int64_t stride_s, int64_t stride_e, int64_t out_b,
                                         int64_t out_c, int64_t out_pixel, int mode, void* stream) {
    UCF_CHECK_ARG(mode == UCFVIT_RESAMPLE_SMOOTH || mode == UCFVIT_RESAMPLE_NEAREST, "ucfvit_octree_deserialize: unknown mode %d", mode);
    UCF_CHECK_ARG(B >= 0 && N > 0 && N <= 256, "ucfvit_octree_deserialize: cubic volumes of side 1..256 (got %lld)", (long long)N);
    UCF_CHECK_ARG(C > 0 && C <= 255 && L > 0 && p > 0 && p <= 256 && B * L < (1ll << 31), "ucfvit_octree_deserialize: bad shape (C=%lld, L=%lld, p=%lld)",
                  (long long)C, (long long)L, (long long)p);
    UCF_CHECK_ARG(stride_b >= 0 && stride_c > 0 && stride_s > 0 && stride_e > 0, "ucfvit_octree_deserialize: sequence strides must be positive");
    int c_fast = 0;
    UCF_CHECK_ARG(out_layout(N * N * N, C, out_b, out_c, out_pixel, &c_fast),
                  "ucfvit_octree_deserialize: output strides (%lld, %lld, %lld) are neither dense [B][C][N][N][N] nor dense [B][N][N][N][C]",
                  (long long)out_b, (long long)out_c, (long long)out_pixel);
    if (B == 0) return UCFVIT_OK;
    UCF_CHECK_ARG(seq && nodes && count && out, "ucfvit_octree_deserialize: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = zero_output(out, B, N * N * N, C, s, "ucfvit_octree_deserialize")) return rc;
    const dim3 grid((unsigned)(B * L), chunk_rows(B * L, N * N * N * C));
    if (mode == UCFVIT_RESAMPLE_NEAREST)
        hipLaunchKernelGGL(octree_deserialize_kernel<true>, grid, dim3(DES_THREADS), 0, s, seq, nodes, count, out, (int)N, (int)C, (int)L, (int)p,
                           stride_b, stride_c, stride_s, stride_e, out_b, out_c, out_pixel, c_fast);
    else
        hipLaunchKernelGGL(octree_deserialize_kernel<false>, grid, dim3(DES_THREADS), 0, s, seq, nodes, count, out, (int)N, (int)C, (int)L, (int)p,
                           stride_b, stride_c, stride_s, stride_e, out_b, out_c, out_pixel, c_fast);
    UCF_LAUNCH_CHECK("ucfvit_octree_deserialize");
    return UCFVIT_OK;
}
