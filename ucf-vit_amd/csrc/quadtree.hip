// GPU-side fixed-length quadtree patcher for gfx950: the adaptive-patching data transform of the reference
// (src/UCF_VIT/dataloaders/quadtree.py:84-174 FixedQuadTree, dataloaders/transform.py:9-55 Patchify) for a whole batch on the device.
//   quadtree_build     : per image, the reference's greedy refinement — repeatedly replace the FIRST node of maximum edge count by
//                        its four quadrants (order lt, rt, lb, rb, in place) until fixed_length nodes exist or that node is 2 pixels
//                        wide.  Integer logic, bit-exact; region sums come from a summed-area table (one pass per image).
//   quadtree_serialize : every node's region resampled to p x p with the cv2.INTER_CUBIC / torch bicubic kernel (A = -0.75, pixel
//                        centres aligned, replicated border), written in the reference's [S][p][p][C] order.
// One workgroup per image (build) / per node (serialize); the greedy loop is sequential by definition, the batch supplies the
// parallelism (166 images = 166 workgroups).  Edge detection (cv2.Canny) is not part of this file: the edge map is an input.
// The tree logic (integers) is patcher_tree.h's, once for both dimensions.  The serializers' sampling loops stay written out per kernel: this
// unit is built with -ffp-contract=fast, and moving such a loop into a helper changed which product is fused into which sum.
#include "common.h"
#include "patcher_tree.h"            // Node, tree_refine, tree_write
#include "resample_rules.h"          // cubic_coeffs

namespace {

__device__ __forceinline__ unsigned sat_sum(const unsigned* __restrict__ sat, int W1, int x1, int x2, int y1, int y2) {
    return sat[y2 * W1 + x2] - sat[y1 * W1 + x2] - sat[y2 * W1 + x1] + sat[y1 * W1 + x1];
}

__global__ __launch_bounds__(256) void quadtree_build_kernel(const unsigned char* __restrict__ edges, int* __restrict__ nodes_out,
                                                             int* __restrict__ values_out, int* __restrict__ count_out,
                                                             float* __restrict__ seq_ps, unsigned* __restrict__ sat_all, int H, int W, int L) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int W1 = W + 1;
    const unsigned char* e = edges + (int64_t)b * H * W;
    unsigned* sat = sat_all + (int64_t)b * (H + 1) * W1;

    // ---- summed-area table: sat[y][x] = sum of e[0..y)[0..x)  (row prefix sums, then column prefix sums)
    for (int x = tid; x < W1; x += blockDim.x) sat[x] = 0;
    for (int y = tid; y < H; y += blockDim.x) {
        unsigned run = 0;
        unsigned* row = sat + (int64_t)(y + 1) * W1;
        row[0] = 0;
        for (int x = 0; x < W; ++x) {
            run += e[(int64_t)y * W + x];
            row[x + 1] = run;
        }
    }
    __syncthreads();
    for (int x = tid; x < W1; x += blockDim.x) {
        unsigned run = 0;
        for (int y = 1; y <= H; ++y) {
            run += sat[(int64_t)y * W1 + x];
            sat[(int64_t)y * W1 + x] = run;
        }
    }
    __syncthreads();

    Node<2>* cur = reinterpret_cast<Node<2>*>(smem_raw);
    const int n = tree_refine<2>(cur, cur + (L + 4), L, Node<2>{{0, (short)W, 0, (short)H}, 0},
                                 [&](const Node<2>& k) { return (int)(sat_sum(sat, W1, k.c[0], k.c[1], k.c[2], k.c[3]) / 255u); });
    tree_write<2>(cur, n, L, b, nodes_out, values_out, count_out, seq_ps);
}

__global__ __launch_bounds__(256) void quadtree_serialize_kernel(const float* __restrict__ img, const int* __restrict__ nodes,
                                                                 const int* __restrict__ count, float* __restrict__ seq, int H, int W, int C,
                                                                 int L, int p) {
    const int64_t bs = blockIdx.x;
    const int b = (int)(bs / L), s = (int)(bs - (int64_t)b * L);
    const int n_out = p * p * C;
    float* out = seq + bs * n_out;
    const int* q = nodes + bs * 4;
    const int x1 = q[0], x2 = q[1], y1 = q[2], y2 = q[3];
    const int w = x2 - x1, h = y2 - y1;
    if (s >= count[b] || w <= 0 || h <= 0) {
        for (int i = threadIdx.x; i < n_out; i += blockDim.x) out[i] = 0.f;
        return;
    }
    const float sx = (float)w / (float)p, sy = (float)h / (float)p;
    const float* src = img + (int64_t)b * H * W * C;
    for (int i = threadIdx.x; i < n_out; i += blockDim.x) {
        const int c = i % C;
        const int px = (i / C) % p, py = i / (C * p);
        const float fy = ((float)py + 0.5f) * sy - 0.5f, fx = ((float)px + 0.5f) * sx - 0.5f;
        const float fyf = floorf(fy), fxf = floorf(fx);
        const int iy = (int)fyf, ix = (int)fxf;
        float wy[4], wx[4];
        cubic_coeffs(fy - fyf, wy);
        cubic_coeffs(fx - fxf, wx);
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            int yy = iy - 1 + a;
            yy = yy < 0 ? 0 : (yy > h - 1 ? h - 1 : yy);
            const float* rowp = src + ((int64_t)(y1 + yy) * W + x1) * C + c;
            float r = 0.f;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                int xx = ix - 1 + d;
                xx = xx < 0 ? 0 : (xx > w - 1 ? w - 1 : xx);
                r += wx[d] * rowp[(int64_t)xx * C];
            }
            acc += wy[a] * r;
        }
        out[i] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Octree (3-D volumes): dataloaders/octree.py:66-151 FixedOctTree.  domain[z][y][x] uint8, cubic; value = sum / norm_factor;
// children n1..n8 = x fastest, then y, then z (:83-103); stop when the first maximum node is 2 wide in x; 7 nodes added per step.
// ---------------------------------------------------------------------------------------------------------------------
// summed-volume table sat[z][y][x] = sum of dom[0..z)[0..y)[0..x), (N+1)^3 entries per volume, zero-initialised by the caller
__global__ void sat3_x_kernel(const unsigned char* __restrict__ dom, unsigned* __restrict__ sat, int B, int N) {
    const int64_t line = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // (b, z, y)
    if (line >= (int64_t)B * N * N) return;
    const int y = (int)(line % N), z = (int)((line / N) % N);
    const int64_t b = line / ((int64_t)N * N);
    const int N1 = N + 1;
    const unsigned char* src = dom + ((b * N + z) * N + y) * (int64_t)N;
    unsigned* dst = sat + ((b * N1 + z + 1) * N1 + y + 1) * (int64_t)N1;
    unsigned run = 0;
    for (int x = 0; x < N; ++x) {
        run += src[x];
        dst[x + 1] = run;
    }
}
__global__ void sat3_y_kernel(unsigned* __restrict__ sat, int B, int N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;        // (b, z, x')
    if (i >= (int64_t)B * N * N) return;
    const int x = (int)(i % N) + 1, z = (int)((i / N) % N) + 1;
    const int64_t b = i / ((int64_t)N * N);
    const int N1 = N + 1;
    unsigned* base = sat + ((b * N1 + z) * N1) * (int64_t)N1 + x;
    unsigned run = 0;
    for (int y = 1; y <= N; ++y) {
        run += base[(int64_t)y * N1];
        base[(int64_t)y * N1] = run;
    }
}
__global__ void sat3_z_kernel(unsigned* __restrict__ sat, int B, int N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;        // (b, y', x')
    if (i >= (int64_t)B * N * N) return;
    const int x = (int)(i % N) + 1, y = (int)((i / N) % N) + 1;
    const int64_t b = i / ((int64_t)N * N);
    const int N1 = N + 1;
    unsigned* base = sat + (b * N1 * N1 + y) * (int64_t)N1 + x;
    unsigned run = 0;
    for (int z = 1; z <= N; ++z) {
        run += base[(int64_t)z * N1 * N1];
        base[(int64_t)z * N1 * N1] = run;
    }
}

__device__ __forceinline__ unsigned sat3_sum(const unsigned* __restrict__ sat, int N1, int x1, int x2, int y1, int y2, int z1, int z2) {
    auto at = [&](int z, int y, int x) { return sat[((int64_t)z * N1 + y) * N1 + x]; };
    return at(z2, y2, x2) - at(z1, y2, x2) - at(z2, y1, x2) - at(z2, y2, x1) + at(z1, y1, x2) + at(z1, y2, x1) + at(z2, y1, x1) - at(z1, y1, x1);
}

__global__ __launch_bounds__(256) void octree_build_kernel(int* __restrict__ nodes_out, int* __restrict__ values_out, int* __restrict__ count_out,
                                                           float* __restrict__ seq_ps, const unsigned* __restrict__ sat_all, int N, int L,
                                                           unsigned norm) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int b = blockIdx.x;
    const int N1 = N + 1;
    const unsigned* sat = sat_all + (int64_t)b * N1 * N1 * N1;
    Node<3>* cur = reinterpret_cast<Node<3>*>(smem_raw);
    const int n = tree_refine<3>(cur, cur + (L + 8), L, Node<3>{{0, (short)N, 0, (short)N, 0, (short)N}, 0},
                                 [&](const Node<3>& k) { return (int)(sat3_sum(sat, N1, k.c[0], k.c[1], k.c[2], k.c[3], k.c[4], k.c[5]) / norm); });
    tree_write<3>(cur, n, L, b, nodes_out, values_out, count_out, seq_ps);
}

// leaf img[z1:z2, y1:y2, x1:x2, :] -> p^3 by linear interpolation with aligned corners (octree.py:120-141), out [S][p][p][p][C]
__global__ __launch_bounds__(256) void octree_serialize_kernel(const float* __restrict__ img, const int* __restrict__ nodes,
                                                               const int* __restrict__ count, float* __restrict__ seq, int N, int C, int L, int p) {
    const int64_t bs = blockIdx.x;
    const int b = (int)(bs / L), s = (int)(bs - (int64_t)b * L);
    const int n_out = p * p * p * C;
    float* out = seq + bs * n_out;
    const int* q = nodes + bs * 6;
    const int x1 = q[0], y1 = q[2], z1 = q[4];
    const int nx = q[1] - x1, ny = q[3] - y1, nz = q[5] - z1;
    if (s >= count[b] || nx <= 0 || ny <= 0 || nz <= 0) {
        for (int i = threadIdx.x; i < n_out; i += blockDim.x) out[i] = 0.f;
        return;
    }
    const float inv = p > 1 ? 1.f / (float)(p - 1) : 0.f;
    const float* src = img + (int64_t)b * N * N * N * C;
    for (int i = threadIdx.x; i < n_out; i += blockDim.x) {
        const int c = i % C;
        int r = i / C;
        const int k = r % p;
        r /= p;
        const int j = r % p, ii = r / p;
        // axis 0 of the leaf is z, axis 1 is y, axis 2 is x
        const float fz = (float)ii * (float)(nz - 1) * inv, fy = (float)j * (float)(ny - 1) * inv, fx = (float)k * (float)(nx - 1) * inv;
        int z0 = (int)fz, y0 = (int)fy, x0 = (int)fx;
        z0 = z0 > nz - 1 ? nz - 1 : z0;
        y0 = y0 > ny - 1 ? ny - 1 : y0;
        x0 = x0 > nx - 1 ? nx - 1 : x0;
        const float tz = fz - (float)z0, ty = fy - (float)y0, tx = fx - (float)x0;
        const int z1i = z0 + 1 < nz ? z0 + 1 : nz - 1, y1i = y0 + 1 < ny ? y0 + 1 : ny - 1, x1i = x0 + 1 < nx ? x0 + 1 : nx - 1;
        auto at = [&](int z, int y, int x) { return src[((((int64_t)(z1 + z) * N + (y1 + y)) * N) + (x1 + x)) * C + c]; };
        const float c00 = at(z0, y0, x0) * (1.f - tx) + at(z0, y0, x1i) * tx;
        const float c01 = at(z0, y1i, x0) * (1.f - tx) + at(z0, y1i, x1i) * tx;
        const float c10 = at(z1i, y0, x0) * (1.f - tx) + at(z1i, y0, x1i) * tx;
        const float c11 = at(z1i, y1i, x0) * (1.f - tx) + at(z1i, y1i, x1i) * tx;
        const float c0 = c00 * (1.f - ty) + c01 * ty, c1 = c10 * (1.f - ty) + c11 * ty;
        out[i] = c0 * (1.f - tz) + c1 * tz;
    }
}

// One launch of a builder, one workgroup per image: the length rule of a 2^ND-ary tree and the two LDS node lists of L + 2^ND nodes (150 KiB at
// most; above 64 KiB the kernel has to opt in); `before` queues what the builder reads, once every check has passed.
template <int ND, typename Before, typename... P, typename... A>
int launch_build(const char* who, void (*kern)(P...), int64_t B, int64_t L, hipStream_t s, Before before, A... args) {
    constexpr int K = 1 << ND;
    UCF_CHECK_ARG(L >= 1 && L % (K - 1) == 1, "%s: fixed_length=%lld must be %dn+1 (every refinement adds %s nodes)", who, (long long)L, K - 1,
                  ND == 2 ? "three" : "seven");
    const size_t smem = 2 * (size_t)(L + K) * sizeof(Node<ND>);
    UCF_CHECK_ARG(smem <= 150 * 1024, "%s: fixed_length=%lld does not fit the LDS node lists", who, (long long)L);
    if (smem > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) {
            ucfvit_set_error("%s: cannot raise dynamic LDS to %zu bytes: %s", who, smem, hipGetErrorString(e));
            return UCFVIT_ERR_HIP;
        }
    }
    if (int rc = before()) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(256), smem, s, args...);
    UCF_LAUNCH_CHECK(who);
    return UCFVIT_OK;
}

}  // namespace

extern "C" int64_t ucfvit_octree_workspace(int64_t B, int64_t N) {
    if (B <= 0 || N <= 0) return 0;
    return B * (N + 1) * (N + 1) * (N + 1) * (int64_t)sizeof(unsigned);
}

extern "C" int ucfvit_octree_build(const uint8_t* domain, int32_t* nodes, int32_t* values, int32_t* count, float* seq_ps, int64_t B, int64_t N,
                                   int64_t L, int norm_factor, void* workspace, void* stream) {
    if (B == 0) return UCFVIT_OK;
    UCF_CHECK_ARG(domain && nodes && values && count && seq_ps && workspace, "ucfvit_octree_build: null pointer");
    UCF_CHECK_ARG(N > 0 && N <= 256, "ucfvit_octree_build: cubic volumes of side 1..256 (got %lld)", (long long)N);
    UCF_CHECK_ARG(norm_factor >= 1 && norm_factor <= 255, "ucfvit_octree_build: norm_factor=%d out of range", norm_factor);
    // node values are int32 (kernel and `values` output): a dense volume's root value N^3 * 255 / norm_factor must stay below 2^31, or the
    // maximum search (which starts at -1) finds no node and indexes the node list out of bounds
    UCF_CHECK_ARG(N * N * N * 255 / norm_factor < (1ll << 31),
                  "ucfvit_octree_build: N=%lld with norm_factor=%d: node values up to N^3 * 255 / norm_factor do not fit int32", (long long)N,
                  norm_factor);
    hipStream_t s = (hipStream_t)stream;
    // the summed-volume table: three passes over the zeroed workspace
    auto table = [&]() -> int {
        if (hipMemsetAsync(workspace, 0, (size_t)ucfvit_octree_workspace(B, N), s) != hipSuccess) {
            ucfvit_set_error("ucfvit_octree_build: hipMemsetAsync failed");
            return UCFVIT_ERR_HIP;
        }
        const int64_t lines = B * N * N;
        const unsigned g = (unsigned)((lines + 255) / 256);
        hipLaunchKernelGGL(sat3_x_kernel, dim3(g), dim3(256), 0, s, domain, (unsigned*)workspace, (int)B, (int)N);
        hipLaunchKernelGGL(sat3_y_kernel, dim3(g), dim3(256), 0, s, (unsigned*)workspace, (int)B, (int)N);
        hipLaunchKernelGGL(sat3_z_kernel, dim3(g), dim3(256), 0, s, (unsigned*)workspace, (int)B, (int)N);
        UCF_LAUNCH_CHECK("ucfvit_octree_build(sat)");
        return UCFVIT_OK;
    };
    return launch_build<3>("ucfvit_octree_build", octree_build_kernel, B, L, s, table, nodes, values, count, seq_ps, (const unsigned*)workspace, (int)N,
                           (int)L, (unsigned)norm_factor);
}

extern "C" int ucfvit_octree_serialize(const float* img, const int32_t* nodes, const int32_t* count, float* seq, int64_t B, int64_t N, int64_t C,
                                       int64_t L, int64_t p, void* stream) {
    if (B == 0) return UCFVIT_OK;
    UCF_CHECK_ARG(img && nodes && count && seq, "ucfvit_octree_serialize: null pointer");
    UCF_CHECK_ARG(N > 0 && C > 0 && L > 0 && p > 0 && B * L < (1ll << 31), "ucfvit_octree_serialize: bad shape");
    hipLaunchKernelGGL(octree_serialize_kernel, dim3((unsigned)(B * L)), dim3(256), 0, (hipStream_t)stream, img, nodes, count, seq, (int)N, (int)C,
                       (int)L, (int)p);
    UCF_LAUNCH_CHECK("ucfvit_octree_serialize");
    return UCFVIT_OK;
}

extern "C" int64_t ucfvit_quadtree_workspace(int64_t B, int64_t H, int64_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return B * (H + 1) * (W + 1) * (int64_t)sizeof(unsigned);
}

extern "C" int ucfvit_quadtree_build(const uint8_t* edges, int32_t* nodes, int32_t* values, int32_t* count, float* seq_ps, int64_t B,
                                     int64_t H, int64_t W, int64_t L, void* workspace, void* stream) {
    if (B == 0) return UCFVIT_OK;
    UCF_CHECK_ARG(edges && nodes && values && count && seq_ps && workspace, "ucfvit_quadtree_build: null pointer");
    UCF_CHECK_ARG(H > 0 && W > 0 && H < 32768 && W < 32768 && H * W * 255 < (1ll << 32), "ucfvit_quadtree_build: image %lld x %lld out of range",
                  (long long)H, (long long)W);
    return launch_build<2>("ucfvit_quadtree_build", quadtree_build_kernel, B, L, (hipStream_t)stream, [] { return (int)UCFVIT_OK; }, edges, nodes, values,
                           count, seq_ps, (unsigned*)workspace, (int)H, (int)W, (int)L);
}

extern "C" int ucfvit_quadtree_serialize(const float* img, const int32_t* nodes, const int32_t* count, float* seq, int64_t B, int64_t H, int64_t W,
                                         int64_t C, int64_t L, int64_t p, void* stream) {
    if (B == 0) return UCFVIT_OK;
    UCF_CHECK_ARG(img && nodes && count && seq, "ucfvit_quadtree_serialize: null pointer");
    UCF_CHECK_ARG(H > 0 && W > 0 && C > 0 && L > 0 && p > 0 && B * L < (1ll << 31), "ucfvit_quadtree_serialize: bad shape");
    hipLaunchKernelGGL(quadtree_serialize_kernel, dim3((unsigned)(B * L)), dim3(256), 0, (hipStream_t)stream, img, nodes, count, seq, (int)H,
                       (int)W, (int)C, (int)L, (int)p);
    UCF_LAUNCH_CHECK("ucfvit_quadtree_serialize");
    return UCFVIT_OK;
}
