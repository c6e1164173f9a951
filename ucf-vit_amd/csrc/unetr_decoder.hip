// HBM-bound kernels of the UNETR convolutional decoder for gfx950: the normalisation / activation / residual chain of
// the residual conv blocks and the Dice + cross-entropy loss, each as ONE read of its inputs per pass instead of torch's chain of
// element-wise kernels.  Two families: the channels-last kernels (incl_*) that sit between the HIP convolution kernels of csrc/conv3d.hip —
// the product path of the 3-D skip-connection decoder — and the N C (D) H W row kernels (a (batch, channel) pair is one contiguous row of
// S voxels) for models whose convolutions the caller opted to run on torch (UNETR(allow_torch_decoder=True): 2-D, other channel counts).
//
//   reference call sites: src/UCF_VIT/simple/arch.py:808-940 (monai UnetrBasicBlock / UnetrPrUpBlock / UnetrUpBlock: UnetResBlock =
//   conv -> instance norm -> LeakyReLU(0.01) -> conv -> instance norm, + (1x1 conv -> instance norm | identity), LeakyReLU),
//   training_scripts/train_unetr_simple.py:38 (monai DiceCELoss(to_onehot_y, softmax, squared_pred)).  monai is absent from the build
//   container: PARITY UNPINNED against it; the oracle is the plain-torch restatement of these published formulas (tests/test_unetr_decoder.py).
//
// At 512 x 512 x 128 one 16-channel activation is 2.1 GB in fp32: norm + LeakyReLU + add + LeakyReLU as separate torch kernels move
// ~20 such tensors per residual block and direction; here: statistics 1 read, apply 1-2 reads + 1 write, backward 3-4 reads + 1-2 writes.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = 16384;       // elements of a row per workgroup in the reduction passes (64 per thread)

__device__ __forceinline__ float block_sum(float v, float* red) {       // red: NT / 64 floats of LDS
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) t += red[w];
    return t;
}

template <typename T> __device__ __forceinline__ float ld(const T* p, int64_t i) { return to_f32<T>(p[i]); }

// ---- instance-norm statistics: per row mean and 1 / sqrt(var + eps) (biased variance, like nn.InstanceNorm) ---------------------------
// pass 1: per chunk the COUNT, MEAN and M2 = sum (x - mean)^2 of its elements, accumulated relative to a per-chunk shift (the chunk's
// first element).  A shift that is far from the rest of the row (one outlier at the start) spoils the fp32 sums of that chunk only; pass 2
// combines the chunks with the parallel-variance formula in double, so a row whose |mean| is far larger than its spread keeps its variance.
template <typename T>
__global__ __launch_bounds__(NT) void in_stats_partial(const T* __restrict__ x, float* __restrict__ part, int64_t S, int chunks) {
    __shared__ float red[NT / 64];
    const int64_t row = blockIdx.y;
    const T* xr = x + row * S;
    const int64_t lo = (int64_t)blockIdx.x * CHUNK, hi = min(S, lo + CHUNK);
    const float shift = ld(xr, lo);
    float s1 = 0.f, s2 = 0.f;
    for (int64_t i = lo + threadIdx.x; i < hi; i += NT) {
        const float v = ld(xr, i) - shift;
        s1 += v;
        s2 += v * v;
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (threadIdx.x == 0) {
        const float n = (float)(hi - lo);
        float* p = part + (row * chunks + blockIdx.x) * 3;
        p[0] = n;
        p[1] = shift + s1 / n;
        p[2] = fmaxf(s2 - s1 * (s1 / n), 0.f);
    }
}

// parallel-variance combination of (count, mean, M2) triples in double: n = na + nb, d = mb - ma, m = ma + d nb / n,
// M2 = M2a + M2b + d^2 na nb / n.  Triples with count 0 drop out.
struct Mom {
    double n, m, m2;
};
__device__ __forceinline__ void mom_add(Mom& a, double nb, double mb, double m2b) {
    if (nb <= 0.0) return;
    const double n = a.n + nb, d = mb - a.m;
    a.m += d * (nb / n);
    a.m2 += m2b + d * d * (a.n * nb / n);
    a.n = n;
}
// one wave: lane l has combined its share of the triples in `a`; butterfly so that every lane ends with the same combination order
__device__ __forceinline__ Mom mom_wave_fold(Mom a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double nb = __shfl_xor(a.n, o, 64), mb = __shfl_xor(a.m, o, 64), m2b = __shfl_xor(a.m2, o, 64);
        const bool lower = (threadIdx.x & o) == 0;              // combine (lower, upper) in that order on both sides
        Mom lo = lower ? a : Mom{nb, mb, m2b};
        if (lower) mom_add(lo, nb, mb, m2b); else mom_add(lo, a.n, a.m, a.m2);
        a = lo;
    }
    return a;
}
// mean and 1 / sqrt(var + eps) of a folded triple (biased variance M2 / n; nothing counted: variance 0)
__device__ __forceinline__ void mom_finish(const Mom& a, float eps, float& mean, float& rstd) {
    const double var = a.n > 0.0 ? fmax(a.m2 / a.n, 0.0) : 0.0;
    mean = (float)a.m;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// pass 2: one wave per row folds the chunk triples in a fixed order (2048 chunks of 16384 at the full volume)
__global__ __launch_bounds__(64) void in_stats_final(const float* __restrict__ part, float* __restrict__ mean, float* __restrict__ rstd, int chunks,
                                                     float eps) {
    const int64_t row = blockIdx.x;
    Mom a = {0.0, 0.0, 0.0};
    for (int c = threadIdx.x; c < chunks; c += 64) {
        const float* p = part + (row * chunks + c) * 3;
        mom_add(a, (double)p[0], (double)p[1], (double)p[2]);
    }
    a = mom_wave_fold(a);
    if (threadIdx.x == 0) mom_finish(a, eps, mean[row], rstd[row]);
}

// ---- apply: y = lrelu((x - mean) rstd [+ res], slope)   (slope 1: no activation) ------------------------------------------------------
template <typename T, bool RES>
__global__ __launch_bounds__(NT) void in_apply(const T* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                               const T* __restrict__ res, T* __restrict__ y, int64_t S, float slope) {
    const int64_t row = blockIdx.y;
    const float m = mean[row], r = rstd[row];
    const int64_t base = row * S;
    constexpr int V = 16 / sizeof(T);
    const int64_t nv = S / V;                                       // S % V == 0 and 16-byte aligned rows are checked by the entry point
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < nv; i += (int64_t)gridDim.x * NT) {
        const Vec16<T> xv = *reinterpret_cast<const Vec16<T>*>(x + base + i * V);
        Vec16<T> rv, o;
        if (RES) rv = *reinterpret_cast<const Vec16<T>*>(res + base + i * V);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float v = (xv.get(e) - m) * r;
            if (RES) v += rv.get(e);
            o.set(e, v >= 0.f ? v : v * slope);
        }
        *reinterpret_cast<Vec16<T>*>(y + base + i * V) = o;
    }
}

// ---- backward of y = lrelu(n + res), n = (x - mean) rstd:  dn = dy * (y > 0 ? 1 : slope);  dres = dn;
//      dx = rstd (dn - mean(dn) - n mean(dn n))   (both means over the row) ------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NT) void in_bwd_partial(const T* __restrict__ dy, const T* __restrict__ y, const T* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ part,
                                                     int64_t S, int chunks, float slope) {
    __shared__ float red[NT / 64];
    const int64_t row = blockIdx.y;
    const float m = mean[row], r = rstd[row];
    const int64_t base = row * S;
    const int64_t lo = (int64_t)blockIdx.x * CHUNK, hi = min(S, lo + CHUNK);
    float s1 = 0.f, s2 = 0.f;
    for (int64_t i = lo + threadIdx.x; i < hi; i += NT) {
        const float g = ld(dy, base + i) * (ld(y, base + i) > 0.f ? 1.f : slope);
        s1 += g;
        s2 += g * (ld(x, base + i) - m) * r;
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (threadIdx.x == 0) {
        part[(row * chunks + blockIdx.x) * 2 + 0] = s1;
        part[(row * chunks + blockIdx.x) * 2 + 1] = s2;
    }
}
// the K means over the S voxels from the chunk sums [B][chunks][K][C] of a backward pass in either layout (the row layout is C = 1): one wave
// per (b, c) adds its chunks lane-strided in double, then the butterfly; table k goes to out.m[k][b C + c]
template <int K> struct Means {
    float* m[K];
};
template <int K>
__global__ __launch_bounds__(64) void bwd_means(const float* __restrict__ part, Means<K> out, int64_t S, int C, int chunks) {
    const int64_t b = blockIdx.x / C;
    const int c = blockIdx.x % C;
    double s[K] = {};
    for (int ch = threadIdx.x; ch < chunks; ch += 64)
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] += part[(b * chunks + ch) * K * C + k * C + c];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = wave_sum(s[k]);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) out.m[k][blockIdx.x] = (float)(s[k] / (double)S);
}
template <typename T, bool RES>
__global__ __launch_bounds__(NT) void in_bwd_apply(const T* __restrict__ dy, const T* __restrict__ y, const T* __restrict__ x,
                                                   const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ m1,
                                                   const float* __restrict__ m2, T* __restrict__ dx, T* __restrict__ dres, int64_t S,
                                                   float slope) {
    const int64_t row = blockIdx.y;
    const float m = mean[row], r = rstd[row], a1 = m1[row], a2 = m2[row];
    const int64_t base = row * S;
    constexpr int V = 16 / sizeof(T);
    const int64_t nv = S / V;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < nv; i += (int64_t)gridDim.x * NT) {
        const Vec16<T> gv = *reinterpret_cast<const Vec16<T>*>(dy + base + i * V);
        const Vec16<T> yv = *reinterpret_cast<const Vec16<T>*>(y + base + i * V);
        const Vec16<T> xv = *reinterpret_cast<const Vec16<T>*>(x + base + i * V);
        Vec16<T> ox, orr;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float dn = gv.get(e) * (yv.get(e) > 0.f ? 1.f : slope);
            const float n = (xv.get(e) - m) * r;
            ox.set(e, r * (dn - a1 - n * a2));
            if (RES) orr.set(e, dn);
        }
        *reinterpret_cast<Vec16<T>*>(dx + base + i * V) = ox;
        if (RES) *reinterpret_cast<Vec16<T>*>(dres + base + i * V) = orr;
    }
}

// ---- Dice + cross-entropy ------------------------------------------------------------------------------------------------------------
// logits [B][n][S] (n <= 8 classes), labels int64 [B][S].  p = softmax over the classes of a voxel.
//   dice_bc = 1 - (2 I_bc + s_nr) / (P_bc + C_bc + s_dr),  I = sum_v p onehot, P = sum_v p^2 (squared_pred), C = sum_v onehot
//   loss = mean_bc dice_bc + mean_bv (-log p[label])
constexpr int MAXC = 8;
constexpr int DSTAT = 3 * MAXC + 1;       // per batch element: I[8], P[8], C[8], CE sum

template <typename T>
__global__ __launch_bounds__(NT) void dice_partial(const T* __restrict__ logits, const int64_t* __restrict__ labels, float* __restrict__ part,
                                                   int n, int64_t S, int chunks, int64_t sb, int64_t sc, int64_t ss) {
    __shared__ float red[NT / 64];
    const int64_t b = blockIdx.y;
    const T* lb = logits + b * sb;
    const int64_t* yb = labels + b * S;
    const int64_t lo = (int64_t)blockIdx.x * CHUNK, hi = min(S, lo + CHUNK);
    float I[MAXC], P[MAXC], Cn[MAXC], ce = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) I[c] = P[c] = Cn[c] = 0.f;
    for (int64_t i = lo + threadIdx.x; i < hi; i += NT) {
        float z[MAXC], mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            z[c] = c < n ? ld(lb, c * sc + i * ss) : -INFINITY;
            mx = fmaxf(mx, z[c]);
        }
        float den = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            z[c] = c < n ? __expf(z[c] - mx) : 0.f;
            den += z[c];
        }
        const float inv = 1.f / den;
        const int lab = (int)yb[i];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const float p = z[c] * inv;
            const float oh = c == lab ? 1.f : 0.f;
            I[c] += p * oh;
            P[c] += p * p;
            Cn[c] += oh;
            ce -= oh * __logf(fmaxf(p, 1e-38f));
        }
    }
    float* out = part + (b * chunks + blockIdx.x) * DSTAT;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const float a = block_sum(I[c], red), q = block_sum(P[c], red), k = block_sum(Cn[c], red);
        if (threadIdx.x == 0) {
            out[c] = a;
            out[MAXC + c] = q;
            out[2 * MAXC + c] = k;
        }
    }
    ce = block_sum(ce, red);
    if (threadIdx.x == 0) out[3 * MAXC] = ce;
}
// one workgroup: fold the chunk sums per batch element (fixed order, double), write stats [B][DSTAT] and the loss
__global__ __launch_bounds__(64) void dice_final(const float* __restrict__ part, float* __restrict__ stats, float* __restrict__ loss, int B, int n,
                                                 int64_t S, int chunks, float s_nr, float s_dr) {
    double total_dice = 0.0, total_ce = 0.0;
    for (int b = 0; b < B; ++b) {
        for (int k = 0; k < DSTAT; ++k) {
            double s = 0.0;
            for (int c = threadIdx.x; c < chunks; c += 64) s += part[((int64_t)b * chunks + c) * DSTAT + k];
            s = wave_sum(s);
            if (threadIdx.x == 0) stats[b * DSTAT + k] = (float)s;
            if (k == 3 * MAXC) total_ce += s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int c = 0; c < n; ++c) {
                const double I = stats[b * DSTAT + c], P = stats[b * DSTAT + MAXC + c], C = stats[b * DSTAT + 2 * MAXC + c];
                total_dice += 1.0 - (2.0 * I + s_nr) / (P + C + s_dr);
            }
        }
    }
    if (threadIdx.x == 0) loss[0] = (float)(total_dice / ((double)B * n) + total_ce / ((double)B * (double)S));
}
// d loss / d logits:  g_c = d(dice term)/dp_c = [ -2 onehot_c / D_c + 2 p_c (2 I_c + s_nr) / D_c^2 ] / (B n),  D_c = P_c + C_c + s_dr;
//                     dz_c = p_c (g_c - sum_k g_k p_k) + (p_c - onehot_c) / (B S)
template <typename T>
__global__ __launch_bounds__(NT) void dice_bwd(const T* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ stats,
                                               T* __restrict__ dlogits, int B, int n, int64_t S, float s_nr, float s_dr, float gscale,
                                               int64_t sb, int64_t sc, int64_t ss, int64_t S_total) {
    const int64_t b = blockIdx.y;
    const T* lb = logits + b * sb;
    T* db = dlogits + b * sb;
    const int64_t* yb = labels + b * S;
    float a[MAXC], bq[MAXC];                   // g_c = a_c onehot_c + bq_c p_c
    const float wb = 1.f / ((float)B * (float)n), wce = 1.f / ((float)B * (float)S_total);      // S_total: voxels of the WHOLE volume (= S unless sharded)
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const float I = stats[b * DSTAT + c], D = stats[b * DSTAT + MAXC + c] + stats[b * DSTAT + 2 * MAXC + c] + s_dr;
        a[c] = c < n ? -2.f / D * wb : 0.f;
        bq[c] = c < n ? 2.f * (2.f * I + s_nr) / (D * D) * wb : 0.f;
    }
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < S; i += (int64_t)gridDim.x * NT) {
        float z[MAXC], mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            z[c] = c < n ? ld(lb, c * sc + i * ss) : -INFINITY;
            mx = fmaxf(mx, z[c]);
        }
        float den = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            z[c] = c < n ? __expf(z[c] - mx) : 0.f;
            den += z[c];
        }
        const float inv = 1.f / den;
        const int lab = (int)yb[i];
        float g[MAXC], dot = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            z[c] *= inv;
            g[c] = (c == lab ? a[c] : 0.f) + bq[c] * z[c];
            dot += g[c] * z[c];
        }
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < n) db[c * sc + i * ss] = from_f32<T>(gscale * (z[c] * (g[c] - dot) + (z[c] - (c == lab ? 1.f : 0.f)) * wce));
    }
}

// ---- channels-last instance norm: x [B][S][C] bf16 (the layout of csrc/conv3d.hip), C = 8 * (a power of two <= 32 ... 256) -----------------
// A thread always meets the same 8 channels (its 16-byte vector index mod C/8 is fixed because both the workgroup size and the chunk
// size are multiples of C/8), so the per-channel sums live in registers and are folded once per workgroup through LDS.
constexpr int CLV = 4096;          // 16-byte vectors per workgroup in the reduction passes

// this thread's 8 consecutive entries, from k0 on, of any number of fp32 tables [B][C]: ld_chan(b * C + cg * 8, Tab{mean, m}, Tab{rstd, r}, ...)
struct Tab {
    const float* t;
    float (&v)[8];
};
template <typename... T> __device__ __forceinline__ void ld_chan(int64_t k0, T... tab) {
#pragma unroll
    for (int e = 0; e < 8; ++e) ((tab.v[e] = tab.t[k0 + e]), ...);
}

// the workgroup fold of K per-thread sums of 8 channels each: cl_stage puts them into LDS (red: NT rows of 8 K + 1 floats), cl_channel_sums adds
// the sums k0 .. k0 + N - 1 of channel c over the NT / cv threads of its channel group in sequence, cl_fold writes all of them as [K][C].  The sums are K separate
// arrays handed over by reference: as one [K][8] array or an array of pointers the callers' loops compile to other registers and, under
// -ffp-contract=fast, to other multiply-add contractions, which changes result bits (profiles/norm_loss_refactor.md)
template <typename... A> __device__ __forceinline__ void cl_stage(float (*red)[8 * sizeof...(A) + 1], const A&... s) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        int k = 0;
        ((red[threadIdx.x][8 * k++ + e] = s[e]), ...);
    }
    __syncthreads();
}
template <int K, int N> __device__ __forceinline__ void cl_channel_sums(const float (*red)[8 * K + 1], int k0, int c, int cv, float (&a)[N]) {
    const int cg = c >> 3, e = c & 7;
#pragma unroll
    for (int j = 0; j < N; ++j) a[j] = 0.f;
    for (int t = cg; t < NT; t += cv)
#pragma unroll
        for (int j = 0; j < N; ++j) a[j] += red[t][(k0 + j) * 8 + e];
}
template <typename... A> __device__ __forceinline__ void cl_fold(float (*red)[8 * sizeof...(A) + 1], float* out, int C, int cv, const A&... s) {
    constexpr int K = sizeof...(A);
    cl_stage(red, s...);
    for (int o = threadIdx.x; o < K * C; o += NT) {
        float a[1];
        cl_channel_sums<K>(red, o / C, o % C, cv, a);
        out[o] = a[0];
    }
}

// per chunk and channel (count, mean, M2) relative to the chunk's first voxel -> rows [B][chunks][3][C] in the layout of the convolution
// epilogue's statistics (conv3d.hip: stats_row_write), folded by ucfvit_instnorm_cl_stats_fold
__global__ __launch_bounds__(NT) void incl_stats_partial(const bf16* __restrict__ x, float* __restrict__ part, int64_t S, int C, int chunks) {
    __shared__ float red[NT][17];
    const int64_t b = blockIdx.y;
    const int cv = C >> 3;
    const int64_t nvec = S * cv, vlo = (int64_t)blockIdx.x * CLV, vhi = min(nvec, vlo + CLV);
    const bf16x8* xb = reinterpret_cast<const bf16x8*>(x + b * S * C);
    const bf16x8 sh = xb[vlo + threadIdx.x % cv];                   // shift = the chunk's first voxel (vlo is a multiple of cv)
    float s1[8] = {}, s2[8] = {};
    for (int64_t i = vlo + threadIdx.x; i < vhi; i += NT) {
        const bf16x8 v = xb[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = (float)v[e] - (float)sh[e];
            s1[e] += d;
            s2[e] += d * d;
        }
    }
    cl_stage(red, s1, s2);
    const float n = (float)((vhi - vlo) / cv);                      // voxels of the chunk
    float* out = part + (b * chunks + blockIdx.x) * 3 * C;
    for (int c = threadIdx.x; c < C; c += NT) {
        float a[2];
        cl_channel_sums<2>(red, 0, c, cv, a);
        const float a1 = a[0], a2 = a[1];
        out[c] = n;
        out[C + c] = (float)x[(b * S + vlo / cv) * C + c] + a1 / n;
        out[2 * C + c] = fmaxf(a2 - a1 * (a1 / n), 0.f);
    }
}
// ---- fold of the convolution kernels' statistics epilogue: partial rows [B][rows][3][C] of (count, mean, M2) per channel (conv3d.hip:
// stats_row_write) combined in double (mom_add).  Rows that stored nothing carry count 0 and drop out.
// first stage when there are many partial rows (a full-resolution layer writes 32768 per batch element): workgroup (g, b) combines the rows
// [g rpg, (g + 1) rpg) -> [B][G][3][C]; a thread owns a channel, NT / C rows in flight, the threads of a channel are combined in a fixed order
__global__ __launch_bounds__(NT) void incl_stats_fold1(const float* __restrict__ part, float* __restrict__ out, int rows, int C, int rpg) {
    __shared__ double red[3][NT];
    const int64_t b = blockIdx.y;
    const int g = blockIdx.x, G = gridDim.x;
    const int lo = g * rpg, hi = min(rows, lo + rpg);
    const int w = min(C, NT);                                   // C <= 256, a power of two
    const int col = threadIdx.x % w, rl = threadIdx.x / w, rs = NT / w;
    Mom a = {0.0, 0.0, 0.0};
    for (int r = lo + rl; r < hi; r += rs) {
        const float* p = part + (b * rows + r) * 3 * C + col;
        mom_add(a, (double)p[0], (double)p[C], (double)p[2 * C]);
    }
    red[0][threadIdx.x] = a.n;
    red[1][threadIdx.x] = a.m;
    red[2][threadIdx.x] = a.m2;
    __syncthreads();
    if (threadIdx.x < w) {
        Mom t = {0.0, 0.0, 0.0};
        for (int k = 0; k < rs; ++k) mom_add(t, red[0][k * w + threadIdx.x], red[1][k * w + threadIdx.x], red[2][k * w + threadIdx.x]);
        float* o = out + (b * G + g) * 3 * C + threadIdx.x;
        o[0] = (float)t.n;
        o[C] = (float)t.m;
        o[2 * C] = (float)t.m2;
    }
}
// final stage: one wave per (b, channel) over the rows of [B][rows][3][C]
__global__ __launch_bounds__(64) void incl_stats_fold(const float* __restrict__ part, float* __restrict__ mean, float* __restrict__ rstd, int64_t S,
                                                      int C, int rows, float eps) {
    const int64_t b = blockIdx.x / C;
    const int c = blockIdx.x % C;
    Mom a = {0.0, 0.0, 0.0};
    for (int r = threadIdx.x; r < rows; r += 64) {
        const float* p = part + (b * rows + r) * 3 * C + c;
        mom_add(a, (double)p[0], (double)p[C], (double)p[2 * C]);
    }
    a = mom_wave_fold(a);
    if (threadIdx.x == 0) mom_finish(a, eps, mean[blockIdx.x], rstd[blockIdx.x]);       // a.n == S: every voxel of the batch element was stored once
}
template <bool RES>
__global__ __launch_bounds__(NT) void incl_apply(const bf16* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                 const bf16* __restrict__ res, bf16* __restrict__ y, int64_t S, int C, float slope) {
    const int64_t b = blockIdx.y;
    const int cv = C >> 3, cg = threadIdx.x % cv;
    float m[8], r[8];
    ld_chan(b * C + cg * 8, Tab{mean, m}, Tab{rstd, r});
    const int64_t nvec = S * cv;
    const bf16x8* xb = reinterpret_cast<const bf16x8*>(x + b * S * C);
    const bf16x8* rb = reinterpret_cast<const bf16x8*>(res + b * S * C);
    bf16x8* yb = reinterpret_cast<bf16x8*>(y + b * S * C);
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * NT) {
        const bf16x8 xv = xb[i];
        bf16x8 rv, o;
        if (RES) rv = rb[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = ((float)xv[e] - m[e]) * r[e];
            if (RES) v += (float)rv[e];
            o[e] = (bf16)(v >= 0.f ? v : v * slope);
        }
        yb[i] = o;
    }
}
// NEED_Y: the activation mask comes from the saved output only when a residual was added before the LeakyReLU; without one
// sign(y) = sign(x - mean) (rstd > 0), which saves the read of y in both backward passes.
template <bool NEED_Y>
__global__ __launch_bounds__(NT) void incl_bwd_partial(const bf16* __restrict__ dy, const bf16* __restrict__ y, const bf16* __restrict__ x,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ part,
                                                       int64_t S, int C, int chunks, float slope, int64_t ldg8) {
    __shared__ float red[NT][17];
    const int64_t b = blockIdx.y;
    const int cv = C >> 3, cg = threadIdx.x % cv, cvs = __builtin_ctz(cv);
    float m[8], r[8], s1[8] = {}, s2[8] = {};
    ld_chan(b * C + cg * 8, Tab{mean, m}, Tab{rstd, r});
    const int64_t nvec = S * cv, vlo = (int64_t)blockIdx.x * CLV, vhi = min(nvec, vlo + CLV);
    const bf16x8* gb = reinterpret_cast<const bf16x8*>(dy) + b * S * ldg8;       // dy rows may be ldg8 16-byte units apart (a channel slice)
    const bf16x8* yb = reinterpret_cast<const bf16x8*>(y + b * S * C);
    const bf16x8* xb = reinterpret_cast<const bf16x8*>(x + b * S * C);
    for (int64_t i = vlo + threadIdx.x; i < vhi; i += NT) {
        const bf16x8 gv = gb[(i >> cvs) * ldg8 + cg], xv = xb[i];
        bf16x8 yv;
        if (NEED_Y) yv = yb[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float n = ((float)xv[e] - m[e]) * r[e];
            const float g = (float)gv[e] * ((NEED_Y ? (float)yv[e] : n) > 0.f ? 1.f : slope);
            s1[e] += g;
            s2[e] += g * n;
        }
    }
    cl_fold(red, part + (b * chunks + blockIdx.x) * 2 * C, C, cv, s1, s2);
}
template <bool RES, bool WRES>
__global__ __launch_bounds__(NT) void incl_bwd_apply(const bf16* __restrict__ dy, const bf16* __restrict__ y, const bf16* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ m1,
                                                     const float* __restrict__ m2, bf16* __restrict__ dx, bf16* __restrict__ dres, int64_t S, int C,
                                                     float slope, int64_t ldg8) {
    const int64_t b = blockIdx.y;
    const int cv = C >> 3, cg = threadIdx.x % cv, cvs = __builtin_ctz(cv);
    float m[8], r[8], a1[8], a2[8];
    ld_chan(b * C + cg * 8, Tab{mean, m}, Tab{rstd, r}, Tab{m1, a1}, Tab{m2, a2});
    const int64_t nvec = S * cv;
    const bf16x8* gb = reinterpret_cast<const bf16x8*>(dy) + b * S * ldg8;
    const bf16x8* yb = reinterpret_cast<const bf16x8*>(y + b * S * C);
    const bf16x8* xb = reinterpret_cast<const bf16x8*>(x + b * S * C);
    bf16x8* dxb = reinterpret_cast<bf16x8*>(dx + b * S * C);
    bf16x8* drb = reinterpret_cast<bf16x8*>(dres + b * S * C);
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * NT) {
        const bf16x8 gv = gb[(i >> cvs) * ldg8 + cg], xv = xb[i];
        bf16x8 yv, ox, orr;
        if (RES) yv = yb[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float n = ((float)xv[e] - m[e]) * r[e];
            const float dn = (float)gv[e] * ((RES ? (float)yv[e] : n) > 0.f ? 1.f : slope);
            ox[e] = (bf16)(r[e] * (dn - a1[e] - n * a2[e]));
            if (WRES) orr[e] = (bf16)dn;
        }
        dxb[i] = ox;
        if (WRES) drb[i] = orr;
    }
}
// ---- residual block tail with a NORMALISED residual branch: out = lrelu(norm(x) + norm(x2)) (monai UnetResBlock with the 1x1x1 projection:
// x = conv2 output, x2 = conv3 output).  Against norm(x2) as its own apply pass + a residual read: the normalised branch is never written or
// re-read (2 tensor passes less forward), and the backward needs ONE pair of passes for both normalisations (3 passes less): the activation
// mask and dn are shared, only the projections differ:  dx = r (dn - mean(dn) - n mean(dn n)),  dx2 = r2 (dn - mean(dn) - n2 mean(dn n2)).
__global__ __launch_bounds__(NT) void incl_apply2(const bf16* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                  const bf16* __restrict__ x2, const float* __restrict__ mean2, const float* __restrict__ rstd2,
                                                  bf16* __restrict__ y, int64_t S, int C, float slope) {
    const int64_t b = blockIdx.y;
    const int cv = C >> 3, cg = threadIdx.x % cv;
    float m[8], r[8], m2[8], r2[8];
    ld_chan(b * C + cg * 8, Tab{mean, m}, Tab{rstd, r}, Tab{mean2, m2}, Tab{rstd2, r2});
    const int64_t nvec = S * cv;
    const bf16x8* xb = reinterpret_cast<const bf16x8*>(x + b * S * C);
    const bf16x8* x2b = reinterpret_cast<const bf16x8*>(x2 + b * S * C);
    bf16x8* yb = reinterpret_cast<bf16x8*>(y + b * S * C);
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * NT) {
        const bf16x8 xv = xb[i], zv = x2b[i];
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = ((float)xv[e] - m[e]) * r[e] + ((float)zv[e] - m2[e]) * r2[e];       // the branch value is never rounded to bf16
            o[e] = (bf16)(v >= 0.f ? v : v * slope);
        }
        yb[i] = o;
    }
}
__global__ __launch_bounds__(NT) void incl_bwd2_partial(const bf16* __restrict__ dy, const bf16* __restrict__ y, const bf16* __restrict__ x,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd, const bf16* __restrict__ x2,
                                                        const float* __restrict__ mean2, const float* __restrict__ rstd2, float* __restrict__ part,
                                                        int64_t S, int C, int chunks, float slope, int64_t ldg8) {
    __shared__ float red[NT][25];
    const int64_t b = blockIdx.y;
    const int cv = C >> 3, cg = threadIdx.x % cv, cvs = __builtin_ctz(cv);
    float m[8], r[8], m2[8], r2[8], s1[8] = {}, s2[8] = {}, s3[8] = {};
    ld_chan(b * C + cg * 8, Tab{mean, m}, Tab{rstd, r}, Tab{mean2, m2}, Tab{rstd2, r2});
    const int64_t nvec = S * cv, vlo = (int64_t)blockIdx.x * CLV, vhi = min(nvec, vlo + CLV);
    const bf16x8* gb = reinterpret_cast<const bf16x8*>(dy) + b * S * ldg8;
    const bf16x8* yb = reinterpret_cast<const bf16x8*>(y + b * S * C);
    const bf16x8* xb = reinterpret_cast<const bf16x8*>(x + b * S * C);
    const bf16x8* x2b = reinterpret_cast<const bf16x8*>(x2 + b * S * C);
    for (int64_t i = vlo + threadIdx.x; i < vhi; i += NT) {
        const bf16x8 gv = gb[(i >> cvs) * ldg8 + cg], yv = yb[i], xv = xb[i], zv = x2b[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float dn = (float)gv[e] * ((float)yv[e] > 0.f ? 1.f : slope);
            s1[e] += dn;
            s2[e] += dn * ((float)xv[e] - m[e]) * r[e];
            s3[e] += dn * ((float)zv[e] - m2[e]) * r2[e];
        }
    }
    cl_fold(red, part + (b * chunks + blockIdx.x) * 3 * C, C, cv, s1, s2, s3);
}
__global__ __launch_bounds__(NT) void incl_bwd2_apply(const bf16* __restrict__ dy, const bf16* __restrict__ y, const bf16* __restrict__ x,
                                                      const float* __restrict__ mean, const float* __restrict__ rstd, const bf16* __restrict__ x2,
                                                      const float* __restrict__ mean2, const float* __restrict__ rstd2, const float* __restrict__ mm,
                                                      bf16* __restrict__ dx, bf16* __restrict__ dx2, int64_t S, int C, float slope, int64_t ldg8,
                                                      int BC) {
    const int64_t b = blockIdx.y;
    const int cv = C >> 3, cg = threadIdx.x % cv, cvs = __builtin_ctz(cv);
    float m[8], r[8], m2[8], r2[8], a1[8], a2[8], a3[8];
    ld_chan(b * C + cg * 8, Tab{mean, m}, Tab{rstd, r}, Tab{mean2, m2}, Tab{rstd2, r2}, Tab{mm, a1}, Tab{mm + BC, a2}, Tab{mm + 2 * BC, a3});
    const int64_t nvec = S * cv;
    const bf16x8* gb = reinterpret_cast<const bf16x8*>(dy) + b * S * ldg8;
    const bf16x8* yb = reinterpret_cast<const bf16x8*>(y + b * S * C);
    const bf16x8* xb = reinterpret_cast<const bf16x8*>(x + b * S * C);
    const bf16x8* x2b = reinterpret_cast<const bf16x8*>(x2 + b * S * C);
    bf16x8* dxb = reinterpret_cast<bf16x8*>(dx + b * S * C);
    bf16x8* dx2b = reinterpret_cast<bf16x8*>(dx2 + b * S * C);
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * NT) {
        const bf16x8 gv = gb[(i >> cvs) * ldg8 + cg], yv = yb[i], xv = xb[i], zv = x2b[i];
        bf16x8 o1, o2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float dn = (float)gv[e] * ((float)yv[e] > 0.f ? 1.f : slope);
            const float n = ((float)xv[e] - m[e]) * r[e], n2 = ((float)zv[e] - m2[e]) * r2[e];
            o1[e] = (bf16)(r[e] * (dn - a1[e] - n * a2[e]));
            o2[e] = (bf16)(r2[e] * (dn - a1[e] - n2 * a3[e]));
        }
        dxb[i] = o1;
        dx2b[i] = o2;
    }
}
int cl_chunks_of(int64_t S, int64_t C) { return (int)((S * (C / 8) + CLV - 1) / CLV); }
unsigned cl_apply_grid(int64_t S, int64_t C, int64_t B) {
    int64_t g = (S * (C / 8) + NT - 1) / NT;
    const int64_t cap = (4096 + B - 1) / B;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

int chunks_of(int64_t S) { return (int)((S + CHUNK - 1) / CHUNK); }
unsigned apply_grid(int64_t S, int64_t rows) {
    int64_t g = (S / 4 + NT - 1) / NT;
    const int64_t cap = (2048 + rows - 1) / rows;          // ~2048 workgroups in all
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace

extern "C" int64_t ucfvit_instnorm_workspace(int64_t rows, int64_t S) { return (rows * chunks_of(S) * 3 + 2 * rows) * (int64_t)sizeof(float); }

#define IN_DISPATCH(T_, ...)                         \
    do {                                             \
        if (dtype == UCFVIT_BF16) {                  \
            typedef bf16 T_;                         \
            __VA_ARGS__                              \
        } else {                                     \
            typedef float T_;                        \
            __VA_ARGS__                              \
        }                                            \
    } while (0)

static int in_check(const char* name, const void* x, int64_t rows, int64_t S, int dtype) {
    UCF_CHECK_ARG(x && rows > 0 && S > 0 && rows < 65536, "%s: need rows in 1..65535 and S > 0", name);
    UCF_CHECK_ARG(dtype == UCFVIT_F32 || dtype == UCFVIT_BF16, "%s: bad dtype %d", name, dtype);
    const int V = dtype == UCFVIT_BF16 ? 8 : 4;
    UCF_CHECK_ARG(S % V == 0 && ucf_is_aligned16(x), "%s: rows must be 16-byte aligned and S a multiple of %d", name, V);
    return UCFVIT_OK;
}

extern "C" int ucfvit_instnorm_fwd(const void* x, const void* res, void* y, float* mean, float* rstd, int64_t rows, int64_t S, float eps,
                                   float slope, void* workspace, int dtype, void* stream) {
    if (int rc = in_check("ucfvit_instnorm_fwd", x, rows, S, dtype)) return rc;
    UCF_CHECK_ARG(y && mean && rstd && workspace, "ucfvit_instnorm_fwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int ch = chunks_of(S);
    float* part = (float*)workspace;
    IN_DISPATCH(T, {
        hipLaunchKernelGGL((in_stats_partial<T>), dim3(ch, (unsigned)rows), dim3(NT), 0, s, (const T*)x, part, S, ch);
        hipLaunchKernelGGL(in_stats_final, dim3((unsigned)rows), dim3(64), 0, s, part, mean, rstd, ch, eps);
        const auto apply = res ? in_apply<T, true> : in_apply<T, false>;
        hipLaunchKernelGGL(apply, dim3(apply_grid(S, rows), (unsigned)rows), dim3(NT), 0, s, (const T*)x, mean, rstd, (const T*)res, (T*)y, S, slope);
    });
    UCF_LAUNCH_CHECK("ucfvit_instnorm_fwd");
    return UCFVIT_OK;
}

extern "C" int ucfvit_instnorm_bwd(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, void* dx, void* dres,
                                   int64_t rows, int64_t S, float slope, void* workspace, int dtype, void* stream) {
    if (int rc = in_check("ucfvit_instnorm_bwd", x, rows, S, dtype)) return rc;
    UCF_CHECK_ARG(dy && y && mean && rstd && dx && workspace, "ucfvit_instnorm_bwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int ch = chunks_of(S);
    float* part = (float*)workspace;
    float* m1 = part + rows * ch * 2;
    float* m2 = m1 + rows;
    IN_DISPATCH(T, {
        hipLaunchKernelGGL((in_bwd_partial<T>), dim3(ch, (unsigned)rows), dim3(NT), 0, s, (const T*)dy, (const T*)y, (const T*)x, mean, rstd, part,
                           S, ch, slope);
        hipLaunchKernelGGL(bwd_means<2>, dim3((unsigned)rows), dim3(64), 0, s, part, Means<2>{{m1, m2}}, S, 1, ch);
        const auto apply = dres ? in_bwd_apply<T, true> : in_bwd_apply<T, false>;
        hipLaunchKernelGGL(apply, dim3(apply_grid(S, rows), (unsigned)rows), dim3(NT), 0, s, (const T*)dy, (const T*)y, (const T*)x, mean, rstd, m1, m2,
                           (T*)dx, (T*)dres, S, slope);
    });
    UCF_LAUNCH_CHECK("ucfvit_instnorm_bwd");
    return UCFVIT_OK;
}

extern "C" int64_t ucfvit_dice_ce_workspace(int64_t B, int64_t S) { return (B * chunks_of(S) * DSTAT + B * DSTAT) * (int64_t)sizeof(float); }

static int dice_check(const char* name, const void* logits, const int64_t* labels, int64_t B, int64_t n, int64_t S, int64_t stride_b,
                      int64_t stride_c, int64_t stride_s, int dtype) {
    UCF_CHECK_ARG(logits && labels, "%s: null pointer", name);
    UCF_CHECK_ARG(B > 0 && B < 65536 && S > 0 && n >= 2 && n <= MAXC, "%s: need 2 <= classes <= %d, B in 1..65535", name, MAXC);
    UCF_CHECK_ARG(dtype == UCFVIT_F32 || dtype == UCFVIT_BF16, "%s: bad dtype %d", name, dtype);
    UCF_CHECK_ARG(stride_b > 0 && stride_c > 0 && stride_s > 0, "%s: strides must be positive", name);
    return UCFVIT_OK;
}
// chunk sums of the local voxels into part, then their fold: the sums to stats [B][DSTAT], the loss of those sums to loss
static void launch_dice_sums(const void* logits, const int64_t* labels, float* part, float* stats, float* loss, int64_t B, int64_t n, int64_t S,
                             int64_t sb, int64_t sc, int64_t ss, float s_nr, float s_dr, int dtype, hipStream_t s) {
    const int ch = chunks_of(S);
    IN_DISPATCH(T, {
        hipLaunchKernelGGL((dice_partial<T>), dim3(ch, (unsigned)B), dim3(NT), 0, s, (const T*)logits, labels, part, (int)n, S, ch, sb, sc, ss);
    });
    hipLaunchKernelGGL(dice_final, dim3(1), dim3(64), 0, s, part, stats, loss, (int)B, (int)n, S, ch, s_nr, s_dr);
}
static void launch_dice_bwd(const void* logits, const int64_t* labels, const float* stats, void* dlogits, int64_t B, int64_t n, int64_t S,
                            int64_t S_total, int64_t sb, int64_t sc, int64_t ss, float s_nr, float s_dr, float gscale, int dtype, hipStream_t s) {
    const dim3 g(apply_grid(S * 4, B), (unsigned)B);
    IN_DISPATCH(T, {
        hipLaunchKernelGGL((dice_bwd<T>), g, dim3(NT), 0, s, (const T*)logits, labels, stats, (T*)dlogits, (int)B, (int)n, S, s_nr, s_dr, gscale, sb, sc,
                           ss, S_total);
    });
}

// logits element (b, class c, voxel i) at logits[b stride_b + c stride_c + i stride_s] (dlogits alike): N C (D) H W is (n S, S, 1), a
// channels-last tensor with row stride ld is (S ld, 1, ld)
extern "C" int ucfvit_dice_ce(const void* logits, const int64_t* labels, float* loss, void* dlogits, int64_t B, int64_t n, int64_t S, int64_t stride_b,
                              int64_t stride_c, int64_t stride_s, float smooth_nr, float smooth_dr, float grad_scale, void* workspace, int dtype,
                              void* stream) {
    if (int rc = dice_check("ucfvit_dice_ce", logits, labels, B, n, S, stride_b, stride_c, stride_s, dtype)) return rc;
    UCF_CHECK_ARG(loss && workspace, "ucfvit_dice_ce: null pointer");
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    float* stats = part + B * chunks_of(S) * DSTAT;
    launch_dice_sums(logits, labels, part, stats, loss, B, n, S, stride_b, stride_c, stride_s, smooth_nr, smooth_dr, dtype, s);
    if (dlogits) launch_dice_bwd(logits, labels, stats, dlogits, B, n, S, S, stride_b, stride_c, stride_s, smooth_nr, smooth_dr, grad_scale, dtype, s);
    UCF_LAUNCH_CHECK("ucfvit_dice_ce");
    return UCFVIT_OK;
}

// The same loss over a volume that is SHARDED across the ranks of a sequence-parallel group (X-slabs of the decoder, fsdp/sharded_decoder.py):
// every term of it is a function of per-(batch, class) SUMS over voxels, so a rank takes the sums of its slab (ucfvit_dice_ce_stats), the
// caller adds them over the group (one all-reduce of B x 25 floats), and ucfvit_dice_ce_from_stats turns the global sums into the loss
// value and into the gradient of the local logits (S_total = voxels of the whole volume per batch element).
extern "C" int ucfvit_dice_ce_stats(const void* logits, const int64_t* labels, float* stats, int64_t B, int64_t n, int64_t S, int64_t stride_b,
                                    int64_t stride_c, int64_t stride_s, void* workspace, int dtype, void* stream) {
    if (int rc = dice_check("ucfvit_dice_ce_stats", logits, labels, B, n, S, stride_b, stride_c, stride_s, dtype)) return rc;
    UCF_CHECK_ARG(stats && workspace, "ucfvit_dice_ce_stats: null pointer");
    float* part = (float*)workspace;
    float* scratch_loss = part + B * chunks_of(S) * DSTAT;      // (the local loss value is of no use: the first word of the stats area of the workspace)
    launch_dice_sums(logits, labels, part, stats, scratch_loss, B, n, S, stride_b, stride_c, stride_s, 1.0f, 1.0f, dtype, (hipStream_t)stream);
    UCF_LAUNCH_CHECK("ucfvit_dice_ce_stats");
    return UCFVIT_OK;
}
extern "C" int ucfvit_dice_ce_stats_floats(void) { return DSTAT; }
extern "C" int ucfvit_dice_ce_from_stats(const void* logits, const int64_t* labels, float* stats, float* loss, void* dlogits, int64_t B, int64_t n,
                                         int64_t S, int64_t S_total, int64_t stride_b, int64_t stride_c, int64_t stride_s, float smooth_nr,
                                         float smooth_dr, float grad_scale, int dtype, void* stream) {
    if (int rc = dice_check("ucfvit_dice_ce_from_stats", logits, labels, B, n, S, stride_b, stride_c, stride_s, dtype)) return rc;
    UCF_CHECK_ARG(stats && loss, "ucfvit_dice_ce_from_stats: null pointer");
    UCF_CHECK_ARG(S_total >= S, "ucfvit_dice_ce_from_stats: S_total < S");
    hipStream_t s = (hipStream_t)stream;
    // one "chunk" per batch element = the global sums themselves: the fold rewrites them in place and evaluates the loss
    hipLaunchKernelGGL(dice_final, dim3(1), dim3(64), 0, s, (const float*)stats, stats, loss, (int)B, (int)n, S_total, 1, smooth_nr, smooth_dr);
    if (dlogits)
        launch_dice_bwd(logits, labels, stats, dlogits, B, n, S, S_total, stride_b, stride_c, stride_s, smooth_nr, smooth_dr, grad_scale, dtype, s);
    UCF_LAUNCH_CHECK("ucfvit_dice_ce_from_stats");
    return UCFVIT_OK;
}

// ---- channels-last instance norm entry points: x, res, y [B][S][C] bf16; mean, rstd [B][C] fp32 ----------------------------------------------
static int incl_check(const char* name, const void* x, int64_t B, int64_t S, int64_t C) {
    UCF_CHECK_ARG(x && B > 0 && B < 65536 && S > 0, "%s: need B in 1..65535 and S > 0", name);
    UCF_CHECK_ARG(C >= 8 && C <= 2048 && (C & (C - 1)) == 0, "%s: C must be a power of two in 8..2048 (got %lld)", name, (long long)C);
    UCF_CHECK_ARG(ucf_is_aligned16(x), "%s: operands must be 16-byte aligned", name);
    return UCFVIT_OK;
}
static int ld_dy_check(const char* name, const void* dy, int64_t C, int64_t ld_dy) {
    UCF_CHECK_ARG(ld_dy >= C && ld_dy % 8 == 0 && ucf_is_aligned16(dy), "%s: ld_dy must be a multiple of 8 and >= C", name);
    return UCFVIT_OK;
}
// statistics rows, then the fold's scratch, then m1 / m2 [2][B][C] for a caller that runs _bwd_sums and _bwd_apply back to back
extern "C" int64_t ucfvit_instnorm_cl_workspace(int64_t B, int64_t S, int64_t C) {
    return (B * cl_chunks_of(S, C) * 3 * C + B * 256 * 3 * C + 2 * B * C) * (int64_t)sizeof(float);
}

// The backward pass in two calls: _bwd_sums leaves the two per-(batch, channel) MEANS over the voxels (of dy' and of dy' xhat) in m1 / m2 [B][C],
// _bwd_apply turns them into dx (and dres).  A volume sharded across ranks (fsdp/sharded_decoder.py) averages m1 / m2 over the group (equal
// slabs) in between.
extern "C" int ucfvit_instnorm_cl_bwd_sums(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, float* m1, float* m2,
                                           int64_t B, int64_t S, int64_t C, int64_t ld_dy, float slope, int had_res, void* workspace, void* stream) {
    if (int rc = incl_check("ucfvit_instnorm_cl_bwd_sums", x, B, S, C)) return rc;
    if (int rc = ld_dy_check("ucfvit_instnorm_cl_bwd_sums", dy, C, ld_dy)) return rc;
    UCF_CHECK_ARG(dy && y && mean && rstd && m1 && m2 && workspace, "ucfvit_instnorm_cl_bwd_sums: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int ch = cl_chunks_of(S, C);
    float* part = (float*)workspace;
    const auto partial = had_res ? incl_bwd_partial<true> : incl_bwd_partial<false>;
    hipLaunchKernelGGL(partial, dim3(ch, (unsigned)B), dim3(NT), 0, s, (const bf16*)dy, (const bf16*)y, (const bf16*)x, mean, rstd, part, S, (int)C,
                       ch, slope, ld_dy / 8);
    hipLaunchKernelGGL(bwd_means<2>, dim3((unsigned)(B * C)), dim3(64), 0, s, part, Means<2>{{m1, m2}}, S, (int)C, ch);
    UCF_LAUNCH_CHECK("ucfvit_instnorm_cl_bwd_sums");
    return UCFVIT_OK;
}
extern "C" int ucfvit_instnorm_cl_bwd_apply(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, const float* m1,
                                            const float* m2, void* dx, void* dres, int64_t B, int64_t S, int64_t C, int64_t ld_dy, float slope,
                                            int had_res, void* stream) {
    if (int rc = incl_check("ucfvit_instnorm_cl_bwd_apply", x, B, S, C)) return rc;
    if (int rc = ld_dy_check("ucfvit_instnorm_cl_bwd_apply", dy, C, ld_dy)) return rc;
    UCF_CHECK_ARG(dy && y && mean && rstd && m1 && m2 && dx, "ucfvit_instnorm_cl_bwd_apply: null pointer");
    UCF_CHECK_ARG(had_res || !dres, "ucfvit_instnorm_cl_bwd_apply: dres without a residual in the forward pass");
    // <RES: the activation mask is read from y, WRES: dres is written>
    const auto apply = dres ? incl_bwd_apply<true, true> : had_res ? incl_bwd_apply<true, false> : incl_bwd_apply<false, false>;
    hipLaunchKernelGGL(apply, dim3(cl_apply_grid(S, C, B), (unsigned)B), dim3(NT), 0, (hipStream_t)stream, (const bf16*)dy, (const bf16*)y,
                       (const bf16*)x, mean, rstd, m1, m2, (bf16*)dx, (bf16*)(dres ? dres : dx), S, (int)C, slope, ld_dy / 8);
    UCF_LAUNCH_CHECK("ucfvit_instnorm_cl_bwd_apply");
    return UCFVIT_OK;
}

// statistics only (mean, rstd [B][C]); the forward pass is this + ucfvit_instnorm_cl_apply
extern "C" int ucfvit_instnorm_cl_stats(const void* x, float* mean, float* rstd, int64_t B, int64_t S, int64_t C, float eps, void* workspace,
                                        void* stream) {
    if (int rc = incl_check("ucfvit_instnorm_cl_stats", x, B, S, C)) return rc;
    UCF_CHECK_ARG(mean && rstd && workspace, "ucfvit_instnorm_cl_stats: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int ch = cl_chunks_of(S, C);
    float* part = (float*)workspace;
    hipLaunchKernelGGL(incl_stats_partial, dim3(ch, (unsigned)B), dim3(NT), 0, s, (const bf16*)x, part, S, (int)C, ch);
    if (int rc = ucfvit_instnorm_cl_stats_fold(part, mean, rstd, B, S, C, ch, eps, part + B * ch * 3 * C, s)) return rc;
    UCF_LAUNCH_CHECK("ucfvit_instnorm_cl_stats");
    return UCFVIT_OK;
}
// y = lrelu((x - mean) rstd + (x2 - mean2) rstd2, slope): both statistics given (ucfvit_instnorm_cl_stats)
extern "C" int ucfvit_instnorm_cl_apply2(const void* x, const float* mean, const float* rstd, const void* x2, const float* mean2, const float* rstd2,
                                         void* y, int64_t B, int64_t S, int64_t C, float slope, void* stream) {
    if (int rc = incl_check("ucfvit_instnorm_cl_apply2", x, B, S, C)) return rc;
    UCF_CHECK_ARG(mean && rstd && x2 && mean2 && rstd2 && y && ucf_is_aligned16(x2) && ucf_is_aligned16(y), "ucfvit_instnorm_cl_apply2: bad pointer");
    const dim3 g(cl_apply_grid(S, C, B), (unsigned)B);
    hipLaunchKernelGGL(incl_apply2, g, dim3(NT), 0, (hipStream_t)stream, (const bf16*)x, mean, rstd, (const bf16*)x2, mean2, rstd2, (bf16*)y, S, (int)C,
                       slope);
    UCF_LAUNCH_CHECK("ucfvit_instnorm_cl_apply2");
    return UCFVIT_OK;
}
extern "C" int64_t ucfvit_instnorm_cl_bwd2_workspace(int64_t B, int64_t S, int64_t C) {
    return (B * cl_chunks_of(S, C) * 3 * C + 3 * B * C) * (int64_t)sizeof(float);
}
// backward of ucfvit_instnorm_cl_apply2: dx, dx2 from dy, the saved output y (activation mask) and the two raw inputs with their statistics
extern "C" int ucfvit_instnorm_cl_bwd2(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, const void* x2,
                                       const float* mean2, const float* rstd2, void* dx, void* dx2, int64_t B, int64_t S, int64_t C, int64_t ld_dy,
                                       float slope, void* workspace, void* stream) {
    if (int rc = incl_check("ucfvit_instnorm_cl_bwd2", x, B, S, C)) return rc;
    if (int rc = ld_dy_check("ucfvit_instnorm_cl_bwd2", dy, C, ld_dy)) return rc;
    UCF_CHECK_ARG(dy && y && mean && rstd && x2 && mean2 && rstd2 && dx && dx2 && workspace, "ucfvit_instnorm_cl_bwd2: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int ch = cl_chunks_of(S, C);
    const int64_t ldg8 = ld_dy / 8;
    float* part = (float*)workspace;
    float* mm = part + B * ch * 3 * C;
    hipLaunchKernelGGL(incl_bwd2_partial, dim3(ch, (unsigned)B), dim3(NT), 0, s, (const bf16*)dy, (const bf16*)y, (const bf16*)x, mean, rstd,
                       (const bf16*)x2, mean2, rstd2, part, S, (int)C, ch, slope, ldg8);
    hipLaunchKernelGGL(bwd_means<3>, dim3((unsigned)(B * C)), dim3(64), 0, s, part, Means<3>{{mm, mm + B * C, mm + 2 * B * C}}, S, (int)C, ch);
    const dim3 g(cl_apply_grid(S, C, B), (unsigned)B);
    hipLaunchKernelGGL(incl_bwd2_apply, g, dim3(NT), 0, s, (const bf16*)dy, (const bf16*)y, (const bf16*)x, mean, rstd, (const bf16*)x2, mean2, rstd2, mm,
                       (bf16*)dx, (bf16*)dx2, S, (int)C, slope, ldg8, (int)(B * C));
    UCF_LAUNCH_CHECK("ucfvit_instnorm_cl_bwd2");
    return UCFVIT_OK;
}

// mean / rstd [B][C] from the partial rows [B][rows][3][C] (count, mean, M2) of ucfvit_conv3d_fwd's statistics epilogue (S = voxels per batch element)
extern "C" int ucfvit_instnorm_cl_stats_fold(const float* partial, float* mean, float* rstd, int64_t B, int64_t S, int64_t C, int64_t rows, float eps,
                                             void* workspace, void* stream) {      // workspace: B * 256 * 3 C floats (may be NULL: single stage)
    UCF_CHECK_ARG(partial && mean && rstd && B > 0 && S > 0 && C > 0 && rows > 0 && B * C < (1ll << 31) && rows < (1ll << 31),
                  "ucfvit_instnorm_cl_stats_fold: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (rows > 512 && workspace && (C & (C - 1)) == 0 && C <= NT) {
        // two stages: 128..256 row groups per batch element first (coalesced), then the per-channel fold over the groups
        const int G = (int)((rows + 255) / 256) > 256 ? 256 : (int)((rows + 255) / 256);
        const int rpg = (int)((rows + G - 1) / G);
        hipLaunchKernelGGL(incl_stats_fold1, dim3(G, (unsigned)B), dim3(NT), 0, s, partial, (float*)workspace, (int)rows, (int)C, rpg);
        hipLaunchKernelGGL(incl_stats_fold, dim3((unsigned)(B * C)), dim3(64), 0, s, (const float*)workspace, mean, rstd, S, (int)C, G, eps);
    } else {
        hipLaunchKernelGGL(incl_stats_fold, dim3((unsigned)(B * C)), dim3(64), 0, s, partial, mean, rstd, S, (int)C, (int)rows, eps);
    }
    UCF_LAUNCH_CHECK("ucfvit_instnorm_cl_stats_fold");
    return UCFVIT_OK;
}

// apply pass alone, statistics given: y = lrelu((x - mean) rstd [+ res], slope)
extern "C" int ucfvit_instnorm_cl_apply(const void* x, const void* res, void* y, const float* mean, const float* rstd, int64_t B, int64_t S, int64_t C,
                                        float slope, void* stream) {
    if (int rc = incl_check("ucfvit_instnorm_cl_apply", x, B, S, C)) return rc;
    UCF_CHECK_ARG(y && mean && rstd && ucf_is_aligned16(y) && (!res || ucf_is_aligned16(res)), "ucfvit_instnorm_cl_apply: bad pointer");
    const auto apply = res ? incl_apply<true> : incl_apply<false>;
    hipLaunchKernelGGL(apply, dim3(cl_apply_grid(S, C, B), (unsigned)B), dim3(NT), 0, (hipStream_t)stream, (const bf16*)x, mean, rstd,
                       (const bf16*)(res ? res : x), (bf16*)y, S, (int)C, slope);      // without res: a valid pointer that is never read
    UCF_LAUNCH_CHECK("ucfvit_instnorm_cl_apply");
    return UCFVIT_OK;
}
