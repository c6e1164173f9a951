// SAP segmentation head and its Dice + BCE loss (reference simple/arch.py:491-536, utils/metrics.py:95-121).
//
// The head is ConvTranspose(D -> K, kernel = stride = p) followed by a 1x1 convolution (K -> C) with NO nonlinearity between them, so
//   header(neck(x)) = x · W_eff + b,   W_eff[d][(delta, c)] = sum_k W_neck[d][k][delta] · W_head[c][k]      (delta: the P = p^nd offsets of a patch)
// and the K-channel map never has to exist: the fold below builds W_eff once per step, ucfvit_gemm multiplies the tokens with it, and the
// scatter moves C channels into the channel-first map.  Backward is the mirror image: inverse scatter, the two GEMMs of a Linear layer, unfold.
//
// Everything here is HBM- or latency-bound: wave64, 16-byte accesses where the row width allows, scalar otherwise.  Reductions run in two
// stages with a fixed order and there is no floating-point atomic, so every result is bitwise reproducible from run to run.
#include "common.h"

namespace {

constexpr int NT = 256;

// ---------------------------------------------------------------------------------------------------------------- logit scatter
// rows  [B·S][P·C], token t = (tx s + ty) s + tz (2-D: tx s + ty), column (delta, c), delta = (kx p + ky) p + kz (2-D: kx p + ky)
// map   [B][C][s p]^nd, voxel (tx p + kx, ty p + ky, tz p + kz)
struct ScatterGeom {
    int p, s, C, nd;
    int side, P, S, PC;        // s p, p^nd, s^nd, P C
    int vox;                   // side^nd
};

// linear index into rows of the map element e = ((b C + c) vox + v)
__device__ __forceinline__ int rows_index_of_map(const ScatterGeom& g, int e, int& c) {
    const int v = e % g.vox, bc = e / g.vox;
    c = bc % g.C;
    const int b = bc / g.C;
    int t, d;
    if (g.nd == 3) {
        const int z = v % g.side, xy = v / g.side, y = xy % g.side, x = xy / g.side;
        t = ((x / g.p) * g.s + y / g.p) * g.s + z / g.p;
        d = ((x % g.p) * g.p + y % g.p) * g.p + z % g.p;
    } else {
        const int y = v % g.side, x = v / g.side;
        t = (x / g.p) * g.s + y / g.p;
        d = (x % g.p) * g.p + y % g.p;
    }
    return (b * g.S + t) * g.PC + d * g.C + c;
}

// linear index into the map of the rows element e = ((b S + t) P + delta) C + c
__device__ __forceinline__ int map_index_of_rows(const ScatterGeom& g, int e) {
    const int c = e % g.C, r = e / g.C, d = r % g.P, bt = r / g.P, t = bt % g.S, b = bt / g.S;
    int v;
    if (g.nd == 3) {
        const int kz = d % g.p, kxy = d / g.p, ky = kxy % g.p, kx = kxy / g.p;
        const int tz = t % g.s, txy = t / g.s, ty = txy % g.s, tx = txy / g.s;
        v = ((tx * g.p + kx) * g.side + ty * g.p + ky) * g.side + tz * g.p + kz;
    } else {
        const int ky = d % g.p, kx = d / g.p, ty = t % g.s, tx = t / g.s;
        v = (tx * g.p + kx) * g.side + ty * g.p + ky;
    }
    return (b * g.C + c) * g.vox + v;
}

// V = 4: four consecutive voxels of one map row (side % 4 == 0) as one 16-byte store; V = 1: the scalar form for every other width
template <int V>
__global__ __launch_bounds__(NT) void scatter_fwd_kernel(const float* __restrict__ rows, const float* __restrict__ bias, float* __restrict__ map,
                                                         ScatterGeom g, int nvec) {
    for (int i = blockIdx.x * NT + threadIdx.x; i < nvec; i += gridDim.x * NT) {
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            int c;
            const int src = rows_index_of_map(g, i * V + j, c);
            o[j] = rows[src] + bias[c];
        }
        if constexpr (V == 4) {
            const f32x4 v = {o[0], o[1], o[2], o[3]};
            reinterpret_cast<f32x4*>(map)[i] = v;
        } else {
            map[i] = o[0];
        }
    }
}

// T = type of the rows; V elements of one row (P C % V == 0) as one 16-byte store, or V = 1
template <typename T, int V>
__global__ __launch_bounds__(NT) void scatter_bwd_kernel(const float* __restrict__ dmap, T* __restrict__ drows, ScatterGeom g, int nvec) {
    for (int i = blockIdx.x * NT + threadIdx.x; i < nvec; i += gridDim.x * NT) {
        if constexpr (V == 1) {
            drows[i] = from_f32<T>(dmap[map_index_of_rows(g, i)]);
        } else {
            Vec16<T> o;
#pragma unroll
            for (int j = 0; j < V; ++j) o.set(j, dmap[map_index_of_rows(g, i * V + j)]);
            reinterpret_cast<decltype(o.v)*>(drows)[i] = o.v;
        }
    }
}

// dbias[c] = sum over b and voxels of dmap[b][c][:]: stage 1 sums one chunk of one (b, c) row per workgroup, stage 2 adds the partials of a
// channel in a fixed order (in double: it costs nothing here)
constexpr int DB_CHUNK = NT * 16;
template <int V>
__global__ __launch_bounds__(NT) void dbias_partial_kernel(const float* __restrict__ dmap, float* __restrict__ part, int vox, int chunks) {
    __shared__ float red[NT / 64];
    const float* row = dmap + (int64_t)blockIdx.y * vox;
    const int lo = blockIdx.x * DB_CHUNK, hi = min(vox, lo + DB_CHUNK);
    float s = 0.f;
    if constexpr (V == 4) {
        for (int i = lo + threadIdx.x * 4; i < hi; i += NT * 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + i);
            s += (v[0] + v[1]) + (v[2] + v[3]);
        }
    } else {
        for (int i = lo + threadIdx.x; i < hi; i += NT) s += row[i];
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.y * chunks + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(64) void dbias_final_kernel(const float* __restrict__ part, float* __restrict__ dbias, int B, int C, int chunks) {
    const int c = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < B * chunks; i += 64) s += part[((i / chunks) * C + c) * chunks + i % chunks];
    s = wave_sum(s);
    if (threadIdx.x == 0) dbias[c] = (float)s;
}

unsigned grid_for(int64_t n) {
    int64_t g = (n + NT - 1) / NT;
    if (g > 4096) g = 4096;
    return (unsigned)(g < 1 ? 1 : g);
}

int scatter_geom(const char* name, ScatterGeom& g, int64_t B, int64_t s, int64_t p, int64_t C, int nd) {
    UCF_CHECK_ARG(nd == 2 || nd == 3, "%s: nd must be 2 or 3 (got %d)", name, nd);
    UCF_CHECK_ARG(B >= 1 && s >= 1 && p >= 1 && C >= 1, "%s: need B, s, p, C >= 1", name);
    UCF_CHECK_ARG(s * p <= 32768 && C <= 65536 && B <= 65535, "%s: extent out of range", name);
    int64_t side = s * p, P = p, S = s, vox = side;
    for (int i = 1; i < nd; ++i) P *= p, S *= s, vox *= side;
    UCF_CHECK_ARG(vox < (1ll << 30) && B * C * vox < (1ll << 30), "%s: more than 2^30 map elements", name);    // int indices, grid-stride headroom
    g.p = (int)p, g.s = (int)s, g.C = (int)C, g.nd = nd;
    g.side = (int)side, g.P = (int)P, g.S = (int)S, g.PC = (int)(P * C), g.vox = (int)vox;
    return UCFVIT_OK;
}

// ---------------------------------------------------------------------------------------------------------------- fold / unfold
// W_neck [D][K][P] fp32 (ConvTranspose weight), W_head [C][K] fp32 (1x1 convolution weight), W_eff [P C][D] (an nn.Linear weight)
constexpr int CT = 4;    // classes per pass over W_neck

// one thread per (d, delta): W_neck is read once per CT classes, coalesced in runs of P; W_head[c][k] is wave-uniform
template <typename T>
__global__ __launch_bounds__(NT) void fold_kernel(const float* __restrict__ wn, const float* __restrict__ wh, T* __restrict__ weff, int D, int K, int P,
                                                  int C) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= D * P) return;
    const int d = e / P, dl = e % P;
    const float* a = wn + (int64_t)d * K * P + dl;
    for (int c0 = 0; c0 < C; c0 += CT) {
        float acc[CT] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int k = 0; k < K; ++k) {
            const float v = a[(int64_t)k * P];
#pragma unroll
            for (int j = 0; j < CT; ++j)
                if (c0 + j < C) acc[j] += v * wh[(c0 + j) * K + k];
        }
#pragma unroll
        for (int j = 0; j < CT; ++j)
            if (c0 + j < C) weff[(int64_t)(dl * C + c0 + j) * D + d] = from_f32<T>(acc[j]);
    }
}

// one workgroup per d: column d of dW_eff ([P C] values) goes to LDS, then
//   dW_neck[d][k][delta] = sum_c col[delta C + c] · W_head[c][k]                              (written coalesced)
__global__ __launch_bounds__(NT) void unfold_neck_kernel(const float* __restrict__ dweff, const float* __restrict__ wh, float* __restrict__ dwn,
                                                         int D, int K, int P, int C) {
    extern __shared__ float col[];
    const int d = blockIdx.x, PC = P * C;
    for (int i = threadIdx.x; i < PC; i += NT) col[i] = dweff[(int64_t)i * D + d];
    __syncthreads();
    float* out = dwn + (int64_t)d * K * P;
    for (int o = threadIdx.x; o < K * P; o += NT) {
        const int k = o / P, dl = o % P;
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += col[dl * C + c] * wh[c * K + k];
        out[o] = s;
    }
}

// stage 1 of dW_head[c][k] = sum_{d, delta} dW_eff[(delta, c)][d] · W_neck[d][k][delta]: one workgroup per d, one wave per k at a time with
// its lanes over delta; part[d][c K + k].  Stage 2 (sum over d, fixed order) is ucfvit_reduce_rows.
__global__ __launch_bounds__(NT) void unfold_head_partial_kernel(const float* __restrict__ dweff, const float* __restrict__ wn,
                                                                 float* __restrict__ part, int D, int K, int P, int C) {
    extern __shared__ float col[];
    const int d = blockIdx.x, PC = P * C, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < PC; i += NT) col[i] = dweff[(int64_t)i * D + d];
    __syncthreads();
    const float* a = wn + (int64_t)d * K * P;
    float* out = part + (int64_t)d * C * K;
    for (int k = wave; k < K; k += NT / 64) {
        for (int c0 = 0; c0 < C; c0 += CT) {
            float acc[CT] = {0.f, 0.f, 0.f, 0.f};
            for (int dl = lane; dl < P; dl += 64) {
                const float v = a[(int64_t)k * P + dl];
#pragma unroll
                for (int j = 0; j < CT; ++j)
                    if (c0 + j < C) acc[j] += v * col[dl * C + c0 + j];
            }
#pragma unroll
            for (int j = 0; j < CT; ++j) {
                const float s = wave_sum(acc[j]);
                if (lane == 0 && c0 + j < C) out[(c0 + j) * K + k] = s;
            }
        }
    }
}

int fold_check(const char* name, int64_t D, int64_t K, int64_t P, int64_t C) {
    UCF_CHECK_ARG(D >= 1 && K >= 1 && P >= 1 && C >= 1, "%s: need D, K, P, C >= 1", name);
    UCF_CHECK_ARG(D * K * P < (1ll << 31) && P * C * D < (1ll << 31) && C * K < (1ll << 31), "%s: more than 2^31 weight elements", name);
    UCF_CHECK_ARG(P * C * (int64_t)sizeof(float) <= 64 * 1024, "%s: P * C = %lld is more than the 16384 floats of LDS one column may take", name,
                  (long long)(P * C));
    return UCFVIT_OK;
}

// ---------------------------------------------------------------------------------------------------------------- Dice + BCE
// logits z [B][C][S] (T), targets t [B][C][S] fp32; the loss reads channels 1..C-1 only: per batch element ONE contiguous run of L = (C-1) S
// values behind the S values of channel 0.
constexpr int DBCE_STATS = 4;                  // sum p t, sum p, sum t, sum BCE
constexpr int DBCE_CHUNK = NT * 16;

struct SigTerms {
    float p, pq, bce;                          // sigmoid(z), p (1 - p), the BCE term of (z, t)
};
// e = exp(-|z|) <= 1 never overflows; p and 1 - p both come from it, so neither is a rounded difference.
// BCE = t min(softplus(-z), 100) + (1 - t) min(softplus(z), 100), softplus(x) = max(x, 0) + log1p(exp(-|x|)): the reference's
// binary_cross_entropy(sigmoid(z), t) with its clamp of the logarithms at -100, in a form that stays exact when sigmoid rounds to 0 or 1.
__device__ __forceinline__ SigTerms sig_terms(float z, float t) {
    const float e = expf(-fabsf(z)), r = 1.0f / (1.0f + e), big = r, small = e * r, l = log1pf(e);
    SigTerms o;
    o.p = z >= 0.f ? big : small;
    o.pq = big * small;
    const float sp_pos = fmaxf(z, 0.f) + l, sp_neg = fmaxf(-z, 0.f) + l;          // softplus(z), softplus(-z)
    o.bce = t * fminf(sp_neg, 100.f) + (1.0f - t) * fminf(sp_pos, 100.f);
    return o;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void dbce_stats_partial_kernel(const T* __restrict__ z, const float* __restrict__ t, float* __restrict__ part,
                                                                int64_t S, int64_t L, int chunks) {
    __shared__ float red[NT / 64][DBCE_STATS];
    const int64_t base = ((int64_t)blockIdx.y * (L + S)) + S;           // channel 1 of batch element blockIdx.y
    const int64_t lo = (int64_t)blockIdx.x * DBCE_CHUNK, hi = lo + DBCE_CHUNK < L ? lo + DBCE_CHUNK : L;
    float a[DBCE_STATS] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (VEC) {
        constexpr int V = Vec16<T>::N;
        for (int64_t i = lo + threadIdx.x * V; i < hi; i += NT * V) {
            Vec16<T> zv;
            zv.v = *reinterpret_cast<const decltype(zv.v)*>(z + base + i);
            float tv[V];
#pragma unroll
            for (int j = 0; j < V; j += 4) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(t + base + i + j);
                tv[j] = q[0], tv[j + 1] = q[1], tv[j + 2] = q[2], tv[j + 3] = q[3];
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const SigTerms q = sig_terms(zv.get(j), tv[j]);
                a[0] += q.p * tv[j], a[1] += q.p, a[2] += tv[j], a[3] += q.bce;
            }
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += NT) {
            const float tt = t[base + i];
            const SigTerms q = sig_terms(to_f32<T>(z[base + i]), tt);
            a[0] += q.p * tt, a[1] += q.p, a[2] += tt, a[3] += q.bce;
        }
    }
#pragma unroll
    for (int k = 0; k < DBCE_STATS; ++k) {
        const float s = wave_sum(a[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < DBCE_STATS) {
        const int k = threadIdx.x;
        part[((int64_t)blockIdx.y * chunks + blockIdx.x) * DBCE_STATS + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}
__global__ __launch_bounds__(64) void dbce_stats_final_kernel(const float* __restrict__ part, float* __restrict__ stats, int n) {
    double s[DBCE_STATS] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 64)
#pragma unroll
        for (int k = 0; k < DBCE_STATS; ++k) s[k] += part[(int64_t)i * DBCE_STATS + k];
#pragma unroll
    for (int k = 0; k < DBCE_STATS; ++k) s[k] = wave_sum(s[k]);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < DBCE_STATS; ++k) stats[k] = (float)s[k];
}

// loss = w BCE_mean + (1 - w) (1 - N / Dn),  N = 2 I + smooth,  Dn = sum p + sum t + smooth
// d loss / d z = w (p - t) / n + (1 - w) p (1 - p) (N / Dn^2 - 2 t / Dn)
struct DbceCoef {
    float bce, dice_a, dice_b;                 // w / n, (1 - w) N / Dn^2, (1 - w) 2 / Dn  (all times the upstream gradient)
};
__device__ __forceinline__ DbceCoef dbce_coef(const float* stats, float w, float smooth, float n, float gs) {
    const float N = 2.0f * stats[0] + smooth, Dn = stats[1] + stats[2] + smooth;
    DbceCoef c;
    c.bce = gs * w / n;
    c.dice_a = gs * (1.0f - w) * N / (Dn * Dn);
    c.dice_b = gs * (1.0f - w) * 2.0f / Dn;
    return c;
}
__global__ void dbce_loss_kernel(const float* __restrict__ stats, float* __restrict__ loss, float w, float smooth, double n) {
    const double N = 2.0 * stats[0] + smooth, Dn = (double)stats[1] + stats[2] + smooth;
    *loss = (float)(w * (stats[3] / n) + (1.0 - w) * (1.0 - N / Dn));
}

// dz is fp32 whatever the type of z: a bf16 rounding of the gradient would be 400 times the error of everything else in it
template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void dbce_grad_kernel(const T* __restrict__ z, const float* __restrict__ t, const float* __restrict__ stats,
                                                       float* __restrict__ dz, int64_t S, int64_t CS, float w, float smooth, float n,
                                                       float grad_scale, const float* __restrict__ grad_scale_dev) {
    const DbceCoef k = dbce_coef(stats, w, smooth, n, grad_scale_dev ? grad_scale * *grad_scale_dev : grad_scale);
    const int64_t base = (int64_t)blockIdx.y * CS;
    constexpr int V = VEC ? Vec16<T>::N : 1;
    for (int64_t i = ((int64_t)blockIdx.x * NT + threadIdx.x) * V; i < CS; i += (int64_t)gridDim.x * NT * V) {
        const bool bg = i < S;                                          // channel 0 (S % V == 0 in the vector form: never straddled)
        if constexpr (VEC) {
            Vec16<T> zv;
            if (!bg) zv.v = *reinterpret_cast<const decltype(zv.v)*>(z + base + i);
#pragma unroll
            for (int j = 0; j < V; j += 4) {
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                if (!bg) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(t + base + i + j);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const SigTerms g = sig_terms(zv.get(j + u), q[u]);
                        o[u] = k.bce * (g.p - q[u]) + g.pq * (k.dice_a - k.dice_b * q[u]);
                    }
                }
                *reinterpret_cast<f32x4*>(dz + base + i + j) = o;
            }
        } else {
            float o = 0.f;
            if (!bg) {
                const float tt = t[base + i];
                const SigTerms g = sig_terms(to_f32<T>(z[base + i]), tt);
                o = k.bce * (g.p - tt) + g.pq * (k.dice_a - k.dice_b * tt);
            }
            dz[base + i] = o;
        }
    }
}

int dbce_chunks(int64_t L) { return (int)((L + DBCE_CHUNK - 1) / DBCE_CHUNK); }

int dbce_check(const char* name, const void* logits, const float* targets, int64_t B, int64_t C, int64_t S, int dtype) {
    UCF_CHECK_ARG(logits && targets, "%s: null pointer", name);
    UCF_CHECK_ARG(B >= 1 && B <= 65535 && C >= 2 && S >= 1, "%s: need B in 1..65535, classes >= 2 and S >= 1", name);
    UCF_CHECK_ARG(dtype == UCFVIT_F32 || dtype == UCFVIT_BF16, "%s: bad dtype %d", name, dtype);
    UCF_CHECK_ARG((C - 1) * S < (1ll << 40) / B, "%s: volume too large", name);
    return UCFVIT_OK;
}
// the 16-byte form needs every channel to start on a vector boundary of both tensors
bool dbce_vec(const void* logits, const void* dlogits, const float* targets, int64_t S, int dtype) {
    const int V = dtype == UCFVIT_BF16 ? 8 : 4;
    return S % V == 0 && ucf_is_aligned16(logits) && ucf_is_aligned16(targets) && (!dlogits || ucf_is_aligned16(dlogits));
}

}  // namespace

#define SAP_DISPATCH(T_, ...)                        \
    do {                                             \
        if (dtype == UCFVIT_BF16) {                  \
            typedef bf16 T_;                         \
            __VA_ARGS__                              \
        } else {                                     \
            typedef float T_;                        \
            __VA_ARGS__                              \
        }                                            \
    } while (0)

extern "C" int ucfvit_sap_scatter_fwd(const float* rows, const float* bias, float* map, int64_t B, int64_t s, int64_t p, int64_t C, int nd,
                                      void* stream) {
    ScatterGeom g;
    if (int rc = scatter_geom("ucfvit_sap_scatter_fwd", g, B, s, p, C, nd)) return rc;
    UCF_CHECK_ARG(rows && bias && map, "ucfvit_sap_scatter_fwd: null pointer");
    const int total = (int)B * g.C * g.vox;
    hipStream_t st = (hipStream_t)stream;
    if (g.side % 4 == 0 && ucf_is_aligned16(map))
        hipLaunchKernelGGL(scatter_fwd_kernel<4>, dim3(grid_for(total / 4)), dim3(NT), 0, st, rows, bias, map, g, total / 4);
    else
        hipLaunchKernelGGL(scatter_fwd_kernel<1>, dim3(grid_for(total)), dim3(NT), 0, st, rows, bias, map, g, total);
    UCF_LAUNCH_CHECK("ucfvit_sap_scatter_fwd");
    return UCFVIT_OK;
}

extern "C" int64_t ucfvit_sap_scatter_bwd_workspace(int64_t B, int64_t s, int64_t p, int64_t C, int nd) {
    ScatterGeom g;
    if (scatter_geom("ucfvit_sap_scatter_bwd_workspace", g, B, s, p, C, nd)) return 0;
    return B * C * ((g.vox + DB_CHUNK - 1) / DB_CHUNK) * (int64_t)sizeof(float);
}

extern "C" int ucfvit_sap_scatter_bwd(const float* dmap, void* drows, float* dbias, int64_t B, int64_t s, int64_t p, int64_t C, int nd,
                                      void* workspace, int dtype, void* stream) {
    ScatterGeom g;
    if (int rc = scatter_geom("ucfvit_sap_scatter_bwd", g, B, s, p, C, nd)) return rc;
    UCF_CHECK_ARG(dmap && drows && (!dbias || workspace), "ucfvit_sap_scatter_bwd: null pointer");
    UCF_CHECK_ARG(dtype == UCFVIT_F32 || dtype == UCFVIT_BF16, "ucfvit_sap_scatter_bwd: bad dtype %d", dtype);
    UCF_CHECK_ARG(!dbias || B * C <= 65535, "ucfvit_sap_scatter_bwd: B * C > 65535");
    const int total = (int)B * g.C * g.vox;
    hipStream_t st = (hipStream_t)stream;
    SAP_DISPATCH(T, {
        constexpr int V = Vec16<T>::N;
        if (g.PC % V == 0 && ucf_is_aligned16(drows))
            hipLaunchKernelGGL((scatter_bwd_kernel<T, V>), dim3(grid_for(total / V)), dim3(NT), 0, st, dmap, (T*)drows, g, total / V);
        else
            hipLaunchKernelGGL((scatter_bwd_kernel<T, 1>), dim3(grid_for(total)), dim3(NT), 0, st, dmap, (T*)drows, g, total);
    });
    UCF_LAUNCH_CHECK("ucfvit_sap_scatter_bwd");
    if (dbias) {
        const int chunks = (g.vox + DB_CHUNK - 1) / DB_CHUNK;
        const dim3 grid(chunks, (unsigned)(B * C));
        if (g.vox % 4 == 0 && ucf_is_aligned16(dmap))
            hipLaunchKernelGGL(dbias_partial_kernel<4>, grid, dim3(NT), 0, st, dmap, (float*)workspace, g.vox, chunks);
        else
            hipLaunchKernelGGL(dbias_partial_kernel<1>, grid, dim3(NT), 0, st, dmap, (float*)workspace, g.vox, chunks);
        hipLaunchKernelGGL(dbias_final_kernel, dim3((unsigned)C), dim3(64), 0, st, (const float*)workspace, dbias, (int)B, (int)C, chunks);
        UCF_LAUNCH_CHECK("ucfvit_sap_scatter_bwd(dbias)");
    }
    return UCFVIT_OK;
}

extern "C" int ucfvit_sap_fold(const float* w_neck, const float* w_head, void* w_eff, int64_t D, int64_t K, int64_t P, int64_t C, int dtype,
                               void* stream) {
    if (int rc = fold_check("ucfvit_sap_fold", D, K, P, C)) return rc;
    UCF_CHECK_ARG(w_neck && w_head && w_eff, "ucfvit_sap_fold: null pointer");
    UCF_CHECK_ARG(dtype == UCFVIT_F32 || dtype == UCFVIT_BF16, "ucfvit_sap_fold: bad dtype %d", dtype);
    const dim3 grid((unsigned)((D * P + NT - 1) / NT));
    SAP_DISPATCH(T, {
        hipLaunchKernelGGL(fold_kernel<T>, grid, dim3(NT), 0, (hipStream_t)stream, w_neck, w_head, (T*)w_eff, (int)D, (int)K, (int)P, (int)C);
    });
    UCF_LAUNCH_CHECK("ucfvit_sap_fold");
    return UCFVIT_OK;
}

extern "C" int64_t ucfvit_sap_unfold_workspace(int64_t D, int64_t K, int64_t C) { return D * C * K * (int64_t)sizeof(float); }

extern "C" int ucfvit_sap_unfold(const float* dw_eff, const float* w_neck, const float* w_head, float* dw_neck, float* dw_head, int64_t D,
                                 int64_t K, int64_t P, int64_t C, void* workspace, void* stream) {
    if (int rc = fold_check("ucfvit_sap_unfold", D, K, P, C)) return rc;
    UCF_CHECK_ARG(dw_eff && w_neck && w_head && dw_neck && dw_head && workspace, "ucfvit_sap_unfold: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)(P * C) * sizeof(float);
    hipLaunchKernelGGL(unfold_neck_kernel, dim3((unsigned)D), dim3(NT), lds, st, dw_eff, w_head, dw_neck, (int)D, (int)K, (int)P, (int)C);
    hipLaunchKernelGGL(unfold_head_partial_kernel, dim3((unsigned)D), dim3(NT), lds, st, dw_eff, w_neck, (float*)workspace, (int)D, (int)K, (int)P,
                       (int)C);
    UCF_LAUNCH_CHECK("ucfvit_sap_unfold");
    return ucfvit_reduce_rows((const float*)workspace, dw_head, D, C * K, 0, stream);
}

extern "C" int ucfvit_dice_bce_stats_floats(void) { return DBCE_STATS; }
extern "C" int64_t ucfvit_dice_bce_workspace(int64_t B, int64_t C, int64_t S) {
    return B * dbce_chunks((C - 1) * S) * DBCE_STATS * (int64_t)sizeof(float);
}

extern "C" int ucfvit_dice_bce_stats(const void* logits, const float* targets, float* stats, int64_t B, int64_t C, int64_t S, void* workspace,
                                     int dtype, void* stream) {
    if (int rc = dbce_check("ucfvit_dice_bce_stats", logits, targets, B, C, S, dtype)) return rc;
    UCF_CHECK_ARG(stats && workspace, "ucfvit_dice_bce_stats: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t L = (C - 1) * S;
    const int ch = dbce_chunks(L);
    const dim3 grid(ch, (unsigned)B);
    const bool vec = dbce_vec(logits, nullptr, targets, S, dtype);
    SAP_DISPATCH(T, {
        if (vec)
            hipLaunchKernelGGL((dbce_stats_partial_kernel<T, true>), grid, dim3(NT), 0, st, (const T*)logits, targets, (float*)workspace, S, L, ch);
        else
            hipLaunchKernelGGL((dbce_stats_partial_kernel<T, false>), grid, dim3(NT), 0, st, (const T*)logits, targets, (float*)workspace, S, L, ch);
    });
    hipLaunchKernelGGL(dbce_stats_final_kernel, dim3(1), dim3(64), 0, st, (const float*)workspace, stats, (int)(B * ch));
    UCF_LAUNCH_CHECK("ucfvit_dice_bce_stats");
    return UCFVIT_OK;
}

extern "C" int ucfvit_dice_bce_from_stats(const void* logits, const float* targets, const float* stats, float* loss, float* dlogits, int64_t B,
                                          int64_t C, int64_t S, float weight, float smooth, float grad_scale, const float* grad_scale_dev,
                                          int dtype, void* stream) {
    if (int rc = dbce_check("ucfvit_dice_bce_from_stats", logits, targets, B, C, S, dtype)) return rc;
    UCF_CHECK_ARG(stats && (loss || dlogits), "ucfvit_dice_bce_from_stats: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const double n = (double)B * (double)(C - 1) * (double)S;
    if (loss) hipLaunchKernelGGL(dbce_loss_kernel, dim3(1), dim3(1), 0, st, stats, loss, weight, smooth, n);
    if (dlogits) {
        const int64_t CS = C * S;
        const bool vec = dbce_vec(logits, dlogits, targets, S, dtype);
        SAP_DISPATCH(T, {
            const int V = vec ? Vec16<T>::N : 1;
            int64_t gx = (CS / V + NT - 1) / NT, cap = (4096 + B - 1) / B;
            if (gx > cap) gx = cap;
            const dim3 grid((unsigned)(gx < 1 ? 1 : gx), (unsigned)B);
            if (vec)
                hipLaunchKernelGGL((dbce_grad_kernel<T, true>), grid, dim3(NT), 0, st, (const T*)logits, targets, stats, (float*)dlogits, S, CS, weight,
                                   smooth, (float)n, grad_scale, grad_scale_dev);
            else
                hipLaunchKernelGGL((dbce_grad_kernel<T, false>), grid, dim3(NT), 0, st, (const T*)logits, targets, stats, (float*)dlogits, S, CS, weight,
                                   smooth, (float)n, grad_scale, grad_scale_dev);
        });
    }
    UCF_LAUNCH_CHECK("ucfvit_dice_bce_from_stats");
    return UCFVIT_OK;
}
