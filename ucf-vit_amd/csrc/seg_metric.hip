// Segmentation tail of the UNETR path for gfx950: the argmax label map of the class logits and every count a Dice accuracy needs, in ONE
// streaming pass over logits and labels (reference: training_scripts/train_unetr_simple.py:399-401,453-460 and inference_unetr_simple.py:
// torch.argmax -> one_hot of prediction and label -> monai DiceMetric, which at 512 x 512 x 128 materialises an fp32 copy of the logits, an
// int64 argmax map, two one-hot tensors and their products).  Per batch element b and class c
//     TP[c] = #{argmax == c and label == c},  PRED[c] = #{argmax == c},  LAB[c] = #{label == c}
// are integers, so any summation order gives the same bits: there is no floating point behind a count and no atomic.
//
// argmax is torch.argmax(dim = 1): the FIRST maximal class wins a tie, a NaN counts as maximal and the first NaN wins, +-inf are ordinary
// values.  A label outside [0, n) adds to no LAB and no TP entry; its voxel is still predicted and counted in PRED (the reference's one_hot
// would raise, which needs a host synchronisation).
//
// Two stages, as dice_partial / dice_final of csrc/unetr_decoder.hip: a grid over (chunk of SEG_CHUNK voxels, batch element) whose
// workgroups write int32 partial counts, then one small kernel that folds the partials into int64.  A thread counts at most
// SEG_CHUNK / NT = 64 voxels of a chunk, so its 3 x 8 counters are BYTES of three 64-bit registers (class c in bits 8c .. 8c + 7); they
// are widened to 16-bit fields for the wave butterfly (<= 64 x 64) and the fold of the four waves (<= 16384).
//
// Three stage-one kernels; seg_route picks one per call on the host:
//   cl      channels-last (stride_c == 1, stride_s == ld >= n; the HIP decoder's logits): a lane loads the NV >= n classes of ONE voxel as
//           one vector (consecutive lanes take consecutive voxels, so a wave's load is one contiguous run of rows); the four lanes of a quad
//           merge their prediction bytes into a word, a wave takes 4 x 64 voxels per step and every lane stores one such word.
//   ncs     N C (D) H W (stride_s == 1): a lane takes SEG_VPT = 8 consecutive voxels, 16-byte loads per class and for the labels, and stores
//           its 8 predictions as one 8-byte word.
//   scalar  any other strides, a base or stride that breaks the alignment of those vectors: one voxel per lane, element loads, byte stores.
// The cl and ncs kernels run the voxels behind the last whole step of a chunk through the same per-voxel code as the scalar kernel.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int MAXC = 8;
constexpr int SEG_CHUNK = 16384;        // voxels of a batch element per workgroup
constexpr int SEG_VPT = 8;              // ncs: consecutive voxels per lane and step
constexpr int SEG_CL_STEP = 4 * NT;     // cl: voxels per workgroup and step (a wave: 4 rounds of 64)
constexpr int SEG_Q = 3;                // TP, PRED, LAB
static_assert(SEG_CHUNK / NT <= 255, "a thread's counters are bytes");
static_assert(SEG_CHUNK % (NT * SEG_VPT) == 0 && SEG_CHUNK % SEG_CL_STEP == 0, "a chunk is a whole number of steps of either vector kernel");
static_assert(SEG_CHUNK <= 65535 && NT == 256, "the workgroup fold adds four 16-bit wave sums of at most 64 x 64 each");

typedef __attribute__((ext_vector_type(2))) long long i64x2;

template <typename T> __device__ __forceinline__ float ldf(const T* p, int64_t i) { return to_f32<T>(p[i]); }

// torch.argmax's order: z replaces the running best when it is larger or NaN, unless the best is NaN already
__device__ __forceinline__ void amax_step(float& best, int& idx, float z, int c) {
    const bool take = !(z <= best) && best == best;
    best = take ? z : best;
    idx = take ? c : idx;
}

struct Cnt {
    unsigned long long tp = 0, pr = 0, lb = 0;
};
__device__ __forceinline__ void tally(Cnt& k, int idx, int64_t lab, int n) {
    k.pr += 1ull << (idx * 8);
    const unsigned long long one = (uint64_t)lab < (uint64_t)n ? 1ull << (((int)lab & 7) * 8) : 0ull;
    k.lb += one;
    k.tp += lab == (int64_t)idx ? one : 0ull;
}

// one voxel through element loads (any strides); pred as a byte
template <typename T>
__device__ __forceinline__ void voxel_scalar(const T* __restrict__ lb, const int64_t* __restrict__ yb, uint8_t* __restrict__ pb, int64_t i, int n,
                                             int64_t sc, int64_t ss, Cnt& k) {
    float best = ldf(lb, i * ss);
    int idx = 0;
#pragma unroll
    for (int c = 1; c < MAXC; ++c)
        if (c < n) amax_step(best, idx, ldf(lb, c * sc + i * ss), c);
    tally(k, idx, yb[i], n);
    if (pb) pb[i] = (uint8_t)idx;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}
// the workgroup's counts of its chunk -> out[q * 8 + c] (int32).  red: (NT / 64) x 12 words of LDS
__device__ __forceinline__ void cnt_store(const Cnt& k, int32_t* __restrict__ out, unsigned* red) {
    constexpr unsigned long long M = 0x00FF00FF00FF00FFull;
    const unsigned long long q3[SEG_Q] = {k.tp, k.pr, k.lb};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < SEG_Q; ++q) {
        const unsigned long long ev = q3[q] & M, od = (q3[q] >> 8) & M;          // 16-bit fields: classes 0 2 4 6 and 1 3 5 7
        const unsigned w[4] = {(unsigned)ev, (unsigned)(ev >> 32), (unsigned)od, (unsigned)(od >> 32)};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned s = wave_sum_u32(w[j]);
            if (lane == 0) red[wave * 12 + q * 4 + j] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x < SEG_Q * MAXC) {
        const int q = threadIdx.x >> 3, c = threadIdx.x & 7;
        const int j = q * 4 + (c & 1) * 2 + (c >> 2), sh = ((c >> 1) & 1) * 16;
        int32_t t = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) t += (int32_t)((red[w * 12 + j] >> sh) & 0xFFFFu);
        out[threadIdx.x] = t;
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void seg_partial_scalar(const T* __restrict__ logits, const int64_t* __restrict__ labels, uint8_t* __restrict__ pred,
                                                         int32_t* __restrict__ part, int n, int64_t S, int chunks, int64_t sb, int64_t sc, int64_t ss) {
    __shared__ unsigned red[(NT / 64) * 12];
    const int64_t b = blockIdx.y;
    const T* lb = logits + b * sb;
    const int64_t* yb = labels + b * S;
    uint8_t* pb = pred ? pred + b * S : nullptr;
    const int64_t lo = (int64_t)blockIdx.x * SEG_CHUNK, hi = min(S, lo + SEG_CHUNK);
    Cnt k;
    for (int64_t i = lo + threadIdx.x; i < hi; i += NT) voxel_scalar(lb, yb, pb, i, n, sc, ss, k);
    cnt_store(k, part + (b * chunks + blockIdx.x) * (SEG_Q * MAXC), red);
}

// NV elements of a channels-last voxel row as one load (two for 8 floats)
template <typename T, int NV> struct alignas(NV * sizeof(T) < 16 ? NV * sizeof(T) : 16) Row {
    T v[NV];
};

template <typename T, int NV>
__global__ __launch_bounds__(NT) void seg_partial_cl(const T* __restrict__ logits, const int64_t* __restrict__ labels, uint8_t* __restrict__ pred,
                                                     int32_t* __restrict__ part, int n, int64_t S, int chunks, int64_t sb, int64_t ld) {
    __shared__ unsigned red[(NT / 64) * 12];
    const int64_t b = blockIdx.y;
    const T* lb = logits + b * sb;
    const int64_t* yb = labels + b * S;
    uint8_t* pb = pred ? pred + b * S : nullptr;
    const int64_t lo = (int64_t)blockIdx.x * SEG_CHUNK, hi = min(S, lo + SEG_CHUNK);
    const int64_t vend = lo + (hi - lo) / SEG_CL_STEP * SEG_CL_STEP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, quad = lane & 3;
    Cnt k;
    for (int64_t base = lo + wave * 256; base < vend; base += SEG_CL_STEP) {
        unsigned word = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t i = base + r * 64 + lane;
            const Row<T, NV> row = *reinterpret_cast<const Row<T, NV>*>(lb + i * ld);
            float best = to_f32<T>(row.v[0]);
            int idx = 0;
#pragma unroll
            for (int c = 1; c < NV; ++c)
                if (c < n) amax_step(best, idx, to_f32<T>(row.v[c]), c);
            tally(k, idx, yb[i], n);
            unsigned x = (unsigned)idx << (quad * 8);                 // the quad's four predictions as one word, in all four lanes
            x |= (unsigned)__shfl_xor((int)x, 1, 64);
            x |= (unsigned)__shfl_xor((int)x, 2, 64);
            word = quad == r ? x : word;
        }
        // lane (4 j + q) keeps the word of round q: voxels base + 64 q + 4 j .. + 3
        if (pb) *reinterpret_cast<unsigned*>(pb + base + quad * 64 + (lane >> 2) * 4) = word;
    }
    for (int64_t i = vend + threadIdx.x; i < hi; i += NT) voxel_scalar(lb, yb, pb, i, n, (int64_t)1, ld, k);
    cnt_store(k, part + (b * chunks + blockIdx.x) * (SEG_Q * MAXC), red);
}

template <typename T>
__global__ __launch_bounds__(NT) void seg_partial_ncs(const T* __restrict__ logits, const int64_t* __restrict__ labels, uint8_t* __restrict__ pred,
                                                      int32_t* __restrict__ part, int n, int64_t S, int chunks, int64_t sb, int64_t sc) {
    __shared__ unsigned red[(NT / 64) * 12];
    constexpr int V = Vec16<T>::N;                     // 4 floats or 8 bf16 per 16-byte load
    const int64_t b = blockIdx.y;
    const T* lb = logits + b * sb;
    const int64_t* yb = labels + b * S;
    uint8_t* pb = pred ? pred + b * S : nullptr;
    const int64_t lo = (int64_t)blockIdx.x * SEG_CHUNK, hi = min(S, lo + SEG_CHUNK);
    const int64_t vend = lo + (hi - lo) / SEG_VPT * SEG_VPT;
    Cnt k;
    for (int64_t i = lo + (int64_t)threadIdx.x * SEG_VPT; i < vend; i += NT * SEG_VPT) {
        float best[SEG_VPT];
        int idx[SEG_VPT];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            if (c < n) {
#pragma unroll
                for (int h = 0; h < SEG_VPT / V; ++h) {
                    const Vec16<T> v = *reinterpret_cast<const Vec16<T>*>(lb + c * sc + i + h * V);
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        if (c == 0) {
                            best[h * V + e] = v.get(e);
                            idx[h * V + e] = 0;
                        } else {
                            amax_step(best[h * V + e], idx[h * V + e], v.get(e), c);
                        }
                    }
                }
            }
        }
        unsigned long long pk = 0;
#pragma unroll
        for (int h = 0; h < SEG_VPT / 2; ++h) {
            const i64x2 y = *reinterpret_cast<const i64x2*>(yb + i + 2 * h);
            tally(k, idx[2 * h], y[0], n);
            tally(k, idx[2 * h + 1], y[1], n);
            pk |= (unsigned long long)(idx[2 * h] | (idx[2 * h + 1] << 8)) << (16 * h);
        }
        if (pb) *reinterpret_cast<unsigned long long*>(pb + i) = pk;
    }
    for (int64_t i = vend + threadIdx.x; i < hi; i += NT) voxel_scalar(lb, yb, pb, i, n, sc, (int64_t)1, k);
    cnt_store(k, part + (b * chunks + blockIdx.x) * (SEG_Q * MAXC), red);
}

// stage two: one workgroup per batch element adds its chunks' int32 partials into counts [B][3][8] int64.  Thread (g, k) of 8 x 24 takes
// entry k of the chunks g, g + 8, ... (a chunk's 24 entries are one contiguous run), then thread k adds the eight group sums.
constexpr int FIN_G = 8;
__global__ __launch_bounds__(FIN_G * SEG_Q * MAXC) void seg_final(const int32_t* __restrict__ part, int64_t* __restrict__ counts, int chunks) {
    constexpr int K = SEG_Q * MAXC;
    __shared__ long long red[FIN_G * K];
    const int64_t b = blockIdx.x;
    const int k = threadIdx.x % K, g = threadIdx.x / K;
    long long s = 0;
    for (int ch = g; ch < chunks; ch += FIN_G) s += part[(b * chunks + ch) * K + k];
    red[g * K + k] = s;
    __syncthreads();
    if (g == 0) {
#pragma unroll
        for (int j = 1; j < FIN_G; ++j) s += red[j * K + k];
        counts[b * K + k] = s;
    }
}

inline int seg_chunks_of(int64_t S) { return (int)((S + SEG_CHUNK - 1) / SEG_CHUNK); }

// ---- the route of a call: every rule of the dispatch is written here once ---------------------------------------------------------------
enum SegKernel { SEG_SCALAR = 0, SEG_CL = 1, SEG_NCS = 2 };
struct SegRoute {
    SegKernel kernel;
    int nv;               // cl: elements per row load (2, 4 or 8)
};
inline bool seg_aligned(const void* p, int64_t bytes) { return (((uintptr_t)p) & (uintptr_t)(bytes - 1)) == 0; }
static SegRoute seg_route(const void* logits, const int64_t* labels, const uint8_t* pred, int64_t B, int64_t n, int64_t S, int64_t sb, int64_t sc,
                          int64_t ss, int dtype) {
    const int64_t es = dtype == UCFVIT_F32 ? 4 : 2;
    if (sc == 1 && ss >= n) {
        // a row load of NV elements, NV the power of two that holds the n classes, in pieces of at most 16 bytes: every row must start on a
        // piece boundary (then ld >= NV, so a load never leaves its row); the packed prediction words need 4-byte aligned rows of pred
        const int nv = n <= 2 ? 2 : n <= 4 ? 4 : 8;
        const int64_t vb = nv * es < 16 ? nv * es : 16;
        const bool ok = seg_aligned(logits, vb) && (ss * es) % vb == 0 && (sb * es) % vb == 0 && seg_aligned(labels, 8) &&
                        (!pred || (seg_aligned(pred, 4) && (B == 1 || S % 4 == 0)));
        if (ok) return {SEG_CL, nv};
    }
    if (ss == 1) {
        // 16-byte loads of every class row and of the labels, 8-byte stores of the predictions, at voxels that are multiples of SEG_VPT
        const bool ok = seg_aligned(logits, 16) && (sc * es) % 16 == 0 && (sb * es) % 16 == 0 && seg_aligned(labels, 16) &&
                        (!pred || seg_aligned(pred, 8)) && (B == 1 || S % SEG_VPT == 0);
        if (ok) return {SEG_NCS, 0};
    }
    return {SEG_SCALAR, 0};
}

static int seg_check(const char* name, const void* logits, const int64_t* labels, int64_t B, int64_t n, int64_t S, int64_t stride_b,
                     int64_t stride_c, int64_t stride_s, int dtype) {
    UCF_CHECK_ARG(logits && labels, "%s: null pointer", name);
    UCF_CHECK_ARG(B > 0 && B < 65536 && S > 0 && n >= 2 && n <= MAXC, "%s: need 2 <= classes <= %d, B in 1..65535", name, MAXC);
    UCF_CHECK_ARG(dtype == UCFVIT_F32 || dtype == UCFVIT_BF16, "%s: bad dtype %d", name, dtype);
    UCF_CHECK_ARG(stride_b > 0 && stride_c > 0 && stride_s > 0, "%s: strides must be positive", name);
    return UCFVIT_OK;
}

template <typename T>
static void seg_launch(SegRoute r, const void* logits, const int64_t* labels, uint8_t* pred, int32_t* part, int64_t B, int64_t n, int64_t S,
                       int64_t sb, int64_t sc, int64_t ss, hipStream_t s) {
    const int ch = seg_chunks_of(S);
    const dim3 grid(ch, (unsigned)B), block(NT);
    const T* lg = (const T*)logits;
    switch (r.kernel) {
    case SEG_CL:
        if (r.nv == 2) hipLaunchKernelGGL((seg_partial_cl<T, 2>), grid, block, 0, s, lg, labels, pred, part, (int)n, S, ch, sb, ss);
        else if (r.nv == 4) hipLaunchKernelGGL((seg_partial_cl<T, 4>), grid, block, 0, s, lg, labels, pred, part, (int)n, S, ch, sb, ss);
        else hipLaunchKernelGGL((seg_partial_cl<T, 8>), grid, block, 0, s, lg, labels, pred, part, (int)n, S, ch, sb, ss);
        break;
    case SEG_NCS:
        hipLaunchKernelGGL((seg_partial_ncs<T>), grid, block, 0, s, lg, labels, pred, part, (int)n, S, ch, sb, sc);
        break;
    default:
        hipLaunchKernelGGL((seg_partial_scalar<T>), grid, block, 0, s, lg, labels, pred, part, (int)n, S, ch, sb, sc, ss);
    }
}

}  // namespace

extern "C" int64_t ucfvit_seg_counts_workspace(int64_t B, int64_t S) {
    if (B <= 0 || S <= 0) return 0;
    return B * seg_chunks_of(S) * SEG_Q * MAXC * (int64_t)sizeof(int32_t);
}

extern "C" int ucfvit_seg_counts(const void* logits, const int64_t* labels, uint8_t* pred, int64_t* counts, int64_t B, int64_t n, int64_t S,
                                 int64_t stride_b, int64_t stride_c, int64_t stride_s, void* workspace, int dtype, void* stream) {
    if (int rc = seg_check("ucfvit_seg_counts", logits, labels, B, n, S, stride_b, stride_c, stride_s, dtype)) return rc;
    UCF_CHECK_ARG(counts && workspace, "ucfvit_seg_counts: null pointer");
    hipStream_t s = (hipStream_t)stream;
    int32_t* part = (int32_t*)workspace;
    const SegRoute r = seg_route(logits, labels, pred, B, n, S, stride_b, stride_c, stride_s, dtype);
    if (dtype == UCFVIT_F32) seg_launch<float>(r, logits, labels, pred, part, B, n, S, stride_b, stride_c, stride_s, s);
    else seg_launch<bf16>(r, logits, labels, pred, part, B, n, S, stride_b, stride_c, stride_s, s);
    hipLaunchKernelGGL(seg_final, dim3((unsigned)B), dim3(FIN_G * SEG_Q * MAXC), 0, s, part, counts, seg_chunks_of(S));
    UCF_LAUNCH_CHECK("ucfvit_seg_counts");
    return UCFVIT_OK;
}

extern "C" int ucfvit_seg_counts_route(const void* logits, const int64_t* labels, const uint8_t* pred, int64_t B, int64_t n, int64_t S,
                                       int64_t stride_b, int64_t stride_c, int64_t stride_s, int dtype, char* out, int64_t cap) {
    UCF_CHECK_ARG(out || cap <= 0, "ucfvit_seg_counts_route: null buffer");
    if (int rc = seg_check("ucfvit_seg_counts_route", logits, labels, B, n, S, stride_b, stride_c, stride_s, dtype)) return rc;
    const SegRoute r = seg_route(logits, labels, pred, B, n, S, stride_b, stride_c, stride_s, dtype);
    char text[64];
    if (r.kernel == SEG_CL) snprintf(text, sizeof text, "cl nv%d chunk%d step%d", r.nv, SEG_CHUNK, SEG_CL_STEP);
    else if (r.kernel == SEG_NCS) snprintf(text, sizeof text, "ncs vpt%d chunk%d step%d", SEG_VPT, SEG_CHUNK, NT * SEG_VPT);
    else snprintf(text, sizeof text, "scalar chunk%d", SEG_CHUNK);
    if (cap > 0) {
        strncpy(out, text, (size_t)cap - 1);
        out[cap - 1] = '\0';
    }
    return (int)strlen(text);
}
