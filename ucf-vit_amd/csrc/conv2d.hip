// Convolutions of the 2-D UNETR decoder (reference: src/UCF_VIT/simple/arch.py:794-797 builds the monai blocks with spatial_dims = 2 when
// twoD is set) for gfx950: 3x3 (stride 1, zero padding 1) as an implicit GEMM on v_mfma_f32_16x16x32_bf16, its weight gradient, and the data
// mover of the 2x2 stride-2 transposed convolution.  The pointwise layers of the 2-D decoder are geometry-free and run on the 1x1x1 kernels
// of csrc/conv3d.hip; this file holds only the neighbourhood arithmetic in the plane.  The oracle is torch.nn.functional.conv2d /
// conv_transpose2d on the same bf16-rounded operands (tests/test_conv2d_ops.py compares per element against float64).
//
// Layout: activations are CHANNELS-LAST bf16, [B][X][Y][C] (= torch.channels_last memory of a [B, C, X, Y] tensor): a pixel's channel vector
// is contiguous, an MFMA operand fragment (8 channels of one pixel) is one 16-byte load, a 16 pixel x 16 channel output block one contiguous
// 512-byte run.  Weights arrive pre-packed per 32-wide contraction step, the 3-D definition with 9 taps (UCF_VIT/_hip/conv.py:
// pack_conv2d_weight): step ts of channel chunk cc holds, for every output channel, 32 values over (tap, ci), tap = dx 3 + dy.
//
// forward / data gradient (same kernel; the data gradient is the convolution of dy with the flipped, transposed weights):
//   one workgroup = TX rows x 16 pixels x 16 NB output channels.  The (TX + 2) x 18 halo of the input chunk (<= 32 channels) is staged in
//   LDS once and read 9 times (once per tap) as the B operand; the weight slab of the chunk is staged next to it (A operand).
//   D[co][pixel] -> each lane holds 4 consecutive output channels of one pixel: 8-byte stores, 512 B contiguous per 16 x 16 block.
//   algorithmic HBM bytes per output pixel: 2 Cin (read once; the halo re-reads are L2 hits) + 2 Cout.
// weight gradient: dW[tap][co][ci] = sum_p dy[p][co] x[p + tap][ci]: contraction over pixels, so both operands come out of their
//   pixel-major LDS images through ds_read_b64_tr_b16 (hardware transpose).  A workgroup walks a range of 8 x 32 pixel tiles with the 9 x
//   (Cout/16) x (Cin/16) accumulator blocks spread over its 4 waves (taps w, w + 4, w + 8), and writes ONE partial per workgroup; the
//   partials are folded by ucfvit_reduce_rows in a fixed order (deterministic, no atomics).
#include "common.h"
#include "conv2d_route.h"

namespace {

constexpr int CT = 256;
typedef bf16x8 frag_t;

__device__ __forceinline__ f32x4 mma(const frag_t& a, const frag_t& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

struct Conv2dGeo {
    int B, X, Y, Cin, Cout;
    int tx, ty;          // tile counts along x, y
    int tiles;           // B tx ty
    int ldy, cout_store; // forward: output row stride (elements) and number of channels written (<= Cout)
    int accumulate;      // forward: y += result (the second data gradient of an input two layers consume)
};

// 16-byte load of 8 channels of pixel (b, gx, gy), zero outside the image (= the convolution's zero padding)
__device__ __forceinline__ u32x4 load_pixel(const bf16* __restrict__ x, const Conv2dGeo& g, int b, int gx, int gy, int C, int ch) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if ((unsigned)gx < (unsigned)g.X && (unsigned)gy < (unsigned)g.Y)
        v = *reinterpret_cast<const u32x4*>(x + (((int64_t)b * g.X + gx) * g.Y + gy) * C + ch);
    return v;
}

__device__ __forceinline__ void decode_tile(const Conv2dGeo& g, int t, int& b, int& ix, int& iy) {
    iy = t % g.ty;
    t /= g.ty;
    ix = t % g.tx;
    b = t / g.tx;
}

// ---------------------------------------------------------------------------------------------------------------- forward / data gradient
template <int CPC, int NB, int TX, typename OutT>
__global__ __launch_bounds__(CT) void conv2d_fwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ wp, const float* __restrict__ bias,
                                                        OutT* __restrict__ y, Conv2dGeo g) {
    constexpr int NT = CONV2D_TAPS, NTS = conv2d_steps(CPC), VS = CPC * 2, PPV = VS / 16;
    constexpr int HX = TX + 2, HY = CONV2D_TY + 2;
    constexpr int HALO_BYTES = HX * HY * VS;
    constexpr int CB = 16 * NB;                     // output channels per workgroup
    constexpr int RPW = TX / 4;                     // 16-pixel rows per wave
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* halo = smem;                              // [HX][HY][CPC] bf16
    char* wl = smem + HALO_BYTES;                   // [NTS][CB][32] bf16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    int b, ix, iy;
    decode_tile(g, xcd_remap(blockIdx.x, gridDim.x), b, ix, iy);
    const int x0 = ix * TX, y0 = iy * CONV2D_TY;
    const int co0 = blockIdx.y * CB;
    f32x4 acc[RPW][NB];
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[r][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nchunks = g.Cin / CPC;
    for (int cc = 0; cc < nchunks; ++cc) {
        if (cc) __syncthreads();
        for (int p = tid; p < HX * HY * PPV; p += CT) {
            const int hv = p / PPV, piece = p % PPV;
            const int hy = hv % HY, hx = hv / HY;
            *reinterpret_cast<u32x4*>(halo + hv * VS + piece * 16) = load_pixel(x, g, b, x0 + hx - 1, y0 + hy - 1, g.Cin, cc * CPC + piece * 8);
        }
        for (int p = tid; p < NTS * CB * 4; p += CT) {
            const int piece = p & 3, row = (p >> 2) % CB, ts = (p >> 2) / CB;
            *reinterpret_cast<u32x4*>(wl + p * 16) =
                *reinterpret_cast<const u32x4*>(wp + ((int64_t)(cc * NTS + ts) * g.Cout + co0 + row) * 32 + piece * 8);
        }
        __syncthreads();
#pragma unroll
        for (int ts = 0; ts < NTS; ++ts) {
            frag_t a[NB];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) a[nb] = *reinterpret_cast<const frag_t*>(wl + ((ts * CB + nb * 16 + li) * 64 + lg * 16));
            int tap, chb;                                       // the tap and channel byte offset this lane's 8 contraction values cover
            if (CPC == 32) {
                tap = ts;
                chb = lg * 16;
            } else if (CPC == 16) {
                tap = 2 * ts + (lg >> 1);
                chb = (lg & 1) * 16;
            } else {
                tap = 4 * ts + lg;
                chb = 0;
            }
            if (tap > NT - 1) tap = NT - 1;                     // padding step: its weights are zero, read any staged pixel
            const int dx = tap / 3, dy = tap % 3;
            const int boff = (dx * HY + dy + li) * VS + chb;
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const frag_t bf = *reinterpret_cast<const frag_t*>(halo + boff + (wave * RPW + r) * HY * VS);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[r][nb] = mma(a[nb], bf, acc[r][nb]);
            }
        }
    }
    // D[co = 4 lg + e][pixel = li]: 4 consecutive channels of one pixel per lane
    const bool vec_ok = (g.ldy & 3) == 0;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int gx = x0 + wave * RPW + r, gy = y0 + li;
        if (gx < g.X && gy < g.Y) {
            OutT* yp = y + (((int64_t)b * g.X + gx) * g.Y + gy) * g.ldy;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int c = co0 + nb * 16 + lg * 4;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[r][nb][e] + (bias ? bias[c + e] : 0.f);
                if (c + 4 <= g.cout_store && vec_ok) {
                    Vec4<OutT> o;
                    if (g.accumulate) {
                        o = *reinterpret_cast<const Vec4<OutT>*>(yp + c);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += o.get(e);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) o.set(e, v[e]);
                    *reinterpret_cast<Vec4<OutT>*>(yp + c) = o;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < g.cout_store) yp[c + e] = from_f32<OutT>(v[e] + (g.accumulate ? to_f32<OutT>(yp[c + e]) : 0.f));
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- weight gradient
// wave w owns taps w, w + 4, w + 8 (3, 2, 2, 2 accumulator sets) and walks every row of the tile; ONE partial per workgroup
template <int CPC, int MB>
__global__ __launch_bounds__(CT) void conv2d_wgrad_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy, float* __restrict__ part,
                                                          Conv2dGeo g, int tiles_per_wg) {
    constexpr int NT = CONV2D_TAPS, VS = CPC * 2, PPV = VS / 16;
    constexpr int TX = CONV2D_WGRAD_TX, TY = CONV2D_WGRAD_TY, HX = TX + 2, HY = TY + 2;
    constexpr int NBK = CPC >= 16 ? CPC / 16 : 1;
    constexpr int VSD = 32 * MB;                    // bytes per pixel of the dy image (16 MB channels)
    constexpr int DY_BYTES = TX * TY * VSD;
    constexpr int WTAPS = CONV2D_WGRAD_WTAPS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* dyt = smem;                               // [TX][TY][16 MB] bf16
    char* halo = smem + DY_BYTES;                   // [HX][HY][CPC] bf16 (+ 64 bytes the CPC 8 transposed reads run into)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4, q = li >> 2, p4 = li & 3;
    const int cin_chunks = g.Cin / CPC;
    const int cib = blockIdx.y % cin_chunks, cob = blockIdx.y / cin_chunks;
    f32x4 acc[WTAPS][MB][NBK];
#pragma unroll
    for (int k = 0; k < WTAPS; ++k)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int nb = 0; nb < NBK; ++nb) acc[k][mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int t_lo = blockIdx.x * tiles_per_wg, t_hi = min(g.tiles, t_lo + tiles_per_wg);
    // software pipeline over the workgroup's tiles: the dy tile and the x halo of tile t + 1 are fetched into registers while tile t is
    // multiplied out of LDS.  A thread's pieces have fixed tile-local coordinates: (xl, yl, piece) packed 8 bits each, -1 = no piece.
    constexpr int DPV = VSD / 16;
    constexpr int NPD = (TX * TY * DPV + CT - 1) / CT, NPH = (HX * HY * PPV + CT - 1) / CT;
    int dyc[NPD], hc[NPH];
#pragma unroll
    for (int i = 0; i < NPD; ++i) {
        const int p = tid + i * CT, v = p / DPV, piece = p % DPV;
        dyc[i] = p < TX * TY * DPV ? ((v / TY) | ((v % TY) << 8) | (piece << 24)) : -1;
    }
#pragma unroll
    for (int i = 0; i < NPH; ++i) {
        const int p = tid + i * CT, hv = p / PPV, piece = p % PPV;
        hc[i] = p < HX * HY * PPV ? ((hv / HY) | ((hv % HY) << 8) | (piece << 24)) : -1;
    }
    u32x4 pd[NPD], ph[NPH];
    auto fetch = [&](int t) {
        int b, ix, iy;
        decode_tile(g, t, b, ix, iy);
        const int x0 = ix * TX, y0 = iy * TY;
#pragma unroll
        for (int i = 0; i < NPD; ++i) {
            const int c = dyc[i];
            pd[i] = c < 0 ? u32x4{0u, 0u, 0u, 0u} : load_pixel(dy, g, b, x0 + (c & 255), y0 + ((c >> 8) & 255), g.Cout, cob * 16 * MB + (c >> 24) * 8);
        }
#pragma unroll
        for (int i = 0; i < NPH; ++i) {
            const int c = hc[i];
            ph[i] = c < 0 ? u32x4{0u, 0u, 0u, 0u} : load_pixel(x, g, b, x0 + (c & 255) - 1, y0 + ((c >> 8) & 255) - 1, g.Cin, cib * CPC + (c >> 24) * 8);
        }
    };
    if (tid < 4) *reinterpret_cast<u32x4*>(halo + HX * HY * VS + tid * 16) = u32x4{0u, 0u, 0u, 0u};      // the run-over bytes: defined values
    if (t_lo < t_hi) fetch(t_lo);
    for (int t = t_lo; t < t_hi; ++t) {
#pragma unroll
        for (int i = 0; i < NPD; ++i)
            if (dyc[i] >= 0) *reinterpret_cast<u32x4*>(dyt + (tid + i * CT) * 16) = pd[i];        // piece p lives at byte 16 p of its image
#pragma unroll
        for (int i = 0; i < NPH; ++i)
            if (hc[i] >= 0) *reinterpret_cast<u32x4*>(halo + (tid + i * CT) * 16) = ph[i];
        __syncthreads();
        if (t + 1 < t_hi) fetch(t + 1);
        for (int xl = 0; xl < TX; ++xl) {
            frag_t a[MB];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const char* ap = dyt + (xl * TY + 8 * lg + q) * VSD + (mb * 16 + 4 * p4) * 2;
                const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(short4v, ap));
                const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(short4v, ap + 4 * VSD));
                const short8v rr = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                a[mb] = __builtin_bit_cast(frag_t, rr);
            }
#pragma unroll
            for (int k = 0; k < WTAPS; ++k) {
                const int tap = wave + 4 * k;
                if (tap < NT) {
                    const int dx = tap / 3, dyy = tap % 3;
                    const char* bp = halo + ((xl + dx) * HY + dyy + 8 * lg + q) * VS + 4 * p4 * 2;
#pragma unroll
                    for (int nb = 0; nb < NBK; ++nb) {
                        const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(short4v, bp + nb * 32));
                        const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(short4v, bp + nb * 32 + 4 * VS));
                        const short8v rr = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                        const frag_t bf = __builtin_bit_cast(frag_t, rr);
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb) acc[k][mb][nb] = mma(a[mb], bf, acc[k][mb][nb]);
                    }
                }
            }
        }
        __syncthreads();                                // every wave is done with these images before the next tile overwrites them
    }
    // partial [workgroup][blockIdx.y][tap][16 MB][16 NBK]; D[co = 4 lg + e][ci = li]
    constexpr int PB = 16 * MB * 16 * NBK;
    float* out = part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * NT * PB;
#pragma unroll
    for (int k = 0; k < WTAPS; ++k) {
        const int tap = wave + 4 * k;
        if (tap < NT) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int nb = 0; nb < NBK; ++nb)
#pragma unroll
                    for (int e = 0; e < 4; ++e) out[tap * PB + (mb * 16 + 4 * lg + e) * (16 * NBK) + nb * 16 + li] = acc[k][mb][nb][e];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- data mover
// depth-to-space of the 2x2 transposed convolution's pointwise output: cols [B Xi Yi][4 C] with the 4 = (dx, dy) -> out [B][2Xi][2Yi][C]
// (to_space = 1), or the inverse gather for the backward pass (to_space = 0).  16 bytes per thread step; C % 8 == 0.  The space tensor may be
// a channel slice of a wider channels-last buffer (row stride lds8 sixteen-byte units); with a skip the Cs / 8 vectors of the skip connection
// follow the C / 8 of the up-sampled map in every pixel row, so a whole row of the concatenation is written by consecutive lanes.  The row
// length cvt is a power of two (cvt_shift): pixel and vector index are a shift and a mask of the thread index.
__global__ __launch_bounds__(CT) void d2s2d_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst, int B, int Xi, int Yi, int C, int to_space,
                                                   int64_t lds8, const bf16* __restrict__ skip, int Cs, int cvt_shift) {
    const int cv = C / 8, cvt = 1 << cvt_shift;
    const unsigned npix = (unsigned)B * (2u * Xi) * (2u * Yi);
    const unsigned ppb = CT >> cvt_shift;                                  // pixels per workgroup step
    const int c = threadIdx.x & (cvt - 1);
    for (unsigned pix = blockIdx.x * ppb + (threadIdx.x >> cvt_shift); pix < npix; pix += gridDim.x * ppb) {
        const int64_t k = (int64_t)pix * lds8 + c;
        if (c >= cv) {                                          // skip half of the concatenation
            reinterpret_cast<u32x4*>(dst)[k] = reinterpret_cast<const u32x4*>(skip)[(int64_t)pix * (Cs / 8) + (c - cv)];
            continue;
        }
        unsigned r = pix;
        const unsigned yo = r % (2u * Yi);
        r /= 2u * Yi;
        const unsigned xo = r % (2u * Xi), b = r / (2u * Xi);
        const int64_t pin = ((int64_t)b * Xi + (xo >> 1)) * Yi + (yo >> 1);
        const int64_t j = (pin * 4 + ((xo & 1) * 2 + (yo & 1))) * cv + c;
        if (to_space)
            reinterpret_cast<u32x4*>(dst)[k] = reinterpret_cast<const u32x4*>(src)[j];
        else
            reinterpret_cast<u32x4*>(dst)[j] = reinterpret_cast<const u32x4*>(src)[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
int conv2d_check(const char* name, const void* x, const void* w, const void* y, int64_t B, int64_t X, int64_t Y, int64_t Cin, int64_t Cout) {
    UCF_CHECK_ARG(x && w && y, "%s: null pointer", name);
    UCF_CHECK_ARG(B > 0 && X > 0 && Y > 0, "%s: empty image", name);
    UCF_CHECK_ARG(B * X * Y < (1ll << 31), "%s: more than 2^31 pixels", name);
    UCF_CHECK_ARG(conv_cin_ok(Cin), "%s: Cin must be 8, 16 or a multiple of 32 (got %lld)", name, (long long)Cin);
    UCF_CHECK_ARG(conv_cout_ok(Cout), "%s: Cout must be a multiple of 16 (got %lld)", name, (long long)Cout);
    UCF_CHECK_ARG(ucf_is_aligned16(x) && ucf_is_aligned16(w) && ucf_is_aligned16(y), "%s: operands must be 16-byte aligned", name);
    return UCFVIT_OK;
}

// the one launch: the kernel's dynamic LDS limit raised once, the launch, its check
template <auto Kernel, typename... Args>
int conv2d_launch(const char* who, int64_t gx, int64_t gy, int smem, hipStream_t s, Args... args) {
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        attr_done = true;
    }
    hipLaunchKernelGGL(Kernel, dim3((unsigned)gx, (unsigned)gy), dim3(CT), smem, s, args...);
    UCF_LAUNCH_CHECK(who);
    return UCFVIT_OK;
}

// CONV2D_SWITCH_CPC: the runtime Cin of a route as the compile-time CPC_ of the statement it is given
#define CONV2D_SWITCH_CPC(CIN, ...)                                      \
    do {                                                                 \
        if ((CIN) == 8) { constexpr int CPC_ = 8; __VA_ARGS__ }          \
        else if ((CIN) == 16) { constexpr int CPC_ = 16; __VA_ARGS__ }   \
        else { constexpr int CPC_ = 32; __VA_ARGS__ }                    \
    } while (0)

// the route's nb as a template argument; the tile height is the one conv2d_fwd_route names for it
template <int CPC, typename OutT>
int run_fwd2d(const Conv2dFwdRoute& r, const bf16* x, const bf16* wp, const float* bias, OutT* y, const Conv2dGeo& g, hipStream_t s) {
    static_assert(conv2d_fwd_smem(CPC, 4, 8) <= 64 * 1024 && conv2d_fwd_smem(CPC, 2, 16) <= 64 * 1024, "LDS budget");
    const char* who = "ucfvit_conv2d_fwd";
    if (r.nb == 4) return conv2d_launch<conv2d_fwd_kernel<CPC, 4, 8, OutT>>(who, r.gx, r.gy, r.smem, s, x, wp, bias, y, g);
    if (r.nb == 2) return conv2d_launch<conv2d_fwd_kernel<CPC, 2, 16, OutT>>(who, r.gx, r.gy, r.smem, s, x, wp, bias, y, g);
    return conv2d_launch<conv2d_fwd_kernel<CPC, 1, 16, OutT>>(who, r.gx, r.gy, r.smem, s, x, wp, bias, y, g);
}

// text into out, cut to cap - 1 characters and terminated; returns the length of the whole text
int conv2d_text(const char* text, char* out, int64_t cap) {
    int n = 0;
    for (; text[n]; ++n)
        if (n < cap - 1) out[n] = text[n];
    if (cap > 0) out[n < cap - 1 ? n : cap - 1] = 0;
    return n;
}

}  // namespace

// x [B][X][Y][Cin] bf16, w_packed [Cin/CPC][NTS][Cout][32] bf16, bias fp32 [Cout] or NULL -> y[pixel * ldy + co] for co < cout_store
extern "C" int ucfvit_conv2d_fwd(const void* x, const void* w_packed, const float* bias, void* y, int64_t B, int64_t X, int64_t Y, int64_t Cin,
                                 int64_t Cout, int64_t ldy, int64_t cout_store, int out_dtype, int accumulate, void* stream) {
    if (int rc = conv2d_check("ucfvit_conv2d_fwd", x, w_packed, y, B, X, Y, Cin, Cout)) return rc;
    UCF_CHECK_ARG(cout_store > 0 && cout_store <= Cout && ldy >= cout_store && ldy < (1ll << 31), "ucfvit_conv2d_fwd: need 0 < cout_store <= Cout, ldy >= cout_store");
    UCF_CHECK_ARG(out_dtype == UCFVIT_BF16 || out_dtype == UCFVIT_F32, "ucfvit_conv2d_fwd: bad out_dtype %d", out_dtype);
    const Conv2dFwdRoute r = conv2d_fwd_route(B, X, Y, Cin, Cout);
    UCF_CHECK_ARG(!r.grid_too_large, "ucfvit_conv2d_fwd: grid too large");
    const Conv2dGeo g{(int)B, (int)X, (int)Y, (int)Cin, (int)Cout, r.tx, r.ty, (int)r.gx, (int)ldy, (int)cout_store, accumulate ? 1 : 0};
    hipStream_t s = (hipStream_t)stream;
    CONV2D_SWITCH_CPC(Cin, {
        if (out_dtype == UCFVIT_BF16) return run_fwd2d<CPC_, bf16>(r, (const bf16*)x, (const bf16*)w_packed, bias, (bf16*)y, g, s);
        return run_fwd2d<CPC_, float>(r, (const bf16*)x, (const bf16*)w_packed, bias, (float*)y, g, s);
    });
    return UCFVIT_OK;
}

// number of fp32 values of the packed weight gradient [Cout/(16 MB)][Cin/CPC][9][16 MB][16 NBK] and bytes of scratch for the partials
// (0: a shape the kernels are not instantiated for)
extern "C" int64_t ucfvit_conv2d_wgrad_size(int64_t Cin, int64_t Cout) {
    return conv2d_shape_ok(Cin, Cout) ? conv2d_wgrad_route(1, 1, 1, Cin, Cout).n_out : 0;
}
extern "C" int64_t ucfvit_conv2d_wgrad_workspace(int64_t B, int64_t X, int64_t Y, int64_t Cin, int64_t Cout) {
    return (conv2d_shape_ok(Cin, Cout) && B > 0 && X > 0 && Y > 0 && B * X * Y < (1ll << 31)) ? conv2d_wgrad_route(B, X, Y, Cin, Cout).workspace_bytes : 0;
}
// x [..][Cin], dy [..][Cout] bf16 -> dw_packed fp32 (layout above; UCF_VIT/_hip/conv.py:unpack_conv2d_wgrad turns it into [Cout][Cin][3][3])
extern "C" int ucfvit_conv2d_wgrad(const void* x, const void* dy, float* dw_packed, void* workspace, int64_t B, int64_t X, int64_t Y, int64_t Cin,
                                   int64_t Cout, void* stream) {
    if (int rc = conv2d_check("ucfvit_conv2d_wgrad", x, dy, dw_packed, B, X, Y, Cin, Cout)) return rc;
    UCF_CHECK_ARG(workspace, "ucfvit_conv2d_wgrad: null workspace");
    const Conv2dWgradRoute r = conv2d_wgrad_route(B, X, Y, Cin, Cout);
    const Conv2dGeo g{(int)B, (int)X, (int)Y, (int)Cin, (int)Cout, r.tx, r.ty, r.tiles, 0, 0, 0};
    hipStream_t s = (hipStream_t)stream;
    const bf16 *xb = (const bf16*)x, *dyb = (const bf16*)dy;
    float* ws = (float*)workspace;
    const char* who = "ucfvit_conv2d_wgrad";
    CONV2D_SWITCH_CPC(Cin, {
        static_assert(conv2d_wgrad_smem(CPC_, 2) <= 64 * 1024, "LDS budget");
        if (int rc = r.mb == 2 ? conv2d_launch<conv2d_wgrad_kernel<CPC_, 2>>(who, r.n_wg, r.gy, r.smem, s, xb, dyb, ws, g, r.tiles_per_wg)
                               : conv2d_launch<conv2d_wgrad_kernel<CPC_, 1>>(who, r.n_wg, r.gy, r.smem, s, xb, dyb, ws, g, r.tiles_per_wg))
            return rc;
    });
    return ucfvit_reduce_rows(ws, dw_packed, (int64_t)r.n_wg, r.n_out, 0, s);
}

// the route of a launch as text (host only): pass 0 = ucfvit_conv2d_fwd, 1 = ucfvit_conv2d_wgrad
extern "C" int ucfvit_conv2d_route(int pass, int64_t B, int64_t X, int64_t Y, int64_t Cin, int64_t Cout, int has_bias, int out_dtype, int64_t ldy,
                                   int64_t cout_store, char* out, int64_t cap) {
    UCF_CHECK_ARG(out || cap <= 0, "ucfvit_conv2d_route: null buffer");
    UCF_CHECK_ARG(pass == 0 || pass == 1, "ucfvit_conv2d_route: pass must be 0 or 1");
    UCF_CHECK_ARG(B > 0 && X > 0 && Y > 0 && B * X * Y < (1ll << 31) && conv2d_shape_ok(Cin, Cout) &&
                      (pass == 1 || (cout_store > 0 && cout_store <= Cout && ldy >= cout_store && ldy < (1ll << 31) &&
                                     (out_dtype == UCFVIT_BF16 || out_dtype == UCFVIT_F32))),
                  "ucfvit_conv2d_route: a shape the convolution entry points refuse");
    char text[160];
    if (pass == 1) {
        const Conv2dWgradRoute w = conv2d_wgrad_route(B, X, Y, Cin, Cout);
        snprintf(text, sizeof text, "wgrad2d cpc%d mb%d n_wg%d tiles_per_wg%d n_out%lld", w.cpc, w.mb, w.n_wg, w.tiles_per_wg, (long long)w.n_out);
        return conv2d_text(text, out, cap);
    }
    const Conv2dFwdRoute r = conv2d_fwd_route(B, X, Y, Cin, Cout);
    snprintf(text, sizeof text, "tile2d cpc%d nb%d %dx%d %s grid%lldx%lld", r.cpc, r.nb, r.TX, CONV2D_TY, out_dtype == UCFVIT_BF16 ? "bf16" : "f32",
             (long long)r.gx, (long long)r.gy);
    return conv2d_text(text, out, cap);
}

// to_space = 1: cols [B Xi Yi][4 C] -> space[pixel * ld_space + c] over [B][2Xi][2Yi] pixels;  to_space = 0: the inverse.  bf16, C % 8 == 0,
// ld_space % 8 == 0 (ld_space = C: a dense tensor; larger: a channel slice of a wider channels-last buffer, pointer at the slice's first channel).
// skip (to_space = 1 only, may be NULL): dense [B][2Xi][2Yi][Cs] map copied behind the C channels of every pixel row in the same pass
// (ld_space >= C + Cs): the concatenation (up-sampled, skip) of UnetrUpBlock written as whole rows.
extern "C" int ucfvit_depth_to_space2_2d(const void* src, void* dst, int64_t B, int64_t Xi, int64_t Yi, int64_t C, int64_t ld_space, int to_space,
                                         const void* skip, int64_t Cs, void* stream) {
    UCF_CHECK_ARG(src && dst && B > 0 && Xi > 0 && Yi > 0 && C > 0 && C % 8 == 0, "ucfvit_depth_to_space2_2d: bad arguments");
    UCF_CHECK_ARG(ld_space >= C && ld_space % 8 == 0, "ucfvit_depth_to_space2_2d: ld_space must be a multiple of 8 and >= C");
    UCF_CHECK_ARG(ucf_is_aligned16(src) && ucf_is_aligned16(dst), "ucfvit_depth_to_space2_2d: operands must be 16-byte aligned");
    if (skip) UCF_CHECK_ARG(to_space == 1 && Cs > 0 && Cs % 8 == 0 && ld_space >= C + Cs && ucf_is_aligned16(skip), "ucfvit_depth_to_space2_2d: bad skip operand");
    const int64_t cvt = (C + (skip ? Cs : 0)) / 8;                           // 16-byte vectors per pixel row handled by this launch
    UCF_CHECK_ARG(cvt <= CT && (cvt & (cvt - 1)) == 0, "ucfvit_depth_to_space2_2d: (C + Cs) / 8 must be a power of two <= 256 (got %lld)", (long long)cvt);
    UCF_CHECK_ARG(B * Xi * Yi * 4 < (1ll << 32), "ucfvit_depth_to_space2_2d: more than 2^32 output pixels");
    int shift = 0;
    while ((1ll << shift) < cvt) ++shift;
    const int64_t total = B * Xi * Yi * 4 * cvt;                             // 16-byte pieces
    int64_t blocks = (total + CT - 1) / CT;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(d2s2d_kernel, dim3((unsigned)blocks), dim3(CT), 0, (hipStream_t)stream, (const bf16*)src, (bf16*)dst, (int)B, (int)Xi, (int)Yi,
                       (int)C, to_space, ld_space / 8, (const bf16*)skip, (int)Cs, shift);
    UCF_LAUNCH_CHECK("ucfvit_depth_to_space2_2d");
    return UCFVIT_OK;
}
