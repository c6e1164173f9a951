// Align-corners trilinear resampling of channels-last bf16 maps for gfx950: nn.Upsample(size, mode='trilinear', align_corners=True) of the
// UNETR skip-connection decoder when the token grid times 16 is not the tile size (patch 4 / adaptive configs: 72^3 -> 64^3 before decoder2).
//
//   reference call sites: src/UCF_VIT/simple/arch.py:887-906, 942-943, 989-991 (self.upsample on dec1).  The oracle is
//   torch.nn.functional.interpolate(..., mode='trilinear', align_corners=True) on the same bf16 operand (tests/test_unetr_resample.py).
//
// Index and weight arithmetic is torch's, per axis and in fp32:  scale = (in - 1) / (out - 1) (0 when out == 1), src = scale * dst (rounded
// on its own, never contracted into the subtraction), i0 = (int) src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1.
//
// forward: a thread owns one 16-byte vector (8 channels) of one output voxel row; consecutive lanes cover a row, then consecutive voxels
//   along Z, so every wave stores whole contiguous rows (1 KiB per instruction) and its eight 16-byte tap loads per lane hit rows that are
//   contiguous along Z as well.  The 8 taps are summed in fp32 in torch's nesting order and rounded to bf16 once.  The output may be a
//   channel slice of a wider buffer (row stride ld_dst), and a dense skip map may be copied behind its channels in the same pass: the
//   concatenation (resampled, skip) of UnetrUpBlock is written as whole rows.
// backward: the transposed operator in gather form.  Along one axis the outputs whose stencil touches input i are a contiguous range
//   [first o with i0(o) >= i - 1, last o with i0(o) <= i] (i0 is monotone in o), found from an estimate and corrected with the exact
//   formula; a thread owns one 16-byte vector of one INPUT voxel and sums w_x w_y w_z dy over the product of the three ranges in a fixed
//   order (fp32, one rounding).  No atomics: the result is bitwise reproducible.
#include "common.h"

namespace {

constexpr int RT = 256;

// taps of output index o along an axis of `in` input samples
__device__ __forceinline__ void ac_taps(int o, int in, float scale, int& i0, int& i1, float& l1) {
    const float src = __fmul_rn(scale, (float)o);
    i0 = min((int)src, in - 1);                             // the min never binds for scale <= (in - 1) / (out - 1): a bounds guard only
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = src - (float)i0;                                   // exact: src in [i0, i0 + 1)
}

// weight of input i in output o along one axis (0 if o does not touch i; l0 + l1 where both taps are i)
__device__ __forceinline__ float ac_weight(int o, int i, int in, float scale) {
    int i0, i1;
    float l1;
    ac_taps(o, in, scale, i0, i1, l1);
    return (i0 == i ? 1.f - l1 : 0.f) + (i1 == i ? l1 : 0.f);
}

// min { o in [0, out) : i0(o) >= t }, out if there is none.  inv = (out - 1) / (in - 1) gives an estimate within a step or two of the answer;
// the exact formula settles it.
__device__ __forceinline__ int ac_first_ge(int t, int out, float scale, float inv) {
    if (t <= 0) return 0;
    if (scale == 0.f) return out;                           // out == 1 or in == 1: every i0 is 0
    int o = (int)fminf((float)t * inv, (float)out);
    while (o > 0 && (int)__fmul_rn(scale, (float)(o - 1)) >= t) --o;
    while (o < out && (int)__fmul_rn(scale, (float)o) < t) ++o;
    return o;
}

struct RsGeo {
    int Xi, Yi, Zi, Xo, Yo, Zo;
    float sx, sy, sz;                                       // align-corners scales (in - 1) / (out - 1)
    float ix, iy, iz;                                       // their inverses (backward estimate; unused where the scale is 0)
};

__global__ __launch_bounds__(RT) void resample_fwd_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, const bf16* __restrict__ skip, RsGeo g,
                                                          unsigned nvec, int cv, int cvt, int64_t ld8, int cs8) {
    const u32x4* __restrict__ x8 = reinterpret_cast<const u32x4*>(x);
    u32x4* __restrict__ y8 = reinterpret_cast<u32x4*>(y);
    for (unsigned t = blockIdx.x * RT + threadIdx.x; t < nvec; t += gridDim.x * RT) {
        const unsigned vox = t / (unsigned)cvt;
        const int c = (int)(t - vox * (unsigned)cvt);
        if (c >= cv) {                                                      // skip half of the concatenation
            y8[(int64_t)vox * ld8 + c] = reinterpret_cast<const u32x4*>(skip)[(int64_t)vox * cs8 + (c - cv)];
            continue;
        }
        unsigned r = vox;
        const int zo = (int)(r % (unsigned)g.Zo);
        r /= (unsigned)g.Zo;
        const int yo = (int)(r % (unsigned)g.Yo);
        r /= (unsigned)g.Yo;
        const int xo = (int)(r % (unsigned)g.Xo);
        const int b = (int)(r / (unsigned)g.Xo);
        int x0, x1, y0, y1, z0, z1;
        float lx, ly, lz;
        ac_taps(xo, g.Xi, g.sx, x0, x1, lx);
        ac_taps(yo, g.Yi, g.sy, y0, y1, ly);
        ac_taps(zo, g.Zi, g.sz, z0, z1, lz);
        const int64_t bx0 = ((int64_t)b * g.Xi + x0) * g.Yi, bx1 = ((int64_t)b * g.Xi + x1) * g.Yi;
        const int64_t r00 = (bx0 + y0) * g.Zi, r01 = (bx0 + y1) * g.Zi, r10 = (bx1 + y0) * g.Zi, r11 = (bx1 + y1) * g.Zi;
        bf16x8 v[8];
        const int64_t rows[4] = {r00, r01, r10, r11};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[2 * k] = __builtin_bit_cast(bf16x8, x8[(rows[k] + z0) * cv + c]);
            v[2 * k + 1] = __builtin_bit_cast(bf16x8, x8[(rows[k] + z1) * cv + c]);
        }
        const float mx = 1.f - lx, my = 1.f - ly, mz = 1.f - lz;
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float a00 = mz * (float)v[0][e] + lz * (float)v[1][e], a01 = mz * (float)v[2][e] + lz * (float)v[3][e];
            const float a10 = mz * (float)v[4][e] + lz * (float)v[5][e], a11 = mz * (float)v[6][e] + lz * (float)v[7][e];
            o[e] = (bf16)(mx * (my * a00 + ly * a01) + lx * (my * a10 + ly * a11));
        }
        y8[(int64_t)vox * ld8 + c] = __builtin_bit_cast(u32x4, o);
    }
}

__global__ __launch_bounds__(RT) void resample_bwd_kernel(const bf16* __restrict__ dy, bf16* __restrict__ dx, RsGeo g, unsigned nvec, int cv,
                                                          int64_t ld8) {
    const u32x4* __restrict__ dy8 = reinterpret_cast<const u32x4*>(dy);
    u32x4* __restrict__ dx8 = reinterpret_cast<u32x4*>(dx);
    for (unsigned t = blockIdx.x * RT + threadIdx.x; t < nvec; t += gridDim.x * RT) {
        const unsigned vox = t / (unsigned)cv;
        const int c = (int)(t - vox * (unsigned)cv);
        unsigned r = vox;
        const int zi = (int)(r % (unsigned)g.Zi);
        r /= (unsigned)g.Zi;
        const int yi = (int)(r % (unsigned)g.Yi);
        r /= (unsigned)g.Yi;
        const int xi = (int)(r % (unsigned)g.Xi);
        const int b = (int)(r / (unsigned)g.Xi);
        const int xlo = ac_first_ge(xi - 1, g.Xo, g.sx, g.ix), xhi = ac_first_ge(xi + 1, g.Xo, g.sx, g.ix);
        const int ylo = ac_first_ge(yi - 1, g.Yo, g.sy, g.iy), yhi = ac_first_ge(yi + 1, g.Yo, g.sy, g.iy);
        const int zlo = ac_first_ge(zi - 1, g.Zo, g.sz, g.iz), zhi = ac_first_ge(zi + 1, g.Zo, g.sz, g.iz);
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int ox = xlo; ox < xhi; ++ox) {
            const float wx = ac_weight(ox, xi, g.Xi, g.sx);
            const int64_t bx = ((int64_t)b * g.Xo + ox) * g.Yo;
            for (int oy = ylo; oy < yhi; ++oy) {
                const float wxy = wx * ac_weight(oy, yi, g.Yi, g.sy);
                const int64_t row = (bx + oy) * g.Zo;
                for (int oz = zlo; oz < zhi; ++oz) {
                    const float w = wxy * ac_weight(oz, zi, g.Zi, g.sz);
                    const bf16x8 d = __builtin_bit_cast(bf16x8, dy8[(row + oz) * ld8 + c]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += w * (float)d[e];
                }
            }
        }
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)acc[e];
        dx8[(int64_t)vox * cv + c] = __builtin_bit_cast(u32x4, o);
    }
}

float ac_scale(int64_t in, int64_t out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }
float ac_inv(int64_t in, int64_t out) { return (in > 1 && out > 1) ? (float)(out - 1) / (float)(in - 1) : 0.f; }

int rs_check(const char* name, int64_t B, int64_t Xi, int64_t Yi, int64_t Zi, int64_t Xo, int64_t Yo, int64_t Zo, int64_t C) {
    UCF_CHECK_ARG(B > 0 && Xi > 0 && Yi > 0 && Zi > 0 && Xo > 0 && Yo > 0 && Zo > 0, "%s: empty volume", name);
    UCF_CHECK_ARG(Xi < (1 << 24) && Yi < (1 << 24) && Zi < (1 << 24) && Xo < (1 << 24) && Yo < (1 << 24) && Zo < (1 << 24),
                  "%s: extents must be below 2^24 (exact in fp32)", name);
    UCF_CHECK_ARG(C > 0 && C % 8 == 0, "%s: C must be a positive multiple of 8 (got %lld)", name, (long long)C);
    return UCFVIT_OK;
}

RsGeo rs_geo(int64_t Xi, int64_t Yi, int64_t Zi, int64_t Xo, int64_t Yo, int64_t Zo) {
    return RsGeo{(int)Xi, (int)Yi, (int)Zi, (int)Xo, (int)Yo, (int)Zo, ac_scale(Xi, Xo), ac_scale(Yi, Yo), ac_scale(Zi, Zo),
                 ac_inv(Xi, Xo), ac_inv(Yi, Yo), ac_inv(Zi, Zo)};
}

unsigned rs_blocks(int64_t nvec) {
    const int64_t blocks = (nvec + RT - 1) / RT;
    return (unsigned)(blocks > 65536 ? 65536 : blocks);
}

}  // namespace

// x dense [B][Xi][Yi][Zi][C] -> y[voxel * ld_dst + c] over [B][Xo][Yo][Zo] voxels; skip (may be NULL): dense [B][Xo][Yo][Zo][Cs] copied
// behind the C channels of every row (ld_dst >= C + Cs).
extern "C" int ucfvit_resample_trilinear_fwd(const void* x, void* y, int64_t B, int64_t Xi, int64_t Yi, int64_t Zi, int64_t Xo, int64_t Yo, int64_t Zo,
                                             int64_t C, int64_t ld_dst, const void* skip, int64_t Cs, void* stream) {
    const char* name = "ucfvit_resample_trilinear_fwd";
    UCF_CHECK_ARG(x && y, "%s: null pointer", name);
    const int rc = rs_check(name, B, Xi, Yi, Zi, Xo, Yo, Zo, C);
    if (rc) return rc;
    UCF_CHECK_ARG(ld_dst >= C && ld_dst % 8 == 0, "%s: ld_dst must be a multiple of 8 and >= C", name);
    UCF_CHECK_ARG(ucf_is_aligned16(x) && ucf_is_aligned16(y), "%s: operands must be 16-byte aligned", name);
    if (skip) UCF_CHECK_ARG(Cs > 0 && Cs % 8 == 0 && ld_dst >= C + Cs && ucf_is_aligned16(skip), "%s: bad skip operand", name);
    const int64_t cvt = (C + (skip ? Cs : 0)) / 8;
    const int64_t nvec = B * Xo * Yo * Zo * cvt;
    UCF_CHECK_ARG(nvec < (1ll << 31) && B * Xi * Yi * Zi * (C / 8) < (1ll << 31), "%s: more than 2^31 16-byte vectors", name);
    hipLaunchKernelGGL(resample_fwd_kernel, dim3(rs_blocks(nvec)), dim3(RT), 0, (hipStream_t)stream, (const bf16*)x, (bf16*)y, (const bf16*)skip,
                       rs_geo(Xi, Yi, Zi, Xo, Yo, Zo), (unsigned)nvec, (int)(C / 8), (int)cvt, ld_dst / 8, (int)(skip ? Cs / 8 : 0));
    UCF_LAUNCH_CHECK(name);
    return UCFVIT_OK;
}

// dy[voxel * ld_dy + c] over [B][Xo][Yo][Zo] voxels -> dense dx [B][Xi][Yi][Zi][C] (every element written).
extern "C" int ucfvit_resample_trilinear_bwd(const void* dy, void* dx, int64_t B, int64_t Xi, int64_t Yi, int64_t Zi, int64_t Xo, int64_t Yo,
                                             int64_t Zo, int64_t C, int64_t ld_dy, void* stream) {
    const char* name = "ucfvit_resample_trilinear_bwd";
    UCF_CHECK_ARG(dy && dx, "%s: null pointer", name);
    const int rc = rs_check(name, B, Xi, Yi, Zi, Xo, Yo, Zo, C);
    if (rc) return rc;
    UCF_CHECK_ARG(ld_dy >= C && ld_dy % 8 == 0, "%s: ld_dy must be a multiple of 8 and >= C", name);
    UCF_CHECK_ARG(ucf_is_aligned16(dy) && ucf_is_aligned16(dx), "%s: operands must be 16-byte aligned", name);
    const int64_t nvec = B * Xi * Yi * Zi * (C / 8);
    UCF_CHECK_ARG(nvec < (1ll << 31) && B * Xo * Yo * Zo * (ld_dy / 8) < (1ll << 31), "%s: more than 2^31 16-byte vectors", name);
    hipLaunchKernelGGL(resample_bwd_kernel, dim3(rs_blocks(nvec)), dim3(RT), 0, (hipStream_t)stream, (const bf16*)dy, (bf16*)dx,
                       rs_geo(Xi, Yi, Zi, Xo, Yo, Zo), (unsigned)nvec, (int)(C / 8), ld_dy / 8);
    UCF_LAUNCH_CHECK(name);
    return UCFVIT_OK;
}
