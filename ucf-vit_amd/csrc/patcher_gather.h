// The gather of the deserializers' adjoints (patcher_labels_bwd.hip), free of anything but the per-axis rules and the decoded leaf: which leaf
// positions reach a token index, with which weights, and how a leaf is cut into slices.
#pragma once
#include "patcher_tree.h"
#include "resample_rules.h"

namespace {

constexpr int BWD_SLICES = 16;                       // most slices of one leaf = grid.y
constexpr int BWD_SLICE_PIXELS = 1024;               // a slice holds at least this many pixels (the last one of a leaf aside)
constexpr unsigned BWD_TILES = 64;                   // most workgroups along grid.z, each striding over the elements of a tile

enum { RULE_CUBIC = 0, RULE_LINEAR = 1, RULE_FLOOR = 2, RULE_GRID = 3 };

// one axis of a leaf: n leaf positions against p token indices under one of the forward's rules
template <int RULE>
struct Axis {
    static constexpr int NT = RULE == RULE_CUBIC ? 4 : (RULE == RULE_LINEAR ? 2 : 1);
    int n, p;
    float s;                                         // cubic: p / n as the forward computes it; linear: linear_inv(n)
    __device__ __forceinline__ void set(int n_, int p_) {
        n = n_;
        p = p_;
        s = RULE == RULE_CUBIC ? (float)p_ / (float)n_ : (RULE == RULE_LINEAR ? linear_inv(n_) : 0.f);
    }
    // the token indices and weights leaf position x reads in the forward
    __device__ __forceinline__ void taps(int x, int (&i)[NT], float (&w)[NT]) const {
        if constexpr (RULE == RULE_CUBIC) {
            const int cell = cubic_axis(x, s, w);
#pragma unroll
            for (int d = 0; d < 4; ++d) i[d] = tap_clamp(cell - 1 + d, p);
        } else if constexpr (RULE == RULE_LINEAR) {
            float t;
            linear_axis(x, p, s, i[0], i[1], t);
            w[0] = 1.f - t;
            w[1] = t;
        } else {
            i[0] = RULE == RULE_FLOOR ? nearest_floor(x, p, n) : nearest_grid(x, p, n);
            w[0] = 1.f;
        }
    }
    // [lo, hi]: a run of leaf positions that holds every x with a tap on k.  The source position of x is affine in x: cubic
    // f = (x + 1/2) p / n - 1/2 with taps floor(f) - 1 .. floor(f) + 2, so k - 2 <= f < k + 2; linear and the grid rule f = x (p - 1) / (n - 1) with
    // taps floor(f), floor(f) + 1; the floor rule f = x p / n with tap floor(f).  The ends are computed in fp32 (below 2^15: off by less than 0.01)
    // and widened by one position; clamped taps gather at the first and last index, whose runs reach the end of the leaf.
    __device__ __forceinline__ void range(int k, int& lo, int& hi) const {
        float a, b;
        if (RULE == RULE_CUBIC) {
            const float r = (float)n / (float)p;
            a = ((float)k - 1.5f) * r - 0.5f;
            b = ((float)k + 2.5f) * r - 0.5f;
        } else if (RULE == RULE_FLOOR) {
            const float r = (float)n / (float)p;
            a = (float)k * r;
            b = (float)(k + 1) * r;
        } else {
            const float r = p > 1 ? (float)(n - 1) / (float)(p - 1) : 0.f;
            a = (float)(k - 1) * r;
            b = (float)(k + 1) * r;
        }
        lo = (int)floorf(a) - 1;
        hi = (int)ceilf(b) + 1;
        if (k == 0) lo = 0;
        if (k >= p - 1) hi = n - 1;
        lo = lo < 0 ? 0 : lo;
        hi = hi > n - 1 ? n - 1 : hi;
    }
};

// sum over the positions lo[A] .. hi[A] of axis A of (weight of the taps on k[A]) x (the same sum over the axes below A); g: channel c of image b,
// pix: the pixel number of the positions fixed so far, pstride[a]: pixels per step along axis a
template <int RULE, int ND, int A>
struct Gather {
    static __device__ __forceinline__ float run(const Axis<RULE> (&ax)[ND], const int (&k)[ND], const int (&lo)[ND], const int (&hi)[ND],
                                                const float* __restrict__ g, int64_t op, int64_t pix, const int64_t (&pstride)[ND]) {
        constexpr int NT = Axis<RULE>::NT;
        float acc = 0.f;
        for (int x = lo[A]; x <= hi[A]; ++x) {
            int ti[NT];
            float tw[NT];
            ax[A].taps(x, ti, tw);
            bool hit = false;
#pragma unroll
            for (int d = 0; d < NT; ++d) hit = hit || ti[d] == k[A];
            if (!hit) continue;
            const int64_t px = pix + (int64_t)x * pstride[A];
            float r;
            if constexpr (A == 0) r = g[px * op];
            else r = Gather<RULE, ND, A - 1>::run(ax, k, lo, hi, g, op, px, pstride);
#pragma unroll
            for (int d = 0; d < NT; ++d)
                if (ti[d] == k[A]) acc += tw[d] * r;
        }
        return acc;
    }
};

// rows (positions along the slowest axis) per slice and the number of slices, from the leaf's extents alone
template <int ND>
__device__ __forceinline__ void slices_of(const Leaf<ND>& lf, int& rows, int& nsl) {
    int inner = 1;                                                          // at most 32767 (2-D) or 256^2 (3-D)
#pragma unroll
    for (int a = 0; a < ND - 1; ++a) inner *= lf.n[a];
    const int outer = lf.n[ND - 1];
    const int by_count = (outer + BWD_SLICES - 1) / BWD_SLICES, by_size = (BWD_SLICE_PIXELS + inner - 1) / inner;
    rows = by_count > by_size ? by_count : by_size;
    nsl = (outer + rows - 1) / rows;                                        // <= BWD_SLICES
}

}  // namespace
