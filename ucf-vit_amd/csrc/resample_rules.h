// Per-axis resampling rules shared by the patcher's serializers (quadtree.hip) and its label / deserialize kernels (patcher_labels.hip).
#pragma once

// cubic convolution coefficients, A = -0.75 (cv2.INTER_CUBIC, torch upsample_bicubic2d)
__device__ __forceinline__ void cubic_coeffs(float t, float (&w)[4]) {
    constexpr float A = -0.75f;
    const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = 2.f - t;
    w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
    w[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
    w[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
    w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

// Cubic resize with half-pixel centres, scale = (float)n_src / (float)n_dst: the source position of destination sample x.  Its cell is
// floorf(f), its taps are cell - 1 .. cell + 2 clamped to the source (tap_clamp) with cubic_coeffs(f - floorf(f)).
__device__ __forceinline__ float half_pixel_pos(int x, float scale) { return ((float)x + 0.5f) * scale - 0.5f; }
__device__ __forceinline__ int tap_clamp(int i, int n_src) { return i < 0 ? 0 : (i > n_src - 1 ? n_src - 1 : i); }
// the same in one call: the cell (returned) and the four coefficients
__device__ __forceinline__ int cubic_axis(int x, float scale, float (&w)[4]) {
    const float f = half_pixel_pos(x, scale), ff = floorf(f);
    cubic_coeffs(f - ff, w);
    return (int)ff;
}

// Aligned-corner linear resize of n_src samples to n_dst, inv = linear_inv(n_dst): destination sample x lies at f = corner_pos(x, n_src, inv)
// between the source samples i0 = linear_cell(f, n_src) and linear_upper(i0, n_src), with weights 1 - t and t = f - i0
__device__ __forceinline__ float linear_inv(int n_dst) { return n_dst > 1 ? 1.f / (float)(n_dst - 1) : 0.f; }
__device__ __forceinline__ float corner_pos(int x, int n_src, float inv) { return (float)x * (float)(n_src - 1) * inv; }
__device__ __forceinline__ int linear_cell(float f, int n_src) {
    const int i = (int)f;
    return i > n_src - 1 ? n_src - 1 : i;
}
__device__ __forceinline__ int linear_upper(int i0, int n_src) { return i0 + 1 < n_src ? i0 + 1 : n_src - 1; }
// the same in one call
__device__ __forceinline__ void linear_axis(int x, int n_src, float inv, int& i0, int& i1, float& t) {
    const float f = corner_pos(x, n_src, inv);
    i0 = linear_cell(f, n_src);
    t = f - (float)i0;
    i1 = linear_upper(i0, n_src);
}

// cv2.resize(INTER_NEAREST): source index of destination index j when n_src samples are resized to n_dst = min(floor(j * n_src / n_dst), n_src - 1)
__device__ __forceinline__ int nearest_floor(int j, int n_src, int n_dst) {
    const int i = (int)(((long long)j * n_src) / n_dst);
    return i < n_src - 1 ? i : n_src - 1;
}

// scipy RegularGridInterpolator(method='nearest') on linspace(0, n, n_src) queried at linspace(0, n, n_dst): position f = j (n_src-1) / (n_dst-1),
// cell i = min(floor(f), n_src-2), take i if the fraction is <= 1/2, else i+1 -- in exact integer arithmetic, so a tie goes to the LOWER index
// (scipy's double arithmetic sends some exact midpoints up; an even n_dst has no ties).  One source sample or one destination sample: index 0.
__device__ __forceinline__ int nearest_grid(int j, int n_src, int n_dst) {
    if (n_src < 2 || n_dst < 2) return 0;
    const int num = j * (n_src - 1), den = n_dst - 1;                       // j < n_dst <= 32768 and n_src <= 32768: below 2^30
    int i = num / den;
    i = i < n_src - 2 ? i : n_src - 2;
    return 2 * (num - i * den) <= den ? i : i + 1;
}
