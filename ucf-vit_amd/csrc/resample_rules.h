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
