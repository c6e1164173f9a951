// What the memory-bound row passes over a [rows, D] token matrix share (csrc/drop_path.hip, csrc/dropout.hip): the 16-byte / one-element
// packs of a lane and the row-chunk count of the grid.  Geometry (that of colsum_kernel, csrc/norm.hip): lanes along D, a wave covers
// 64 x 16 B = 1 KiB of contiguous columns of one row, the 4 waves of a workgroup take rows r, r+1, r+2, r+3 of their row chunk and step
// by 4, four rows in flight per lane; grid = (column blocks, row chunks).
#pragma once
#include "common.h"

constexpr int DP_BLOCK = 256;          // 4 waves
constexpr int DP_WAVES = DP_BLOCK / 64;
constexpr int DP_UNROLL = 4;           // rows in flight per lane
constexpr int DP_MAX_CHUNKS = 1024;

// W consecutive elements of T: one 16-byte vector (W = Vec16<T>::N) or one element (W = 1, the scalar path)
template <typename T, int W> struct Pack;
template <typename T> struct Pack<T, 1> {
    T v;
    __device__ __forceinline__ static Pack load(const T* p) { Pack r; r.v = *p; return r; }
    __device__ __forceinline__ void store(T* p) const { *p = v; }
    __device__ __forceinline__ float get(int) const { return to_f32<T>(v); }
    __device__ __forceinline__ void set(int, float x) { v = from_f32<T>(x); }
};
template <> struct Pack<float, 4> {
    Vec16<float> v;
    __device__ __forceinline__ static Pack load(const float* p) { Pack r; r.v = *reinterpret_cast<const Vec16<float>*>(p); return r; }
    __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<Vec16<float>*>(p) = v; }
    __device__ __forceinline__ float get(int i) const { return v.get(i); }
    __device__ __forceinline__ void set(int i, float x) { v.set(i, x); }
};
template <> struct Pack<bf16, 8> {
    Vec16<bf16> v;
    __device__ __forceinline__ static Pack load(const bf16* p) { Pack r; r.v = *reinterpret_cast<const Vec16<bf16>*>(p); return r; }
    __device__ __forceinline__ void store(bf16* p) const { *reinterpret_cast<Vec16<bf16>*>(p) = v; }
    __device__ __forceinline__ float get(int i) const { return v.get(i); }
    __device__ __forceinline__ void set(int i, float x) { v.set(i, x); }
};

// row chunks: 16 rows (four steps of the 4 waves) at least, so that a small problem does not pay for partial rows it cannot fill; at
// most 1024 workgroups at one column block per 512 columns (the bf16 vector path), never more than DP_MAX_CHUNKS.  Measured at
// [665 x 197, 1024] bf16, one box: scale takes 0.099 ms with 1024 workgroups (4 per CU), 0.110 with 2048, 0.109 with 768, 0.132 with 512
inline int dp_chunks(int64_t rows, int64_t D) {
    int64_t cap = 1024 / ((D + 511) / 512);
    if (cap > DP_MAX_CHUNKS) cap = DP_MAX_CHUNKS;
    if (cap < 64) cap = 64;
    int64_t c = (rows + 15) / 16;
    if (c > cap) c = cap;
    if (c < 1) c = 1;
    return (int)c;
}
