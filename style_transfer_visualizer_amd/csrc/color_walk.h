// The walk the colour kernels (color.hip) and the k-means assignment (kmeans.hip) share over an NCHW fp32 image
// [3][H][W]: a work item is four consecutive pixels of one row, read from all three planes (three 16-byte vectors);
// items are numbered row by row, W4 = ceil(W / 4) to a row.  kVec: W % 4 == 0 behind 16-byte aligned bases, so every row
// of every plane starts on a vector; otherwise the same items are walked with guarded scalar accesses, in the same order.
#pragma once
#include "stv_common.h"

// The four pixels of item i: px[c][k] = x[c][r][x0 + k], 0 where the row has ended (k >= nv).
struct ColorItem { int r, x0, nv; };
template <bool kVec>
__device__ __forceinline__ ColorItem color_item(unsigned i, int W4, int W) {
  ColorItem it;
  it.r = (int)(i / (unsigned)W4);
  it.x0 = (int)(i - (unsigned)it.r * (unsigned)W4) * 4;
  it.nv = kVec ? 4 : (W - it.x0 < 4 ? W - it.x0 : 4);
  return it;
}
template <bool kVec>
__device__ __forceinline__ void color_load(const float* x, size_t plane, size_t at, int nv, float (&px)[3][4]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* p = x + (size_t)c * plane + at;
    if constexpr (kVec) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
      for (int k = 0; k < 4; ++k) px[c][k] = v[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) px[c][k] = k < nv ? p[k] : 0.0f;
    }
  }
}
template <bool kVec>
__device__ __forceinline__ void color_store(float* y, size_t plane, size_t at, int nv, const float (&px)[3][4]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float* p = y + (size_t)c * plane + at;
    if constexpr (kVec) {
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = px[c][k];
      *reinterpret_cast<f32x4*>(p) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nv) p[k] = px[c][k];
    }
  }
}

// The shape check the entry points over this walk share: positive sides and 3*H*W*4 bytes below 2 GiB.
static inline bool color_shape_ok(int H, int W) {
  if (H <= 0 || W <= 0) return false;
  return 3ull * (unsigned long long)H * (unsigned long long)W * 4ull < (1ull << 31);
}
