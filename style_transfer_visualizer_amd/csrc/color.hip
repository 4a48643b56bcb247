// Colour preservation (--preserve-color): three streaming passes over the NCHW fp32 image [3][H][W].
//   stv_color_stats    raw first and second colour moments, double partial sums per workgroup
//   stv_color_affine   y = M x + b per pixel (the colour-statistics match of the style image)
//   stv_luma_transfer  luminance of the result, chrominance of the content image
// They share one walk: a work item is four consecutive pixels of one row, read from all three planes (three 16-byte
// vectors); items are numbered row by row, and a pass of the capped grid covers gridDim.x * kColorThreads consecutive
// items.  kVec: W % 4 == 0 behind 16-byte aligned bases, so every row of every plane starts on a vector; otherwise the
// same items are walked with guarded scalar accesses, in the same order.  12 to 36 bytes per pixel and a handful of
// operations: memory-bound where they are not launch-bound.  None of them runs inside the step.
#include <hip/hip_runtime.h>

#include "color_walk.h"
#include "stv_common.h"

namespace {

constexpr int kColorThreads = STV_COLOR_THREADS;
constexpr int kColorStatsBlocks = STV_COLOR_STATS_PARTS;
constexpr int kColorBlocks = STV_COLOR_MAX_BLOCKS;
constexpr int kColorWaves = kColorThreads / STV_WAVE;

// ------------------------------------------------------------------ statistics
// parts[blockIdx.x][0..8] = sum x0, x1, x2, x0x0, x0x1, x0x2, x1x1, x1x2, x2x2 over this workgroup's pixels.  Products
// and sums in double (the product of two fp32 numbers is exact there): sum xx / n - mean^2 cancels, fp32 partials would
// not leave the covariance of a flat image.  Order: a thread adds its pixels in item order, pixel by pixel; the wave
// butterfly; thread 0 adds the wave sums in wave order.  No atomics; every entry is written, zeros without items.
template <bool kVec>
__global__ __launch_bounds__(kColorThreads) void color_stats_kernel(const float* __restrict__ x, double* __restrict__ parts,
                                                                    int H, int W) {
  __shared__ double red[kColorWaves][9];
  const int W4 = (W + 3) >> 2;
  const unsigned items = (unsigned)H * (unsigned)W4;             // < 2^28: the entry point bounds 3*H*W*4 bytes by 2 GiB
  const size_t plane = (size_t)H * W;
  double acc[9];
#pragma unroll
  for (int m = 0; m < 9; ++m) acc[m] = 0.0;
  for (unsigned i = blockIdx.x * kColorThreads + threadIdx.x; i < items; i += (unsigned)gridDim.x * kColorThreads) {
    const ColorItem it = color_item<kVec>(i, W4, W);
    float px[3][4];
    color_load<kVec>(x, plane, (size_t)it.r * W + it.x0, it.nv, px);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= it.nv) continue;
      const double a = (double)px[0][k], b = (double)px[1][k], c = (double)px[2][k];
      acc[0] += a; acc[1] += b; acc[2] += c;
      acc[3] += a * a; acc[4] += a * b; acc[5] += a * c;
      acc[6] += b * b; acc[7] += b * c; acc[8] += c * c;
    }
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < 9; ++m) {
    const double s = wave_sum_d(acc[m]);
    if ((threadIdx.x & 63) == 0) red[wave][m] = s;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    double s = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kColorWaves; ++w) s += red[w][threadIdx.x];
    parts[(size_t)blockIdx.x * 9 + threadIdx.x] = s;
  }
}

// --------------------------------------------------------------------- affine
// y[c] = ((m[c][0]*x[0] + m[c][1]*x[1]) + m[c][2]*x[2]) + b[c]: every product and every sum rounded to fp32 on its own,
// so that an fp32 twin reproduces every bit (plain * and + under `fp contract(off)`; see resize2x_kernel in
// pointwise.hip on why __fmul_rn / __fadd_rn would not keep the compiler from fusing).  y may BE x: an item reads its
// twelve values before it writes them and no other item touches them (hence no __restrict__).
struct ColorAffine { float m[3][3], b[3]; };
template <bool kVec>
__global__ __launch_bounds__(kColorThreads) void color_affine_kernel(const float* x, float* y, ColorAffine t, int H, int W) {
#pragma clang fp contract(off)
  const int W4 = (W + 3) >> 2;
  const unsigned items = (unsigned)H * (unsigned)W4;
  const size_t plane = (size_t)H * W;
  for (unsigned i = blockIdx.x * kColorThreads + threadIdx.x; i < items; i += (unsigned)gridDim.x * kColorThreads) {
    const ColorItem it = color_item<kVec>(i, W4, W);
    const size_t at = (size_t)it.r * W + it.x0;
    float px[3][4], out[3][4];
    color_load<kVec>(x, plane, at, it.nv, px);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float p0 = t.m[c][0] * px[0][k], p1 = t.m[c][1] * px[1][k], p2 = t.m[c][2] * px[2][k];
        const float s01 = p0 + p1;
        const float s012 = s01 + p2;
        out[c][k] = s012 + t.b[c];
      }
    }
    color_store<kVec>(y, plane, at, it.nv, out);
  }
}

// ----------------------------------------------------------------------- luma
// out = content + (Y(result) - Y(content)) in [0,1] RGB, Rec.601 Y, mapped back into the space the tensors are in.
// Both images go through prepare_image_for_output's rule first (denormalise, nan -> 0, +inf -> 1, -inf -> 0, clamp),
// exactly as frame_u8 in pointwise.hip applies it; the sum itself is not clamped (the export path clamps).  Every
// operation is rounded on its own, in the order stv.h states.  out may BE result.
struct LumaStats { float mean[3], std[3], inv_std[3]; };
__device__ __forceinline__ float luma_rgb01(float v, float mean, float stdv, int normalize) {
#pragma clang fp contract(off)
  if (normalize) {
    const float scaled = v * stdv;
    v = scaled + mean;
  }
  if (v != v) v = 0.0f;
  return fminf(fmaxf(v, 0.0f), 1.0f);                            // +-inf land on 1 / 0 like nan_to_num + clamp
}
__device__ __forceinline__ float luma_y(float r, float g, float b) {
#pragma clang fp contract(off)
  const float yr = 0.299f * r, yg = 0.587f * g, yb = 0.114f * b;
  const float s = yr + yg;
  return s + yb;
}
template <bool kVec>
__global__ __launch_bounds__(kColorThreads) void luma_transfer_kernel(const float* result, const float* __restrict__ content,
                                                                      float* out, LumaStats st, int normalize, int H, int W) {
#pragma clang fp contract(off)
  const int W4 = (W + 3) >> 2;
  const unsigned items = (unsigned)H * (unsigned)W4;
  const size_t plane = (size_t)H * W;
  for (unsigned i = blockIdx.x * kColorThreads + threadIdx.x; i < items; i += (unsigned)gridDim.x * kColorThreads) {
    const ColorItem it = color_item<kVec>(i, W4, W);
    const size_t at = (size_t)it.r * W + it.x0;
    float r[3][4], k[3][4], o[3][4];
    color_load<kVec>(result, plane, at, it.nv, r);
    color_load<kVec>(content, plane, at, it.nv, k);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[c][j] = luma_rgb01(r[c][j], st.mean[c], st.std[c], normalize);
        k[c][j] = luma_rgb01(k[c][j], st.mean[c], st.std[c], normalize);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = luma_y(r[0][j], r[1][j], r[2][j]) - luma_y(k[0][j], k[1][j], k[2][j]);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = k[c][j] + d;
        if (normalize) {
          const float centred = v - st.mean[c];
          o[c][j] = centred * st.inv_std[c];
        } else {
          o[c][j] = v;
        }
      }
    }
    color_store<kVec>(out, plane, at, it.nv, o);
  }
}

// the byte ranges [a, a + bytes) and [b, b + bytes) share a byte
bool ranges_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb ? pb - pa < bytes : pa - pb < bytes;
}
unsigned color_grid(int H, int W) {
  const size_t items = (size_t)H * ((W + 3) / 4);
  size_t grid = (items + kColorThreads - 1) / kColorThreads;
  if (grid > (size_t)kColorBlocks) grid = kColorBlocks;
  return (unsigned)grid;
}
}  // namespace

extern "C" int stv_color_stats(const float* x_nchw, double* parts, int H, int W, void* stream) {
  if (!x_nchw || !parts || !color_shape_ok(H, W)) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = (W % 4 == 0) && ((uintptr_t)x_nchw % 16 == 0);
  // every row of `parts` is written on every launch: always the full grid
  if (vec) hipLaunchKernelGGL(color_stats_kernel<true>, dim3(kColorStatsBlocks), dim3(kColorThreads), 0, st, x_nchw, parts, H, W);
  else hipLaunchKernelGGL(color_stats_kernel<false>, dim3(kColorStatsBlocks), dim3(kColorThreads), 0, st, x_nchw, parts, H, W);
  STV_CHECK_LAUNCH();
  return STV_OK;
}

extern "C" int stv_color_affine(const float* x_nchw, float* y_nchw, const float* m12, int H, int W, void* stream) {
  if (!x_nchw || !y_nchw || !m12 || !color_shape_ok(H, W)) return STV_ERR_ARG;
  const size_t bytes = (size_t)3 * H * W * sizeof(float);
  if (x_nchw != y_nchw && ranges_overlap(x_nchw, y_nchw, bytes)) return STV_ERR_ARG;
  ColorAffine t;
  for (int c = 0; c < 3; ++c) {                                  // m12: a HOST array, row-major matrix then offset
    for (int j = 0; j < 3; ++j) t.m[c][j] = m12[3 * c + j];
    t.b[c] = m12[9 + c];
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = (W % 4 == 0) && ((uintptr_t)x_nchw % 16 == 0) && ((uintptr_t)y_nchw % 16 == 0);
  const dim3 g(color_grid(H, W)), b(kColorThreads);
  if (vec) hipLaunchKernelGGL(color_affine_kernel<true>, g, b, 0, st, x_nchw, y_nchw, t, H, W);
  else hipLaunchKernelGGL(color_affine_kernel<false>, g, b, 0, st, x_nchw, y_nchw, t, H, W);
  STV_CHECK_LAUNCH();
  return STV_OK;
}

extern "C" int stv_luma_transfer(const float* result, const float* content, float* out, int H, int W, const float* mean3,
                                 const float* std3, void* stream) {
  if (!result || !content || !out || !color_shape_ok(H, W)) return STV_ERR_ARG;
  if ((mean3 == nullptr) != (std3 == nullptr)) return STV_ERR_ARG;
  const size_t bytes = (size_t)3 * H * W * sizeof(float);
  if (ranges_overlap(content, out, bytes)) return STV_ERR_ARG;   // out == content included
  if (result != out && ranges_overlap(result, out, bytes)) return STV_ERR_ARG;
  LumaStats s{};
  const int normalize = mean3 != nullptr;
  for (int c = 0; c < 3 && normalize; ++c) {                     // HOST arrays
    s.mean[c] = mean3[c];
    s.std[c] = std3[c];
    s.inv_std[c] = 1.0f / std3[c];
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = (W % 4 == 0) && ((uintptr_t)result % 16 == 0) && ((uintptr_t)content % 16 == 0) && ((uintptr_t)out % 16 == 0);
  const dim3 g(color_grid(H, W)), b(kColorThreads);
  if (vec) hipLaunchKernelGGL(luma_transfer_kernel<true>, g, b, 0, st, result, content, out, s, normalize, H, W);
  else hipLaunchKernelGGL(luma_transfer_kernel<false>, g, b, 0, st, result, content, out, s, normalize, H, W);
  STV_CHECK_LAUNCH();
  return STV_OK;
}
