// General resize (--content-size, --style-size, --style-scale): one pass of a separable, antialiased resampler over an
// NCHW fp32 image, any output size, up or down.  The filter lives in the tables the host builds (resize.py): output index
// i along the resized axis reads inputs start[i] .. start[i] + count[i] - 1 with weights[i*K .. i*K + count[i] - 1].
//   axis 0 (rows):    x [planes][H][W] -> y [planes][n_out][W]
//   axis 1 (columns): x [planes][H][W] -> y [planes][H][n_out]
// The walk is resize2x_kernel's (pointwise.hip): a work item is four consecutive OUTPUT pixels of one row (one 16-byte
// store); items are numbered row by row over all output rows of all planes, and a pass of the capped grid covers
// kAxisBlocks * kAxisThreads consecutive items.  kVec: every row that is read or written as a vector starts on a
// 16-byte boundary and no row end is ragged; otherwise the same items are walked with guarded scalar accesses.
//   rows:    the four columns of an item share one table row, and so do all items of an output row: the table reads are
//            uniform over a wave wherever a row holds 64 items or more.  Tap k is one 16-byte load from input row
//            start + k of the same plane.
//   columns: each of the four outputs has its own table row; the input reads are scalar, from the item's own input row
//            (neighbouring outputs share most of their taps: the reads hit the cache).
// Arithmetic, fixed to the bit (the convention stated above resize2x_kernel: plain * and + under `fp contract(off)`):
//   acc = 0.0f;  for k = 0 .. count-1 ascending:  acc = acc + (w[k] * x[start + k])
// Nothing is read across a row end or a channel plane: a tap index stays inside [0, n_in) (the tables promise
// start + count <= n_in; the kernel clips a row that does not keep the promise instead of following it), and entries of
// a table row behind `count` are never read.
#include <hip/hip_runtime.h>

#include "stv_common.h"

namespace {

constexpr int kAxisThreads = STV_RESIZE_AXIS_THREADS;
constexpr int kAxisBlocks = STV_RESIZE_AXIS_MAX_BLOCKS;

// first tap and number of taps of table row i, clipped into [0, n_in) and to the K entries a row holds
struct Taps { int s, n; };
__device__ __forceinline__ Taps taps_of(const int32_t* __restrict__ start, const int32_t* __restrict__ count, int i,
                                        int n_in, int K) {
  Taps t;
  t.s = start[i];
  t.n = count[i];
  if (t.s < 0) t.s = 0;
  if (t.n > K) t.n = K;
  if (t.n > n_in - t.s) t.n = n_in - t.s;
  return t;
}

template <int kAxis, bool kVec>
__global__ __launch_bounds__(kAxisThreads) void resize_axis_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                   int out_rows, int H, int W, int n_out,
                                                                   const int32_t* __restrict__ start,
                                                                   const int32_t* __restrict__ count,
                                                                   const float* __restrict__ weights, int K) {
#pragma clang fp contract(off)
  const int Wo = kAxis == 0 ? W : n_out;
  const int W4 = (Wo + 3) >> 2;
  const unsigned items = (unsigned)out_rows * (unsigned)W4;      // < 2^29: the entry point bounds both sizes by 2 GiB
  for (unsigned i = blockIdx.x * kAxisThreads + threadIdx.x; i < items; i += (unsigned)gridDim.x * kAxisThreads) {
    const int r = (int)(i / (unsigned)W4);
    const int x0 = (int)(i - (unsigned)r * (unsigned)W4) * 4;
    const int nv = kVec ? 4 : (Wo - x0 < 4 ? Wo - x0 : 4);        // pixels of this item inside the row
    float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (kAxis == 0) {
      const int c = r / n_out, yy = r - c * n_out;
      const Taps t = taps_of(start, count, yy, H, K);
      const float* w = weights + (size_t)yy * K;
      const float* row = x + ((size_t)c * H + t.s) * W + x0;
      for (int k = 0; k < t.n; ++k, row += W) {
        const float wk = w[k];
        float v[4];
        if constexpr (kVec) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(row);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = q[j];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = j < nv ? row[j] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = out[j] + (wk * v[j]);
      }
    } else {
      const float* row = x + (size_t)r * W;                       // output row r is input row r: H is kept
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < nv) {
          const Taps t = taps_of(start, count, x0 + j, W, K);
          const float* w = weights + (size_t)(x0 + j) * K;
          const float* p = row + t.s;
          float acc = 0.0f;
          for (int k = 0; k < t.n; ++k) acc = acc + (w[k] * p[k]);
          out[j] = acc;
        }
      }
    }
    float* o = y + (size_t)r * Wo + x0;
    if constexpr (kVec) {
      f32x4 q;
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = out[j];
      *reinterpret_cast<f32x4*>(o) = q;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nv) o[j] = out[j];
    }
  }
}

}  // namespace

extern "C" int stv_resize_axis(const float* x, float* y, int planes, int H, int W, int n_out, int axis,
                               const int32_t* start, const int32_t* count, const float* weights, int K, void* stream) {
  if (!x || !y || x == y || !start || !count || !weights) return STV_ERR_ARG;
  if (planes <= 0 || H <= 0 || W <= 0 || n_out <= 0 || K < 1) return STV_ERR_ARG;
  if (axis != 0 && axis != 1) return STV_ERR_ARG;
  const int Ho = axis == 0 ? n_out : H, Wo = axis == 0 ? W : n_out;
  const unsigned long long in_bytes = (unsigned long long)planes * (unsigned long long)H * (unsigned long long)W * 4ull;
  const unsigned long long out_bytes = (unsigned long long)planes * (unsigned long long)Ho * (unsigned long long)Wo * 4ull;
  if (in_bytes >= (1ull << 31) || out_bytes >= (1ull << 31)) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int out_rows = planes * Ho;
  const size_t items = (size_t)out_rows * ((Wo + 3) / 4);
  size_t grid = (items + kAxisThreads - 1) / kAxisThreads;
  if (grid > (size_t)kAxisBlocks) grid = kAxisBlocks;
  // rows: input and output rows are both W floats, read and written as vectors; columns: only the output is
  const bool vec = (Wo % 4 == 0) && ((uintptr_t)y % 16 == 0) && (axis == 1 || (uintptr_t)x % 16 == 0);
  const dim3 g((unsigned)grid), b(kAxisThreads);
  if (axis == 0 && vec)
    hipLaunchKernelGGL((resize_axis_kernel<0, true>), g, b, 0, st, x, y, out_rows, H, W, n_out, start, count, weights, K);
  else if (axis == 0)
    hipLaunchKernelGGL((resize_axis_kernel<0, false>), g, b, 0, st, x, y, out_rows, H, W, n_out, start, count, weights, K);
  else if (vec)
    hipLaunchKernelGGL((resize_axis_kernel<1, true>), g, b, 0, st, x, y, out_rows, H, W, n_out, start, count, weights, K);
  else
    hipLaunchKernelGGL((resize_axis_kernel<1, false>), g, b, 0, st, x, y, out_rows, H, W, n_out, start, count, weights, K);
  STV_CHECK_LAUNCH();
  return STV_OK;
}
