// Automatic masks (--auto-mask): the assignment pass of the joint colour k-means over a pooled NCHW fp32 image [3][H][W].
//   stv_kmeans_assign   label every pixel with its nearest centroid, sum the pixels and count them per label, count the
//                       labels that changed
// It is color_stats_kernel (color.hip) with a label in between and walks the image the same way (color_walk.h): a work item
// is four consecutive pixels of one row read from all three planes, and their four labels - one 32-bit load and store on the
// vector path, bytes on the scalar path.  12 bytes read and 2 bytes of labels moved per pixel, 9 K fp32 operations: memory-
// bound where it is not launch-bound.  Set-up work: it does not run inside the step.
#include <hip/hip_runtime.h>

#include "color_walk.h"
#include "stv_common.h"

namespace {

constexpr int kKmThreads = STV_KMEANS_THREADS;
constexpr int kKmBlocks = STV_KMEANS_PARTS;
constexpr int kKmDoubles = STV_KMEANS_PART_DOUBLES;
constexpr int kKmWaves = kKmThreads / STV_WAVE;
constexpr int kKmMaxK = 4;
static_assert(kKmDoubles == 4 * kKmMaxK + 1, "a row of parts: four doubles per cluster, then the changed count");

// d_k = ((e0*e0 + e1*e1) + e2*e2), e_j = x_j - c_k[j]: every difference, product and sum rounded to fp32 on its own, so
// that an fp32 twin reproduces every bit (plain operators under `fp contract(off)`, as color_affine_kernel).  The label
// is the first k with d_k < the best so far, starting from +inf: the lowest index wins a tie, a NaN distance never wins,
// and a pixel whose every distance is NaN or +inf gets label 0.
template <int K>
__device__ __forceinline__ int km_label(float x0, float x1, float x2, const float (&c)[K][3]) {
#pragma clang fp contract(off)
  float best = __builtin_inff();
  int label = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float e0 = x0 - c[k][0], e1 = x1 - c[k][1], e2 = x2 - c[k][2];
    const float q0 = e0 * e0, q1 = e1 * e1, q2 = e2 * e2;
    const float s01 = q0 + q1;
    const float d = s01 + q2;
    if (d < best) {
      best = d;
      label = k;
    }
  }
  return label;
}

// parts[blockIdx.x][4k .. 4k+3] = sum x0, x1, x2 and the number of this workgroup's pixels with label k (zeros for k >= K);
// parts[blockIdx.x][16] = the number of its pixels whose label differs from the one `labels` held.  Sums in double.  Order: a
// thread adds its pixels in item order, pixel by pixel; the wave butterfly; one thread per entry adds the wave sums in wave
// order.  No atomics; every entry is written, zeros without items.  `labels` is read and written by the item that owns the
// four bytes, the read first: in place is the contract (hence no __restrict__ on it).
template <bool kVec, int K>
__global__ __launch_bounds__(kKmThreads) void kmeans_assign_kernel(const float* __restrict__ x, const float* __restrict__ centroids,
                                                                   uint8_t* labels, double* __restrict__ parts, int H, int W) {
  __shared__ double red[kKmWaves][kKmDoubles];
  const int W4 = (W + 3) >> 2;
  const unsigned items = (unsigned)H * (unsigned)W4;             // < 2^28: the entry point bounds 3*H*W*4 bytes by 2 GiB
  const size_t plane = (size_t)H * W;
  float c[K][3];                                                 // uniform over the launch: once, into registers
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < 3; ++j) c[k][j] = centroids[3 * k + j];
  }
  double acc[4 * K];
#pragma unroll
  for (int m = 0; m < 4 * K; ++m) acc[m] = 0.0;
  unsigned changed = 0;                                          // <= items * 4 / gridDim.x: far below 2^32
  for (unsigned i = blockIdx.x * kKmThreads + threadIdx.x; i < items; i += (unsigned)gridDim.x * kKmThreads) {
    const ColorItem it = color_item<kVec>(i, W4, W);
    const size_t at = (size_t)it.r * W + it.x0;
    float px[3][4];
    color_load<kVec>(x, plane, at, it.nv, px);
    uint32_t prev = 0, next = 0;
    if constexpr (kVec) {
      prev = *reinterpret_cast<const uint32_t*>(labels + at);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < it.nv) prev |= (uint32_t)labels[at + k] << (8 * k);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= it.nv) continue;
      const int label = km_label<K>(px[0][k], px[1][k], px[2][k], c);
      next |= (uint32_t)label << (8 * k);
      changed += ((prev >> (8 * k)) & 0xFFu) != (uint32_t)label;
      const double a = (double)px[0][k], b = (double)px[1][k], g = (double)px[2][k];
#pragma unroll
      for (int q = 0; q < K; ++q) {                              // selects, not an indexed accumulator: registers, no scratch
        const bool mine = label == q;
        acc[4 * q + 0] += mine ? a : 0.0;
        acc[4 * q + 1] += mine ? b : 0.0;
        acc[4 * q + 2] += mine ? g : 0.0;
        acc[4 * q + 3] += mine ? 1.0 : 0.0;
      }
    }
    if constexpr (kVec) {
      *reinterpret_cast<uint32_t*>(labels + at) = next;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < it.nv) labels[at + k] = (uint8_t)(next >> (8 * k));
    }
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < 4 * K; ++m) {
    const double s = wave_sum_d(acc[m]);
    if ((threadIdx.x & 63) == 0) red[wave][m] = s;
  }
  const double ch = wave_sum_d((double)changed);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int m = 4 * K; m < kKmDoubles - 1; ++m) red[wave][m] = 0.0;
    red[wave][kKmDoubles - 1] = ch;
  }
  __syncthreads();
  if (threadIdx.x < kKmDoubles) {
    double s = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kKmWaves; ++w) s += red[w][threadIdx.x];
    parts[(size_t)blockIdx.x * kKmDoubles + threadIdx.x] = s;
  }
}

template <int K>
void kmeans_launch(bool vec, hipStream_t st, const float* x, const float* centroids, uint8_t* labels, double* parts, int H, int W) {
  // every row of `parts` is written on every launch: always the full grid
  if (vec) hipLaunchKernelGGL((kmeans_assign_kernel<true, K>), dim3(kKmBlocks), dim3(kKmThreads), 0, st, x, centroids, labels, parts, H, W);
  else hipLaunchKernelGGL((kmeans_assign_kernel<false, K>), dim3(kKmBlocks), dim3(kKmThreads), 0, st, x, centroids, labels, parts, H, W);
}
}  // namespace

extern "C" int stv_kmeans_assign(const float* x_nchw, const float* centroids, uint8_t* labels, double* parts, int H, int W, int K,
                                 void* stream) {
  if (!x_nchw || !centroids || !labels || !parts || !color_shape_ok(H, W) || K < 1 || K > kKmMaxK) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = (W % 4 == 0) && ((uintptr_t)x_nchw % 16 == 0) && ((uintptr_t)labels % 4 == 0);
  switch (K) {
    case 1: kmeans_launch<1>(vec, st, x_nchw, centroids, labels, parts, H, W); break;
    case 2: kmeans_launch<2>(vec, st, x_nchw, centroids, labels, parts, H, W); break;
    case 3: kmeans_launch<3>(vec, st, x_nchw, centroids, labels, parts, H, W); break;
    default: kmeans_launch<4>(vec, st, x_nchw, centroids, labels, parts, H, W); break;
  }
  STV_CHECK_LAUNCH();
  return STV_OK;
}
