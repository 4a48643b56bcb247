// Automatic masks in VGG feature space (--auto-mask-space features): the joint k-means over one layer's activations, NHWC
// [n][C] of bf16 or fp32 (the definitions and the launch geometry: stv.h, "Automatic masks in VGG feature space").
//   stv_kmeans_feat_assign   label every pixel with its nearest centroid, sum the pixels and count them per label, count the
//                            labels that changed: one row of doubles per workgroup
//   stv_kmeans_feat_update   add the rows of both images and form the new centroids in place; nine doubles for the host
// A pixel is spread over Q = C/8 lanes of one wave (one octet of channels each), so the distance is a reduction across lanes
// (the xor butterfly over the pixel's lanes) and the sums are a reduction across pixels (registers, then the butterfly over
// the lanes that hold the same octet, then the waves through LDS).  One read of F per launch: memory-bound where it is not
// launch-bound.  Set-up work: neither kernel runs inside the step.
#include <hip/hip_runtime.h>

#include "stv_common.h"

namespace {

constexpr int kKfThreads = STV_KMF_THREADS;
constexpr int kKfWaves = STV_KMF_WAVES;
constexpr int kKfParts = STV_KMF_PARTS;
constexpr int kKfMaxK = STV_KMF_MAX_K;
constexpr int kKfMaxC = STV_KMF_MAX_C;
constexpr int kKfMaxRow = STV_KMF_ROW_DOUBLES(STV_KMF_MAX_C);
static_assert(kKfThreads == kKfWaves * STV_WAVE, "a workgroup is STV_KMF_WAVES waves");

// the lane's octet of pixel `p` as eight floats: 16 bytes of bf16 (the exact bit shift) or 2 x 16 bytes of fp32
template <typename T>
__device__ __forceinline__ void kf_load(const T* __restrict__ F, size_t at, float (&x)[8]) {
  const u32x4* src = reinterpret_cast<const u32x4*>(F + at);
  if constexpr (sizeof(T) == 2) {
    unpack16<bf16_t>(src[0], x);
  } else {
    unpack16<float>(src[0], x);
    unpack16<float>(src[1], x + 4);
  }
}

// parts[blockIdx.x]: the row stv.h describes.  The loop over the passes is uniform over a wave (its condition is the wave's
// first pixel), so every lane takes part in every shuffle; a lane whose pixel is past n loads nothing, holds zeros and adds
// +0.0.  `labels` carries no __restrict__: in place is the contract.
template <typename T, int K, bool kKeep>
__global__ __launch_bounds__(kKfThreads) void kmeans_feat_assign_kernel(const T* __restrict__ F, const float* __restrict__ centroids,
                                                                        uint8_t* labels, double* __restrict__ parts, int n, int C) {
  __shared__ double red[kKfMaxRow];
  const int Q = C >> 3;                                          // lanes per pixel: 8, 16, 32 or 64 (the entry point checks)
  const int G = STV_WAVE / Q;                                    // pixels per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int octet = lane & (Q - 1), group = lane / Q;
  const int row = 4 * (C + 1) + 1;
  float c[K][8];                                                 // uniform over the launch: once, into registers
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < 8; ++j) c[k][j] = kKeep ? 0.0f : centroids[(size_t)k * C + 8 * octet + j];
  }
  double acc[K][8], cnt[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    cnt[k] = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = 0.0;
  }
  unsigned changed = 0;                                          // <= passes of the grid: far below 2^32
  const long long per_pass = (long long)kKfParts * kKfWaves * G;
  for (long long base = (long long)(blockIdx.x * kKfWaves + wave) * G; base < n; base += per_pass) {
    const long long p = base + group;
    const bool valid = p < n;
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = 0.0f;
    if (valid) kf_load<T>(F, (size_t)p * C + 8 * octet, x);
    int label = 0;
    if constexpr (kKeep) {
      label = valid ? (int)labels[p] : 0;                        // every lane of the pixel reads the byte; nobody writes
    } else {
#pragma clang fp contract(off)
      float best = __builtin_inff();
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float d = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float e = x[j] - c[k][j];
          const float q = e * e;
          d = d + q;
        }
        for (int s = Q >> 1; s > 0; s >>= 1) d = d + __shfl_xor(d, s, 64);      // a + b == b + a: the same d in every lane
        if (d < best) {
          best = d;
          label = k;
        }
      }
      if (valid && octet == 0) {                                 // the read first, then the write, by the same lane
        const int prev = labels[p];
        labels[p] = (uint8_t)label;
        changed += prev != label;
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {                                // selects, not an indexed accumulator: registers, no scratch
      const bool mine = valid && label == k;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[k][j] += mine ? (double)x[j] : 0.0;
      cnt[k] += mine ? 1.0 : 0.0;
    }
  }
  // the lanes of the wave that hold the same octet: lane bits >= log2(Q)
  double ch = (double)changed;
  for (int s = 32; s >= Q; s >>= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[k][j] += __shfl_xor(acc[k][j], s, 64);
      cnt[k] += __shfl_xor(cnt[k], s, 64);
    }
    ch += __shfl_xor(ch, s, 64);
  }
  for (int i = threadIdx.x; i < row; i += kKfThreads) red[i] = 0.0;
  __syncthreads();
  for (int w = 0; w < kKfWaves; ++w) {                           // wave order
    if (wave == w && lane < Q) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[k * (C + 1) + 8 * lane + j] += acc[k][j];
        if (lane == 0) red[k * (C + 1) + C] += cnt[k];
      }
      if (lane == 0) red[row - 1] += ch;
    }
    __syncthreads();
  }
  double* out = parts + (size_t)blockIdx.x * row;
  for (int i = threadIdx.x; i < row; i += kKfThreads) out[i] = red[i];
}

// One work item per (k, c).  The rows of both images in index order; the c-fastest rows make the reads of neighbouring
// items neighbours.  Every item of a cluster adds the cluster's count column itself (256 broadcast reads per image).
__global__ __launch_bounds__(kKfThreads) void kmeans_feat_update_kernel(const double* __restrict__ parts_c, const double* __restrict__ parts_s,
                                                                        float* __restrict__ centroids, double* __restrict__ result,
                                                                        int n_c, int n_s, int C, int K) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * kKfThreads + threadIdx.x;
  if (i >= K * C) return;
  const int k = i / C, ch = i - k * C;
  const size_t row = (size_t)(4 * (C + 1) + 1);
  const size_t at = (size_t)k * (C + 1) + ch, at_n = (size_t)k * (C + 1) + C;
  double sc = parts_c[at], ss = parts_s[at], nc = parts_c[at_n], ns = parts_s[at_n];
  for (int r = 1; r < kKfParts; ++r) {
    sc += parts_c[r * row + at];
    ss += parts_s[r * row + at];
    nc += parts_c[r * row + at_n];
    ns += parts_s[r * row + at_n];
  }
  const double dc = (double)n_c, ds = (double)n_s;
  const double wc = nc / dc, ws = ns / ds;
  const double weight = wc + ws;
  if (weight > 0.0) {
    const double mc = sc / dc, ms = ss / ds;
    const double m = mc + ms;
    centroids[i] = (float)(m / weight);
  }
  if (ch == 0) {
    result[k] = nc;
    result[4 + k] = ns;
  }
  if (i == 0) {
    for (int q = K; q < kKfMaxK; ++q) result[q] = result[4 + q] = 0.0;
    double cc = parts_c[row - 1], cs = parts_s[row - 1];
    for (int r = 1; r < kKfParts; ++r) {
      cc += parts_c[r * row + row - 1];
      cs += parts_s[r * row + row - 1];
    }
    result[8] = cc + cs;
  }
}

template <typename T, int K>
void kf_launch(bool keep, hipStream_t st, const T* F, const float* centroids, uint8_t* labels, double* parts, int n, int C) {
  // every row of `parts` is written on every launch: always the full grid
  if (keep) hipLaunchKernelGGL((kmeans_feat_assign_kernel<T, K, true>), dim3(kKfParts), dim3(kKfThreads), 0, st, F, centroids, labels, parts, n, C);
  else hipLaunchKernelGGL((kmeans_feat_assign_kernel<T, K, false>), dim3(kKfParts), dim3(kKfThreads), 0, st, F, centroids, labels, parts, n, C);
}

template <typename T>
void kf_dispatch(int K, bool keep, hipStream_t st, const void* F, const float* centroids, uint8_t* labels, double* parts, int n, int C) {
  const T* f = static_cast<const T*>(F);
  switch (K) {
    case 1: kf_launch<T, 1>(keep, st, f, centroids, labels, parts, n, C); break;
    case 2: kf_launch<T, 2>(keep, st, f, centroids, labels, parts, n, C); break;
    case 3: kf_launch<T, 3>(keep, st, f, centroids, labels, parts, n, C); break;
    default: kf_launch<T, 4>(keep, st, f, centroids, labels, parts, n, C); break;
  }
}

// C = 64, 128, 256 or 512: Q = C/8 lanes per pixel must be a power of two - the octet is `lane & (Q - 1)`, a wave holds 64/Q
// whole pixels and both butterflies halve their offsets down to 1 or Q
bool kf_shape_ok(int C, int K) {
  return C >= 64 && C <= kKfMaxC && (C & (C - 1)) == 0 && K >= 1 && K <= kKfMaxK;
}
}  // namespace

extern "C" int stv_kmeans_feat_assign(const void* F, int dtype, const float* centroids, uint8_t* labels, double* parts, int n, int C,
                                      int K, int keep_labels, void* stream) {
  if (!F || !centroids || !labels || !parts || n < 1 || !kf_shape_ok(C, K)) return STV_ERR_ARG;
  if (dtype != STV_F32 && dtype != STV_BF16) return STV_ERR_ARG;
  if ((long long)n * C >= (1ll << 31) || (uintptr_t)F % 16 != 0) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == STV_BF16) kf_dispatch<bf16_t>(K, keep_labels != 0, st, F, centroids, labels, parts, n, C);
  else kf_dispatch<float>(K, keep_labels != 0, st, F, centroids, labels, parts, n, C);
  STV_CHECK_LAUNCH();
  return STV_OK;
}

extern "C" int stv_kmeans_feat_update(const double* parts_c, const double* parts_s, float* centroids, double* result, int n_c,
                                      int n_s, int C, int K, void* stream) {
  if (!parts_c || !parts_s || !centroids || !result || n_c < 1 || n_s < 1 || !kf_shape_ok(C, K)) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kmeans_feat_update_kernel, dim3(ceil_div(K * C, kKfThreads)), dim3(kKfThreads), 0, st, parts_c, parts_s,
                     centroids, result, n_c, n_s, C, K);
  STV_CHECK_LAUNCH();
  return STV_OK;
}
