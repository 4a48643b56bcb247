// AvgPool2d(2, 2) forward / backward on NHWC maps (--pooling avg; Gatys et al. 2016 pool by the mean instead of the maximum).
//   x: [H][W][C] -> y: [Hp][Wp][C],  Hp = H / 2, Wp = W / 2 (floor: an odd last row / column takes no part).
// Forward, per channel, in fp32, every sum rounded on its own (there is no product in front of a sum: nothing to contract):
//   y[i,j] = (((x[2i,2j] + x[2i,2j+1]) + x[2i+1,2j]) + x[2i+1,2j+1]) * 0.25f        rounded once to the storage type;
//   with STV_RELU_IN each operand is max(0, x) first.  This is the order of torch's CPU avg_pool2d, bit for bit.
// Backward:
//   v = 0.25f * dy[y/2, x/2] for y < 2*Hp and x < 2*Wp, else 0;  STV_MASK: v = 0 where !(ref > 0);
//   dx = v, or with STV_ACCUM dx = dx + v (one fp32 sum, rounded once to storage).  Without STV_ACCUM the rows and columns
//   the floor drops are written +0; with it they are not touched.
// The walk: a work item is 16 bytes of channels (kVec elements) of one pooled pixel (forward: four 16-byte loads, one
// store) or of one 2x2 window of the un-pooled map, odd tails included (backward: one load of dy, up to four of ref and of
// dx, up to four stores); consecutive lanes take consecutive channel vectors, then consecutive pixels of a row, so a wave
// instruction covers contiguous bytes.  A pass of the capped grid covers kBlocks * kThreads items.  Vector path: C a
// multiple of kVec behind 16-byte aligned bases; otherwise the scalar path - a work item is one element (forward: of y,
// backward: of dx), the same rule.  Offsets: every tensor is under 2 GiB, indices are size_t.
#include <hip/hip_runtime.h>

#include "stv_common.h"

namespace {

constexpr int kThreads = STV_AVGPOOL_THREADS;
constexpr int kBlocks = STV_AVGPOOL_MAX_BLOCKS;

inline unsigned grid_for(size_t items) {
  size_t b = (items + kThreads - 1) / kThreads;
  if (b < 1) b = 1;
  if (b > (size_t)kBlocks) b = kBlocks;
  return (unsigned)b;
}

__device__ __forceinline__ float mean4(float a, float b, float c, float d, bool relu) {
#pragma clang fp contract(off)
  if (relu) {
    a = fmaxf(a, 0.0f);
    b = fmaxf(b, 0.0f);
    c = fmaxf(c, 0.0f);
    d = fmaxf(d, 0.0f);
  }
  const float s0 = a + b;
  const float s1 = s0 + c;
  const float s2 = s1 + d;
  return s2 * 0.25f;
}

// the backward value of one element: g = 0.25f * dy (0 outside the pooled range), masked, optionally added to `old`
__device__ __forceinline__ float spread(float g, float ref, float old, bool mask, bool accum) {
#pragma clang fp contract(off)
  float v = g;
  if (mask && !(ref > 0.0f)) v = 0.0f;
  if (accum) {
    const float s = old + v;
    v = s;
  }
  return v;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void avgpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int H, int W, int C,
                                                               int relu) {
  constexpr int kVec = elem_traits<T>::kVec;
  const int Ho = H / 2, Wo = W / 2, CV = C / kVec;
  const size_t total = (size_t)Ho * Wo * CV;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    const int cv = (int)(i % CV);
    const size_t p = i / CV;
    const int ox = (int)(p % Wo), oy = (int)(p / Wo);
    const T* b = x + ((size_t)(2 * oy) * W + 2 * ox) * C + cv * kVec;
    float v00[kVec], v01[kVec], v10[kVec], v11[kVec], o[kVec];
    unpack16<T>(*reinterpret_cast<const u32x4*>(b), v00);
    unpack16<T>(*reinterpret_cast<const u32x4*>(b + C), v01);
    unpack16<T>(*reinterpret_cast<const u32x4*>(b + (size_t)W * C), v10);
    unpack16<T>(*reinterpret_cast<const u32x4*>(b + (size_t)W * C + C), v11);
#pragma unroll
    for (int e = 0; e < kVec; ++e) o[e] = mean4(v00[e], v01[e], v10[e], v11[e], relu != 0);
    *reinterpret_cast<u32x4*>(y + p * C + cv * kVec) = pack16<T>(o);
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void avgpool_bwd_kernel(const T* __restrict__ ref, const T* __restrict__ dy,
                                                               T* __restrict__ dx, int H, int W, int C, int flags) {
  constexpr int kVec = elem_traits<T>::kVec;
  const int Ho = H / 2, Wo = W / 2, CV = C / kVec;
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;  // cover odd tails
  const bool mask = (flags & STV_MASK) != 0;
  const bool accum = (flags & STV_ACCUM) != 0;
  const size_t total = (size_t)Hc * Wc * CV;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    const int cv = (int)(i % CV);
    const size_t p = i / CV;
    const int ox = (int)(p % Wc), oy = (int)(p / Wc);
    const int iy = 2 * oy, ix = 2 * ox;
    float g[kVec];
#pragma unroll
    for (int e = 0; e < kVec; ++e) g[e] = 0.0f;
    if (oy < Ho && ox < Wo) {
      unpack16<T>(*reinterpret_cast<const u32x4*>(dy + ((size_t)oy * Wo + ox) * C + cv * kVec), g);
#pragma unroll
      for (int e = 0; e < kVec; ++e) g[e] = 0.25f * g[e];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int yy = iy + (q >> 1), xx = ix + (q & 1);
      if (yy >= H || xx >= W) continue;
      if (accum && (yy >= 2 * Ho || xx >= 2 * Wo)) continue;      // the dropped rows / columns keep what they hold
      const size_t off = ((size_t)yy * W + xx) * C + cv * kVec;
      float r[kVec], old[kVec], out[kVec];
#pragma unroll
      for (int e = 0; e < kVec; ++e) { r[e] = 0.0f; old[e] = 0.0f; }
      if (mask) unpack16<T>(*reinterpret_cast<const u32x4*>(ref + off), r);
      if (accum) unpack16<T>(*reinterpret_cast<const u32x4*>(dx + off), old);
#pragma unroll
      for (int e = 0; e < kVec; ++e) out[e] = spread(g[e], r[e], old[e], mask, accum);
      *reinterpret_cast<u32x4*>(dx + off) = pack16<T>(out);
    }
  }
}

// scalar variants: channel counts that are not a multiple of the vector width, or bases off a 16-byte boundary
template <typename T>
__global__ __launch_bounds__(kThreads) void avgpool_fwd_scalar(const T* __restrict__ x, T* __restrict__ y, int H, int W, int C,
                                                               int relu) {
  const int Ho = H / 2, Wo = W / 2;
  const size_t total = (size_t)Ho * Wo * C;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    const int c = (int)(i % C);
    const size_t p = i / C;
    const int ox = (int)(p % Wo), oy = (int)(p / Wo);
    const T* b = x + ((size_t)(2 * oy) * W + 2 * ox) * C + c;
    const float m = mean4(elem_traits<T>::load(b), elem_traits<T>::load(b + C), elem_traits<T>::load(b + (size_t)W * C),
                          elem_traits<T>::load(b + (size_t)W * C + C), relu != 0);
    elem_traits<T>::store(y + i, m);
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void avgpool_bwd_scalar(const T* __restrict__ ref, const T* __restrict__ dy,
                                                               T* __restrict__ dx, int H, int W, int C, int flags) {
  const int Ho = H / 2, Wo = W / 2;
  const bool mask = (flags & STV_MASK) != 0;
  const bool accum = (flags & STV_ACCUM) != 0;
  const size_t total = (size_t)H * W * C;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    const int c = (int)(i % C);
    const size_t p = i / C;
    const int xx = (int)(p % W), yy = (int)(p / W);
    const bool inside = yy < 2 * Ho && xx < 2 * Wo;
    if (accum && !inside) continue;
    float g = 0.0f;
    if (inside) g = 0.25f * elem_traits<T>::load(dy + ((size_t)(yy / 2) * Wo + xx / 2) * C + c);
    const float r = mask ? elem_traits<T>::load(ref + i) : 0.0f;
    const float old = accum ? elem_traits<T>::load(dx + i) : 0.0f;
    elem_traits<T>::store(dx + i, spread(g, r, old, mask, accum));
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T>
int fwd_typed(const void* x, void* y, int H, int W, int C, int flags, hipStream_t st) {
  const size_t outs = (size_t)(H / 2) * (W / 2) * C;
  const int relu = (flags & STV_RELU_IN) ? 1 : 0;
  if (C % elem_traits<T>::kVec == 0 && aligned16(x) && aligned16(y))
    hipLaunchKernelGGL(avgpool_fwd_kernel<T>, dim3(grid_for(outs / elem_traits<T>::kVec)), dim3(kThreads), 0, st,
                       static_cast<const T*>(x), static_cast<T*>(y), H, W, C, relu);
  else
    hipLaunchKernelGGL(avgpool_fwd_scalar<T>, dim3(grid_for(outs)), dim3(kThreads), 0, st, static_cast<const T*>(x),
                       static_cast<T*>(y), H, W, C, relu);
  STV_CHECK_LAUNCH();
  return STV_OK;
}

template <typename T>
int bwd_typed(const void* ref, const void* dy, void* dx, int H, int W, int C, int flags, hipStream_t st) {
  if (C % elem_traits<T>::kVec == 0 && aligned16(dy) && aligned16(dx) && (!(flags & STV_MASK) || aligned16(ref))) {
    const size_t items = (size_t)((H + 1) / 2) * ((W + 1) / 2) * (C / elem_traits<T>::kVec);
    hipLaunchKernelGGL(avgpool_bwd_kernel<T>, dim3(grid_for(items)), dim3(kThreads), 0, st, static_cast<const T*>(ref),
                       static_cast<const T*>(dy), static_cast<T*>(dx), H, W, C, flags);
  } else {
    hipLaunchKernelGGL(avgpool_bwd_scalar<T>, dim3(grid_for((size_t)H * W * C)), dim3(kThreads), 0, st,
                       static_cast<const T*>(ref), static_cast<const T*>(dy), static_cast<T*>(dx), H, W, C, flags);
  }
  STV_CHECK_LAUNCH();
  return STV_OK;
}

// sizes a launch can take: positive, a pooled map that exists, the un-pooled tensor (the largest one) under 2 GiB
bool sizes_ok(int H, int W, int C, int dtype) {
  if (H <= 0 || W <= 0 || C <= 0 || H / 2 == 0 || W / 2 == 0) return false;
  const unsigned long long es = dtype == STV_BF16 ? 2 : 4;
  const unsigned long long hw = (unsigned long long)H * (unsigned long long)W;
  if (hw >= (1ull << 31)) return false;
  return hw * (unsigned long long)C * es < (1ull << 31);
}

}  // namespace

extern "C" int stv_avgpool_fwd(const void* x, void* y, int H, int W, int C, int flags, int dtype, void* stream) {
  if (dtype != STV_F32 && dtype != STV_BF16) return STV_ERR_ARG;
  if (!x || !y || (flags & ~STV_RELU_IN) || !sizes_ok(H, W, C, dtype)) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == STV_F32) return fwd_typed<float>(x, y, H, W, C, flags, st);
  return fwd_typed<bf16_t>(x, y, H, W, C, flags, st);
}

extern "C" int stv_avgpool_bwd(const void* ref, const void* dy, void* dx, int H, int W, int C, int flags, int dtype,
                               void* stream) {
  if (dtype != STV_F32 && dtype != STV_BF16) return STV_ERR_ARG;
  if (!dy || !dx || (flags & ~(STV_MASK | STV_ACCUM)) || ((flags & STV_MASK) && !ref) || !sizes_ok(H, W, C, dtype))
    return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == STV_F32) return bwd_typed<float>(ref, dy, dx, H, W, C, flags, st);
  return bwd_typed<bf16_t>(ref, dy, dx, H, W, C, flags, st);
}
