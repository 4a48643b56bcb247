// HBM-bound pointwise / small-reduction kernels around the conv stacks:
// MaxPool2d(2,2) forward/backward, ReLU forward/backward, content MSE and its
// gradient (content_loss_kernel<T, GRAD>: the loss partials alone or, in the
// same loop, with the gradient written; content_grad_kernel: the gradient
// alone, scaled by a device scalar and optionally accumulated), the total
// variation of the image and its gradient, the 2x resize between the levels of
// a coarse-to-fine run, and the final score combine.  All activation traffic is
// 16-byte vectors per lane (1 KiB per wave instruction); grids are capped and
// grid-strided.
#include <string.h>

#include "stv_common.h"

namespace {

constexpr int kMaxBlocks = 256 * 8;

inline unsigned grid_for(size_t work_items) {
  size_t b = (work_items + 255) / 256;
  if (b < 1) b = 1;
  if (b > (size_t)kMaxBlocks) b = kMaxBlocks;
  return (unsigned)b;
}

// ---------------------------------------------------------------- max pool
// x: [H][W][C] -> y: [H/2][W/2][C] (floor), vectors of kVec channels.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                          int H, int W, int C) {
  constexpr int kVec = elem_traits<T>::kVec;
  const int Ho = H / 2, Wo = W / 2, CV = C / kVec;
  const size_t total = (size_t)Ho * Wo * CV;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
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
    for (int e = 0; e < kVec; ++e) o[e] = fmaxf(fmaxf(v00[e], v01[e]), fmaxf(v10[e], v11[e]));
    *reinterpret_cast<u32x4*>(y + p * C + cv * kVec) = pack16<T>(o);
  }
}

// dx[window] = dy routed to the first maximum in scan order (torch semantics),
// optionally masked by (x > 0) for a fused ReLU backward; rows/cols dropped by
// the floor get zero.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ x,
                                                          const T* __restrict__ dy, T* __restrict__ dx,
                                                          int H, int W, int C, int flags) {
  constexpr int kVec = elem_traits<T>::kVec;
  const int Ho = H / 2, Wo = W / 2, CV = C / kVec;
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;  // cover odd tails
  const bool mask = (flags & STV_MASK) != 0;
  const bool accum = (flags & STV_ACCUM) != 0;
  const size_t total = (size_t)Hc * Wc * CV;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int cv = (int)(i % CV);
    const size_t p = i / CV;
    const int ox = (int)(p % Wc), oy = (int)(p / Wc);
    const int iy = 2 * oy, ix = 2 * ox;
    const bool inside = oy < Ho && ox < Wo;
    float g[kVec], v[4][kVec], out[4][kVec];
#pragma unroll
    for (int e = 0; e < kVec; ++e) g[e] = 0.0f;
    if (inside) unpack16<T>(*reinterpret_cast<const u32x4*>(dy + ((size_t)oy * Wo + ox) * C + cv * kVec), g);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int yy = iy + (q >> 1), xx = ix + (q & 1);
      if (yy < H && xx < W)
        unpack16<T>(*reinterpret_cast<const u32x4*>(x + ((size_t)yy * W + xx) * C + cv * kVec), v[q]);
      else
#pragma unroll
        for (int e = 0; e < kVec; ++e) v[q][e] = 0.0f;
    }
#pragma unroll
    for (int e = 0; e < kVec; ++e) {
      int best = 0;
      float bv = v[0][e];
      // strict '>' keeps the first maximum; NaN wins like torch's (val > max || isnan(val))
#pragma unroll
      for (int q = 1; q < 4; ++q)
        if (v[q][e] > bv || (v[q][e] != v[q][e] && bv == bv)) { bv = v[q][e]; best = q; }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float gq = (inside && q == best) ? g[e] : 0.0f;
        if (mask && !(v[q][e] > 0.0f)) gq = 0.0f;
        out[q][e] = gq;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int yy = iy + (q >> 1), xx = ix + (q & 1);
      if (yy < H && xx < W) {
        T* o = dx + ((size_t)yy * W + xx) * C + cv * kVec;
        if (accum) {
          float old[kVec];
          unpack16<T>(*reinterpret_cast<const u32x4*>(o), old);
#pragma unroll
          for (int e = 0; e < kVec; ++e) out[q][e] += old[e];
        }
        *reinterpret_cast<u32x4*>(o) = pack16<T>(out[q]);
      }
    }
  }
}

// Same routing from the arg-max byte map of the fused conv+pool epilogue (one byte per pooled
// element: bits 0-1 = window position of the first maximum, bit 2 = maximum > 0): the pass reads
// dy and kVec bytes per window instead of four activation vectors.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_idx_kernel(const unsigned char* __restrict__ idx,
                                                              const T* __restrict__ dy, T* __restrict__ dx,
                                                              int H, int W, int C, int flags) {
  constexpr int kVec = elem_traits<T>::kVec;
  const int Ho = H / 2, Wo = W / 2, CV = C / kVec;
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;  // cover odd tails
  const bool mask = (flags & STV_MASK) != 0;
  const bool accum = (flags & STV_ACCUM) != 0;
  const size_t total = (size_t)Hc * Wc * CV;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int cv = (int)(i % CV);
    const size_t p = i / CV;
    const int ox = (int)(p % Wc), oy = (int)(p / Wc);
    const int iy = 2 * oy, ix = 2 * ox;
    const bool inside = oy < Ho && ox < Wo;
    float g[kVec], out[4][kVec];
    unsigned char code[kVec];
#pragma unroll
    for (int e = 0; e < kVec; ++e) { g[e] = 0.0f; code[e] = 0; }
    if (inside) {
      const size_t o = ((size_t)oy * Wo + ox) * C + cv * kVec;
      unpack16<T>(*reinterpret_cast<const u32x4*>(dy + o), g);
      if constexpr (kVec == 8) {
        const unsigned long long w = *reinterpret_cast<const unsigned long long*>(idx + o);
#pragma unroll
        for (int e = 0; e < 8; ++e) code[e] = (unsigned char)(w >> (8 * e));
      } else {
        const unsigned int w = *reinterpret_cast<const unsigned int*>(idx + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) code[e] = (unsigned char)(w >> (8 * e));
      }
    }
#pragma unroll
    for (int e = 0; e < kVec; ++e) {
      const bool live = inside && (!mask || (code[e] & 4));
#pragma unroll
      for (int q = 0; q < 4; ++q) out[q][e] = (live && (code[e] & 3) == q) ? g[e] : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int yy = iy + (q >> 1), xx = ix + (q & 1);
      if (yy < H && xx < W) {
        T* o = dx + ((size_t)yy * W + xx) * C + cv * kVec;
        if (accum) {
          float old[kVec];
          unpack16<T>(*reinterpret_cast<const u32x4*>(o), old);
#pragma unroll
          for (int e = 0; e < kVec; ++e) out[q][e] += old[e];
        }
        *reinterpret_cast<u32x4*>(o) = pack16<T>(out[q]);
      }
    }
  }
}

// scalar variants for channel counts that are not a multiple of the vector width
template <typename T>
__global__ void maxpool_fwd_scalar(const T* __restrict__ x, T* __restrict__ y, int H, int W, int C) {
  const int Ho = H / 2, Wo = W / 2;
  const size_t total = (size_t)Ho * Wo * C;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const size_t p = i / C;
    const int ox = (int)(p % Wo), oy = (int)(p / Wo);
    const T* b = x + ((size_t)(2 * oy) * W + 2 * ox) * C + c;
    const float m = fmaxf(fmaxf(elem_traits<T>::load(b), elem_traits<T>::load(b + C)),
                          fmaxf(elem_traits<T>::load(b + (size_t)W * C),
                                elem_traits<T>::load(b + (size_t)W * C + C)));
    elem_traits<T>::store(y + i, m);
  }
}
template <typename T>
__global__ void maxpool_bwd_scalar(const T* __restrict__ x, const T* __restrict__ dy,
                                   T* __restrict__ dx, int H, int W, int C, int flags) {
  const int Ho = H / 2, Wo = W / 2;
  const size_t total = (size_t)H * W * C;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const size_t p = i / C;
    const int xx = (int)(p % W), yy = (int)(p / W);
    const int oy = yy / 2, ox = xx / 2;
    float g = 0.0f;
    const float mine = elem_traits<T>::load(x + i);
    if (oy < Ho && ox < Wo) {
      int best = 0;
      float bv = 0.0f;
      for (int q = 0; q < 4; ++q) {
        const float v = elem_traits<T>::load(x + ((size_t)(2 * oy + (q >> 1)) * W + 2 * ox + (q & 1)) * C + c);
        if (q == 0 || v > bv || (v != v && bv == bv)) { bv = v; best = q; }
      }
      if (best == ((yy & 1) * 2 + (xx & 1))) g = elem_traits<T>::load(dy + ((size_t)oy * Wo + ox) * C + c);
    }
    if ((flags & STV_MASK) && !(mine > 0.0f)) g = 0.0f;
    if (flags & STV_ACCUM) g += elem_traits<T>::load(dx + i);
    elem_traits<T>::store(dx + i, g);
  }
}

// -------------------------------------------------------------------- relu
template <typename T>
__global__ __launch_bounds__(256) void relu_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, size_t n) {
  constexpr int kVec = elem_traits<T>::kVec;
  const size_t nv = n / kVec;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256)
    reinterpret_cast<u32x4*>(y)[i] = relu16<T>(reinterpret_cast<const u32x4*>(x)[i]);
  for (size_t i = nv * kVec + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    elem_traits<T>::store(y + i, fmaxf(elem_traits<T>::load(x + i), 0.0f));
}
template <typename T>
__global__ __launch_bounds__(256) void relu_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                       T* __restrict__ dx, size_t n, int flags) {
  const bool accum = (flags & STV_ACCUM) != 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float g = (elem_traits<T>::load(x + i) > 0.0f) ? elem_traits<T>::load(dy + i) : 0.0f;
    if (accum) g += elem_traits<T>::load(dx + i);
    elem_traits<T>::store(dx + i, g);
  }
}

// ----------------------------------------------------------------- content
// One partial sum per workgroup, STV_CONTENT_LOSS_PARTS workgroups (the caller's buffer has that many entries; they are
// added in index order by loss_combine).  Workgroups of 1,024 threads: 256 x 256 threads walking 25-50 MB were four waves
// per CU with one 16-byte load pair in flight each - 3.2 TB/s (15.7 us for 50 MB at 1024^2); sixteen waves per CU
// stream.  Per-thread sums are added wave by wave in fixed order: deterministic.
constexpr int kContentThreads = 1024;
__device__ __forceinline__ float block_sum_1024(float v, float* smem16) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) smem16[w] = v;
  __syncthreads();
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < kContentThreads / 64; ++i) s += smem16[i];
  return s;
}
// GRAD: loss and gradient of the content term in one pass over (F, target) - the same partial sums in the same order
// (same grid, same stride), and dF = coef * 2/n * (F - target) WRITTEN (the dgrad that produces this layer's gradient
// later accumulates onto it): one read of the two maps instead of two.
template <typename T, bool GRAD>
__global__ __launch_bounds__(kContentThreads) void content_loss_kernel(const T* __restrict__ f, const T* __restrict__ t,
                                                                       float* __restrict__ part, T* __restrict__ df, size_t n,
                                                                       float coef) {
  constexpr int kVec = elem_traits<T>::kVec;
  constexpr int BT = kContentThreads;
  __shared__ float red[BT / 64];
  float k = 0.0f;
  if constexpr (GRAD) k = coef * (2.0f / (float)n);
  float s = 0.0f;
  const size_t nv = n / kVec;
  for (size_t i = (size_t)blockIdx.x * BT + threadIdx.x; i < nv; i += (size_t)gridDim.x * BT) {
    float a[kVec], b[kVec];
    [[maybe_unused]] float o[kVec];
    unpack16<T>(reinterpret_cast<const u32x4*>(f)[i], a);
    unpack16<T>(reinterpret_cast<const u32x4*>(t)[i], b);
#pragma unroll
    for (int e = 0; e < kVec; ++e) {
      const float d = a[e] - b[e];
      s = fmaf(d, d, s);
      if constexpr (GRAD) o[e] = k * d;
    }
    if constexpr (GRAD) reinterpret_cast<u32x4*>(df)[i] = pack16<T>(o);
  }
  for (size_t i = nv * kVec + (size_t)blockIdx.x * BT + threadIdx.x; i < n; i += (size_t)gridDim.x * BT) {
    const float d = elem_traits<T>::load(f + i) - elem_traits<T>::load(t + i);
    s = fmaf(d, d, s);
    if constexpr (GRAD) elem_traits<T>::store(df + i, k * d);
  }
  s = block_sum_1024(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
template <typename T>
__global__ __launch_bounds__(256) void content_grad_kernel(const T* __restrict__ f, const T* __restrict__ t,
                                                           T* __restrict__ df, size_t n, float coef,
                                                           const float* __restrict__ coef_dev, int flags) {
  constexpr int kVec = elem_traits<T>::kVec;
  const float k = coef * (coef_dev ? *coef_dev : 1.0f) * (2.0f / (float)n);
  const bool accum = (flags & STV_ACCUM) != 0;
  const size_t nv = n / kVec;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
    float a[kVec], b[kVec], o[kVec];
    unpack16<T>(reinterpret_cast<const u32x4*>(f)[i], a);
    unpack16<T>(reinterpret_cast<const u32x4*>(t)[i], b);
    if (accum) unpack16<T>(reinterpret_cast<const u32x4*>(df)[i], o);
#pragma unroll
    for (int e = 0; e < kVec; ++e) o[e] = k * (a[e] - b[e]) + (accum ? o[e] : 0.0f);
    reinterpret_cast<u32x4*>(df)[i] = pack16<T>(o);
  }
  for (size_t i = nv * kVec + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float g = k * (elem_traits<T>::load(f + i) - elem_traits<T>::load(t + i));
    if (accum) g += elem_traits<T>::load(df + i);
    elem_traits<T>::store(df + i, g);
  }
}

// ---------------------------------------------------------- total variation
// TV(x) of the NCHW fp32 image and its gradient.  A work item is four consecutive pixels of one row (one 16-byte
// vector); items are numbered row by row over all C*H rows, and a pass of the capped grid covers kTvBlocks * kTvThreads
// consecutive items - whole rows side by side - so the rows above and below an item are read by a neighbouring
// workgroup in the same pass and come out of the L2.  kVec: W % 4 == 0 and 16-byte aligned bases, every row starts on
// a vector; otherwise the same items are walked with guarded scalar accesses (same partial sums in the same order).
// Loss partials: per thread in item order, then wave, then workgroup (block_sum_1024) - fixed order, no atomics;
// a workgroup without items writes 0.
constexpr int kTvThreads = 1024;
constexpr int kTvBlocks = STV_TV_LOSS_PARTS;
template <bool kVec, bool kLoss, bool kGrad>
__global__ __launch_bounds__(kTvThreads) void tv_kernel(const float* __restrict__ x, float* __restrict__ part,
                                                        float* __restrict__ dx, int rows, int H, int W, float coef,
                                                        int accum) {
  __shared__ float red[kTvThreads / 64];
  const int W4 = (W + 3) >> 2;
  const unsigned items = (unsigned)rows * (unsigned)W4;          // < 2^29: the entry point bounds C*H*W*4 bytes by 2 GiB
  float loss = 0.0f;
  for (unsigned i = blockIdx.x * kTvThreads + threadIdx.x; i < items; i += (unsigned)gridDim.x * kTvThreads) {
    const int r = (int)(i / (unsigned)W4);
    const int x0 = (int)(i - (unsigned)r * (unsigned)W4) * 4;
    const int y = r % H;
    const bool has_up = y > 0, has_down = y < H - 1;
    const float* row = x + (size_t)r * W;
    const int nv = kVec ? 4 : (W - x0 < 4 ? W - x0 : 4);          // pixels of this item inside the row
    float c[4], up[4], dn[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = up[k] = dn[k] = 0.0f;
    if constexpr (kVec) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + x0);
#pragma unroll
      for (int k = 0; k < 4; ++k) c[k] = v[k];
      if (kGrad && has_up) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(row - W + x0);
#pragma unroll
        for (int k = 0; k < 4; ++k) up[k] = u[k];
      }
      if (has_down) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(row + W + x0);
#pragma unroll
        for (int k = 0; k < 4; ++k) dn[k] = d[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < nv) {
          c[k] = row[x0 + k];
          if (kGrad && has_up) up[k] = row[x0 + k - W];
          if (has_down) dn[k] = row[x0 + k + W];
        }
      }
    }
    const float left = (kGrad && x0 > 0) ? row[x0 - 1] : 0.0f;
    const float right = (x0 + 4 < W) ? row[x0 + 4] : 0.0f;
    float out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      out[k] = 0.0f;
      if (k >= nv) continue;
      const int xx = x0 + k;
      const bool has_left = xx > 0, has_right = xx < W - 1;
      const float lv = k > 0 ? c[k - 1] : left;
      const float rv = k < 3 ? c[k + 1] : right;
      if constexpr (kLoss) {
        if (has_down) { const float d = dn[k] - c[k]; loss = fmaf(d, d, loss); }
        if (has_right) { const float d = rv - c[k]; loss = fmaf(d, d, loss); }
      }
      if constexpr (kGrad) {
        float s = 0.0f;                                            // existing differences, in the order up, down, left, right
        if (has_up) s = __fadd_rn(s, c[k] - up[k]);
        if (has_down) s = __fadd_rn(s, c[k] - dn[k]);
        if (has_left) s = __fadd_rn(s, c[k] - lv);
        if (has_right) s = __fadd_rn(s, c[k] - rv);
        out[k] = __fmul_rn(coef, s);                               // no contraction with the accumulate below
      }
    }
    if constexpr (kGrad) {
      float* o = dx + (size_t)r * W + x0;
      if constexpr (kVec) {
        f32x4 v;
        if (accum) {
          const f32x4 old = *reinterpret_cast<const f32x4*>(o);
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = __fadd_rn(old[k], out[k]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = out[k];
        }
        *reinterpret_cast<f32x4*>(o) = v;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < nv) o[k] = accum ? __fadd_rn(o[k], out[k]) : out[k];
      }
    }
  }
  if constexpr (kLoss) {
    loss = block_sum_1024(loss, red);
    if (threadIdx.x == 0) part[blockIdx.x] = loss;
  }
}

template <bool kVec>
void tv_launch(const float* x, float* part, float* dx, int rows, int H, int W, float coef, int accum, unsigned grid,
               hipStream_t st) {
  if (part && dx)
    hipLaunchKernelGGL((tv_kernel<kVec, true, true>), dim3(grid), dim3(kTvThreads), 0, st, x, part, dx, rows, H, W, coef, accum);
  else if (part)
    hipLaunchKernelGGL((tv_kernel<kVec, true, false>), dim3(grid), dim3(kTvThreads), 0, st, x, part, dx, rows, H, W, coef, accum);
  else
    hipLaunchKernelGGL((tv_kernel<kVec, false, true>), dim3(grid), dim3(kTvThreads), 0, st, x, part, dx, rows, H, W, coef, accum);
}

// ------------------------------------------------------------------ 2x resize
// The change of size between the levels of a coarse-to-fine run, NCHW fp32 -> NCHW fp32.  A work item is four consecutive
// OUTPUT pixels of one row (one 16-byte store); items are numbered row by row over all output rows of all planes, and a
// pass of the capped grid covers kResizeBlocks * kResizeThreads consecutive items.  kVec: every output row (and, where the
// inputs are read as vectors, every input row) starts on a 16-byte boundary and no row end is ragged; otherwise the same
// items are walked with guarded scalar accesses.  Every product and every sum is rounded on its own, in the order stv.h
// states, so the outputs are reproducible bit for bit: plain * and + under `fp contract(off)`.  (__fmul_rn / __fadd_rn
// would not do: the header defines them as x * y and x + y, compiled under the default contraction mode, and the compiler
// fuses the inlined pair into an FMA whatever the caller's pragma says.)
//   DOWN2: rows 2r and 2r + 1 of the input hold the window of output row r (H = 2 * Ho: planes stay apart by themselves).
//   UP2:   separable, columns first; near/far indices are clamped inside the row and inside the plane.
constexpr int kResizeThreads = STV_RESIZE_THREADS;
constexpr int kResizeBlocks = STV_RESIZE_MAX_BLOCKS;
typedef __attribute__((ext_vector_type(2))) float f32x2;
__device__ __forceinline__ float lerp_3_1(float near, float far) {
#pragma clang fp contract(off)
  const float a = 0.75f * near, b = 0.25f * far;
  return a + b;
}
template <int kMode, bool kVec>
__global__ __launch_bounds__(kResizeThreads) void resize2x_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                  int out_rows, int H, int W, int Ho, int Wo) {
#pragma clang fp contract(off)
  const int W4 = (Wo + 3) >> 2;
  const unsigned items = (unsigned)out_rows * (unsigned)W4;      // < 2^29: the entry point bounds both sizes by 2 GiB
  for (unsigned i = blockIdx.x * kResizeThreads + threadIdx.x; i < items; i += (unsigned)gridDim.x * kResizeThreads) {
    const int r = (int)(i / (unsigned)W4);
    const int x0 = (int)(i - (unsigned)r * (unsigned)W4) * 4;
    const int nv = kVec ? 4 : (Wo - x0 < 4 ? Wo - x0 : 4);        // pixels of this item inside the row
    float out[4];
    if constexpr (kMode == STV_RESIZE_DOWN2) {
      const float* top = x + (size_t)(2 * r) * W + 2 * x0;
      const float* bot = top + W;
      float t[8], b[8];
      if constexpr (kVec) {
        const f32x4 t0 = *reinterpret_cast<const f32x4*>(top), t1 = *reinterpret_cast<const f32x4*>(top + 4);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(bot), b1 = *reinterpret_cast<const f32x4*>(bot + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { t[k] = t0[k]; t[4 + k] = t1[k]; b[k] = b0[k]; b[4 + k] = b1[k]; }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const bool in = (k >> 1) < nv;
          t[k] = in ? top[k] : 0.0f;
          b[k] = in ? bot[k] : 0.0f;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        out[k] = ((t[2 * k] + t[2 * k + 1]) + (b[2 * k] + b[2 * k + 1])) * 0.25f;
    } else {
      const int c = r / Ho, yy = r - c * Ho;
      const int rn = yy >> 1;
      int rf = (yy & 1) ? rn + 1 : rn - 1;
      rf = rf < 0 ? 0 : (rf > H - 1 ? H - 1 : rf);
      const float* near = x + ((size_t)c * H + rn) * W;
      const float* far = x + ((size_t)c * H + rf) * W;
      // output columns x0 .. x0 + 3 read input columns a - 1 .. a + 2 (a = x0 / 2, even), clamped into the row
      const int a = x0 >> 1;
      const int cl = a > 0 ? a - 1 : 0;
      const int cr = a + 2 < W ? a + 2 : W - 1;
      float n[4], f[4];
      n[0] = near[cl]; f[0] = far[cl];
      n[3] = near[cr]; f[3] = far[cr];
      if constexpr (kVec) {
        const f32x2 nm = *reinterpret_cast<const f32x2*>(near + a), fm = *reinterpret_cast<const f32x2*>(far + a);
        n[1] = nm[0]; n[2] = nm[1]; f[1] = fm[0]; f[2] = fm[1];
      } else {
        const int a1 = a + 1 < W ? a + 1 : W - 1;
        n[1] = near[a]; f[1] = far[a];
        n[2] = near[a1]; f[2] = far[a1];
      }
      // (near, far) input column of the four outputs: (a, a-1), (a, a+1), (a+1, a), (a+1, a+2)
      const float hn[4] = {lerp_3_1(n[1], n[0]), lerp_3_1(n[1], n[2]), lerp_3_1(n[2], n[1]), lerp_3_1(n[2], n[3])};
      const float hf[4] = {lerp_3_1(f[1], f[0]), lerp_3_1(f[1], f[2]), lerp_3_1(f[2], f[1]), lerp_3_1(f[2], f[3])};
#pragma unroll
      for (int k = 0; k < 4; ++k) out[k] = lerp_3_1(hn[k], hf[k]);
    }
    float* o = y + (size_t)r * Wo + x0;
    if constexpr (kVec) {
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = out[k];
      *reinterpret_cast<f32x4*>(o) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nv) o[k] = out[k];
    }
  }
}

// ------------------------------------------------------------ score combine
// One workgroup of 1024 threads.  losses[k] = scale[k] * sum(parts[off..off+cnt)) with a
// fixed summation tree (deterministic); then the reference's sequential fp32
// stack().sum() per kind and the weighted total.
__global__ __launch_bounds__(1024) void loss_combine_kernel(const float* __restrict__ parts,
                                                            const int32_t* __restrict__ table,
                                                            const float* __restrict__ scale, int n_terms,
                                                            float style_w, float content_w,
                                                            float* __restrict__ losses, float* __restrict__ scores,
                                                            float* __restrict__ log_ring, int log_cap,
                                                            uint32_t* __restrict__ log_count, uint32_t* log_seq) {
  constexpr int MAXT = 64, NW = 16;
  __shared__ int s_off[MAXT], s_cnt[MAXT], s_kind[MAXT], s_start[MAXT + 1];
  __shared__ float s_scale[MAXT], s_term[MAXT];
  __shared__ double s_part[MAXT][NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = n_terms < MAXT ? n_terms : MAXT;        // the schedule never builds more (5 style + 1 content)
  if (tid < nt) {
    s_off[tid] = table[3 * tid];
    s_cnt[tid] = table[3 * tid + 1];
    s_kind[tid] = table[3 * tid + 2];
    s_scale[tid] = scale[tid];
  }
  for (int i = tid; i < nt * NW; i += 1024) s_part[i / NW][i % NW] = 0.0;
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int k = 0; k < nt; ++k) { s_start[k] = acc; acc += s_cnt[k]; }
    s_start[nt] = acc;
  }
  __syncthreads();
  // The partials of all terms form one virtual array; wave w reduces its 1/16 of it, term by
  // term, with every load of its share in flight at once (a lone wave walking an 8192-entry term
  // four loads at a time was the whole cost of this kernel).  Fixed assignment -> deterministic.
  const int total = s_start[nt];
  const int chunk = (total + NW - 1) / NW;
  const int lo = wave * chunk, hi = (lo + chunk < total) ? lo + chunk : total;
  for (int k = 0; k < nt; ++k) {
    const int a = s_start[k] > lo ? s_start[k] : lo;
    const int b = s_start[k + 1] < hi ? s_start[k + 1] : hi;
    if (a >= b) continue;                                    // wave-uniform
    const float* __restrict__ src = parts + s_off[k] - s_start[k];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int i = a + lane;
    for (; i + 192 < b; i += 256) {
      const float v0 = src[i], v1 = src[i + 64], v2 = src[i + 128], v3 = src[i + 192];
      s0 += (double)v0; s1 += (double)v1; s2 += (double)v2; s3 += (double)v3;
    }
    for (; i < b; i += 64) s0 += (double)src[i];
    const double tot = wave_sum_d((s0 + s1) + (s2 + s3));
    if (lane == 0) s_part[k][wave] = tot;
  }
  __syncthreads();
  if (tid < nt) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) tot += s_part[tid][w];
    const float v = (float)(tot * (double)s_scale[tid]);
    losses[tid] = v;
    s_term[tid] = v;
  }
  __syncthreads();
  if (tid == 0) {
    float style = 0.0f, content = 0.0f;
    for (int k = 0; k < nt; ++k) {
      if (s_kind[k] == 0) style += s_term[k];
      else if (s_kind[k] == 1) content += s_term[k];
    }
    float total_loss = style_w * style + content_w * content;
    // kind 2: a term on the image itself (total variation), weight already in its scale - joins the total only, in
    // index order, one fp32 add each
    for (int k = 0; k < nt; ++k)
      if (s_kind[k] == 2) total_loss += s_term[k];
    scores[0] = style;
    scores[1] = content;
    scores[2] = total_loss;
    scores[3] = (isfinite(style) && isfinite(content) && isfinite(total_loss)) ? 1.0f : 0.0f;
    if (log_ring) {          // per-evaluation history kept by the producer: slot = evaluations so far (mod capacity)
      const uint32_t k = *log_count;
      const uint32_t slot = k % (uint32_t)log_cap;
      if (log_seq) {
        // the ring lives in host memory the CPU reads while this step is still running: system-scope stores, then the
        // record count with release semantics - a reader that sees count k + 1 sees record k
        __hip_atomic_store(&log_ring[slot], style, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&log_ring[(size_t)log_cap + slot], content, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&log_ring[2 * (size_t)log_cap + slot], total_loss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        *log_count = k + 1;
        __hip_atomic_store(log_seq, k + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      } else {
        log_ring[slot] = style;
        log_ring[(size_t)log_cap + slot] = content;
        log_ring[2 * (size_t)log_cap + slot] = total_loss;
        *log_count = k + 1;
      }
    }
  }
}

template <typename T>
int pool_fwd_typed(const void* x, void* y, int H, int W, int C, hipStream_t st) {
  const size_t outs = (size_t)(H / 2) * (W / 2) * C;
  if (outs == 0) return STV_OK;
  if (C % elem_traits<T>::kVec == 0)
    hipLaunchKernelGGL(maxpool_fwd_kernel<T>, dim3(grid_for(outs / elem_traits<T>::kVec)), dim3(256), 0,
                       st, static_cast<const T*>(x), static_cast<T*>(y), H, W, C);
  else
    hipLaunchKernelGGL(maxpool_fwd_scalar<T>, dim3(grid_for(outs)), dim3(256), 0, st,
                       static_cast<const T*>(x), static_cast<T*>(y), H, W, C);
  STV_CHECK_LAUNCH();
  return STV_OK;
}
template <typename T>
int pool_bwd_typed(const void* x, const void* dy, void* dx, int H, int W, int C, int flags, hipStream_t st) {
  if (flags & STV_POOL_IDX) {
    if (C % elem_traits<T>::kVec) return STV_ERR_ARG;      // the byte map only exists for matrix-core shapes
    const size_t items = (size_t)((H + 1) / 2) * ((W + 1) / 2) * (C / elem_traits<T>::kVec);
    hipLaunchKernelGGL(maxpool_bwd_idx_kernel<T>, dim3(grid_for(items)), dim3(256), 0, st,
                       static_cast<const unsigned char*>(x), static_cast<const T*>(dy), static_cast<T*>(dx), H, W, C,
                       flags);
    STV_CHECK_LAUNCH();
    return STV_OK;
  }
  if (C % elem_traits<T>::kVec == 0) {
    const size_t items = (size_t)((H + 1) / 2) * ((W + 1) / 2) * (C / elem_traits<T>::kVec);
    hipLaunchKernelGGL(maxpool_bwd_kernel<T>, dim3(grid_for(items)), dim3(256), 0, st,
                       static_cast<const T*>(x), static_cast<const T*>(dy), static_cast<T*>(dx), H, W, C, flags);
  } else {
    hipLaunchKernelGGL(maxpool_bwd_scalar<T>, dim3(grid_for((size_t)H * W * C)), dim3(256), 0, st,
                       static_cast<const T*>(x), static_cast<const T*>(dy), static_cast<T*>(dx), H, W, C, flags);
  }
  STV_CHECK_LAUNCH();
  return STV_OK;
}


// ------------------------------------------------------------- frame export
// prepare_image_for_output + the uint8 conversion of the frame / PNG path (reference
// image_io.py:118-152, optimization.py:445-451, torchvision save_image at runtime/output.py:101):
//   v = x*std + mean (two roundings, as torch evaluates it) when `normalize`;
//   nan -> 0, +inf -> 1, -inf -> 0; clamp to [0,1];
//   round == 0: (uint8)(v*255)            (frames: numpy astype truncation)
//   round == 1: (uint8)clamp(v*255+0.5)   (save_image)
// x: NCHW fp32 [3][H][W] -> out: HWC uint8 [H][W][3].  One thread converts four pixels.
struct FrameStats { float mean[3], std[3]; };

__device__ __forceinline__ uint32_t frame_u8(float v, float mean, float stdv, int normalize, int round) {
#pragma clang fp contract(off)      // torch evaluates mul and add as two ops: an fma here changes last bits -> other bytes
  if (normalize) {
    const float scaled = v * stdv;
    v = scaled + mean;
  }
  if (v != v) v = 0.0f;
  v = fminf(fmaxf(v, 0.0f), 1.0f);                               // +-inf land on 1 / 0 like nan_to_num + clamp
  float s = v * 255.0f;
  if (round) {
    const float r = s + 0.5f;
    s = fminf(fmaxf(r, 0.0f), 255.0f);
  }
  return (uint32_t)s;
}

__global__ __launch_bounds__(256) void frame_u8_kernel(const float* __restrict__ x, uint8_t* __restrict__ out,
                                                       size_t npix, FrameStats st, int normalize, int round) {
  const size_t quads = (npix + 3) / 4;
  const bool vec_ok = (npix % 4) == 0;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (size_t)gridDim.x * 256) {
    const size_t p0 = q * 4;
    uint32_t b[12];
    if (vec_ok) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)c * npix + p0);
#pragma unroll
        for (int k = 0; k < 4; ++k) b[3 * k + c] = frame_u8(v[k], st.mean[c], st.std[c], normalize, round);
      }
      uint32_t w[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) w[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | (b[4 * j + 3] << 24);
      uint32_t* o = reinterpret_cast<uint32_t*>(out + p0 * 3);
      o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
    } else {
      for (int k = 0; k < 4 && p0 + k < npix; ++k)
        for (int c = 0; c < 3; ++c)
          out[(p0 + k) * 3 + c] = (uint8_t)frame_u8(x[(size_t)c * npix + p0 + k], st.mean[c], st.std[c], normalize, round);
    }
  }
}
}  // namespace

extern "C" int stv_maxpool_fwd(const void* x, void* y, int H, int W, int C, int dtype, void* stream) {
  if (!x || !y || H <= 0 || W <= 0 || C <= 0) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == STV_F32) return pool_fwd_typed<float>(x, y, H, W, C, st);
  if (dtype == STV_BF16) return pool_fwd_typed<bf16_t>(x, y, H, W, C, st);
  return STV_ERR_ARG;
}
extern "C" int stv_maxpool_bwd(const void* x, const void* dy, void* dx, int H, int W, int C, int flags,
                               int dtype, void* stream) {
  if (!x || !dy || !dx || H <= 0 || W <= 0 || C <= 0) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == STV_F32) return pool_bwd_typed<float>(x, dy, dx, H, W, C, flags, st);
  if (dtype == STV_BF16) return pool_bwd_typed<bf16_t>(x, dy, dx, H, W, C, flags, st);
  return STV_ERR_ARG;
}

extern "C" int stv_relu_fwd(const void* x, void* y, size_t n, int dtype, void* stream) {
  if (!x || !y) return STV_ERR_ARG;
  if (n == 0) return STV_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == STV_F32)
    hipLaunchKernelGGL(relu_fwd_kernel<float>, dim3(grid_for(n / 4 + 1)), dim3(256), 0, st,
                       static_cast<const float*>(x), static_cast<float*>(y), n);
  else if (dtype == STV_BF16)
    hipLaunchKernelGGL(relu_fwd_kernel<bf16_t>, dim3(grid_for(n / 8 + 1)), dim3(256), 0, st,
                       static_cast<const bf16_t*>(x), static_cast<bf16_t*>(y), n);
  else
    return STV_ERR_ARG;
  STV_CHECK_LAUNCH();
  return STV_OK;
}
extern "C" int stv_relu_bwd(const void* x, const void* dy, void* dx, size_t n, int flags, int dtype,
                            void* stream) {
  if (!x || !dy || !dx) return STV_ERR_ARG;
  if (n == 0) return STV_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == STV_F32)
    hipLaunchKernelGGL(relu_bwd_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st,
                       static_cast<const float*>(x), static_cast<const float*>(dy), static_cast<float*>(dx), n, flags);
  else if (dtype == STV_BF16)
    hipLaunchKernelGGL(relu_bwd_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st,
                       static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(dy), static_cast<bf16_t*>(dx), n, flags);
  else
    return STV_ERR_ARG;
  STV_CHECK_LAUNCH();
  return STV_OK;
}

// dF == nullptr: the loss partials alone
template <typename T>
static void launch_content_loss(const void* F, const void* target, float* loss_part, void* dF, size_t n, float coef, hipStream_t st) {
  const dim3 grid(STV_CONTENT_LOSS_PARTS), block(kContentThreads);
  const T* f = static_cast<const T*>(F);
  const T* t = static_cast<const T*>(target);
  if (dF) hipLaunchKernelGGL((content_loss_kernel<T, true>), grid, block, 0, st, f, t, loss_part, static_cast<T*>(dF), n, coef);
  else hipLaunchKernelGGL((content_loss_kernel<T, false>), grid, block, 0, st, f, t, loss_part, static_cast<T*>(nullptr), n, 0.0f);
}
static int content_loss(const void* F, const void* target, float* loss_part, void* dF, size_t n, float coef, int dtype,
                        void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == STV_F32) launch_content_loss<float>(F, target, loss_part, dF, n, coef, st);
  else if (dtype == STV_BF16) launch_content_loss<bf16_t>(F, target, loss_part, dF, n, coef, st);
  else return STV_ERR_ARG;
  STV_CHECK_LAUNCH();
  return STV_OK;
}
extern "C" int stv_content_loss(const void* F, const void* target, float* loss_part, size_t n, int dtype,
                                void* stream) {
  if (!F || !target || !loss_part || n == 0) return STV_ERR_ARG;
  return content_loss(F, target, loss_part, nullptr, n, 0.0f, dtype, stream);
}
extern "C" int stv_content_loss_grad(const void* F, const void* target, float* loss_part, void* dF, size_t n, float coef,
                                     int dtype, void* stream) {
  if (!F || !target || !loss_part || !dF || n == 0) return STV_ERR_ARG;
  return content_loss(F, target, loss_part, dF, n, coef, dtype, stream);
}
extern "C" int stv_content_grad(const void* F, const void* target, void* dF, size_t n, float coef,
                                const float* coef_dev, int flags, int dtype, void* stream) {
  if (!F || !target || !dF || n == 0) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == STV_F32)
    hipLaunchKernelGGL(content_grad_kernel<float>, dim3(grid_for(n / 4 + 1)), dim3(256), 0, st,
                       static_cast<const float*>(F), static_cast<const float*>(target),
                       static_cast<float*>(dF), n, coef, coef_dev, flags);
  else if (dtype == STV_BF16)
    hipLaunchKernelGGL(content_grad_kernel<bf16_t>, dim3(grid_for(n / 8 + 1)), dim3(256), 0, st,
                       static_cast<const bf16_t*>(F), static_cast<const bf16_t*>(target),
                       static_cast<bf16_t*>(dF), n, coef, coef_dev, flags);
  else
    return STV_ERR_ARG;
  STV_CHECK_LAUNCH();
  return STV_OK;
}

extern "C" int stv_tv(const float* x_nchw, float* loss_part, float* dx_nchw, int C, int H, int W, float coef, int flags,
                      void* stream) {
  if (!x_nchw || (!loss_part && !dx_nchw) || C <= 0 || H <= 0 || W <= 0 || x_nchw == dx_nchw) return STV_ERR_ARG;
  if ((unsigned long long)C * (unsigned long long)H * (unsigned long long)W * 4ull >= (1ull << 31)) return STV_ERR_ARG;
  if (flags & ~STV_ACCUM) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rows = C * H;
  const size_t items = (size_t)rows * ((W + 3) / 4);
  // every loss partial is written on every launch: the loss form always runs the full grid
  size_t grid = loss_part ? (size_t)kTvBlocks : (items + kTvThreads - 1) / kTvThreads;
  if (grid > (size_t)kTvBlocks) grid = kTvBlocks;
  const bool vec = (W % 4 == 0) && ((uintptr_t)x_nchw % 16 == 0) && ((uintptr_t)dx_nchw % 16 == 0);
  if (vec)
    tv_launch<true>(x_nchw, loss_part, dx_nchw, rows, H, W, coef, (flags & STV_ACCUM) != 0, (unsigned)grid, st);
  else
    tv_launch<false>(x_nchw, loss_part, dx_nchw, rows, H, W, coef, (flags & STV_ACCUM) != 0, (unsigned)grid, st);
  STV_CHECK_LAUNCH();
  return STV_OK;
}

extern "C" int stv_resize2x(const float* x, float* y, int C, int H, int W, int mode, void* stream) {
  if (!x || !y || x == y || C <= 0 || H <= 0 || W <= 0) return STV_ERR_ARG;
  if (mode != STV_RESIZE_DOWN2 && mode != STV_RESIZE_UP2) return STV_ERR_ARG;
  const bool down = mode == STV_RESIZE_DOWN2;
  if (down && ((H | W) & 1)) return STV_ERR_ARG;
  const unsigned long long in_bytes = (unsigned long long)C * (unsigned long long)H * (unsigned long long)W * 4ull;
  if (in_bytes >= (1ull << 31) || (!down && in_bytes * 4ull >= (1ull << 31))) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int Ho = down ? H / 2 : 2 * H, Wo = down ? W / 2 : 2 * W;
  const int out_rows = C * Ho;
  const size_t items = (size_t)out_rows * ((Wo + 3) / 4);
  size_t grid = (items + kResizeThreads - 1) / kResizeThreads;
  if (grid > (size_t)kResizeBlocks) grid = kResizeBlocks;
  // all rows start on a vector: output rows of Wo % 4 == 0 floats (then input rows are 8-byte multiples for UP2, 16-byte
  // multiples for DOWN2) behind 16-byte aligned bases
  const bool vec = (Wo % 4 == 0) && ((uintptr_t)x % 16 == 0) && ((uintptr_t)y % 16 == 0);
  const dim3 g((unsigned)grid), b(kResizeThreads);
  if (down && vec)
    hipLaunchKernelGGL((resize2x_kernel<STV_RESIZE_DOWN2, true>), g, b, 0, st, x, y, out_rows, H, W, Ho, Wo);
  else if (down)
    hipLaunchKernelGGL((resize2x_kernel<STV_RESIZE_DOWN2, false>), g, b, 0, st, x, y, out_rows, H, W, Ho, Wo);
  else if (vec)
    hipLaunchKernelGGL((resize2x_kernel<STV_RESIZE_UP2, true>), g, b, 0, st, x, y, out_rows, H, W, Ho, Wo);
  else
    hipLaunchKernelGGL((resize2x_kernel<STV_RESIZE_UP2, false>), g, b, 0, st, x, y, out_rows, H, W, Ho, Wo);
  STV_CHECK_LAUNCH();
  return STV_OK;
}

extern "C" int stv_loss_combine_log(const float* parts, const int32_t* table, const float* scale, int n_terms,
                                    float style_w, float content_w, float* losses, float* scores, float* log_ring,
                                    int log_capacity, uint32_t* log_count, uint32_t* log_seq, void* stream) {
  if (!parts || !table || !scale || !losses || !scores || n_terms < 0) return STV_ERR_ARG;
  if (n_terms > 64) return STV_ERR_ARG;
  if ((log_ring == nullptr) != (log_count == nullptr) || (log_ring && log_capacity <= 0)) return STV_ERR_ARG;
  if (log_seq && !log_ring) return STV_ERR_ARG;
  hipLaunchKernelGGL(loss_combine_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), parts,
                     table, scale, n_terms, style_w, content_w, losses, scores, log_ring, log_capacity, log_count, log_seq);
  STV_CHECK_LAUNCH();
  return STV_OK;
}

// Host memory the GPU writes while the CPU reads (the loss history of a run in flight): pinned, mapped into the device's
// address space under the same pointer, fine-grained coherent.  Zeroed.
extern "C" int stv_host_mailbox_alloc(size_t bytes, void** out) {
  if (!out || bytes == 0) return STV_ERR_ARG;
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess || !p) {
    (void)hipGetLastError();
    return STV_ERR_ALLOC;
  }
  memset(p, 0, bytes);
  *out = p;
  return STV_OK;
}

extern "C" void stv_host_mailbox_free(void* p) {
  if (p) (void)hipHostFree(p);
}

extern "C" int stv_loss_combine(const float* parts, const int32_t* table, const float* scale, int n_terms,
                                float style_w, float content_w, float* losses, float* scores, void* stream) {
  return stv_loss_combine_log(parts, table, scale, n_terms, style_w, content_w, losses, scores, nullptr, 0, nullptr, nullptr, stream);
}

extern "C" int stv_image_to_u8(const float* x_nchw, uint8_t* out_hwc, int H, int W, const float* mean3,
                               const float* std3, int round, void* stream) {
  if (!x_nchw || !out_hwc || H <= 0 || W <= 0 || (round != 0 && round != 1)) return STV_ERR_ARG;
  if ((mean3 == nullptr) != (std3 == nullptr)) return STV_ERR_ARG;
  FrameStats st{};
  const int normalize = mean3 != nullptr;
  for (int c = 0; c < 3 && normalize; ++c) { st.mean[c] = mean3[c]; st.std[c] = std3[c]; }   // HOST arrays
  const size_t npix = (size_t)H * W;
  hipLaunchKernelGGL(frame_u8_kernel, dim3(grid_for((npix + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     x_nchw, out_hwc, npix, st, normalize, round);
  STV_CHECK_LAUNCH();
  return STV_OK;
}
