// Laplacian loss of the image against the content image (Li et al., "Laplacian-steered neural style transfer", 2017): for a
// pool size p the NCHW fp32 image is box-pooled to [C][Hp][Wp] cells (Hp = H / p, Wp = W / p, rows and columns past Hp*p
// and Wp*p take no part), e = P(x) - P(content), r = L e with L the 5-point graph Laplacian over the pooled grid (tv_kernel's
// stencil: the sum over the EXISTING 4-neighbours n of (e - n), inside one plane), lap(x) = sum r^2 / (C*Hp*Wp) and
// d lap / dx[c,y,x] = 2 / (C*Hp*Wp*p*p) * (L r)[c, y/p, x/p].  Three modes of one entry point, stv_lap:
//   POOL  one cell per thread: the cell means of the content image, captured once as the target.
//   LOSS  a workgroup owns a tile of kLapTileH x kLapTileW cells of one plane.  It forms e for the tile and a one-cell halo in
//         LDS (halo cells outside the plane do not exist and are not formed: the stencil never asks for them), and after a
//         barrier one thread per cell forms r from LDS, stores it and adds r^2 to its sum.  e is fixed to the bit, so the
//         halo cells a neighbouring workgroup recomputes agree with that workgroup's own.  The grid is always
//         STV_LAP_LOSS_PARTS workgroups with a stride loop over the tiles: one partial per workgroup, every partial written
//         on every launch (a workgroup without tiles writes 0), fixed order (thread in tile order, wave, workgroup), no atomics.
//   GRAD  a work item is four consecutive pixels of one image row, items numbered row by row (stv_tv's walk): g = L r at
//         the pixel's cell, out = coef * g, dx = out or dx + out.  kVec (W % 4 == 0, 16-byte aligned bases): one 16-byte
//         load / store per item, and for p >= 4 one stencil for the whole vector (its pixels share a cell, and a vector is
//         covered whole or not at all); otherwise guarded scalar accesses with the same values.
// Arithmetic, fixed to the bit (stv.h states it; the convention above resize2x_kernel in pointwise.hip: plain * and + under
// `fp contract(off)`): every add, subtraction and product is rounded to fp32 on its own.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "stv_common.h"

namespace {

constexpr int kLapThreads = STV_LAP_THREADS;
constexpr int kLapTileH = STV_LAP_TILE_H;
constexpr int kLapTileW = STV_LAP_TILE_W;
constexpr int kLapLossBlocks = STV_LAP_LOSS_PARTS;
constexpr int kLapGradBlocks = STV_LAP_GRAD_MAX_BLOCKS;
constexpr int kLapHaloH = kLapTileH + 2;
constexpr int kLapHaloW = kLapTileW + 2;
static_assert(kLapTileH * kLapTileW == kLapThreads, "one thread per cell of a tile");
typedef __attribute__((ext_vector_type(2))) float f32x2;

// Mean of cell (cy, cx) of one plane: each of the p rows summed left to right, the row sums summed top to bottom (the first
// element starts a sum), then * 1/p^2 - a power of two, exact.  kVec: every row of the image starts on a 16-byte boundary,
// so a cell's row does for p >= 4 (and on an 8-byte one for p = 2).  The pool size is a template argument: the loads of a
// cell row are all issued before the first add needs one, and the row loop is unrolled by kLapRowUnroll, so a thread keeps up
// to kLapRowUnroll * p / 4 vector loads in flight - with few workgroups on the chip (large pools) the kernel is bound by that.
constexpr int kLapRowUnroll = 4;
template <bool kVec, int p>
__device__ __forceinline__ float lap_cell_mean(const float* __restrict__ plane, int W, int cy, int cx) {
#pragma clang fp contract(off)
  const float* q = plane + (size_t)(cy * p) * W + (size_t)cx * p;
  float total = 0.0f;
#pragma unroll kLapRowUnroll
  for (int j = 0; j < p; ++j, q += W) {
    float row;
    if constexpr (kVec && p >= 4) {
      f32x4 v[p / 4];
#pragma unroll
      for (int k = 0; k < p / 4; ++k) v[k] = *reinterpret_cast<const f32x4*>(q + 4 * k);
      row = ((v[0][0] + v[0][1]) + v[0][2]) + v[0][3];
#pragma unroll
      for (int k = 1; k < p / 4; ++k) row = (((row + v[k][0]) + v[k][1]) + v[k][2]) + v[k][3];
    } else if constexpr (kVec && p == 2) {
      const f32x2 v = *reinterpret_cast<const f32x2*>(q);
      row = v[0] + v[1];
    } else {
      row = q[0];
#pragma unroll
      for (int k = 1; k < p; ++k) row = row + q[k];
    }
    total = j == 0 ? row : total + row;
  }
  return total * (1.0f / (float)(p * p));
}

// (L v)[cy, cx] over a grid of Hp x Wp with row stride `stride`, `at` pointing at [cy, cx]: from +0, the existing
// differences in the order up, down, left, right
__device__ __forceinline__ float lap_stencil(const float* at, int stride, int cy, int cx, int Hp, int Wp) {
#pragma clang fp contract(off)
  const float v = at[0];
  float s = 0.0f;
  if (cy > 0) s = s + (v - at[-stride]);
  if (cy < Hp - 1) s = s + (v - at[stride]);
  if (cx > 0) s = s + (v - at[-1]);
  if (cx < Wp - 1) s = s + (v - at[1]);
  return s;
}

template <bool kVec, int p>
__global__ __launch_bounds__(kLapThreads) void lap_pool_kernel(const float* __restrict__ x, float* __restrict__ cells, int C,
                                                               int H, int W, int Hp, int Wp) {
  const unsigned n = (unsigned)C * (unsigned)Hp * (unsigned)Wp;      // < 2^29: the entry point bounds C*H*W*4 bytes by 2 GiB
  for (unsigned i = blockIdx.x * kLapThreads + threadIdx.x; i < n; i += (unsigned)gridDim.x * kLapThreads) {
    const int row = (int)(i / (unsigned)Wp);
    const int cx = (int)(i - (unsigned)row * (unsigned)Wp);
    const int c = row / Hp, cy = row - c * Hp;
    cells[i] = lap_cell_mean<kVec, p>(x + (size_t)c * H * W, W, cy, cx);
  }
}

template <bool kVec, int p>
__global__ __launch_bounds__(kLapThreads) void lap_loss_kernel(const float* __restrict__ x, const float* __restrict__ target,
                                                               float* __restrict__ resid, float* __restrict__ part, int C,
                                                               int H, int W, int Hp, int Wp, int tiles_y, int tiles_x) {
#pragma clang fp contract(off)
  __shared__ float e[kLapHaloH][kLapHaloW + 1];
  __shared__ float red[kLapThreads / 64];
  const int per_plane = tiles_y * tiles_x;
  const int n_tiles = C * per_plane;                                 // <= C*Hp*Wp < 2^29
  const int ly = threadIdx.x / kLapTileW, lx = threadIdx.x - ly * kLapTileW;
  float loss = 0.0f;
  for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int c = t / per_plane;
    const int ty = (t - c * per_plane) / tiles_x, tx = t - c * per_plane - ty * tiles_x;
    const int cy0 = ty * kLapTileH, cx0 = tx * kLapTileW;
    const float* plane = x + (size_t)c * H * W;
    const float* tplane = target + (size_t)c * Hp * Wp;
    for (int idx = threadIdx.x; idx < kLapHaloH * kLapHaloW; idx += kLapThreads) {
      const int hy = idx / kLapHaloW, hx = idx - hy * kLapHaloW;
      const int cy = cy0 - 1 + hy, cx = cx0 - 1 + hx;
      if (cy >= 0 && cy < Hp && cx >= 0 && cx < Wp)
        e[hy][hx] = lap_cell_mean<kVec, p>(plane, W, cy, cx) - tplane[(size_t)cy * Wp + cx];
    }
    __syncthreads();
    const int cy = cy0 + ly, cx = cx0 + lx;
    if (cy < Hp && cx < Wp) {
      const float r = lap_stencil(&e[ly + 1][lx + 1], kLapHaloW + 1, cy, cx, Hp, Wp);
      resid[(size_t)c * Hp * Wp + (size_t)cy * Wp + cx] = r;
      const float sq = r * r;
      loss = loss + sq;
    }
    __syncthreads();                                                  // the next tile overwrites e
  }
  loss = block_sum_256(loss, red);
  if (threadIdx.x == 0) part[blockIdx.x] = loss;
}

template <bool kVec>
__global__ __launch_bounds__(kLapThreads) void lap_grad_kernel(const float* __restrict__ resid, float* __restrict__ dx, int rows,
                                                               int H, int W, int Hp, int Wp, int p, int log2p, float coef,
                                                               int accum) {
#pragma clang fp contract(off)
  const int W4 = (W + 3) >> 2;
  const unsigned items = (unsigned)rows * (unsigned)W4;              // < 2^29
  const int Hc = Hp << log2p, Wc = Wp << log2p;                      // the covered part of a plane
  for (unsigned i = blockIdx.x * kLapThreads + threadIdx.x; i < items; i += (unsigned)gridDim.x * kLapThreads) {
    const int row = (int)(i / (unsigned)W4);
    const int x0 = (int)(i - (unsigned)row * (unsigned)W4) * 4;
    const int c = row / H, y = row - c * H;
    const int cy = y >> log2p;
    const bool row_covered = y < Hc;
    const float* rrow = resid + (size_t)c * Hp * Wp + (size_t)cy * Wp;       // (read only where row_covered)
    float* o = dx + (size_t)row * W + x0;
    if constexpr (kVec) {
      // W % 4 == 0: Wc is a multiple of 4 for every p (p <= 2 covers all of W), so a vector is covered whole or not at all
      const bool covered = row_covered && x0 < Wc;
      if (!covered) {
        if (!accum) *reinterpret_cast<f32x4*>(o) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        continue;
      }
      float out[4];
      if (p >= 4) {
        const int cx = x0 >> log2p;
        const float g = coef * lap_stencil(rrow + cx, Wp, cy, cx, Hp, Wp);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = g;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int cx = (x0 + k) >> log2p;
          out[k] = coef * lap_stencil(rrow + cx, Wp, cy, cx, Hp, Wp);
        }
      }
      f32x4 v;
      if (accum) {
        const f32x4 old = *reinterpret_cast<const f32x4*>(o);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = old[k] + out[k];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = out[k];
      }
      *reinterpret_cast<f32x4*>(o) = v;
    } else {
      const int nv = W - x0 < 4 ? W - x0 : 4;                          // pixels of this item inside the row
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k >= nv) continue;
        if (row_covered && x0 + k < Wc) {
          const int cx = (x0 + k) >> log2p;
          const float out = coef * lap_stencil(rrow + cx, Wp, cy, cx, Hp, Wp);
          o[k] = accum ? o[k] + out : out;
        } else if (!accum) {
          o[k] = 0.0f;
        }
      }
    }
  }
}

bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

template <int p>
void lap_pool_launch(bool vec, unsigned grid, hipStream_t st, const float* x, float* cells, int C, int H, int W, int Hp, int Wp) {
  if (vec) hipLaunchKernelGGL((lap_pool_kernel<true, p>), dim3(grid), dim3(kLapThreads), 0, st, x, cells, C, H, W, Hp, Wp);
  else hipLaunchKernelGGL((lap_pool_kernel<false, p>), dim3(grid), dim3(kLapThreads), 0, st, x, cells, C, H, W, Hp, Wp);
}

template <int p>
void lap_loss_launch(bool vec, hipStream_t st, const float* x, const float* target, float* resid, float* part, int C, int H, int W,
                     int Hp, int Wp) {
  const int tiles_y = ceil_div(Hp, kLapTileH), tiles_x = ceil_div(Wp, kLapTileW);
  // every loss partial is written on every launch: always the full grid
  if (vec)
    hipLaunchKernelGGL((lap_loss_kernel<true, p>), dim3(kLapLossBlocks), dim3(kLapThreads), 0, st, x, target, resid, part, C, H, W,
                       Hp, Wp, tiles_y, tiles_x);
  else
    hipLaunchKernelGGL((lap_loss_kernel<false, p>), dim3(kLapLossBlocks), dim3(kLapThreads), 0, st, x, target, resid, part, C, H, W,
                       Hp, Wp, tiles_y, tiles_x);
}

// the pool size as a template argument: `call(std::integral_constant<int, p>{})` for the p that `pool` is
template <typename F>
void lap_dispatch_pool(int pool, F&& call) {
  switch (pool) {
    case 1: call(std::integral_constant<int, 1>{}); break;
    case 2: call(std::integral_constant<int, 2>{}); break;
    case 4: call(std::integral_constant<int, 4>{}); break;
    case 8: call(std::integral_constant<int, 8>{}); break;
    case 16: call(std::integral_constant<int, 16>{}); break;
    default: call(std::integral_constant<int, 32>{}); break;
  }
}

}  // namespace

extern "C" int stv_lap(const float* x_nchw, const float* target, float* cells, float* loss_part, float* dx_nchw, int C, int H,
                       int W, int pool, float coef, int mode, int flags, void* stream) {
  if (C <= 0 || H <= 0 || W <= 0) return STV_ERR_ARG;
  int log2p = -1;
  for (int k = 0; k <= 5; ++k)
    if (pool == (1 << k)) log2p = k;
  if (log2p < 0) return STV_ERR_ARG;
  const int Hp = H / pool, Wp = W / pool;
  if (Hp == 0 || Wp == 0) return STV_ERR_ARG;
  const unsigned long long image_bytes = (unsigned long long)C * (unsigned long long)H * (unsigned long long)W * 4ull;
  if (image_bytes >= (1ull << 31)) return STV_ERR_ARG;
  if (mode != STV_LAP_POOL && mode != STV_LAP_LOSS && mode != STV_LAP_GRAD) return STV_ERR_ARG;
  if (flags & ~STV_ACCUM) return STV_ERR_ARG;
  if ((flags & STV_ACCUM) && mode != STV_LAP_GRAD) return STV_ERR_ARG;
  if (!cells) return STV_ERR_ARG;
  if (mode != STV_LAP_GRAD && !x_nchw) return STV_ERR_ARG;
  if (mode == STV_LAP_LOSS && (!target || !loss_part)) return STV_ERR_ARG;
  const unsigned long long cell_bytes = (unsigned long long)C * (unsigned long long)Hp * (unsigned long long)Wp * 4ull;
  if (mode == STV_LAP_GRAD) {
    if (!dx_nchw) return STV_ERR_ARG;
    // dx shares no byte with the residual: an item of another thread may still have to read what this one writes
    const uintptr_t pr = (uintptr_t)cells, pd = (uintptr_t)dx_nchw;
    if (pd < pr + cell_bytes && pr < pd + image_bytes) return STV_ERR_ARG;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 block(kLapThreads);
  if (mode == STV_LAP_POOL) {
    const size_t n = (size_t)C * Hp * Wp;
    size_t grid = (n + kLapThreads - 1) / kLapThreads;
    if (grid > (size_t)kLapGradBlocks) grid = kLapGradBlocks;
    const bool vec = (W % 4 == 0) && aligned16(x_nchw);
    lap_dispatch_pool(pool, [&](auto p) { lap_pool_launch<decltype(p)::value>(vec, (unsigned)grid, st, x_nchw, cells, C, H, W, Hp, Wp); });
  } else if (mode == STV_LAP_LOSS) {
    const bool vec = (W % 4 == 0) && aligned16(x_nchw);
    lap_dispatch_pool(pool, [&](auto p) { lap_loss_launch<decltype(p)::value>(vec, st, x_nchw, target, cells, loss_part, C, H, W, Hp, Wp); });
  } else {
    const int rows = C * H;
    const size_t items = (size_t)rows * ((W + 3) / 4);
    size_t grid = (items + kLapThreads - 1) / kLapThreads;
    if (grid > (size_t)kLapGradBlocks) grid = kLapGradBlocks;
    const int accum = (flags & STV_ACCUM) != 0;
    if ((W % 4 == 0) && aligned16(dx_nchw))
      hipLaunchKernelGGL(lap_grad_kernel<true>, dim3((unsigned)grid), block, 0, st, cells, dx_nchw, rows, H, W, Hp, Wp, pool,
                         log2p, coef, accum);
    else
      hipLaunchKernelGGL(lap_grad_kernel<false>, dim3((unsigned)grid), block, 0, st, cells, dx_nchw, rows, H, W, Hp, Wp, pool,
                         log2p, coef, accum);
  }
  STV_CHECK_LAUNCH();
  return STV_OK;
}
