// Spatial guidance (guidance.py; Gatys et al. 2017, section 4.2): one activation map split into region slabs,
//   out[r][p][c] = labels[p] == r ? F[p][c] : +0          r < R <= STV_MASK_MAX_REGIONS,  p < n_pixels,  c < C
// for an NHWC map F [n_pixels][C], a uint8 label per pixel and contiguous slabs out [R][n_pixels][C].  No arithmetic:
// an element of a slab is the bit pattern of its source (NaN payloads and -0 survive) or the bit pattern of +0; a label
// >= R (255: "no region") leaves the pixel zero in every slab.  Every element of every slab is written.
// The walk: a work item is 16 bytes of one pixel's channels - one 16-byte load of F, one byte of the label map, R 16-byte
// stores - so F is read once, whatever R; a pass of the capped grid covers kSplitBlocks * kSplitThreads items.  Vector
// path: C * element size is a multiple of 16 behind 16-byte aligned F and out (every pixel and every slab then starts on
// a 16-byte boundary).  Otherwise the scalar path: a work item is one element, the same rule.
// Offsets: an item index stays below 2^31 (one slab is under 2 GiB); the slab stride is added as size_t.
#include <hip/hip_runtime.h>

#include "stv_common.h"

namespace {

constexpr int kSplitThreads = STV_MASK_SPLIT_THREADS;
constexpr int kSplitBlocks = STV_MASK_SPLIT_MAX_BLOCKS;
constexpr int kSplitRegions = STV_MASK_MAX_REGIONS;

// T: the unit a work item moves (u32x4 on the vector path, uint16_t / uint32_t on the scalar one); per_pixel: units per pixel
template <typename T>
__global__ __launch_bounds__(kSplitThreads) void mask_split_kernel(const T* __restrict__ F, const uint8_t* __restrict__ labels,
                                                                   T* __restrict__ out, unsigned items, unsigned per_pixel,
                                                                   int R) {
  const T zero = T{};
  for (unsigned i = blockIdx.x * kSplitThreads + threadIdx.x; i < items; i += (unsigned)gridDim.x * kSplitThreads) {
    const T v = F[i];
    const int label = labels[i / per_pixel];
    T* o = out + i;
#pragma unroll
    for (int r = 0; r < kSplitRegions; ++r) {
      if (r < R) o[(size_t)r * items] = (label == r) ? v : zero;
    }
  }
}

template <typename T>
void launch(const void* F, const uint8_t* labels, void* out, size_t items, size_t per_pixel, int R, hipStream_t st) {
  size_t grid = (items + kSplitThreads - 1) / kSplitThreads;
  if (grid > (size_t)kSplitBlocks) grid = kSplitBlocks;
  hipLaunchKernelGGL(mask_split_kernel<T>, dim3((unsigned)grid), dim3(kSplitThreads), 0, st, static_cast<const T*>(F), labels,
                     static_cast<T*>(out), (unsigned)items, (unsigned)per_pixel, R);
}

}  // namespace

extern "C" int stv_mask_split(const void* F, const uint8_t* labels, void* out, size_t n_pixels, int C, int R, int dtype,
                              void* stream) {
  if (!F || !labels || !out) return STV_ERR_ARG;
  if (R < 1 || R > kSplitRegions || n_pixels < 1 || C < 1) return STV_ERR_ARG;
  if (dtype != STV_F32 && dtype != STV_BF16) return STV_ERR_ARG;
  const size_t es = dtype == STV_BF16 ? 2 : 4;
  if (n_pixels >= (1ull << 31) || (unsigned long long)n_pixels * (unsigned long long)C * es >= (1ull << 31)) return STV_ERR_ARG;
  const size_t slab = n_pixels * (size_t)C * es;
  // `out` shares no byte with an input: an item of another thread may still have to read what this one writes
  const uintptr_t pf = (uintptr_t)F, pl = (uintptr_t)labels, po = (uintptr_t)out;
  const uintptr_t out_end = po + (uintptr_t)R * slab;
  if ((po < pf + slab && pf < out_end) || (po < pl + n_pixels && pl < out_end)) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t row = (size_t)C * es;
  if (row % 16 == 0 && pf % 16 == 0 && po % 16 == 0) launch<u32x4>(F, labels, out, slab / 16, row / 16, R, st);
  else if (es == 2) launch<uint16_t>(F, labels, out, slab / 2, (size_t)C, R, st);
  else launch<uint32_t>(F, labels, out, slab / 4, (size_t)C, R, st);
  STV_CHECK_LAUNCH();
  return STV_OK;
}
