// Timelapse GIF output (--gif): the two device passes over the captured frames, HWC uint8 [H][W][3].
//   stv_frame_hist   add a frame's pixels to the 32x32x32 colour histogram the palette is cut from
//   stv_gif_map      map a frame to indices into that palette: ordered dither, exact nearest entry
// Integer arithmetic only, defined to the bit in stv.h.  Both walk a frame as a flat run of pixels, a work item four
// consecutive pixels: 12 bytes in as three 32-bit loads on the vector path (and one 32-bit store of the four indices),
// bytes on the scalar path, which every misaligned base and the last n % 4 pixels take.  Neither runs inside the step:
// the histogram pass follows a frame's capture (one launch per saved frame), the map runs when the file is written.
#include <hip/hip_runtime.h>

#include "stv_common.h"

namespace {

constexpr int kGifThreads = STV_GIF_THREADS;
constexpr int kGifMaxBlocks = STV_GIF_MAX_BLOCKS;
constexpr size_t kGifMaxBytes = (size_t)1 << 31;      // a frame stays below 2 GiB: item counts fit 32 bits

inline unsigned gif_grid(size_t items) {
  size_t b = (items + kGifThreads - 1) / kGifThreads;
  if (b < 1) b = 1;
  if (b > (size_t)kGifMaxBlocks) b = kGifMaxBlocks;
  return (unsigned)b;
}

// The four pixels of item i as px[k] = r | g << 8 | b << 16; nv = how many of them exist.
template <bool kVec>
__device__ __forceinline__ int gif_load(const uint8_t* __restrict__ frame, unsigned i, unsigned n, uint32_t (&px)[4]) {
  const unsigned p0 = 4u * i;
  const int nv = n - p0 < 4u ? (int)(n - p0) : 4;
  const uint8_t* src = frame + (size_t)p0 * 3;
  if (kVec && nv == 4) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(src);      // 12 * i bytes behind a 4-byte aligned base
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    px[0] = w0 & 0xFFFFFFu;
    px[1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
    px[2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
    px[3] = w2 >> 8;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      px[k] = 0;
      if (k < nv) px[k] = (uint32_t)src[3 * k] | ((uint32_t)src[3 * k + 1] << 8) | ((uint32_t)src[3 * k + 2] << 16);
    }
  }
  return nv;
}

// hist[(r>>3)<<10 | (g>>3)<<5 | (b>>3)] += 1 per pixel.  Integer adds commute, so the result does not depend on the order
// the atomics arrive in, nor on how pixels are grouped into one add: no-return global atomics, with two merges in front of
// them.  (One atomic per pixel measured the same on a random frame and 3 ms at 512^2 on a constant one, against 19 us:
// profiles/gif_bench.json, profiles/patches/gif_hist_plain_arm.patch.)
template <bool kVec>
__global__ __launch_bounds__(kGifThreads) void frame_hist_kernel(const uint8_t* __restrict__ frame, unsigned n,
                                                                 uint32_t* __restrict__ hist) {
  const unsigned items = (n + 3u) >> 2;
  for (unsigned i = blockIdx.x * kGifThreads + threadIdx.x; i < items; i += gridDim.x * kGifThreads) {
    uint32_t px[4], bin[4];
    const int nv = gif_load<kVec>(frame, i, n, px);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      bin[k] = (((px[k] >> 3) & 31u) << 10) | (((px[k] >> 11) & 31u) << 5) | ((px[k] >> 19) & 31u);      // < 32768
    {
      // a wave whose 256 pixels share one bin (flat paint) adds them with one atomic: adds to one counter are served one
      // after the other, and a constant frame would otherwise queue every pixel behind it
      const bool same = nv == 4 && bin[0] == bin[1] && bin[1] == bin[2] && bin[2] == bin[3] &&
                        bin[0] == (uint32_t)__builtin_amdgcn_readfirstlane((int)bin[0]);
      const unsigned long long active = __ballot(1);
      if (__ballot(same) == active) {
        if ((int)__lane_id() == __ffsll((long long)active) - 1) atomicAdd(hist + bin[0], 4u * (uint32_t)__popcll(active));
        continue;
      }
    }
    // runs of equal bins among the item's own pixels are added as one
    uint32_t run_bin = bin[0], run = 1;       // nv >= 1
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      if (k >= nv) continue;
      if (bin[k] == run_bin) {
        ++run;
      } else {
        atomicAdd(hist + run_bin, run);
        run_bin = bin[k];
        run = 1;
      }
    }
    atomicAdd(hist + run_bin, run);
  }
}

// B8[y & 7][x & 7]: the 8x8 Bayer matrix, bit-interleaved from the low three bits of x ^ y and of y.
__device__ __forceinline__ int bayer8(unsigned x, unsigned y) {
  const unsigned q = x ^ y;
  int t = 0;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    t |= (int)((q >> b) & 1u) << (2 * (2 - b) + 1);
    t |= (int)((y >> b) & 1u) << (2 * (2 - b));
  }
  return t;
}

// The palette is staged once per workgroup as {r, g, b, 0} ints: the search reads entry k as one 16-byte LDS broadcast and
// takes the four pixels of the item against it.  Exact and brute force: 256 entries x 4 pixels, int32, a strict `<` from
// INT_MAX downwards, so the lowest k wins a tie.
template <bool kVec>
__global__ __launch_bounds__(kGifThreads) void gif_map_kernel(const uint8_t* __restrict__ frame, uint8_t* __restrict__ index,
                                                              unsigned n, unsigned W, const uint8_t* __restrict__ palette,
                                                              int n_colors, int spread) {
  __shared__ int4 pal[256];
  for (int k = threadIdx.x; k < n_colors; k += kGifThreads)
    pal[k] = make_int4(palette[3 * k], palette[3 * k + 1], palette[3 * k + 2], 0);
  __syncthreads();
  const unsigned items = (n + 3u) >> 2;
  for (unsigned i = blockIdx.x * kGifThreads + threadIdx.x; i < items; i += gridDim.x * kGifThreads) {
    uint32_t px[4];
    const int nv = gif_load<kVec>(frame, i, n, px);
    const unsigned p0 = 4u * i;
    unsigned y = p0 / W, x = p0 - y * W;
    int v[4][3], best[4], arg[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int off = ((2 * bayer8(x, y) - 63) * spread) >> 7;      // arithmetic shift: floor
#pragma unroll
      for (int c = 0; c < 3; ++c) v[k][c] = min(max((int)((px[k] >> (8 * c)) & 0xFFu) + off, 0), 255);
      best[k] = 0x7FFFFFFF;
      arg[k] = 0;
      if (++x == W) { x = 0; ++y; }
    }
    for (int q = 0; q < n_colors; ++q) {
      const int4 e = pal[q];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int dr = v[k][0] - e.x, dg = v[k][1] - e.y, db = v[k][2] - e.z;
        const int d = dr * dr + dg * dg + db * db;                  // <= 3 * 255^2
        if (d < best[k]) {
          best[k] = d;
          arg[k] = q;
        }
      }
    }
    uint8_t* dst = index + p0;
    if (kVec && nv == 4) {
      *reinterpret_cast<uint32_t*>(dst) = (uint32_t)arg[0] | ((uint32_t)arg[1] << 8) | ((uint32_t)arg[2] << 16) | ((uint32_t)arg[3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nv) dst[k] = (uint8_t)arg[k];
    }
  }
}
}  // namespace

extern "C" int stv_frame_hist(const uint8_t* frame_hwc, size_t n_pixels, uint32_t* hist, void* stream) {
  if (!frame_hwc || !hist || n_pixels == 0 || n_pixels >= kGifMaxBytes || n_pixels * 3 >= kGifMaxBytes) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned n = (unsigned)n_pixels;
  const dim3 grid(gif_grid((n_pixels + 3) / 4)), block(kGifThreads);
  if ((uintptr_t)frame_hwc % 4 == 0) hipLaunchKernelGGL(frame_hist_kernel<true>, grid, block, 0, st, frame_hwc, n, hist);
  else hipLaunchKernelGGL(frame_hist_kernel<false>, grid, block, 0, st, frame_hwc, n, hist);
  STV_CHECK_LAUNCH();
  return STV_OK;
}

extern "C" int stv_gif_map(const uint8_t* frame_hwc, uint8_t* index_hw, int H, int W, const uint8_t* palette, int n_colors,
                           int spread, void* stream) {
  if (!frame_hwc || !index_hw || !palette || H <= 0 || W <= 0 || n_colors < 1 || n_colors > 256 || spread < 0 || spread > 64)
    return STV_ERR_ARG;
  const size_t n_pixels = (size_t)H * (size_t)W;
  if (n_pixels * 3 >= kGifMaxBytes) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned n = (unsigned)n_pixels;
  const dim3 grid(gif_grid((n_pixels + 3) / 4)), block(kGifThreads);
  const bool vec = (uintptr_t)frame_hwc % 4 == 0 && (uintptr_t)index_hw % 4 == 0;
  if (vec) hipLaunchKernelGGL(gif_map_kernel<true>, grid, block, 0, st, frame_hwc, index_hw, n, (unsigned)W, palette, n_colors, spread);
  else hipLaunchKernelGGL(gif_map_kernel<false>, grid, block, 0, st, frame_hwc, index_hw, n, (unsigned)W, palette, n_colors, spread);
  STV_CHECK_LAUNCH();
  return STV_OK;
}
