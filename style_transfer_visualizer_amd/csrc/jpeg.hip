// Motion-JPEG timelapse (--video-format mjpeg): the device side of a baseline JPEG encoder, 4:2:0, Annex K Huffman tables.
//   stv_jpeg_dct         frame u8 HWC -> quantised int16 coefficients in zigzag order (colour, chroma, DCT, quantisation)
//   stv_jpeg_block_bits  the length of every block's Huffman code
//   stv_jpeg_scan        exclusive prefix sum of those lengths per frame: the bit offset of every block
//   stv_jpeg_emit        the codes, written into a zeroed byte stream at those offsets
// Integer arithmetic only, defined to the bit in stv.h.  The DCT kernel runs behind a frame's capture (one launch per
// saved frame); the other three run once over all frames when the file is written.  None runs inside the step.
#include <hip/hip_runtime.h>

#include "stv_common.h"

namespace {

constexpr int kDctThreads = STV_JPEG_DCT_THREADS;
constexpr int kDctBlocks = kDctThreads / 8;       // 8x8 blocks per workgroup: 8 lanes each
constexpr int kRowStride = 72;                    // dwords between two blocks' row-pass results: 64 + 8, so that the four
                                                  // blocks of a 32-lane group read eight different banks each in the column pass
constexpr int kThreads = STV_JPEG_THREADS;
constexpr int kMaxBlockBits = STV_JPEG_MAX_BLOCK_BITS;

__device__ constexpr int kT[8][8] = STV_JPEG_DCT_TABLE;

struct ZigZag {
  uint8_t of[64];      // of[v*8 + u]: the position of coefficient (v, u) in zigzag order
};
constexpr ZigZag make_zigzag() {
  ZigZag z{};
  int v = 0, u = 0;
  for (int i = 0; i < 64; ++i) {
    z.of[v * 8 + u] = (uint8_t)i;
    if ((v + u) % 2 == 0) {      // up and to the right
      if (u == 7) ++v;
      else if (v == 0) ++u;
      else { --v; ++u; }
    } else {                     // down and to the left
      if (v == 7) ++u;
      else if (u == 0) ++v;
      else { ++v; --u; }
    }
  }
  return z;
}
__device__ const ZigZag kZigZag = make_zigzag();

// ---- the four "typical" Huffman tables of ITU T.81 Annex K.3: BITS (codes per length 1..16) and HUFFVAL ----------------
constexpr uint8_t kDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kAcChrVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// code and length per symbol; class 0: luminance, class 1: chrominance.  A symbol without a code has length 0 (the walk
// below produces none: categories stop at 11 for the DC and at 10 for an AC coefficient).
struct Huffman {
  uint16_t dc_code[2][12];
  uint8_t dc_len[2][12];
  uint16_t ac_code[2][256];
  uint8_t ac_len[2][256];
};
constexpr void huffman_fill(const uint8_t* bits, const uint8_t* vals, uint16_t* code, uint8_t* len) {
  unsigned next = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i, ++k) {
      code[vals[k]] = (uint16_t)next++;
      len[vals[k]] = (uint8_t)l;
    }
    next <<= 1;
  }
}
constexpr Huffman make_huffman() {
  Huffman h{};
  huffman_fill(kDcLumBits, kDcVals, h.dc_code[0], h.dc_len[0]);
  huffman_fill(kDcChrBits, kDcVals, h.dc_code[1], h.dc_len[1]);
  huffman_fill(kAcLumBits, kAcLumVals, h.ac_code[0], h.ac_len[0]);
  huffman_fill(kAcChrBits, kAcChrVals, h.ac_code[1], h.ac_len[1]);
  return h;
}
__device__ const Huffman kHuffman = make_huffman();

struct QTabs {
  uint8_t q[2][64];
};

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
// which = 0: Cb, 1: Cr
__device__ __forceinline__ int chroma(int r, int g, int b, int which) {
  return which == 0 ? (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
                    : (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16;
}

// 8 lanes per block.  Row pass: lane r forms the eight samples of row r of its block (a luminance block: eight pixels;
// a chroma block: eight 2x2 pixel groups) and their eight row sums, which go to LDS.  Column pass: lane u reads column u,
// forms the eight coefficients (v, u), quantises them and scatters them as int16 to their zigzag places in LDS.  Store:
// lane r moves the 16 bytes r of the block's 128 to global memory.
__global__ __launch_bounds__(kDctThreads) void jpeg_dct_kernel(const uint8_t* __restrict__ frame, int H, int W, unsigned mcu_w,
                                                               unsigned n_blocks, QTabs qt, int16_t* __restrict__ coef) {
  __shared__ int rows[kDctBlocks * kRowStride];
  __shared__ __attribute__((aligned(16))) int16_t zz[kDctBlocks * 64];
  const unsigned lb = threadIdx.x >> 3, r = threadIdx.x & 7u;
  const unsigned blk = blockIdx.x * kDctBlocks + lb;
  const bool live = blk < n_blocks;
  const unsigned m = blk / 6u, k = blk - 6u * m;
  if (live) {
    const unsigned my = m / mcu_w, mx = m - my * mcu_w;
    int s[8];
    if (k < 4u) {
      const int y = min((int)(my * 16u + (k >> 1) * 8u + r), H - 1);
      const int x0 = (int)(mx * 16u + (k & 1u) * 8u);
      const uint8_t* row = frame + (size_t)y * (size_t)W * 3;
      const uint8_t* src = row + (size_t)x0 * 3;
      if (x0 + 8 <= W && ((uintptr_t)src & 3u) == 0) {
        const uint32_t* wp = reinterpret_cast<const uint32_t*>(src);      // 24 bytes inside the row
        uint32_t w[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) w[j] = wp[j];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int n = 3 * j;
          const int cr = (int)((w[n >> 2] >> (8 * (n & 3))) & 0xFFu);
          const int cg = (int)((w[(n + 1) >> 2] >> (8 * ((n + 1) & 3))) & 0xFFu);
          const int cb = (int)((w[(n + 2) >> 2] >> (8 * ((n + 2) & 3))) & 0xFFu);
          s[j] = luma(cr, cg, cb) - 128;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint8_t* p = row + (size_t)min(x0 + j, W - 1) * 3;
          s[j] = luma(p[0], p[1], p[2]) - 128;
        }
      }
    } else {
      const int which = (int)k - 4;
      const int y0 = min((int)(my * 16u + 2u * r), H - 1), y1 = min((int)(my * 16u + 2u * r + 1u), H - 1);
      const uint8_t* row0 = frame + (size_t)y0 * (size_t)W * 3;
      const uint8_t* row1 = frame + (size_t)y1 * (size_t)W * 3;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const size_t xa = (size_t)min((int)(mx * 16u) + 2 * j, W - 1) * 3, xb = (size_t)min((int)(mx * 16u) + 2 * j + 1, W - 1) * 3;
        const int sum = chroma(row0[xa], row0[xa + 1], row0[xa + 2], which) + chroma(row0[xb], row0[xb + 1], row0[xb + 2], which) +
                        chroma(row1[xa], row1[xa + 1], row1[xa + 2], which) + chroma(row1[xb], row1[xb + 1], row1[xb + 2], which);
        s[j] = ((sum + 2) >> 2) - 128;
      }
    }
    int* dst = rows + lb * kRowStride + r * 8u;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int a = 0;
#pragma unroll
      for (int x = 0; x < 8; ++x) a += kT[u][x] * s[x];
      dst[u] = (a + 128) >> 8;
    }
  }
  __syncthreads();
  if (live) {
    const unsigned u = r;
    int col[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) col[y] = rows[lb * kRowStride + y * 8 + u];
    const unsigned tab = k >= 4u ? 1u : 0u;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      int b = 0;
#pragma unroll
      for (int y = 0; y < 8; ++y) b += kT[v][y] * col[y];
      const unsigned d = (unsigned)qt.q[tab][v * 8 + u] << 18;
      const int mag = (int)(((unsigned)abs(b) + (d >> 1)) / d);
      int c = b < 0 ? -mag : mag;
      const int lo = (v == 0 && u == 0u) ? -1024 : -1023;
      c = min(max(c, lo), 1023);
      zz[lb * 64u + kZigZag.of[v * 8 + u]] = (int16_t)c;
    }
  }
  __syncthreads();
  if (live) {
    const int4 out = *reinterpret_cast<const int4*>(zz + lb * 64u + r * 8u);
    *reinterpret_cast<int4*>(coef + (size_t)blk * 64 + r * 8u) = out;
  }
}

__device__ __forceinline__ int category(int v) { return 32 - __clz(abs(v)); }      // bit length of |v|; 0 for 0

// The code of one block, handed to `sink.put(code, length)` piece by piece: the same walk gives the length and the bits.
// z: the block's 64 coefficients in zigzag order, 16-byte aligned; pred: the DC predictor; cls: 0 luminance, 1 chrominance.
template <class Sink>
__device__ __forceinline__ void encode_block(const int16_t* __restrict__ z, int pred, unsigned cls, Sink& sink) {
  const int4* zv = reinterpret_cast<const int4*>(z);
  int run = 0;
  for (int c = 0; c < 8; ++c) {
    const int4 w4 = zv[c];
    const int w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int v = (int)(int16_t)((uint32_t)w[j >> 1] >> (16 * (j & 1)));
      if (c == 0 && j == 0) {
        const int diff = v - pred;
        const int cat = category(diff);
        sink.put(kHuffman.dc_code[cls][cat], kHuffman.dc_len[cls][cat]);
        sink.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u), cat);
        continue;
      }
      if (v == 0) {
        ++run;
        continue;
      }
      while (run >= 16) {
        sink.put(kHuffman.ac_code[cls][0xF0], kHuffman.ac_len[cls][0xF0]);
        run -= 16;
      }
      const int cat = category(v);
      const int sym = (run << 4) | cat;
      sink.put(kHuffman.ac_code[cls][sym], kHuffman.ac_len[cls][sym]);
      sink.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u), cat);
      run = 0;
    }
  }
  if (run > 0) sink.put(kHuffman.ac_code[cls][0], kHuffman.ac_len[cls][0]);
}

// The DC predictor of block b of a frame (b = 6*m + k): the DC of the previous block of the same component.
__device__ __forceinline__ int dc_pred(const int16_t* __restrict__ frame_coef, unsigned b) {
  const unsigned m = b / 6u, k = b - 6u * m;
  if (k >= 1u && k <= 3u) return frame_coef[(size_t)(b - 1u) * 64];
  if (m == 0u) return 0;
  return frame_coef[(size_t)(b - (k == 0u ? 3u : 6u)) * 64];
}

struct BitCounter {
  uint32_t bits = 0;
  __device__ __forceinline__ void put(uint32_t, int len) { bits += (uint32_t)len; }
};

__global__ __launch_bounds__(kThreads) void jpeg_bits_kernel(const int16_t* __restrict__ coef, unsigned n_total, unsigned bpf,
                                                             uint32_t* __restrict__ bits) {
  const unsigned i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_total) return;
  const unsigned f = i / bpf, b = i - f * bpf;
  const int16_t* frame_coef = coef + (size_t)f * bpf * 64;
  BitCounter counter;
  encode_block(frame_coef + (size_t)b * 64, dc_pred(frame_coef, b), b % 6u >= 4u ? 1u : 0u, counter);
  bits[i] = counter.bits;
}

// offsets: the exclusive prefix sum of one frame's lengths.  A thread owns one contiguous run of the frame; the 256 run
// sums are scanned in LDS (Hillis-Steele), then every thread walks its run again.
__global__ __launch_bounds__(kThreads) void jpeg_scan_kernel(const uint32_t* __restrict__ bits, unsigned bpf,
                                                             uint32_t* __restrict__ offsets, uint32_t* __restrict__ totals) {
  __shared__ uint32_t part[kThreads];
  const unsigned f = blockIdx.x, t = threadIdx.x;
  const uint32_t* src = bits + (size_t)f * bpf;
  uint32_t* dst = offsets + (size_t)f * bpf;
  const unsigned chunk = (bpf + kThreads - 1) / kThreads;
  const unsigned lo = min(t * chunk, bpf), hi = min(lo + chunk, bpf);
  uint32_t own = 0;
  for (unsigned i = lo; i < hi; ++i) own += src[i];
  part[t] = own;
  __syncthreads();
  for (unsigned o = 1; o < (unsigned)kThreads; o <<= 1) {
    const uint32_t add = t >= o ? part[t - o] : 0u;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  uint32_t at = part[t] - own;
  for (unsigned i = lo; i < hi; ++i) {
    dst[i] = at;
    at += src[i];
  }
  if (t == (unsigned)kThreads - 1u) totals[f] = part[t];
}

// Bits MSB first into big-endian 32-bit words.  The first word of a block may hold the end of its predecessor and the last
// the start of its successor: those two are OR-ed in atomically (the buffer starts zeroed); every word in between belongs
// to this block alone and is stored.
struct BitWriter {
  uint32_t* words;
  uint32_t word, cap;      // the word being filled; words in the buffer
  uint64_t acc = 0;
  int n;                   // bits in acc, counted from the word's top
  bool shared = true;
  __device__ __forceinline__ BitWriter(uint32_t* words_, uint32_t bit, uint32_t cap_) : words(words_), word(bit >> 5), cap(cap_), n((int)(bit & 31u)) {}
  __device__ __forceinline__ void put(uint32_t code, int len) {
    acc = (acc << len) | code;
    n += len;
    if (n >= 32) {
      n -= 32;
      const uint32_t w = __builtin_bswap32((uint32_t)(acc >> n));
      if (word < cap) {
        if (shared) atomicOr(words + word, w);
        else words[word] = w;
      }
      shared = false;
      ++word;
      acc &= (1ull << n) - 1ull;
    }
  }
  __device__ __forceinline__ uint32_t bit_position() const { return word * 32u + (uint32_t)n; }
  __device__ __forceinline__ void finish() {
    if (n > 0 && word < cap) atomicOr(words + word, __builtin_bswap32((uint32_t)(acc << (32 - n))));
  }
};

__global__ __launch_bounds__(kThreads) void jpeg_emit_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ offsets,
                                                             const uint32_t* __restrict__ base, unsigned n_total, unsigned bpf,
                                                             uint32_t* __restrict__ words, uint32_t cap_words) {
  const unsigned i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_total) return;
  const unsigned f = i / bpf, b = i - f * bpf;
  const int16_t* frame_coef = coef + (size_t)f * bpf * 64;
  const uint32_t first_word = base[f] >> 2;
  if (first_word >= cap_words) return;
  // (bit positions are relative to the frame's first word: the words left in the buffer bound them)
  BitWriter writer(words + first_word, offsets[i], cap_words - first_word);
  encode_block(frame_coef + (size_t)b * 64, dc_pred(frame_coef, b), b % 6u >= 4u ? 1u : 0u, writer);
  if (b == bpf - 1u) {
    const int pad = (int)((8u - (writer.bit_position() & 7u)) & 7u);
    writer.put((1u << pad) - 1u, pad);
  }
  writer.finish();
}

bool counts_ok(int n_frames, int bpf) {
  if (n_frames <= 0 || bpf <= 0 || bpf % 6 != 0) return false;
  if ((uint64_t)bpf * (uint64_t)kMaxBlockBits >= ((uint64_t)1 << 32)) return false;
  return (uint64_t)n_frames * (uint64_t)bpf < ((uint64_t)1 << 31);
}
bool coef_ok(const void* coef) { return coef && (uintptr_t)coef % 16 == 0; }

}  // namespace

extern "C" int stv_jpeg_dct(const uint8_t* frame_hwc, const int* qtabs, int H, int W, int16_t* coef, void* stream) {
  if (!frame_hwc || !qtabs || !coef || H <= 0 || W <= 0 || H > STV_JPEG_MAX_DIM || W > STV_JPEG_MAX_DIM) return STV_ERR_ARG;
  if ((uintptr_t)coef % 16 != 0) return STV_ERR_ARG;
  QTabs qt;
  for (int i = 0; i < 128; ++i) {
    if (qtabs[i] < 1 || qtabs[i] > 255) return STV_ERR_ARG;
    qt.q[i >> 6][i & 63] = (uint8_t)qtabs[i];
  }
  const unsigned mcu_w = ((unsigned)W + 15u) / 16u, mcu_h = ((unsigned)H + 15u) / 16u;
  const unsigned n_blocks = mcu_w * mcu_h * 6u;      // <= 4096 * 4096 * 6
  const dim3 grid((n_blocks + kDctBlocks - 1) / kDctBlocks), block(kDctThreads);
  hipLaunchKernelGGL(jpeg_dct_kernel, grid, block, 0, static_cast<hipStream_t>(stream), frame_hwc, H, W, mcu_w, n_blocks, qt, coef);
  STV_CHECK_LAUNCH();
  return STV_OK;
}

extern "C" int stv_jpeg_block_bits(const int16_t* coef, int n_frames, int blocks_per_frame, uint32_t* bits, void* stream) {
  if (!bits || !coef_ok(coef) || !counts_ok(n_frames, blocks_per_frame)) return STV_ERR_ARG;
  const unsigned n_total = (unsigned)n_frames * (unsigned)blocks_per_frame;
  const dim3 grid((n_total + kThreads - 1) / kThreads), block(kThreads);
  hipLaunchKernelGGL(jpeg_bits_kernel, grid, block, 0, static_cast<hipStream_t>(stream), coef, n_total, (unsigned)blocks_per_frame, bits);
  STV_CHECK_LAUNCH();
  return STV_OK;
}

extern "C" int stv_jpeg_scan(const uint32_t* bits, int n_frames, int blocks_per_frame, uint32_t* offsets, uint32_t* totals,
                             void* stream) {
  if (!bits || !offsets || !totals || !counts_ok(n_frames, blocks_per_frame)) return STV_ERR_ARG;
  const dim3 grid((unsigned)n_frames), block(kThreads);
  hipLaunchKernelGGL(jpeg_scan_kernel, grid, block, 0, static_cast<hipStream_t>(stream), bits, (unsigned)blocks_per_frame, offsets, totals);
  STV_CHECK_LAUNCH();
  return STV_OK;
}

extern "C" int stv_jpeg_emit(const int16_t* coef, const uint32_t* offsets, const uint32_t* base, int n_frames, int blocks_per_frame,
                             uint8_t* stream_bytes, size_t capacity, void* stream) {
  if (!offsets || !base || !stream_bytes || !coef_ok(coef) || !counts_ok(n_frames, blocks_per_frame)) return STV_ERR_ARG;
  if (capacity == 0 || capacity % 4 != 0 || capacity >= ((size_t)1 << 32) || (uintptr_t)stream_bytes % 4 != 0) return STV_ERR_ARG;
  const unsigned n_total = (unsigned)n_frames * (unsigned)blocks_per_frame;
  const dim3 grid((n_total + kThreads - 1) / kThreads), block(kThreads);
  hipLaunchKernelGGL(jpeg_emit_kernel, grid, block, 0, static_cast<hipStream_t>(stream), coef, offsets, base, n_total,
                     (unsigned)blocks_per_frame, reinterpret_cast<uint32_t*>(stream_bytes), (uint32_t)(capacity / 4));
  STV_CHECK_LAUNCH();
  return STV_OK;
}
