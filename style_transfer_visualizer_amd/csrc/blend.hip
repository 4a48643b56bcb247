// Blended Gram targets (several style images, style_mix.py): one weighted sum of K tables of n floats each,
//   out[i] = (...((w[0]*G_0[i]) + w[1]*G_1[i]) + ...) + w[K-1]*G_{K-1}[i]        i < n,  1 <= K <= STV_BLEND_MAX_TABLES
// over a contiguous stack [K][n].  It runs once per style layer when targets are set, never inside the step.
// Arithmetic, fixed to the bit: every product and every sum is rounded to fp32 on its own, tables in ascending order, the
// first product is the start of the sum (no 0 + ...).  Plain * and + under `fp contract(off)`, the convention stated above
// resize2x_kernel in pointwise.hip (__fmul_rn / __fadd_rn are x * y and x + y in the header and are fused after inlining
// whatever the caller's pragma says).
// The walk: a work item is four consecutive elements (one 16-byte load per table, one 16-byte store); a pass of the capped
// grid covers kBlendBlocks * kBlendThreads items; the n % 4 elements behind the last full item are walked one by one by the
// first threads of the grid.  kAligned: every table and `out` start on a 16-byte boundary (n % 4 == 0 behind aligned
// bases).  Otherwise - table k starts n*k floats behind an aligned base - the same items are read and written through
// vectors of 4-byte alignment, which the compiler is free to issue as one access or as four.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "stv_common.h"

namespace {

constexpr int kBlendThreads = STV_BLEND_THREADS;
constexpr int kBlendBlocks = STV_BLEND_MAX_BLOCKS;
constexpr int kBlendTables = STV_BLEND_MAX_TABLES;

struct BlendWeights { float w[kBlendTables]; };
typedef float f32x4_any __attribute__((ext_vector_type(4), aligned(4)));

template <bool kAligned>
__global__ __launch_bounds__(kBlendThreads) void gram_blend_kernel(const float* __restrict__ stack, float* __restrict__ out,
                                                                   BlendWeights t, int K, unsigned n) {
#pragma clang fp contract(off)
  using vec = typename std::conditional<kAligned, f32x4, f32x4_any>::type;
  const unsigned items = n >> 2;                                   // n < 2^29: the entry point bounds K*n*4 by 2 GiB
  const unsigned first = blockIdx.x * kBlendThreads + threadIdx.x;
  for (unsigned i = first; i < items; i += (unsigned)gridDim.x * kBlendThreads) {
    const size_t at = (size_t)i * 4;
    const vec g0 = *reinterpret_cast<const vec*>(stack + at);
    float acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = t.w[0] * g0[j];
    for (int k = 1; k < K; ++k) {
      const vec g = *reinterpret_cast<const vec*>(stack + (size_t)k * n + at);
      const float wk = t.w[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = wk * g[j];
        acc[j] = acc[j] + p;
      }
    }
    vec q;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = acc[j];
    *reinterpret_cast<vec*>(out + at) = q;
  }
  if (first < (n & 3u)) {                                          // the scalar tail: elements 4*items .. n-1
    const size_t at = (size_t)items * 4 + first;
    float acc = t.w[0] * stack[at];
    for (int k = 1; k < K; ++k) {
      const float p = t.w[k] * stack[(size_t)k * n + at];
      acc = acc + p;
    }
    out[at] = acc;
  }
}

}  // namespace

extern "C" int stv_gram_blend(const float* stack, float* out, const float* weights, int K, long long n, void* stream) {
  if (!stack || !out || !weights) return STV_ERR_ARG;
  if (K < 1 || K > kBlendTables || n < 1) return STV_ERR_ARG;
  const unsigned long long in_bytes = (unsigned long long)K * (unsigned long long)n * 4ull;
  if (in_bytes >= (1ull << 31)) return STV_ERR_ARG;
  BlendWeights t{};
  for (int k = 0; k < K; ++k) {                                    // weights: a HOST array
    const float w = weights[k];
    if (!(w >= 0.0f) || w > 3.402823466e+38f) return STV_ERR_ARG;  // negative, NaN, infinite
    t.w[k] = w;
  }
  // `out` shares no byte with the stack: an item of another thread may still have to read what this one writes
  const uintptr_t ps = (uintptr_t)stack, po = (uintptr_t)out;
  if (po < ps + in_bytes && ps < po + (unsigned long long)n * 4ull) return STV_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t items = (size_t)n / 4;
  size_t grid = (items + kBlendThreads - 1) / kBlendThreads;
  if (grid < 1) grid = 1;                                          // n < 4: the tail alone
  if (grid > (size_t)kBlendBlocks) grid = kBlendBlocks;
  const bool aligned = (n % 4 == 0) && (ps % 16 == 0) && (po % 16 == 0);
  const dim3 g((unsigned)grid), b(kBlendThreads);
  if (aligned) hipLaunchKernelGGL(gram_blend_kernel<true>, g, b, 0, st, stack, out, t, K, (unsigned)n);
  else hipLaunchKernelGGL(gram_blend_kernel<false>, g, b, 0, st, stack, out, t, K, (unsigned)n);
  STV_CHECK_LAUNCH();
  return STV_OK;
}
