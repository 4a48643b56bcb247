// Launch arguments shared by the implicit-GEMM convolution kernels (conv_igemm.hip, conv_ws.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>

struct ConvArgs {
  const void* x;
  const void* w;
  const float* bias;
  const void* ref;
  void* y;
  int H, W, cin, cout, flags;
  void* pool;   // optional second output: MaxPool2d(2,2) of y, [H/2][W/2][cout]
  void* pool_idx;  // optional third output with it: one byte per pooled element (stv.h: stv_conv_igemm_pool)
  // optional fused 1x1 term: y = epilogue(mask(ref) * conv3x3(x, w) + x2 . w2^T), x2 [H][W][cin2],
  // w2 [cout][cin2] plain rows (the Gram backward product riding in the dgrad that shares its output)
  const void* x2;
  const void* w2;
  int cin2;
  // optional (bf16 dgrad in front of a max-pool, stv_conv_igemm_route): instead of storing y, route every
  // element to its window's arg-max position in route_out [2H][2W][cout] (zeros elsewhere), reading the
  // forward pass's arg-max byte map route_idx [H][W][cout] - MaxPool2d's backward without a pass of its own
  const void* route_idx = nullptr;
  void* route_out = nullptr;
  // optional: weights of the conv that runs NEXT (stv_conv_next_weights).  Each lane touches one 128-byte line of
  // them between its main loop and its epilogue, so that launch finds them on chip instead of in HBM.
  const void* pf = nullptr;
  uint32_t pf_bytes = 0;
};

// ---- the size guard of every conv entry point ---------------------------------------------------------------------------
// The matrix-core kernels (conv_igemm_kernel.h) address every tensor through a raw buffer descriptor: a 32-bit record
// count in BYTES, 32-bit byte offsets, and kOob = 0x80000000 as the offset of everything that must be dropped or
// zero-filled (padding taps, dead lanes, channels past cout).  The hardware drops an access whose offset is >= the
// record count, so the one invariant is  records <= 2^31  for every descriptor: then kOob is out of range, every live
// offset (< records) fits 31 bits and no sum of a live offset and a K-stage step wraps.  A tensor of EXACTLY 2^31 bytes
// is therefore addressable; one 16-byte group more is not (kOob would name a live element).
// The descriptors, per form (es = element bytes: 2 bf16, 4 fp32 and bf16x3; taps = 9 or 1):
//   every form   x    [H][W][cin]         H*W*cin*es            (conv_mainloop: x_bytes)
//                w    [taps][cout][cin]   taps*cout*cin*es      (w_bytes; K-blocked and pre-split forms: same count)
//                y    [H][W][cout]        H*W*cout*es           (out_bytes: the store, the ReLU-mask map `ref` and the
//                                                                accumulate read-back share this count; formed, and the
//                                                                offsets with it, under STV_POOL_ONLY and a route too)
//                bias fp32[cout]          cout*4
//   pooled       pool [H/2][W/2][cout]    (H/2)*(W/2)*cout*es   and the arg-max byte map, (H/2)*(W/2)*cout: both are
//                                                                below y for every H, W (floor), they never decide alone
//   dual         x2   [H][W][cin2]        H*W*cin2*es           (the 1x1 phase's x_bytes)
//                w2   [cout][cin2]        cout*cin2*es
//   route        out  [2H][2W][cout]      4*H*W*cout*2          (4 * out_bytes; bf16 only); the byte map H*W*cout is
//                                                                read at `off >> 1` of an offset below y: no tighter bound
// The unit-16 tiles (conv_igemm16.hip) are the same template.  The direct fallback indexes with size_t and could take
// more; it is held to the same bound so that a shape's limit does not depend on its channel alignment.  The
// weight-stationary kernel (conv_ws.hip) keeps its own, stricter test (below 2^31) and leaves the rest to the general kernel.
enum ConvForm { kFormPlain = 0, kFormPool = 1, kFormDual = 2, kFormRoute = 3 };    // stv.h: STV_CONV_PLAIN ..
constexpr size_t kConvMaxBytes = (size_t)1 << 31;
inline bool conv_fits(int H, int W, int cin, int cout, int taps, int cin2, int es, int form) {
  if (H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || (taps != 9 && taps != 1) || (es != 2 && es != 4)) return false;
  if (form < kFormPlain || form > kFormRoute || (form != kFormPlain && taps != 9)) return false;
  if ((form == kFormDual) != (cin2 > 0) || (form == kFormRoute && es != 2)) return false;
  // a product of factors below 2^32 each, tested factor by factor: the running value never leaves 64 bits
  auto fits = [](size_t a, size_t b, size_t c = 1, size_t d = 1, size_t f = 1) {
    size_t r = a;
    for (const size_t m : {b, c, d, f}) {
      if (r > kConvMaxBytes) return false;
      r *= m;
    }
    return r <= kConvMaxBytes;
  };
  const size_t h = (size_t)H, w = (size_t)W, e = (size_t)es, ci = (size_t)cin, co = (size_t)cout, c2 = (size_t)cin2;
  bool ok = fits(h, w, ci, e) && fits(h, w, co, e) && fits((size_t)taps, co, ci, e) && fits(co, 4);
  if (form == kFormPool) ok = ok && fits(h / 2, w / 2, co, e) && fits(h / 2, w / 2, co);
  if (form == kFormDual) ok = ok && fits(h, w, c2, e) && fits(co, c2, e);
  if (form == kFormRoute) ok = ok && fits(h, w, co, e, 4) && fits(h, w, co);
  return ok;
}

// conv_ws.hip: weight-stationary persistent kernel for 3x3, Cin = 64, bf16 (the short-K layers).
// stv_conv_ws_supported() says whether a launch with these arguments can take it.
bool stv_conv_ws_supported(const ConvArgs& a, int dtype, int taps);
int stv_conv_ws_launch(const ConvArgs& a, hipStream_t st);

// conv_igemm16.hip: the general kernel's tiles that are built there (conv_tiles.h: kUnit16; bf16, cin % 32 == 0).
int stv_conv_launch_unit16(const ConvArgs& a, int cfg, int taps, hipStream_t st);
