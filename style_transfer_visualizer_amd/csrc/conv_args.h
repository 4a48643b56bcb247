// Launch arguments shared by the implicit-GEMM convolution kernels (conv_igemm.hip, conv_ws.hip).
#pragma once
#include <hip/hip_runtime.h>

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

// conv_ws.hip: weight-stationary persistent kernel for 3x3, Cin = 64, bf16 (the short-K layers).
// stv_conv_ws_supported() says whether a launch with these arguments can take it.
bool stv_conv_ws_supported(const ConvArgs& a, int dtype, int taps);
int stv_conv_ws_launch(const ConvArgs& a, hipStream_t st);

// conv_igemm16.hip: the general kernel's tiles that are built there (conv_tiles.h: kUnit16; bf16, cin % 32 == 0).
int stv_conv_launch_unit16(const ConvArgs& a, int cfg, int taps, hipStream_t st);
