// The second translation unit of the implicit-GEMM convolution's tiles (conv_tiles.h: the rows with unit = kUnit16 - the
// tiles whose main loop runs on v_mfma_f32_16x16x32_bf16, conv_igemm_kernel.h: Cfg<..., M16 = true>, conv_mainloop16, and
// the 16x128 tile).  bf16 only; a file of its own so that it builds beside conv_igemm.hip.  Dispatch: conv_igemm.hip::launch_mfma.
#include "conv_igemm_kernel.h"

int stv_conv_launch_unit16(const ConvArgs& a, int cfg, int taps, hipStream_t st) {
  return taps == 9 ? launch_tile<kUnit16, bf16_t, 9>(a, cfg, st) : launch_tile<kUnit16, bf16_t, 1>(a, cfg, st);
}
