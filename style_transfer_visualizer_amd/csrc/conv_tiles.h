// The tile configurations of the implicit-GEMM convolution (conv_igemm_kernel.h), one row per tile index.  The index is
// an interface (conv_tiles_gfx950.json, STV_CONV_CFG, stv_conv_config): rows are appended, never renumbered.
// Everything that depends on a tile - its Cfg<...>, who builds it, what stands in for it, whether the tuner times it -
// is read from its row.
#pragma once

enum TileUnit { kUnitMain, kUnit16 };   // built in conv_igemm.hip / conv_igemm16.hip (two translation units: a parallel build)

struct Tile {
  int TH, BN;          // rows of 32 pixels and output channels of a workgroup
  int WM, WN;          // waves along the rows / the channels (per K group)
  int KS;              // 2: two wave groups split K and meet in the LDS C tile (a layer too small for two workgroups per CU)
  int NBUF;            // LDS ring depth (3: DMA two stages ahead; 2: one ahead, more workgroups per CU; 4: two slot pairs, M16)
  bool M16;            // main loop on v_mfma_f32_16x16x32_bf16 (two K-stages per MFMA) instead of 32x32x16
  bool kpairs;         // runs only on whole pairs of 16-channel K-stages: bf16, cin % 32 == 0 (and cin2 % 32 == 0)
  int alt;             // the tile that stands in where the element is 4 bytes wide (fp32, bf16x3) or `kpairs` is not met
  bool tuned;          // offered to the tuner by default (STV_CONV_TUNE_CFGS=n offers rows 0 .. n-1 instead)
  TileUnit unit;
};

// fp32 (parity mode) keeps a second accumulator set per K-stage (blocked summation): the eight-wave tiles with 64+
// accumulator registers per lane (8x128, 16x64) would spill at their 256-register budget, so their `alt` is the
// four-wave 4x128 tile (512 registers per wave) or an 8x64 tile; the 32-channel tiles have no fp32 form either.
constexpr Tile kTiles[] = {
    // TH   BN WM WN KS NBUF  M16  kpairs alt tuned unit
    // 0-3: the cost model's range (model_cfg).  The two 8-row tiles run 8 waves: two per SIMD, one wave's waits hide
    // under the other's MFMAs
    {8, 128, 4, 2, 1, 3, false, false, 2, true, kUnitMain},    //  0: 8x128, 64 px x 64 couts per wave
    {8, 64, 4, 2, 1, 3, false, false, 1, true, kUnitMain},     //  1: 8x64, 64 px x 32 couts per wave
    {4, 128, 1, 4, 1, 3, false, false, 2, true, kUnitMain},    //  2: 4x128, four waves
    {4, 64, 2, 2, 1, 3, false, false, 3, true, kUnitMain},     //  3: 4x64, four waves
    {4, 64, 2, 2, 2, 3, false, false, 4, true, kUnitMain},     //  4: 4x64, K split over two wave groups (small layers)
    {8, 64, 4, 2, 1, 2, false, false, 5, true, kUnitMain},     //  5: 8x64 on a two-deep ring: two workgroups per CU
    {4, 64, 2, 2, 1, 2, false, false, 6, true, kUnitMain},     //  6: 4x64 on a two-deep ring: three workgroups per CU
    {2, 64, 2, 2, 2, 3, false, false, 7, true, kUnitMain},     //  7: 2x64, K split (the 32x32-pixel layers: four times the workgroups of tile 4)
    {1, 64, 1, 2, 2, 3, false, false, 8, true, kUnitMain},     //  8: 1x64, K split in four-wave workgroups (a 32x32-pixel layer covers all 256 CUs)
    {16, 64, 4, 2, 1, 3, false, false, 1, true, kUnitMain},    //  9: 16x64: four row blocks per wave, half the weight traffic per output
    {16, 64, 4, 2, 1, 2, false, false, 5, true, kUnitMain},    // 10: 16x64 on the two-deep ring
    // 11: on a 32x32-pixel layer still one workgroup per CU, which stages 434 KB instead of 1x64's 694 KB
    {2, 32, 2, 1, 2, 3, false, false, 7, true, kUnitMain},     // 11: 2x32, K split (four waves: 2 rows x 2 K groups)
    {4, 32, 4, 1, 2, 3, false, false, 4, true, kUnitMain},     // 12: 4x32, K split (eight waves)
    // 13-17: tiles 1, 9, 3, 11, 12 with the main loop on v_mfma_f32_16x16x32_bf16, out of a ring of four stage slots
    {8, 64, 4, 2, 1, 4, true, true, 1, true, kUnit16},         // 13: 8x64, 64 px x 32 couts per wave, eight waves
    {16, 64, 4, 2, 1, 4, true, true, 1, true, kUnit16},        // 14: 16x64, 128 px x 32 couts per wave
    {4, 64, 2, 2, 1, 4, true, true, 3, true, kUnit16},         // 15: 4x64, four waves
    {2, 32, 2, 1, 2, 4, true, true, 7, true, kUnit16},         // 16: 2x32, K split over two wave groups (the 32x32-pixel layers)
    {4, 32, 4, 1, 2, 4, true, true, 4, true, kUnit16},         // 17: 4x32, K split
    // 18: 16 rows x 128 couts on the two-deep ring, 32x32x16 MFMAs (built beside the 16x16x32 tiles only to balance the
    // two translation units, and like them bf16 on whole stage pairs only): 0.58 of the 8x128 tile's LDS-DMA pieces
    // per FLOP - the term that binds this kernel's issue port.  Not offered to the tuner: it wins the
    // hot loop by 7-9 % on every shape with >= 512 tiles and LOSES in the step (round 4: closure +1.9 % at 1024^2 with
    // it on the 256^2 layers, nothing at 3840x2160)
    {16, 128, 4, 2, 1, 2, false, true, 2, false, kUnit16},     // 18: 16x128
};
constexpr int kNumCfg = (int)(sizeof(kTiles) / sizeof(kTiles[0]));

constexpr int kRouteTile = 3;   // untuned routed dgrad (stv_conv_igemm_route) where the cost model says 128 wide
constexpr int kPoolTile = 4;    // stands in for a tile without a pooling window when a pooled output is asked for

// a wave that owns an odd number of rows has no 2x2 pooling window of its own
constexpr bool tile_pools(int cfg) { return (kTiles[cfg].TH / kTiles[cfg].WM) % 2 == 0; }
// the rows that 4-byte elements (fp32, bf16x3) run on, and so the only ones instantiated for them
constexpr bool tile_serves_f32(int cfg) { return kTiles[cfg].alt == cfg && !kTiles[cfg].M16; }

constexpr bool tiles_consistent() {
  for (int i = 0; i < kNumCfg; ++i) {
    const Tile& t = kTiles[i];
    if (t.alt < 0 || t.alt >= kNumCfg) return false;
    const Tile& s = kTiles[t.alt];
    if (s.alt != t.alt) return false;                                     // the stand-in of a stand-in is itself
    if (s.M16 || s.kpairs || s.unit != kUnitMain) return false;           // a stand-in takes every element kind and K
    if (t.M16 && (t.NBUF != 4 || !t.kpairs)) return false;                // 16x16x32: two pairs of stage slots
  }
  return tile_pools(kPoolTile) && tile_serves_f32(kPoolTile) && tile_serves_f32(kRouteTile);
}
static_assert(kNumCfg == 19 && tiles_consistent(), "tile table");
