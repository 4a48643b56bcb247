/*
 * stv.h - C ABI of libstv_hip.so: the MI355X (gfx950) kernels behind the
 * per-step optimisation path of style_transfer_visualizer.
 *
 * The reference has no FFI; its boundary for this path is the Python API of
 * core_model.py / optimization.py, whose arithmetic is delegated to torch.
 * Each entry point below replaces the torch op(s) issued at the cited
 * reference line (paths relative to
 * /root/reference/src/style_transfer_visualizer/).  See INTEGRATION.md for the
 * ctypes binding a maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch allocates);
 *    the library never frees or retains a pointer past the call, except the
 *    command buffer of stv_exec_*, which is copied at creation;
 *  - activations are NHWC ([H][W][C], batch 1) in `dtype` storage
 *    (STV_F32 | STV_BF16); the image and its gradient are NCHW fp32, exactly
 *    the tensors the reference optimises (core_model.py:66-100);
 *  - `stream` is a hipStream_t; all work is enqueued on it, nothing syncs;
 *  - return value: 0 = ok, otherwise an STV_ERR_* code (Python raises
 *    RuntimeError).  No CPU fallback exists.
 */
#ifndef STV_H_
#define STV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* STV_BF16X3: fp32 storage (exactly as STV_F32), split-bf16 products - every product of a conv or Gram contraction
 * is formed as ah*bh + ah*bl + al*bh on the bf16 matrix cores (hi = bf16(x), lo = bf16(x - hi)), fp32 accumulation.
 * Accepted only by the entry points that form products: stv_conv_igemm, stv_conv_igemm_pool, stv_conv_igemm_dual,
 * stv_conv_config, stv_conv_tune, stv_conv_uses_ws (always 0), stv_gram_partial and stv_gram_multi; every other
 * entry point returns STV_ERR_ARG for it.  K-blocked conv weights (STV_W_BLOCKED) are pre-split: each 16-byte group of
 * four fp32 weights holds their four bf16 hi parts, then their four bf16 lo parts (same byte count); plain-layout
 * weights are fp32 and split in the kernel: a 3x3 takes K-blocked weights only, a 1x1 plain weights only.  Size guards count bytes (stv_conv_fits). */
enum { STV_F32 = 0, STV_BF16 = 1, STV_BF16X3 = 2 };

enum {
  STV_OK = 0,
  STV_ERR_ARG = 1,      /* unsupported shape / null pointer / bad dtype */
  STV_ERR_LAUNCH = 2,   /* hipGetLastError() after a launch */
  STV_ERR_ALLOC = 3,
  STV_ERR_GRAPH = 4
};

/* flags */
enum {
  STV_RELU_IN = 1,   /* apply max(0,.) to the input while staging it */
  STV_RELU_OUT = 2,  /* apply max(0,.) before storing (conv+ReLU fusion) */
  STV_MASK = 4,      /* multiply result by (ref > 0): ReLU backward */
  STV_ACCUM = 8,     /* out += result instead of out = result */
  STV_W_BLOCKED = 16, /* conv weights are K-blocked: [taps][cin/CK][cout][CK], CK = 32 bytes of `dtype` */
  STV_POOL_IDX = 32,  /* stv_maxpool_bwd: `x` is the arg-max byte map of stv_conv_igemm_pool, not the activation */
  STV_POOL_ROUTE = 64, /* stv_op_t only: the CONV op is stv_conv_igemm_route (p2 = arg-max map, q1 = routed output) */
  STV_POOL_ONLY = 128  /* stv_conv_igemm_pool: do not store the full-resolution map `y` (only y_pool / pool_idx are wanted) */
};

int stv_version(void);
/* Algorithmic workspace sizing helpers (bytes). */
size_t stv_gram_partials_bytes(int n_pixels, int channels);
int stv_gram_ksplit(int n_pixels, int channels);

/* ---- VGG conv3x3 stacks: replaces F.conv2d / relu / max_pool2d issued by
 *      `x = block(x)` (core_model.py:316) and their autograd backward
 *      (`loss.backward()`, optimization.py:313). ---------------------------- */

/* First conv.  Its weights are frozen, so every caller packs them once: stv_conv_first_pack() writes the
 * kernel-side form of `wf` ([9][cout][cin] fp32, tap = ky*3+kx) into a caller-owned buffer of
 * stv_conv_first_packed_bytes(cin, cout) bytes, and both directions read that buffer only.  For 3 -> 64 it
 * holds the orders and matrix-core fragments the VGG kernels read; for every other shape the packed form is
 * the weights as given.  The library keeps no scratch of its own. */
size_t stv_conv_first_packed_bytes(int cin, int cout);
int stv_conv_first_pack(const float* wf, float* packed, int cin, int cout, void* stream);
/* Forward: NCHW fp32 image [cin][H][W] -> NHWC `dtype` [H][W][cout]; bias fp32[cout] or NULL.
 * gram_partials (NULL, or where stv_conv_first_gram_supported says so: bf16, 3 -> 64) is for a first layer
 * that is a STYLE TAP (conv1_1 in the default layer set, core_model.py:213-226 / 297-314): besides y the
 * kernel leaves the split-K slabs of R = F^T F exactly as stv_gram_partial(y) would (stv_gram_ksplit(H*W, cout)
 * slabs of [cout][cout] fp32, to be reduced by stv_gram_finish / a stv_gram_multi tap with F == NULL),
 * computed from the rounded values it stores, so the map is not read back for the Gram matrix. */
int stv_conv_first_fwd(const float* x_nchw, const float* packed, const float* bias, void* y,
                       float* gram_partials, int H, int W, int cin, int cout, int dtype, void* stream);
/* Its input-gradient: dy NHWC `dtype` [H][W][cout] -> dx NCHW fp32 [cin][H][W] (written, not accumulated). */
int stv_conv_first_dgrad(const void* dy, const float* packed, float* dx_nchw,
                         int H, int W, int cin, int cout, int dtype, void* stream);
int stv_conv_first_gram_supported(int H, int W, int cin, int cout, int dtype);

/* Implicit-GEMM 3x3 conv, pad 1, stride 1, NHWC.  `w` is [taps][cout][cin] in
 * `dtype` (K-contiguous rows); bias fp32[cout] or NULL.  taps = 9 (3x3) or 1
 * (1x1, used for the Gram backward product).  flags: RELU_IN, RELU_OUT,
 * MASK (needs `ref`, NHWC [H][W][cout]), ACCUM, W_BLOCKED.  The same entry
 * computes the input gradient when given the flipped/transposed weights (dgrad).
 * With W_BLOCKED `w` is [taps][cin/CK][cout][CK] (CK = 16 bf16 / 8 fp32 channels,
 * cin % CK == 0): the 32-byte K slices a workgroup stages for its output channels
 * are then contiguous, so every weight load is a fully used cache line. */
/* Optional, once per shape (e.g. when a schedule is built): time every tile
 * configuration of stv_conv_igemm for this shape on scratch data and remember the
 * fastest for later calls (process-wide table keyed by shape; the analytic choice
 * is kept unless another tile is > 3 % faster).  Returns the configuration index
 * (>= 0; the value stv_conv_config reports afterwards), -1 when the shape runs on
 * the direct kernel (nothing to tune), or -(100 + STV_ERR_*) on failure.
 * Synchronises `stream` when it measures: only with STV_CONV_TUNE=1 / 2 in the environment (see the table
 * functions below); STV_CONV_TUNE=0 ignores the table and pins the analytic choice.
 * Different tiles sum K in different orders: results agree to fp32 rounding, not
 * bit for bit, across configurations.
 * taps = STV_TUNE_ROUTE (bf16): the shape is measured as stv_conv_igemm_route runs it (dgrad + pooling backward in
 * the epilogue, 2H x 2W output) and remembered under its own key - the routed epilogue prefers smaller tiles. */
#define STV_TUNE_ROUTE 109
/* the `element bytes` field of a tile-table entry for a STV_BF16X3 shape: its own key, fp32 tiles */
#define STV_TUNE_BF16X3 6
int stv_conv_tune(int H, int W, int cin, int cout, int taps, int dtype, void* stream);
/* The tile table as data (7 ints per entry: H, W, cin, cout, taps - 9, 1 or STV_TUNE_ROUTE -, element bytes, tile
 * index).  Measuring only happens with STV_CONV_TUNE=1 (or 2) in the environment; otherwise stv_conv_tune and every
 * conv launch look a shape up in this table and fall back to the analytic choice.  The host persists measured
 * tables (conv_tiles_gfx950.json) and imports them at load time, so that a shape runs on the same tile - same
 * summation order, same kernel name in a profile - in every process.  stv_conv_tune_export returns the number of
 * entries (and writes up to max_entries of them); stv_conv_tune_import adds / overwrites entries (0 entries: clears
 * the table), STV_ERR_ARG on a malformed entry. */
int stv_conv_tune_export(int* out7, int max_entries);
int stv_conv_tune_import(const int* in7, int n_entries);

/* Hint for the NEXT stv_conv_igemm* launch issued from this thread: `bytes` of weights that the conv launched AFTER
 * it will read.  That next launch touches them (one 128-byte line per lane, between its main loop and its epilogue) so
 * they are on chip when their own launch starts.  One shot: the launch that follows on this thread consumes the hint
 * (whichever kernel serves it), so a hint can never reach a later, unrelated launch; the tile tuner runs without one.  No
 * counterpart in the reference (cuDNN / oneDNN own their weights' residency). */
void stv_conv_next_weights(const void* w, size_t bytes);

/* Number of tile configurations stv_conv_config() can return (0 .. n-1): tools and the bench that name the kernel
 * instantiation of a tile check their tables against it. */
int stv_conv_num_configs(void);
/* What the calling thread's most recent stv_conv_igemm* call launched: the tile-table row (0 .. n-1) after every
 * stand-in rule (4-byte elements, whole stage pairs in both K extents, a pooled output on a tile without a pooling
 * window), -1 for the direct kernel, -2 for the weight-stationary kernel.  Host bookkeeping, no device work: the
 * tests use it to check that a forced tile (STV_CONV_CFG) is the tile that ran.  Since version 102. */
int stv_conv_last_launch(void);
int stv_conv_igemm(const void* x, const void* w, const float* bias, const void* ref,
                   void* y, int H, int W, int cin, int cout, int taps, int flags,
                   int dtype, void* stream);

/* Forward 3x3 conv that also emits MaxPool2d(2,2) of its output (`y_pool`,
 * NHWC [H/2][W/2][cout]) from the same epilogue: replaces the conv2d + relu +
 * max_pool2d run of `x = block(x)` (core_model.py:316) where a pool follows the
 * conv.  Matrix-core shapes only (stv_conv_config >= 0), else STV_ERR_ARG and the
 * caller pools with stv_maxpool_fwd.  flags: RELU_IN, RELU_OUT, W_BLOCKED.
 * `pool_idx` (optional, [H/2][W/2][cout] bytes) receives what max_pool2d's backward needs
 * instead of the full-resolution activation: bits 0-1 = window position (2*dy + dx) of the
 * first maximum in scan order, bit 2 = that maximum is > 0 (the ReLU mask of the winner);
 * decided on the values as stored in `y`.  stv_maxpool_bwd takes it with STV_POOL_IDX.
 * STV_POOL_ONLY: `y` is not written (it may be NULL) - for a conv whose full-resolution output nobody reads again:
 * the forward pass continues from `y_pool`, the backward pass routes through `pool_idx` (stv_conv_igemm_route /
 * stv_maxpool_bwd with STV_POOL_IDX), so the pre-pool map - four times the pooled one - never has to reach HBM.
 * The pooled map and the arg-max map are bit-identical to the ones written without the flag. */
int stv_conv_igemm_pool(const void* x, const void* w, const float* bias, void* y, void* y_pool,
                        void* pool_idx, int H, int W, int cin, int cout, int flags, int dtype,
                        void* stream);

/* Two-term gradient in one launch:
 *   y = [accumulate onto y +] mask(ref > 0) * conv3x3(x, w)  +  x2 . w2^T
 * x2 is NHWC [H][W][cin2], w2 plain [cout][cin2].  This is the backward of a layer whose
 * output feeds both the next conv (first term: that conv's dgrad, masked by this layer's
 * ReLU) and a Gram loss tap (second term: dF = F.S, `core_model.py:56-63` backward) - the
 * second term no longer needs its own launch nor a read-modify-write of y.
 * flags: MASK (applies to the first term only), ACCUM, W_BLOCKED (for w).  Matrix-core
 * shapes only (stv_conv_config(H,W,cin,cout,9,dtype) >= 0 and cin2 a multiple of the K
 * stage), else STV_ERR_ARG and the caller issues the two launches. */
int stv_conv_igemm_dual(const void* x, const void* w, const void* x2, const void* w2, const void* ref,
                        void* y, int H, int W, int cin, int cin2, int cout, int flags, int dtype,
                        void* stream);

/* Input gradient of the conv BEHIND a MaxPool2d(2,2), with the pooling backward folded into its epilogue:
 *   y_full[2H][2W][cout] <- route( conv3x3(x, w) )   (x = dy of that conv, w = its flipped/transposed weights)
 * every computed element goes to the position of its window's first maximum, as recorded by
 * stv_conv_igemm_pool in `pool_idx` ([H][W][cout] bytes), and - with STV_MASK - only where that maximum was
 * positive (the ReLU mask of the pre-pool activation, bit 2 of the byte); the other three positions of the
 * window receive zeros.  Replaces convolution_backward + max_pool2d_backward + threshold_backward of
 * `loss.backward()` (optimization.py:313) for that pair of layers, without the pooled-resolution gradient
 * ever being stored.  bf16 only, matrix-core shapes only, even 2H x 2W (the caller falls back to
 * stv_conv_igemm + stv_maxpool_bwd otherwise).  flags: MASK, W_BLOCKED. */
int stv_conv_igemm_route(const void* x, const void* w, const void* pool_idx, void* y_full, int H, int W, int cin,
                         int cout, int flags, int dtype, void* stream);

/* The size guard of the conv entry points, as a query (host arithmetic, no device work; since version 119).  The
 * kernels address every tensor with 32-bit byte offsets and use offset 2^31 for "nothing here", so every tensor of a
 * launch may hold AT MOST 2^31 bytes (exactly 2 GiB is accepted, 16 bytes more are not).  Counted in bytes of the
 * storage type (bf16 2, fp32 and bf16x3 4), per form:
 *   every form        x [H][W][cin], y [H][W][cout] (also `ref` and the STV_ACCUM read-back, and also under
 *                     STV_POOL_ONLY), w [taps][cout][cin], bias
 *   STV_CONV_POOL     + y_pool [H/2][W/2][cout] and the byte map (both below y: they never decide)
 *   STV_CONV_DUAL     + x2 [H][W][cin2], w2 [cout][cin2]   (cin2 > 0; every other form takes cin2 = 0)
 *   STV_CONV_ROUTE    + y_full [2H][2W][cout] = 4 x y, and the byte map [H][W][cout]   (bf16 only)
 * taps = 9, or 1 with STV_CONV_PLAIN.  STV_OK when stv_conv_igemm (PLAIN), _pool, _dual, _route would pass their size
 * guard for this shape, else STV_ERR_ARG - the value those entry points return for such a shape before any HIP call.
 * Says nothing about the other reasons an entry point refuses a shape (channel granularity, flags). */
enum { STV_CONV_PLAIN = 0, STV_CONV_POOL = 1, STV_CONV_DUAL = 2, STV_CONV_ROUTE = 3 };
int stv_conv_fits(int H, int W, int cin, int cout, int taps, int cin2, int form, int dtype);

/* Which tile the dispatcher picks for a shape: -1 = scalar fallback (channel counts not a
 * multiple of the MFMA K-slice), else 0..3 = {8x128, 8x64, 4x128, 4x64} (rows x couts) and
 * 4 = 4x64 with K split over two wave groups, 5 = 8x64 and 6 = 4x64 with a two-deep LDS ring,
 * 7 = 2x64 and 8 = 1x64 (four waves) with the K split.
 * -(100 + STV_ERR_ARG), like stv_conv_tune, for a shape the size guard refuses.  Both queries see neither a form nor
 * cin2: with taps = 9 or 1 they answer for STV_CONV_PLAIN - which is also the answer for STV_CONV_POOL, whose extra
 * tensors never decide - and with taps = STV_TUNE_ROUTE for STV_CONV_ROUTE; a dual launch asks stv_conv_fits. */
int stv_conv_config(int H, int W, int cin, int cout, int taps, int dtype);

/* 1 when stv_conv_igemm / _pool / _dual run this launch on the weight-stationary persistent kernel
 * (csrc/conv_ws.hip: 3x3, cin = 64, bf16, cout a multiple of 64; with a ReLU-mask / fused 1x1 term
 * only for cout = 64 and ref == x2), 0 when the general implicit-GEMM kernel takes it.  has_ref: the
 * launch carries `ref` (STV_MASK) and/or the fused term's x2; has_pool: it emits the pooled map. */
int stv_conv_uses_ws(int H, int W, int cin, int cout, int taps, int dtype, int flags, int has_ref, int has_pool);

/* MaxPool2d(2,2) forward / backward (first-max-wins like torch); backward
 * optionally applies the ReLU mask of the stored pre-pool activation (STV_MASK) and
 * accumulates (STV_ACCUM).  With STV_POOL_IDX `x` is the [H/2][W/2][C] byte map written by
 * stv_conv_igemm_pool: the pass then reads 1 byte instead of 4 activations per window. */
int stv_maxpool_fwd(const void* x, void* y, int H, int W, int C, int dtype, void* stream);
int stv_maxpool_bwd(const void* x, const void* dy, void* dx, int H, int W, int C,
                    int flags, int dtype, void* stream);
/* ---- AvgPool2d(2,2) forward / backward (--pooling avg; Gatys et al. 2016 replace VGG's max pooling by the mean).  Since
 *      version 113.  H, W: the un-pooled size; Hp = H / 2, Wp = W / 2 (floor: an odd last row / column takes no part).
 *   forward, per channel, in fp32, every sum rounded on its own (no FMA contraction), in exactly this order:
 *     y[i,j] = (((x[2i,2j] + x[2i,2j+1]) + x[2i+1,2j]) + x[2i+1,2j+1]) * 0.25f
 *   rounded once to the storage type (bf16: to nearest even); with STV_RELU_IN each operand is max(0, x) first.  This is
 *   what torch's CPU avg_pool2d computes, bit for bit, in fp32 and in bf16; the pairwise order (a+b)+(c+d) is not.
 *   backward:  v = 0.25f * dy[y/2, x/2] for y < 2*Hp and x < 2*Wp, else 0;  with STV_MASK v = 0 where !(ref > 0)
 *     (ref: the un-pooled activation, read only with STV_MASK);  dx = v, or with STV_ACCUM dx = dx + v - one fp32 sum,
 *     rounded once to storage.  Without STV_ACCUM the rows and columns the floor drops are written +0 (as stv_maxpool_bwd
 *     does); with it they are left as they are. ------------------------------------------------------------------------- */
/* launch constants: a work item is 16 bytes of one pooled pixel's channels (forward) or of one 2x2 window's channels, odd
 * tails included (backward); a pass of the capped grid covers STV_AVGPOOL_MAX_BLOCKS * STV_AVGPOOL_THREADS items.  Vector
 * path: C * element size a multiple of 16 behind 16-byte aligned bases; otherwise a work item is one element (forward: of
 * y, backward: of dx). */
#define STV_AVGPOOL_THREADS 256
#define STV_AVGPOOL_MAX_BLOCKS 2048
/* x, ref, dx: NHWC [H][W][C]; y, dy: NHWC [Hp][Wp][C]; all in `dtype` storage (STV_F32 | STV_BF16; STV_BF16X3 is
 * STV_ERR_ARG as for every op that forms no product - its storage is fp32).  flags: forward STV_RELU_IN; backward STV_MASK,
 * STV_ACCUM.
 * STV_ERR_ARG, before any HIP call: another dtype; a null pointer the mode needs (ref only with STV_MASK); H, W or C <= 0;
 * H / 2 == 0 or W / 2 == 0; a tensor of 2 GiB or more; any other flag. */
int stv_avgpool_fwd(const void* x, void* y, int H, int W, int C, int flags, int dtype, void* stream);
int stv_avgpool_bwd(const void* ref, const void* dy, void* dx, int H, int W, int C, int flags, int dtype, void* stream);
int stv_relu_fwd(const void* x, void* y, size_t n, int dtype, void* stream);
/* dx (=|+=) (x > 0) * dy ; dx may alias dy */
int stv_relu_bwd(const void* x, const void* dy, void* dx, size_t n, int flags,
                 int dtype, void* stream);

/* ---- Gram / style loss: replaces gram_matrix (core_model.py:29-63:
 *      mm(F,F^T).clamp(max).div(b*c*h*w)) + mse_loss (core_model.py:264) and
 *      their backward. ----------------------------------------------------- */

/* Split-K partial sums of F^T F over pixels.  F is NHWC [n_pixels][C];
 * partials is fp32 [ksplit][C][C] (upper tile triangle valid). */
int stv_gram_partial(const void* F, float* partials, int n_pixels, int C,
                     int dtype, void* stream);
/* Reduce partials -> raw Gram R; G = min(R, clamp_max) / norm.
 *  gram_out  (optional) fp32 [C][C]  <- G            (target capture)
 *  target    (optional) fp32 [C][C]
 *  loss_part (optional) fp32 [stv_gram_loss_parts(C)] <- partial sums of (G-T)^2
 *  sgrad     (optional) `dtype` [C][C] <- coef*(*coef_dev)*4/(C*C*norm) * (R<=clamp) * (G-T)
 */
int stv_gram_loss_parts(int channels);
int stv_gram_finish(const float* partials, const float* target, float* gram_out,
                    float* loss_part, void* sgrad, int n_pixels, int C, float clamp_max,
                    float norm, float coef, const float* coef_dev, int dtype, void* stream);

/* The Gram chain of several taps (layers) in one call: one batched stv_gram_partial launch per
 * tile size present plus one batched stv_gram_finish launch per slab-depth class, instead of two launches per tap.
 * The chain of a step is five small latency-bound problems; side by side in one grid they cost
 * the slowest, not the sum.  Fields as the arguments of the two calls above; at most 8 taps.
 * Same arithmetic, same fixed summation order as the per-tap calls. */
typedef struct {
  const void* F;          /* features, NHWC [n_pixels][channels] in `dtype`; NULL: `partials` is already filled
                             (stv_conv_first_fwd with gram_partials) and only the finish pass runs for this tap */
  float* partials;        /* stv_gram_partials_bytes(n_pixels, channels) */
  const float* target;    /* [C][C] or NULL */
  float* gram_out;        /* [C][C] or NULL */
  float* loss_part;       /* stv_gram_loss_parts(channels) floats, or NULL */
  void* sgrad;            /* backward seed [C][C] in `dtype`, or NULL */
  const float* coef_dev;  /* optional device scalar multiplying the seed */
  int n_pixels, channels;
  float clamp_max, norm, coef;
} stv_gram_tap_t;
int stv_gram_multi(const stv_gram_tap_t* taps, int n_taps, int dtype, void* stream);

/* ---- Content loss: mse_loss(features, target) (core_model.py:295). -------- */
#define STV_CONTENT_LOSS_PARTS 256
int stv_content_loss(const void* F, const void* target, float* loss_part, size_t n,
                     int dtype, void* stream);
/* Both at once for a step whose coefficient is known up front (the fused step: reference optimization.py:298-313
 * with content_w folded in): the loss partials exactly as stv_content_loss leaves them, and dF = coef*(2/n)*(F - target)
 * WRITTEN - the dgrad that later produces this layer's gradient accumulates onto it (STV_ACCUM). */
int stv_content_loss_grad(const void* F, const void* target, float* loss_part, void* dF, size_t n,
                          float coef, int dtype, void* stream);
/* dF (=|+=) coef*(*coef_dev)*(2/n)*(F - target) */
int stv_content_grad(const void* F, const void* target, void* dF, size_t n, float coef,
                     const float* coef_dev, int flags, int dtype, void* stream);

/* ---- Total variation of the image (no counterpart in the reference).  Since version 105.
 *      TV(x) = ( sum_{c,y<H-1,x} (x[c,y+1,x] - x[c,y,x])^2 + sum_{c,y,x<W-1} (x[c,y,x+1] - x[c,y,x])^2 ) / (C*H*W);
 *      differences never cross a row end or a channel plane. ---------------------------------------------------- */
#define STV_TV_LOSS_PARTS 256
/* x NCHW fp32 [C][H][W].  loss_part (optional): STV_TV_LOSS_PARTS raw partial sums of the squared forward
 * differences (unscaled; stv_loss_combine applies the scale), one per workgroup, fixed order, every entry written.
 * dx (optional): dx (=|+=, STV_ACCUM) coef * sum over the existing 4-neighbours n of (x - n), the differences added in
 * the order up, down, left, right; the product is rounded before it is added to dx (accumulate == write, then an fp32
 * add).  At least one of the two is non-NULL.  x != dx.  STV_ERR_ARG: null x, both outputs null, a non-positive
 * dimension, C*H*W*4 >= 2 GiB, a flag other than STV_ACCUM. */
int stv_tv(const float* x_nchw, float* loss_part, float* dx_nchw, int C, int H, int W, float coef, int flags, void* stream);

/* ---- Laplacian loss of the image against the content image (Li et al., "Laplacian-steered neural style transfer", ACM MM
 *      2017; no counterpart in the reference).  Since version 111.  For a pool size p (1, 2, 4, 8, 16 or 32):
 *        Hp = H / p, Wp = W / p (rows and columns past Hp*p and Wp*p take no part, as in avg_pool2d);
 *        P(x)[c,i,j] = the mean of cell (i, j) of plane c;   t = P(content), captured once;   e = P(x) - t;
 *        r = L e,  (L e)[i,j] = sum over the EXISTING 4-neighbours n of (e[i,j] - n), inside one plane (stv_tv's stencil);
 *        lap(x) = sum r^2 / (C*Hp*Wp);   d lap / dx[c,y,x] = 2 / (C*Hp*Wp*p*p) * (L r)[c, y/p, x/p] for y < Hp*p and x < Wp*p.
 *      Arithmetic, fixed to the bit (every add, subtraction and product rounded to fp32 on its own, no FMA contraction):
 *        cell mean: each of the p rows of the cell summed left to right, the p row sums summed top to bottom (the first
 *                   element starts a sum), then * 1/p^2 (a power of two: exact);
 *        residual:  e = mean - t, one subtraction (POOL stores the mean itself);
 *        stencil:   s = +0, then s = s + (e - n) for the existing neighbours in the order up, down, left, right;
 *        gradient:  g = L r with the same stencil, out = coef * g, dx = out, or dx = dx + out with STV_ACCUM. ---------------- */
enum { STV_LAP_POOL = 0, STV_LAP_LOSS = 1, STV_LAP_GRAD = 2 };
/* launch constants: every kernel runs workgroups of STV_LAP_THREADS.  LOSS: a workgroup owns a tile of STV_LAP_TILE_H x
 * STV_LAP_TILE_W cells of one plane and always runs as a grid of STV_LAP_LOSS_PARTS workgroups with a stride loop over the
 * tiles (planes, then tile rows, then tiles of a row).  GRAD: a work item is four consecutive pixels of one row, a pass of
 * the capped grid covers STV_LAP_GRAD_MAX_BLOCKS * STV_LAP_THREADS items. */
#define STV_LAP_THREADS 256
#define STV_LAP_TILE_H 8
#define STV_LAP_TILE_W 32
#define STV_LAP_LOSS_PARTS 256
#define STV_LAP_GRAD_MAX_BLOCKS 512
/* x NCHW fp32 [C][H][W] (H, W always the image's); target, cells fp32 [C][Hp][Wp]; dx NCHW fp32 [C][H][W].
 *   STV_LAP_POOL: cells = P(x).                                              needs x, cells
 *   STV_LAP_LOSS: cells = r; loss_part = STV_LAP_LOSS_PARTS raw partial sums of r^2 (unscaled; stv_loss_combine applies
 *                 the scale), one per workgroup, fixed order, no atomics, every entry written on every launch.
 *                                                                            needs x, target, cells, loss_part
 *   STV_LAP_GRAD: cells holds r (input); dx (=|+=, STV_ACCUM) coef * (L r) of the pixel's cell.  With STV_ACCUM the pixels
 *                 outside Hp*p x Wp*p are left untouched, without it they are written +0.     needs cells, dx
 * STV_ERR_ARG, before any HIP call: a null pointer the mode needs; C, H or W <= 0; a pool other than 1, 2, 4, 8, 16, 32;
 * H / pool == 0 or W / pool == 0; C*H*W*4 >= 2 GiB; an unknown mode; a flag other than STV_ACCUM, or STV_ACCUM outside
 * STV_LAP_GRAD; dx sharing a byte with cells. */
int stv_lap(const float* x_nchw, const float* target, float* cells, float* loss_part, float* dx_nchw, int C, int H, int W,
            int pool, float coef, int mode, int flags, void* stream);

/* ---- 2x resize of the image between the levels of a coarse-to-fine run (no counterpart in the reference).  Since
 *      version 106.  Every product and every sum below is rounded to fp32 on its own (no FMA contraction), in the order
 *      written, so that an fp32 twin reproduces every output bit.
 *      DOWN2, the 2x2 box mean:
 *        y[c,Y,X] = ((x[c,2Y,2X] + x[c,2Y,2X+1]) + (x[c,2Y+1,2X] + x[c,2Y+1,2X+1])) * 0.25f
 *      UP2, bilinear with half-pixel centres and clamped edges (F.interpolate(scale_factor=2, mode="bilinear",
 *      align_corners=False)), separable, columns first: for output column X the near column is n = X >> 1 and the far
 *      column f = clamp(n + (X odd ? +1 : -1), 0, W-1);  h[r,X] = 0.75f*x[r,n] + 0.25f*x[r,f];  the same rule along rows
 *      on h:  y[Y,X] = 0.75f*h[near row,X] + 0.25f*h[far row,X].  Nothing is read across a channel plane. ------------- */
enum { STV_RESIZE_DOWN2 = 0, STV_RESIZE_UP2 = 1 };
/* launch constants: a work item is four consecutive output pixels of one row, a pass of the capped grid covers
 * STV_RESIZE_MAX_BLOCKS * STV_RESIZE_THREADS items */
#define STV_RESIZE_THREADS 256
#define STV_RESIZE_MAX_BLOCKS 1024
/* x NCHW fp32 [C][H][W] -> y NCHW fp32: DOWN2 [C][H/2][W/2] (H, W even), UP2 [C][2H][2W].  x != y.
 * STV_ERR_ARG: a null pointer, x == y, a non-positive dimension, odd H or W with DOWN2, an unknown mode, an input or
 * an output of 2 GiB or more. */
int stv_resize2x(const float* x, float* y, int C, int H, int W, int mode, void* stream);

/* ---- General resize of an input image (--content-size, --style-size, --style-scale; no counterpart in the reference).
 *      Since version 109.  One pass of a separable, antialiased resampler: the image is resized along one axis by the
 *      tables the host builds (resize.py: triangle, Keys cubic or Lanczos-3, stretched by the scale factor on a
 *      downscale).  Output index i along that axis is
 *        acc = 0.0f;  for k = 0 .. count[i]-1 ascending:  acc = acc + (weights[i*K + k] * x[.. start[i] + k ..])
 *      with every product and every sum rounded to fp32 on its own (no FMA contraction), so that an fp32 twin reproduces
 *      every output bit.  A full resize is the column pass (axis 1) into an intermediate [planes][H][Wo], then the row
 *      pass (axis 0); the caller owns the intermediate and the tables, and skips a pass whose axis keeps its size.
 *      Nothing is read across a row end or a channel plane; entries of `weights` behind count[i] are never read. ------ */
/* launch constants: a work item is STV_RESIZE_AXIS_VEC consecutive output pixels of one row, a pass of the capped grid
 * covers STV_RESIZE_AXIS_MAX_BLOCKS * STV_RESIZE_AXIS_THREADS items.  Vector path: output rows of a multiple of four
 * floats behind a 16-byte aligned y (and, for axis 0, x); otherwise the same items with guarded scalar accesses. */
#define STV_RESIZE_AXIS_VEC 4
#define STV_RESIZE_AXIS_THREADS 256
#define STV_RESIZE_AXIS_MAX_BLOCKS 1024
/* x NCHW fp32 [planes][H][W] -> y NCHW fp32: axis 0 [planes][n_out][W] (rows), axis 1 [planes][H][n_out] (columns).
 * start, count: int32 [n_out] on the device, start[i] >= 0 and start[i] + count[i] <= the input's size along the axis;
 * weights: fp32 [n_out][K] on the device, K >= max(count).  x != y.
 * STV_ERR_ARG, before any device work: a null pointer, x == y, a non-positive size, an axis other than 0 or 1, K < 1,
 * an input or an output of 2 GiB or more. */
int stv_resize_axis(const float* x, float* y, int planes, int H, int W, int n_out, int axis, const int32_t* start,
                    const int32_t* count, const float* weights, int K, void* stream);

/* ---- Colour preservation (--preserve-color; no counterpart in the reference; Gatys et al. 2017, "Controlling
 *      perceptual factors in neural style transfer", section 5).  Since version 107.  Three streaming passes over the
 *      image, none of them inside the step.  All three take NCHW fp32 [3][H][W] and return STV_ERR_ARG, before any HIP
 *      call, for a null pointer, a non-positive dimension or 3*H*W*4 >= 2 GiB. ------------------------------------------ */
/* launch constants: a work item is STV_COLOR_VEC consecutive pixels of one row, read from all three planes; the three
 * kernels run STV_COLOR_THREADS threads per workgroup; stv_color_stats always launches STV_COLOR_STATS_PARTS workgroups
 * (one row of `parts` each: the constant is its grid and its grid cap), the other two at most STV_COLOR_MAX_BLOCKS, so
 * a pass of the capped grid covers STV_COLOR_STATS_PARTS * STV_COLOR_THREADS, respectively STV_COLOR_MAX_BLOCKS *
 * STV_COLOR_THREADS items.  Vector path (16-byte loads and stores): W % 4 == 0 behind 16-byte aligned bases; otherwise
 * the same items with guarded scalar accesses, same results in the same order. */
#define STV_COLOR_VEC 4
#define STV_COLOR_THREADS 256
#define STV_COLOR_STATS_PARTS 256
#define STV_COLOR_MAX_BLOCKS 1024
/* Raw colour moments.  parts is double [STV_COLOR_STATS_PARTS][9], one row per workgroup, each row
 *   sum x0, sum x1, sum x2, sum x0x0, sum x0x1, sum x0x2, sum x1x1, sum x1x2, sum x2x2
 * over that workgroup's pixels; products and sums are formed in double from the fp32 values (a product of two fp32
 * numbers is exact in double: cov = sum xx / n - mean^2 cancels, and the pass is memory-bound either way).  Fixed order
 * - thread in item order, then wave, then workgroup -, no atomics; every entry is written, a workgroup without items
 * writes zeros.  The caller adds the rows (in float64, on the host). */
int stv_color_stats(const float* x_nchw, double* parts, int H, int W, void* stream);
/* Per-pixel affine map of the three channels.  m12: HOST array of 12 floats, the row-major 3x3 matrix m followed by the
 * offset b, passed by value into the launch (as stv_image_to_u8 takes mean3 / std3).
 *   y[c] = ((m[c][0]*x[0] + m[c][1]*x[1]) + m[c][2]*x[2]) + b[c]
 * every product and every sum rounded to fp32 on its own, in that order (no FMA contraction).  y == x (in place) is
 * allowed; any other overlap of the two ranges is STV_ERR_ARG. */
int stv_color_affine(const float* x_nchw, float* y_nchw, const float* m12, int H, int W, void* stream);
/* Luminance of `result`, chrominance of `content`.  mean3 / std3: HOST arrays of 3 floats, or both NULL for an
 * un-normalised image.  Per pixel and channel c, every operation rounded to fp32 on its own:
 *   r_c = result[c]*std[c] + mean[c]  (result[c] when un-normalised), then prepare_image_for_output's rule
 *         (image_io.py:129-152): nan -> 0, +inf -> 1, -inf -> 0, clamp to [0,1];  k_c: the same function of content[c];
 *   Yr = (0.299f*r_0 + 0.587f*r_1) + 0.114f*r_2  (Rec.601), Yk likewise;  d = Yr - Yk;  o_c = k_c + d;
 *   out[c] = (o_c - mean[c]) * inv_std[c], inv_std[c] = 1.0f / std[c] formed on the host  (out[c] = o_c un-normalised).
 * o_c is not clamped: the export path (stv_image_to_u8) clamps.  out == result is allowed.  STV_ERR_ARG also for
 * out == content or any other overlap of `out` with an input, and for one of mean3 / std3 without the other. */
int stv_luma_transfer(const float* result, const float* content, float* out, int H, int W, const float* mean3,
                      const float* std3, void* stream);

/* ---- Automatic masks (--auto-mask; no counterpart in the reference): the assignment pass of a joint colour k-means over
 *      the pooled content and style images, which gives the two label maps of a guided run.  Since version 114.  One launch
 *      per image and iteration while the run is set up, none inside the step.  Per pixel p of x, NCHW fp32 [3][H][W]:
 *   e_j  = x_j(p) - c_k[j]                          j = 0, 1, 2;  c: the K centroids
 *   d_k  = ((e0*e0 + e1*e1) + e2*e2)                every difference, product and sum rounded to fp32 on its own (no FMA
 *                                                   contraction): an fp32 twin reproduces every bit
 *   label(p) = the first k, ascending, with d_k < the best so far, which starts at +inf (a strict `<`: the lowest index
 *              wins a tie; a pixel whose every distance is NaN or +inf gets label 0)
 *      Inputs are taken as finite.  A NaN distance never wins and nothing faults, but the sums are then meaningless. ---- */
/* launch constants: a work item is four consecutive pixels of one row read from all three planes, as for the colour kernels
 * (STV_COLOR_VEC), and their four labels; the kernel always launches STV_KMEANS_PARTS workgroups of STV_KMEANS_THREADS
 * threads (one row of `parts` each: the constant is its grid and its grid cap), a stride loop over the items, so a pass
 * covers STV_KMEANS_PARTS * STV_KMEANS_THREADS items.  Vector path (three 16-byte loads, one 32-bit load and store of the
 * labels): W % 4 == 0 behind a 16-byte aligned x and 4-byte aligned labels; otherwise the same items with guarded scalar
 * and byte accesses, same results in the same order. */
#define STV_KMEANS_THREADS 256
#define STV_KMEANS_PARTS 256
#define STV_KMEANS_PART_DOUBLES 17
/* centroids: fp32 [K][3] on the device, 1 <= K <= 4, uniform over the launch.  labels: uint8 [H][W] on the device; in: the
 * labels of the previous iteration (any bytes before the first), out: the new ones - an item reads its four before it
 * writes them and no other item touches them, so in place is the contract.  parts: double [STV_KMEANS_PARTS]
 * [STV_KMEANS_PART_DOUBLES], one row per workgroup: for k < 4 at 4k .. 4k+3 the sums of x0, x1, x2 over the workgroup's
 * pixels with label k and their number, at [16] the number of its pixels whose label changed.  Sums in double, fixed order -
 * thread in item order, pixel by pixel, then wave, then workgroup -, no atomics; every entry is written on every launch,
 * zeros for k >= K and for a workgroup without items.  The caller adds the rows (in float64, on the host).
 * STV_ERR_ARG, before any HIP call: a null pointer, a non-positive dimension, K outside 1..4, 3*H*W*4 >= 2 GiB. */
int stv_kmeans_assign(const float* x_nchw, const float* centroids, uint8_t* labels, double* parts, int H, int W, int K,
                      void* stream);

/* ---- Automatic masks in VGG feature space (--auto-mask-space features; no counterpart in the reference): the joint
 *      k-means over one VGG layer's activations of the content and of the style image.  Since version 118.  Two assignment
 *      launches and one update launch per iteration while the run is set up, none inside the step.  A point is a pixel of
 *      F, NHWC [n][C] of bf16 or fp32 (bf16 -> fp32 by the exact bit shift), C = 64, 128, 256 or 512 (the channel
 *      counts of VGG; Q below must be a power of two: the lane maps and the pairwise sums halve it down to 1).  The channel axis
 *      is cut into Q = C/8 octets of 8 consecutive channels; with o the octet and k the centroid:
 *   p_k[o]   = (...((0 + e_0*e_0) + e_1*e_1) ...) + e_7*e_7,  e_j = x[8o+j] - c_k[8o+j]     ascending j
 *   d_k      = the Q octet sums combined pairwise: for s = Q/2, Q/4, ..., 1:  p_k[o] = p_k[o] + p_k[o+s]  (o < s);  d_k = p_k[0]
 *              every difference, product and sum rounded to fp32 on its own (no FMA contraction): an fp32 twin reproduces
 *              every bit
 *   label(p) = the first k, ascending, with d_k < the best so far, which starts at +inf (a strict `<`: the lowest index
 *              wins a tie; a NaN distance never wins; a pixel whose every distance is NaN or +inf gets label 0)
 *      Inputs are taken as finite. ---- */
/* launch constants.  A pixel belongs to Q lanes of one wave (one octet each: a 16-byte load of bf16, two of fp32), so a wave
 * holds G = 64/Q pixels at a time, a workgroup of STV_KMF_THREADS threads STV_KMF_WAVES * G, and the kernel always launches
 * STV_KMF_PARTS workgroups (one row of `parts` each): a pass of the grid covers STV_KMF_PARTS * STV_KMF_WAVES * G pixels.
 * Pixel p sits in
 *   pass = p / (STV_KMF_PARTS * STV_KMF_WAVES * G),   r = p % (STV_KMF_PARTS * STV_KMF_WAVES * G),
 *   workgroup = r / (STV_KMF_WAVES * G),   wave = (r / G) % STV_KMF_WAVES,   group = r % G,   lane = group * Q + octet
 * so the 64 lanes of a wave read 64 * 8 consecutive elements.  Order of the double sums of one entry: a lane adds its pixels
 * in pass order (a pixel of another label, and a pixel past n, adds +0.0); the G lanes of a wave that hold the same octet
 * combine pairwise, for h = G/2, ..., 1: v[g] = v[g] + v[g+h] (g < h); the waves add into a zeroed entry in wave order. */
#define STV_KMF_THREADS 256
#define STV_KMF_WAVES 4
#define STV_KMF_PARTS 256
#define STV_KMF_MAX_K 4
#define STV_KMF_MAX_C 512
/* doubles in one row of `parts` for C channels: for k < 4 at k*(C+1) .. k*(C+1)+C-1 the channel sums of the workgroup's
 * pixels with label k and at k*(C+1)+C their number; at 4*(C+1) the number of its pixels whose label changed */
#define STV_KMF_ROW_DOUBLES(C) (4 * ((C) + 1) + 1)
/* F: [n][C] on the device, 16-byte aligned, dtype STV_F32 or STV_BF16.  centroids: fp32 [K][C] on the device, uniform over
 * the launch.  labels: uint8 [n]; in: the previous labels (any bytes before the first iteration), out: the new ones - the
 * octet-0 lane of a pixel reads its byte before it writes it and no other lane touches it, so in place is the contract.
 * keep_labels != 0: labels are read and not written, no distance is formed, the changed count is 0 and a pixel whose
 * label is >= K is in no sum (the pass that gives the mean: all labels 0, K = 1).  parts: double [STV_KMF_PARTS]
 * [STV_KMF_ROW_DOUBLES(C)]; no atomics; every entry is written on every launch, zeros for k >= K and for a workgroup
 * without pixels.
 * STV_ERR_ARG, before any HIP call: a null pointer, n < 1, C other than 64, 128, 256, 512 (192, 320, 384 and 448 included),
 * K outside 1..4, a dtype other than the two, n*C of 2^31 elements or more, F not 16-byte aligned. */
int stv_kmeans_feat_assign(const void* F, int dtype, const float* centroids, uint8_t* labels, double* parts, int n, int C,
                           int K, int keep_labels, void* stream);
/* The centroid update on the device, one work item per (k, c), k < K, c < C.  With i = content (parts_c, n_c) and style:
 *   S_k^i[c], N_k^i, changed^i = the STV_KMF_PARTS rows of parts_i added in index order (from the first row's value)
 *   w_k      = N_k^c/n_c + N_k^s/n_s
 *   c_k[c]   = fp32((S_k^c[c]/n_c + S_k^s[c]/n_s) / w_k)     every operation a double operation of its own (no FMA
 *              contraction), one rounding to fp32; where w_k == 0 (a cluster empty in both images) c_k is left as it is
 * centroids: fp32 [K][C], updated in place.  result: double [9] on the device - [0..3] N_k^c, [4..7] N_k^s (zeros for
 * k >= K), [8] changed^c + changed^s: all the host reads per iteration.
 * STV_ERR_ARG, before any HIP call: a null pointer, n_c < 1, n_s < 1, C other than 64, 128, 256, 512, K outside 1..4. */
int stv_kmeans_feat_update(const double* parts_c, const double* parts_s, float* centroids, double* result, int n_c, int n_s,
                           int C, int K, void* stream);

/* ---- Blended Gram targets (several style images with blend weights; no counterpart in the reference; jcjohnson's
 *      -style_blend_weights).  Since version 110.  One launch per style layer when targets are set, none inside the step.
 *   out[i] = (...((w[0]*G_0[i]) + w[1]*G_1[i]) + ...) + w[K-1]*G_{K-1}[i]      i < n
 *      every product and every sum rounded to fp32 on its own, tables in ascending order, no FMA contraction: an fp32
 *      twin reproduces every bit. ----------------------------------------------------------------------------------- */
/* launch constants: a work item is STV_BLEND_VEC consecutive elements (16-byte loads and a 16-byte store), a pass of the
 * capped grid covers STV_BLEND_MAX_BLOCKS * STV_BLEND_THREADS items; the n % STV_BLEND_VEC last elements are a scalar tail. */
#define STV_BLEND_MAX_TABLES 8
#define STV_BLEND_VEC 4
#define STV_BLEND_THREADS 256
#define STV_BLEND_MAX_BLOCKS 128
/* stack: fp32 [K][n] on the device, contiguous; weights: HOST array of K floats, passed to the kernel by value;
 * out: fp32 [n] on the device, sharing no byte with the stack.
 * STV_ERR_ARG, before any HIP call: a null pointer, K < 1 or K > STV_BLEND_MAX_TABLES, n < 1, a weight that is negative
 * or not finite, a stack of 2 GiB or more, `out` overlapping the stack. */
int stv_gram_blend(const float* stack, float* out, const float* weights, int K, long long n, void* stream);

/* ---- Spatial guidance (--content-mask, --style-mask; no counterpart in the reference; Gatys et al. 2017, "Controlling
 *      perceptual factors in neural style transfer", section 4.2, the guided Gram matrices).  Since version 112.  One launch
 *      per style tap and evaluation, in front of that tap's Gram chains:
 *   out[r][p][c] = labels[p] == r ? F[p][c] : +0        r < R,  p < n_pixels,  c < C
 *      No arithmetic: an element of a slab holds the bits of its source (NaN payloads and -0 survive) or the bits of +0.
 *      A label >= R (255 by convention: no region) leaves the pixel zero in every slab.  Every element is written. ------ */
/* launch constants: a work item is 16 bytes of one pixel's channels (one 16-byte load, R 16-byte stores: F is read once,
 * whatever R), a pass of the capped grid covers STV_MASK_SPLIT_MAX_BLOCKS * STV_MASK_SPLIT_THREADS items.  Vector path:
 * C * element size a multiple of 16 behind 16-byte aligned F and out; otherwise a work item is one element. */
#define STV_MASK_MAX_REGIONS 4
#define STV_MASK_SPLIT_THREADS 256
#define STV_MASK_SPLIT_MAX_BLOCKS 1024
/* F: NHWC [n_pixels][C] in `dtype` storage (STV_F32 | STV_BF16; STV_BF16X3 is STV_ERR_ARG as for every op that forms no
 * product - its storage is fp32); labels: uint8 [n_pixels] on the device; out: [R][n_pixels][C], contiguous slabs, the
 * offsets between them 64-bit.
 * STV_ERR_ARG, before any HIP call: a null pointer, R < 1 or R > STV_MASK_MAX_REGIONS, n_pixels < 1, C < 1, a slab of
 * 2 GiB or more, `out` overlapping F or labels. */
int stv_mask_split(const void* F, const uint8_t* labels, void* out, size_t n_pixels, int C, int R, int dtype, void* stream);

/* ---- Frame / PNG export: prepare_image_for_output (image_io.py:129-152: denormalise,
 *      nan_to_num(nan=0, posinf=1, neginf=0), clamp 0..1) fused with the uint8 conversion, on the
 *      device, so only H*W*3 bytes cross to the host.  x NCHW fp32 [3][H][W] -> out HWC uint8.
 *      mean3/std3: HOST arrays of 3 floats (ImageNet statistics, constants.py:11-12) or both NULL
 *      for an un-normalised image.  round = 0: (uint8)(v*255), the truncating frame conversion of
 *      optimization.py:445-451; round = 1: (uint8)clamp(v*255 + 0.5, 0, 255), what
 *      torchvision.utils.save_image does for the final PNG (runtime/output.py:101). */
int stv_image_to_u8(const float* x_nchw, uint8_t* out_hwc, int H, int W, const float* mean3,
                    const float* std3, int round, void* stream);

/* ---- Timelapse GIF output (--gif; the reference encodes its timelapse on the host): the two device passes over the
 *      captured frames, HWC uint8 [H][W][3] as stv_image_to_u8 (round = 0) writes them.  Since version 115.  One
 *      stv_frame_hist launch per saved frame, behind its capture; one stv_gif_map launch per frame when the file is
 *      written; none inside the step.  All arithmetic is integer and fixed to the bit.
 *   stv_frame_hist:   hist[(r>>3)<<10 | (g>>3)<<5 | (b>>3)] += 1            for every pixel (r, g, b) of the frame
 *   stv_gif_map, per pixel (y, x):
 *     t      = B8[y & 7][x & 7]                     the 8x8 Bayer matrix, a permutation of 0..63:
 *              B8[y][x] = OR over b = 0..2 of  (((x>>b)&1) ^ ((y>>b)&1)) << (2*(2-b)+1)  and  ((y>>b)&1) << (2*(2-b))
 *              (row 0 starts 0, 32, 8, 40; row 1 starts 48, 16, 56, 24)
 *     off    = ((2*t - 63) * spread) >> 7           arithmetic shift (floor); spread 0 = no dither, spread 16 gives -8..7
 *     v[c]   = clamp(frame[y][x][c] + off, 0, 255)  the same offset for the three channels
 *     index  = argmin_k  sum_c (v[c] - palette[k][c])^2     over k < n_colors, in int32; the lowest k wins a tie
 *      The search is exact and brute force (no lookup table). ------------------------------------------------------- */
/* launch constants: a frame is walked as a flat run of pixels, a work item is four consecutive pixels (12 bytes in, the
 * map: 4 bytes out), a pass of the capped grid covers STV_GIF_MAX_BLOCKS * STV_GIF_THREADS items.  Vector path (three
 * 32-bit loads, the map: one 32-bit store): a 4-byte aligned frame - and, for the map, a 4-byte aligned index plane -, for
 * every item with four pixels; otherwise, and for the last n % 4 pixels, the same items with byte accesses and the same
 * results.  Frame i of a packed store starts at byte i*H*W*3 and its index plane at byte i*H*W: aligned or not. */
#define STV_GIF_THREADS 256
#define STV_GIF_MAX_BLOCKS 2048
#define STV_GIF_HIST_BINS 32768
/* hist: uint32 [STV_GIF_HIST_BINS] on the device.  The kernel ACCUMULATES: the caller zeroes hist once and adds any number
 * of frames.  No-return global atomic adds: integer adds commute, so - unlike the floating-point statistics kernels -
 * the result depends neither on their order nor on how pixels are grouped into one add (a run of equal bins inside a work
 * item, and a wave whose 256 pixels share one bin, are added at once: a constant frame does not queue on one counter).
 * STV_ERR_ARG, before any HIP call: a null pointer, n_pixels == 0, n_pixels*3 >= 2 GiB. */
int stv_frame_hist(const uint8_t* frame_hwc, size_t n_pixels, uint32_t* hist, void* stream);
/* index_hw: uint8 [H][W] on the device, every byte written, sharing no byte with the frame.  palette: uint8 [n_colors][3]
 * on the device, staged once per workgroup in LDS.
 * STV_ERR_ARG, before any HIP call: a null pointer, H or W <= 0, n_colors outside 1..256, spread outside 0..64,
 * H*W*3 >= 2 GiB. */
int stv_gif_map(const uint8_t* frame_hwc, uint8_t* index_hw, int H, int W, const uint8_t* palette, int n_colors, int spread,
                void* stream);

/* ---- Motion-JPEG timelapse (--video-format mjpeg; the reference encodes H.264 through ffmpeg on the host): every saved
 *      frame becomes one baseline JPEG, 4:2:0, Annex K Huffman tables (ITU T.81).  Since version 116.  One stv_jpeg_dct
 *      launch per saved frame, behind its capture; stv_jpeg_block_bits, stv_jpeg_scan and stv_jpeg_emit run over all frames
 *      when the file is written; none inside the step.  All arithmetic is integer and fixed to the bit.
 *   MCU and edges: an MCU is 16x16 pixels, MCUs are row-major, mcu_w = (W+15)/16, mcu_h = (H+15)/16; the blocks of an MCU
 *     are Y00 Y01 Y10 Y11 Cb Cr (Yrc: row r, column c of the 2x2 luminance blocks).  A pixel past the right or the bottom
 *     edge is the last pixel of its row / the last row (coordinates clamped to W-1, H-1).
 *   Colour, int32 per pixel (r, g, b):
 *     Y  = ( 19595*r + 38470*g +  7471*b + 32768) >> 16
 *     Cb = (-11059*r - 21709*g + 32768*b + 8388608 + 32767) >> 16
 *     Cr = ( 32768*r - 27439*g -  5329*b + 8388608 + 32767) >> 16           all three in 0..255
 *   Chroma sample (cy, cx) of an MCU: the Cb (Cr) values of pixels (2cy..2cy+1, 2cx..2cx+1), (sum + 2) >> 2.
 *   Level shift: s = sample - 128.
 *   DCT table: T[u][x] = rint(8192 * c(u)/2 * cos((2x+1) u pi / 16)), c(0) = 1/sqrt(2), c(u) = 1: STV_JPEG_DCT_TABLE.
 *   Rows:    a[y][u] = sum_x T[u][x] * s[y][x];   a1 = (a + 128) >> 8        (arithmetic shift)
 *   Columns: b[v][u] = sum_y T[v][y] * a1[y][u]                              (the coefficient times 2^18)
 *     |a| <= 2965504, |a1| <= 11584, |b| <= 268378112: int32 throughout.
 *   Quantisation with q = qtab[v*8 + u] (table 0 for Y, table 1 for Cb and Cr; row-major, v the vertical frequency):
 *     d = q << 18;  c = sign(b) * ((|b| + (d >> 1)) / d)                     (round half away from zero)
 *     c is clamped to -1023..1023, the DC (v = u = 0) to -1024..1023, and stored as int16 at the zigzag position of (v, u).
 *   Entropy code of a block (baseline Huffman, class 0 tables for Y, class 1 for Cb and Cr): the DC difference against
 *     the previous block of the same component in scan order (0 in front of a frame's first): the code of its category
 *     (bit length of its magnitude, 0..11), then that many value bits (v for v > 0, the low bits of v - 1 for v < 0);
 *     every non-zero AC coefficient as the code of (run << 4 | category) and its value bits, a run of 16 or more zeros in
 *     front of it as one ZRL (0xF0) per 16; an EOB (0x00) unless coefficient 63 is non-zero.  Bits are MSB first.  The
 *     last block of a frame pads the stream to a byte with 1-bits.  0xFF stuffing is left to the host. ------------------ */
#define STV_JPEG_DCT_TABLE                                        \
  {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},              \
   {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},            \
   {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784},          \
   {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},            \
   {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896},          \
   {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},            \
   {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567},          \
   {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}}
/* launch constants: stv_jpeg_dct runs workgroups of STV_JPEG_DCT_THREADS, 8 lanes per 8x8 block (a lane is one row of the
 * block in the row pass and one column in the column pass, LDS in between), one workgroup per 32 blocks; the three entropy
 * kernels run workgroups of STV_JPEG_THREADS, a work item one block (stv_jpeg_scan: one workgroup per frame).  A block's
 * code is at most STV_JPEG_MAX_BLOCK_BITS long (DC 11 + 11, 63 AC of 16 + 10, rounded up to 32), and bit offsets are 32
 * bits wide: a frame has fewer than 2^32 / STV_JPEG_MAX_BLOCK_BITS blocks. */
#define STV_JPEG_DCT_THREADS 256
#define STV_JPEG_THREADS 256
#define STV_JPEG_MAX_BLOCK_BITS 1664
#define STV_JPEG_MAX_DIM 65535
/* frame_hwc: uint8 [H][W][3] on the device, at any byte address (32-bit loads where a row of a block is 4-byte aligned and
 * inside the frame, byte loads elsewhere: the same results).  qtabs: HOST array of 128 ints, table 0 then table 1, row-major,
 * passed by value into the launch.  coef: int16 [mcu_h*mcu_w*6][64] on the device, 16-byte aligned, every element written
 * (16-byte stores).  STV_ERR_ARG, before any HIP call: a null pointer, H or W outside 1..STV_JPEG_MAX_DIM, a table entry
 * outside 1..255, a misaligned coef. */
int stv_jpeg_dct(const uint8_t* frame_hwc, const int* qtabs, int H, int W, int16_t* coef, void* stream);
/* coef: int16 [n_frames][blocks_per_frame][64], 16-byte aligned; bits: uint32 [n_frames][blocks_per_frame], the length of
 * each block's code in bits (without the padding of a frame's last block).  blocks_per_frame: a multiple of 6.
 * STV_ERR_ARG, before any HIP call: a null pointer, n_frames or blocks_per_frame <= 0, blocks_per_frame no multiple of 6 or
 * >= 2^32 / STV_JPEG_MAX_BLOCK_BITS, n_frames * blocks_per_frame >= 2^31, a misaligned coef. */
int stv_jpeg_block_bits(const int16_t* coef, int n_frames, int blocks_per_frame, uint32_t* bits, void* stream);
/* offsets[f][b] = bits[f][0] + ... + bits[f][b-1] (an exclusive prefix sum per frame), totals[f] = the sum of frame f.
 * One workgroup per frame; integer sums, so the result does not depend on how the sum is split.  STV_ERR_ARG as above. */
int stv_jpeg_scan(const uint32_t* bits, int n_frames, int blocks_per_frame, uint32_t* offsets, uint32_t* totals, void* stream);
/* Writes the code of every block at bit offsets[f][b] of frame f's stream, which starts at byte base[f] of `stream_bytes`
 * (base: uint32 [n_frames] on the device, multiples of 4).  `stream_bytes`: capacity bytes on the device, 4-byte aligned,
 * capacity a multiple of 4, ZEROED by the caller; frame f occupies ((totals[f] + 7) / 8) bytes from base[f], and the caller
 * leaves at least that, rounded up to 4, between two bases.  The stream is written as big-endian 32-bit words: a word a
 * block shares with a neighbour (its first and its last) is combined with a vector atomic OR, a word it owns is stored.
 * Integer OR commutes, so the bytes do not depend on any order.  No word at or past `capacity` is touched.
 * STV_ERR_ARG, before any HIP call: as stv_jpeg_block_bits, and capacity == 0, capacity % 4 != 0 or capacity >= 2^32, a misaligned stream. */
int stv_jpeg_emit(const int16_t* coef, const uint32_t* offsets, const uint32_t* base, int n_frames, int blocks_per_frame,
                  uint8_t* stream_bytes, size_t capacity, void* stream);

/* ---- Score combine: torch.stack(losses).sum() and
 *      loss = style_w*style + content_w*content (optimization.py:298-312).
 *  table: int32 [n_terms][3] = {offset into parts, count, kind(0 style,1 content,2 extra)}
 *  scale: fp32 [n_terms] (1/C^2 for style, 1/n for content)
 *  losses: fp32 [n_terms]; scores: fp32 [4] = {style, content, total, finite_flag}
 *  kind 2 (since version 105): a term that belongs to neither score - the total-variation term, whose weight the host
 *  folds into its scale, fp32(tv_w / (C*H*W)).  After total = style_w*style + content_w*content is formed as before,
 *  the kind-2 terms are added to it in index order, one fp32 add each; losses[k] is the weighted term.
 *  Since version 111 the Laplacian terms are kind-2 rows too, one per pool size, scale fp32(lap_w / (C*Hp*Wp)).
 *  n_terms <= 64 (STV_ERR_ARG beyond). */
int stv_loss_combine(const float* parts, const int32_t* table, const float* scale,
                     int n_terms, float style_w, float content_w, float* losses,
                     float* scores, void* stream);
/* The same, and the producer also keeps the per-step history the reference's LossAccumulator keeps on the
 * device (loss_accumulator.py:97-118: one ring slot per step): log_ring fp32 [3][log_capacity] (style, content,
 * total), log_count = evaluations so far (device counter, advanced here), slot = count % capacity.  Saves the
 * per-step copy kernel between two replays of the captured step.  log_ring and log_count both NULL: as above.
 * log_seq (optional): the ring is HOST memory from stv_host_mailbox_alloc and *log_seq, in the same allocation, receives
 * the record count after the record (system-scope release): the host reads a step's scores as soon as the combine kernel
 * has run - no copy, no stream synchronisation, the rest of the step still in flight (the reference's logging point,
 * optimization.py:375-391, blocks on .item() there). */
int stv_loss_combine_log(const float* parts, const int32_t* table, const float* scale,
                         int n_terms, float style_w, float content_w, float* losses,
                         float* scores, float* log_ring, int log_capacity, uint32_t* log_count,
                         uint32_t* log_seq, void* stream);
/* Pinned host memory, mapped under the same pointer on the device, fine-grained coherent, zeroed. */
int stv_host_mailbox_alloc(size_t bytes, void** out);
void stv_host_mailbox_free(void* p);

/* ---- Optimizer updates (torch.optim.LBFGS.step / Adam.step driven from
 *      optimization.py:175), device resident: no host synchronisation. ----- */

typedef struct stv_lbfgs_state stv_lbfgs_state;  /* opaque, lives in device memory */
size_t stv_lbfgs_state_bytes(int history);
size_t stv_lbfgs_workspace_bytes(size_t n, int history);
/* state/workspace zero-initialised by the caller before the first step. */
int stv_lbfgs_step(float* x, const float* grad, void* state, void* workspace, size_t n,
                   int history, int m_max, float lr, float tol_grad, float tol_change,
                   void* stream);
/* Same update with the history read twice per step instead of through 2m dependent
 * passes (inner products of {s_i},{y_i},g kept in S x S tables; see lbfgs_compact.hip).
 * Own state/workspace layout; both zero-initialised by the caller. */
size_t stv_lbfgsc_state_bytes(int history);
size_t stv_lbfgsc_workspace_bytes(size_t n, int history);
int stv_lbfgsc_step(float* x, const float* grad, void* state, void* workspace, size_t n,
                    int history, int m_max, float lr, float tol_grad, float tol_change,
                    void* stream);
/* The same step in two halves, for an image sharded over several processes (one 4K image as row strips,
 * DESIGN.md §6): stv_lbfgsc_dots leaves the step's inner products - partial sums over THIS shard - as
 * doubles in the workspace at stv_lbfgsc_dots_offset(); the caller all-reduces them (SUM, except entry
 * *max_index = max|g|: MAX) and stv_lbfgsc_apply then runs the identical scalar recursion on every shard
 * and updates its own elements.  stv_lbfgsc_step == dots + apply. */
int stv_lbfgsc_dots(const float* grad, void* state, void* workspace, size_t n, int history, int m_max, void* stream);
int stv_lbfgsc_apply(float* x, const float* grad, void* state, void* workspace, size_t n, int history, float lr,
                     float tol_grad, float tol_change, void* stream);
size_t stv_lbfgsc_dots_offset(size_t n, int history, int* count, int* max_index);
/* Since version 117.  The launch geometry a step over n elements will use (host arithmetic: no launch, no device
 * access), with the STV_LBFGS_TILE / STV_LBFGS_TILE_B / STV_LBFGS_PGROUPS overrides applied: *nn = n padded to the pitch
 * (d, prev_g and every S / Y row are *nn floats, laid out d | prev_g | S[history+1] | Y[history+1]), sweep A's tile in
 * floats, its tile count and the number of workgroups a tile's history pairs are dealt to, sweep B's tile in floats.
 * Any out pointer may be NULL.  For tests and tools: which kernel instantiation a size reaches. */
int stv_lbfgsc_geometry(size_t n, int history, size_t* nn, int* tile_a, int* ntiles, int* pgroups, int* tile_b);
/* Since version 103.  torch.optim.LBFGS.step with max_iter > 1 (no line search), one call per iteration:
 * `iters_per_step` consecutive calls on one state block are ONE optimizer step, each behind the evaluation of the
 * image the previous call left.  iters_per_step = min(max_iter, max(1, max_eval - 1)) is known on the host; the step's
 * data-dependent exits are decided on the device and nothing is read back: the position inside the step and a
 * live/dead flag live in the state block, so the same call (one captured program) serves every position.
 *   call 1:  max|g| <= tol_grad                              -> nothing changes (torch's early return), rest of the step dead
 *   call k>1, tested in front of any state change, each:      -> nothing changes, rest of the step dead
 *            max|g| <= tol_grad,  max|fl32(d*t)| <= tol_change (d, t of the previous iteration),
 *            |loss - prev_loss| < tol_change (formed in double from the two fp32 values; NaN never stops)
 *   g.d > -tol_change                                         -> state saved, image not moved, rest of the step dead
 * A dead call is a no-op, so the caller keeps issuing the step's remaining evaluations + calls: they see an unchanged
 * image.  `loss`: device fp32 scalar, the total score of the evaluation that produced `grad`.  With
 * iters_per_step = 1 the call is bit-identical to stv_lbfgsc_step (image and workspace).  State and workspace are the
 * ones of stv_lbfgsc_step; m_max counts iterations.  stv_lbfgsc_iter_reset: the step was abandoned midway (the closure
 * raised) - the next call is call 1 of a new step; an enqueue on `stream`, not a synchronisation.
 * The sharded halves (stv_lbfgsc_dots / _apply) and stv_lbfgs_step stay one iteration per step. */
int stv_lbfgsc_iter(float* x, const float* grad, const float* loss, void* state, void* workspace, size_t n,
                    int history, int m_max, int iters_per_step, float lr, float tol_grad, float tol_change,
                    void* stream);
int stv_lbfgsc_iter_reset(void* state, void* stream);
/* scalars are computed in double on the host exactly as torch does
 * (1-beta1, 1-beta2, 1-beta1**t, sqrt(1-beta2**t)) and passed rounded to fp32 */
int stv_adam_step(float* x, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                  float lr, float one_minus_beta1, float beta2, float one_minus_beta2, float eps,
                  float bias_c1, float bias_c2_sqrt, void* stream);

/* ---- Command-buffer executor: one call runs a whole forward(+backward)
 *      schedule built by the host (style_transfer_visualizer_amd/plan.py);
 *      optionally captured into a hipGraph and replayed. ------------------- */
enum {
  STV_OP_CONV_FIRST_FWD = 1, STV_OP_CONV_FIRST_DGRAD, STV_OP_CONV, STV_OP_POOL_FWD,
  STV_OP_POOL_BWD, STV_OP_RELU_FWD, STV_OP_RELU_BWD, STV_OP_GRAM_PARTIAL,
  STV_OP_GRAM_FINISH, STV_OP_CONTENT_LOSS, STV_OP_CONTENT_GRAD, STV_OP_LOSS_COMBINE,
  STV_OP_MEMSET, STV_OP_GRAM_MULTI, STV_OP_LBFGS_STEP, STV_OP_LBFGS_ITER, STV_OP_TV,
  STV_OP_LAP, STV_OP_MASK_SPLIT, STV_OP_AVGPOOL_FWD, STV_OP_AVGPOOL_BWD
};
/* Operands follow the direct entry points' argument order (inputs p0.., outputs q0..).
 * CONV_FIRST_FWD takes the stv_conv_first_pack buffer in p3 (p1 unused) and gram_partials, or NULL, in q1;
 * CONV_FIRST_DGRAD takes the buffer in p2 (p1 unused); without the buffer either is STV_ERR_ARG.
 * CONV with q1 set runs stv_conv_igemm_pool (q1 = pooled output, q2 = optional arg-max map); CONV with q2 AND q3 set runs
 * stv_conv_igemm_dual (q2 = x2, q3 = w2, n = cin2: inputs, despite the slot names).
 * GRAM_MULTI: p0 = HOST pointer to an array of stv_gram_tap_t, n = its length; the array is
 * copied into the program when it is created.
 * CONTENT_LOSS with q1 set runs stv_content_loss_grad (q1 = dF, f0 = coef).
 * LOSS_COMBINE with q2 AND q3 set runs stv_loss_combine_log (q2 = log_ring, q3 = log_count, n = log_capacity, p3 = log_seq).
 * LBFGS_STEP runs stv_lbfgsc_step as the LAST op of a step's schedule (p0 = grad, q0 = x, q1 = state, q2 = workspace,
 * n = elements, cin = history, cout = m_max, f0 = lr, f1 = tol_grad, f2 = tol_change): closure and optimizer update are
 * then one replayed hipGraph - the reference's optimizer.step(closure), optimization.py:186, without a graph boundary
 * between the two.
 * LBFGS_ITER runs stv_lbfgsc_iter in the same place with the same operands, plus p1 = loss (device fp32 scalar: the
 * total score LOSS_COMBINE wrote) and taps = iters_per_step: the one program replays for every iteration of every step.
 * TV (since version 105) runs stv_tv: p0 = x, q0 = loss_part, q1 = dx, cin = C, H, W, f0 = coef, flags.
 * LAP (since version 111) runs stv_lap: p0 = x, p1 = target, q0 = cells, q1 = loss_part, q2 = dx, cin = C, H, W, cout = pool,
 * taps = mode, f0 = coef, flags.
 * MASK_SPLIT (since version 112) runs stv_mask_split: p0 = F, p1 = labels, q0 = out, n = n_pixels, cin = C, cout = R.
 * AVGPOOL_FWD (= 20, since version 113) runs stv_avgpool_fwd: p0 = x, q0 = y, H, W, cin = C, flags.
 * AVGPOOL_BWD (= 21, since version 113) runs stv_avgpool_bwd: p0 = ref (or unset), p1 = dy, q0 = dx, H, W, cin = C, flags;
 * the operand slots of POOL_FWD / POOL_BWD. */
typedef struct {
  int32_t op, dtype, flags, taps;
  int32_t H, W, cin, cout;
  int64_t n;
  float f0, f1, f2, f3;
  const void* p0; const void* p1; const void* p2; const void* p3;
  void* q0; void* q1; void* q2; void* q3;
} stv_op_t;
/* Since version 104, stv_op_t.flags holds kernel flags only (the scheduling hints of earlier versions are gone):
 * the ops of a program run in program order on the caller's stream, so a captured step is a chain of graph nodes. */

typedef struct stv_program stv_program;  /* host object */
int stv_program_create(const stv_op_t* ops, int n_ops, stv_program** out);
/* use_graph != 0: capture on first run, replay afterwards. */
int stv_program_run(stv_program* prog, int use_graph, void* stream);
/* Measurement helper: eager run with a hipEvent pair around every op (recorded on
 * `stream`); ms_out[i] = device milliseconds of op i.  Synchronises. */
int stv_program_profile(stv_program* prog, void* stream, float* ms_out, int n_out);
/* The same with each op launched `reps` times back to back inside its event pair (time divided by
 * reps): amortises the event pair's own few microseconds.  Leaves the buffers meaningless. */
int stv_program_profile_reps(stv_program* prog, void* stream, int reps, float* ms_out, int n_out);
int stv_program_op_count(const stv_program* prog);
void stv_program_destroy(stv_program* prog);

#ifdef __cplusplus
}
#endif
#endif /* STV_H_ */
