"""ctypes binding of ``libstv_hip.so`` (C ABI declared in ``include/stv.h``).

The library is the product: there is no eager/PyTorch or CPU fallback.  If it
is missing or a call fails, a ``RuntimeError`` is raised.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STV_LIB_PATH") or os.path.join(_HERE, "libstv_hip.so")   # override: diagnostic builds

STV_F32, STV_BF16, STV_BF16X3 = 0, 1, 2     # STV_BF16X3: fp32 storage, split-bf16 products
TUNE_BF16X3 = 6     # stv.h STV_TUNE_BF16X3: the `elem_bytes` key of a bf16x3 tile-table entry
RELU_IN, RELU_OUT, MASK, ACCUM, W_BLOCKED, POOL_IDX, POOL_ROUTE, POOL_ONLY = 1, 2, 4, 8, 16, 32, 64, 128

(OP_CONV_FIRST_FWD, OP_CONV_FIRST_DGRAD, OP_CONV, OP_POOL_FWD, OP_POOL_BWD, OP_RELU_FWD,
 OP_RELU_BWD, OP_GRAM_PARTIAL, OP_GRAM_FINISH, OP_CONTENT_LOSS, OP_CONTENT_GRAD,
 OP_LOSS_COMBINE, OP_MEMSET, OP_GRAM_MULTI, OP_LBFGS_STEP, OP_LBFGS_ITER, OP_TV, OP_LAP, OP_MASK_SPLIT, OP_AVGPOOL_FWD, OP_AVGPOOL_BWD) = range(1, 22)

CONTENT_LOSS_PARTS = 256
TV_LOSS_PARTS = 256       # stv.h STV_TV_LOSS_PARTS: one loss partial per workgroup of stv_tv, which is also its grid cap
# launch constants of stv_tv (csrc/pointwise.hip: kTvThreads, pixels per work item): a work item is TV_VEC consecutive
# pixels of one row, a pass of the capped grid covers TV_LOSS_PARTS * TV_THREADS items
TV_THREADS, TV_VEC = 1024, 4
KIND_STYLE, KIND_CONTENT, KIND_EXTRA = 0, 1, 2      # third column of the combine table
# stv_lap (stv.h STV_LAP_*; csrc/lap.hip): its modes; the pool sizes it takes; its launch constants - workgroups of LAP_THREADS,
# the LOSS mode one tile of LAP_TILE_H x LAP_TILE_W pooled cells per workgroup on a grid of always LAP_LOSS_PARTS workgroups
# (one loss partial each) with a stride loop over the tiles, the GRAD mode LAP_VEC consecutive pixels of a row per work item,
# a pass of its capped grid LAP_GRAD_MAX_BLOCKS * LAP_THREADS items
LAP_POOL, LAP_LOSS, LAP_GRAD = 0, 1, 2
LAP_POOLS = (1, 2, 4, 8, 16, 32)
LAP_THREADS, LAP_TILE_H, LAP_TILE_W, LAP_LOSS_PARTS, LAP_GRAD_MAX_BLOCKS, LAP_VEC = 256, 8, 32, 256, 512, 4
# launch constants of stv_mask_split (stv.h STV_MASK_*; csrc/guide.hip): at most MASK_MAX_REGIONS slabs, a work item is 16 bytes
# of one pixel's channels, a pass of the capped grid covers MASK_SPLIT_MAX_BLOCKS * MASK_SPLIT_THREADS items
MASK_MAX_REGIONS, MASK_SPLIT_THREADS, MASK_SPLIT_MAX_BLOCKS = 4, 256, 1024
# launch constants of stv_avgpool_fwd / stv_avgpool_bwd (stv.h STV_AVGPOOL_*; csrc/avgpool.hip): a work item is 16 bytes of one
# pooled pixel's (forward) or one 2x2 window's (backward, odd tails included) channels, a pass of the capped grid covers
# AVGPOOL_MAX_BLOCKS * AVGPOOL_THREADS items
AVGPOOL_THREADS, AVGPOOL_MAX_BLOCKS = 256, 2048
RESIZE_DOWN2, RESIZE_UP2 = 0, 1                     # stv.h STV_RESIZE_*: the modes of stv_resize2x
# launch constants of stv_resize2x (stv.h STV_RESIZE_THREADS, STV_RESIZE_MAX_BLOCKS; pixels per work item): a work item is
# RESIZE_VEC consecutive OUTPUT pixels of one row, a pass of the capped grid covers RESIZE_MAX_BLOCKS * RESIZE_THREADS items
RESIZE_THREADS, RESIZE_MAX_BLOCKS, RESIZE_VEC = 256, 1024, 4
# launch constants of stv_resize_axis (stv.h STV_RESIZE_AXIS_*; csrc/resize.hip), with the same meaning: a work item is
# RESIZE_AXIS_VEC consecutive OUTPUT pixels of one row, a pass covers RESIZE_AXIS_MAX_BLOCKS * RESIZE_AXIS_THREADS items
RESIZE_AXIS_THREADS, RESIZE_AXIS_MAX_BLOCKS, RESIZE_AXIS_VEC = 256, 1024, 4
# launch constants of the three colour kernels (stv.h STV_COLOR_*; csrc/color.hip): a work item is COLOR_VEC consecutive
# pixels of one row read from all three planes; stv_color_stats always runs COLOR_STATS_PARTS workgroups (one row of nine
# doubles each), stv_color_affine and stv_luma_transfer at most COLOR_MAX_BLOCKS, all of COLOR_THREADS threads
COLOR_VEC, COLOR_THREADS, COLOR_STATS_PARTS, COLOR_MAX_BLOCKS = 4, 256, 256, 1024
# launch constants of stv_kmeans_assign (stv.h STV_KMEANS_*; csrc/kmeans.hip): the walk of the colour kernels, always
# KMEANS_PARTS workgroups of KMEANS_THREADS threads, one row of KMEANS_PART_DOUBLES doubles each - for k < KMEANS_MAX_K at
# 4k..4k+3 the sums of the three channels and the count of label k, at [16] the changed labels
KMEANS_THREADS, KMEANS_PARTS, KMEANS_PART_DOUBLES, KMEANS_MAX_K = 256, 256, 17, 4
# launch constants of stv_kmeans_feat_assign / stv_kmeans_feat_update (stv.h STV_KMF_*; csrc/kmeans_feat.hip): a pixel of C
# channels belongs to C/8 lanes of one wave, a wave holds 64 / (C/8) pixels at a time, always KMF_PARTS workgroups of
# KMF_THREADS threads (KMF_WAVES waves), one row of kmf_row_doubles(C) doubles each
KMF_THREADS, KMF_WAVES, KMF_PARTS, KMF_MAX_K, KMF_MAX_C = 256, 4, 256, 4, 512
KMF_CHANNELS = (64, 128, 256, 512)      # the channel counts the kernels take: C/8 lanes per pixel, a power of two


def kmf_row_doubles(C: int) -> int:
    """``STV_KMF_ROW_DOUBLES(C)``: per cluster ``k < 4`` the ``C`` channel sums and the count at ``k*(C+1)``, then the changed
    count."""
    return 4 * (C + 1) + 1


def kmf_geometry(C: int) -> tuple[int, int, int]:
    """``(Q, G, pixels per pass of the grid)`` for ``C`` channels: lanes per pixel, pixels per wave, ``KMF_PARTS * KMF_WAVES * G``."""
    Q = C // 8
    G = 64 // Q
    return Q, G, KMF_PARTS * KMF_WAVES * G

# launch constants of stv_gram_blend (stv.h STV_BLEND_*; csrc/blend.hip): at most BLEND_MAX_TABLES tables per launch, a work
# item is BLEND_VEC consecutive elements, a pass of the capped grid covers BLEND_MAX_BLOCKS * BLEND_THREADS items
BLEND_MAX_TABLES, BLEND_VEC, BLEND_THREADS, BLEND_MAX_BLOCKS = 8, 4, 256, 128
# launch constants of stv_frame_hist / stv_gif_map (stv.h STV_GIF_*; csrc/gif.hip): a work item is GIF_VEC consecutive pixels
# of the flat frame, a pass of the capped grid covers GIF_MAX_BLOCKS * GIF_THREADS items; the histogram has GIF_HIST_BINS
# 32-bit counters (five bits per channel)
GIF_THREADS, GIF_MAX_BLOCKS, GIF_VEC, GIF_HIST_BINS = 256, 2048, 4, 32768
# constants of the four JPEG kernels (stv.h STV_JPEG_*; csrc/jpeg.hip): stv_jpeg_dct runs workgroups of JPEG_DCT_THREADS, eight
# lanes per 8x8 block; the entropy kernels workgroups of JPEG_THREADS, a work item one block; a block's code has at most
# JPEG_MAX_BLOCK_BITS bits and bit offsets are 32 bits wide; a frame side is at most JPEG_MAX_DIM; JPEG_DCT_TABLE is
# T[u][x] = rint(8192 * c(u)/2 * cos((2x+1) u pi / 16)) as the header spells it
JPEG_DCT_THREADS, JPEG_THREADS, JPEG_MAX_BLOCK_BITS, JPEG_MAX_DIM = 256, 256, 1664, 65535
JPEG_DCT_TABLE = (
    (2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896),
    (4017, 3406, 2276, 799, -799, -2276, -3406, -4017),
    (3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784),
    (3406, -799, -4017, -2276, 2276, 4017, 799, -3406),
    (2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896),
    (2276, -4017, 799, 3406, -3406, -799, 4017, -2276),
    (1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567),
    (799, -2276, 3406, -4017, 4017, -3406, 2276, -799),
)

_ERRORS = {1: "STV_ERR_ARG (unsupported shape / null pointer / dtype)",
           2: "STV_ERR_LAUNCH (HIP launch failed)", 3: "STV_ERR_ALLOC", 4: "STV_ERR_GRAPH"}


class StvOp(ctypes.Structure):
    """Mirror of ``stv_op_t`` (include/stv.h)."""

    _fields_ = [
        ("op", c_int32), ("dtype", c_int32), ("flags", c_int32), ("taps", c_int32),
        ("H", c_int32), ("W", c_int32), ("cin", c_int32), ("cout", c_int32),
        ("n", c_int64),
        ("f0", c_float), ("f1", c_float), ("f2", c_float), ("f3", c_float),
        ("p0", c_void_p), ("p1", c_void_p), ("p2", c_void_p), ("p3", c_void_p),
        ("q0", c_void_p), ("q1", c_void_p), ("q2", c_void_p), ("q3", c_void_p),
    ]


class StvGramTap(ctypes.Structure):
    """Mirror of ``stv_gram_tap_t`` (include/stv.h)."""

    _fields_ = [
        ("F", c_void_p), ("partials", c_void_p), ("target", c_void_p), ("gram_out", c_void_p),
        ("loss_part", c_void_p), ("sgrad", c_void_p), ("coef_dev", c_void_p),
        ("n_pixels", c_int32), ("channels", c_int32),
        ("clamp_max", c_float), ("norm", c_float), ("coef", c_float),
    ]

    def fill(self, *, n_pixels: int, channels: int, clamp_max: float, coef: float, partials: int, F: int | None = None,
             target: int | None = None, gram_out: int | None = None, loss_part: int | None = None,
             sgrad: int | None = None, coef_dev: int | None = None, norm: float | None = None) -> None:
        """One tap of a batched Gram chain from device addresses (None: absent; ``F`` absent: the slabs are already
        filled).  ``norm`` is the reference's ``b*c*h*w`` unless given (a guided region: ``c`` times its pixel count)."""
        self.F, self.partials, self.target, self.gram_out = F, partials, target, gram_out
        self.loss_part, self.sgrad, self.coef_dev = loss_part, sgrad, coef_dev
        self.n_pixels, self.channels = n_pixels, channels
        self.clamp_max, self.norm, self.coef = clamp_max, float(channels * n_pixels) if norm is None else float(norm), float(coef)


# name -> (restype, argtypes); every symbol include/stv.h declares
SIGNATURES = {
    "stv_version": (c_int, []),
    "stv_gram_partials_bytes": (c_size_t, [c_int, c_int]),
    "stv_gram_ksplit": (c_int, [c_int, c_int]),
    "stv_gram_loss_parts": (c_int, [c_int]),
    "stv_conv_first_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "stv_conv_first_dgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "stv_conv_first_packed_bytes": (c_size_t, [c_int, c_int]),
    "stv_conv_first_pack": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "stv_conv_first_gram_supported": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "stv_conv_igemm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "stv_conv_igemm_pool": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_void_p]),
    "stv_conv_igemm_route": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "stv_conv_igemm_dual": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                    c_int, c_int, c_int, c_void_p]),
    "stv_conv_tune": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "stv_conv_tune_export": (c_int, [ctypes.POINTER(c_int), c_int]),
    "stv_conv_tune_import": (c_int, [ctypes.POINTER(c_int), c_int]),
    "stv_conv_next_weights": (None, [c_void_p, c_size_t]),
    "stv_conv_num_configs": (c_int, []),
    "stv_conv_last_launch": (c_int, []),
    "stv_conv_uses_ws": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "stv_conv_config": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "stv_conv_fits": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "stv_maxpool_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "stv_maxpool_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "stv_avgpool_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "stv_avgpool_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "stv_relu_fwd": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "stv_relu_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p]),
    "stv_gram_partial": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "stv_gram_finish": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float, c_void_p, c_int, c_void_p]),
    "stv_gram_multi": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "stv_content_loss": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "stv_content_loss_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_float, c_int, c_void_p]),
    "stv_content_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_float, c_void_p, c_int, c_int, c_void_p]),
    "stv_tv": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p]),
    "stv_lap": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p]),
    "stv_mask_split": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p]),
    "stv_resize2x": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "stv_resize_axis": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "stv_color_stats": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "stv_color_affine": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_float), c_int, c_int, c_void_p]),
    "stv_luma_transfer": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.POINTER(c_float), ctypes.POINTER(c_float), c_void_p]),
    "stv_kmeans_assign": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "stv_kmeans_feat_assign": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "stv_kmeans_feat_update": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "stv_gram_blend": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_float), c_int, c_int64, c_void_p]),
    "stv_image_to_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.POINTER(c_float), ctypes.POINTER(c_float), c_int, c_void_p]),
    "stv_frame_hist": (c_int, [c_void_p, c_size_t, c_void_p, c_void_p]),
    "stv_gif_map": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "stv_jpeg_dct": (c_int, [c_void_p, ctypes.POINTER(c_int), c_int, c_int, c_void_p, c_void_p]),
    "stv_jpeg_block_bits": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "stv_jpeg_scan": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "stv_jpeg_emit": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "stv_loss_combine": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "stv_loss_combine_log": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                     c_int, c_void_p, c_void_p, c_void_p]),
    "stv_host_mailbox_alloc": (c_int, [c_size_t, ctypes.POINTER(c_void_p)]),
    "stv_host_mailbox_free": (None, [c_void_p]),
    "stv_lbfgs_state_bytes": (c_size_t, [c_int]),
    "stv_lbfgs_workspace_bytes": (c_size_t, [c_size_t, c_int]),
    "stv_lbfgs_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_float, c_float, c_float, c_void_p]),
    "stv_lbfgsc_state_bytes": (c_size_t, [c_int]),
    "stv_lbfgsc_workspace_bytes": (c_size_t, [c_size_t, c_int]),
    "stv_lbfgsc_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_float, c_float, c_float, c_void_p]),
    "stv_lbfgsc_dots": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p]),
    "stv_lbfgsc_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_float, c_float, c_float, c_void_p]),
    "stv_lbfgsc_dots_offset": (c_size_t, [c_size_t, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "stv_lbfgsc_geometry": (c_int, [c_size_t, c_int, ctypes.POINTER(c_size_t), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                                    ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "stv_lbfgsc_iter": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_float, c_float, c_float,
                                c_void_p]),
    "stv_lbfgsc_iter_reset": (c_int, [c_void_p, c_void_p]),
    "stv_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_float, c_float, c_float, c_float, c_float, c_float, c_float, c_void_p]),
    "stv_program_create": (c_int, [ctypes.POINTER(StvOp), c_int, ctypes.POINTER(c_void_p)]),
    "stv_program_run": (c_int, [c_void_p, c_int, c_void_p]),
    "stv_program_profile": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_float), c_int]),
    "stv_program_profile_reps": (c_int, [c_void_p, c_void_p, c_int, ctypes.POINTER(c_float), c_int]),
    "stv_program_op_count": (c_int, [c_void_p]),
    "stv_program_destroy": (None, [c_void_p]),
}

_lib = None


def load() -> ctypes.CDLL:
    """Load the HIP library or fail loudly (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    # Load order matters: PyTorch ships its own libamdhip64; if this library pulled in the system copy
    # first, the process would hold two HIP runtimes and every pointer / stream handed over from torch
    # would be foreign to the kernels here (seen as STV_ERR_LAUNCH on the first call).
    import torch  # noqa: F401, PLC0415
    if not os.path.exists(LIB_PATH):
        msg = (f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
               "(hipcc --offload-arch=gfx950). There is no CPU/eager fallback for this path.")
        raise RuntimeError(msg)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    _import_tile_table(lib)
    return lib


TILE_TABLE_PATH = os.environ.get("STV_TILE_TABLE") or os.path.join(_HERE, "conv_tiles_gfx950.json")
tile_table_info: dict = {"source": None, "entries": 0}


def _import_tile_table(lib: ctypes.CDLL) -> None:
    """Hand the persisted tile choices (tools/tune_tiles.py, measured on an MI355X) to the library: which tile a
    conv shape runs on is then the same in every process (results bit-reproducible run to run, kernel names in a
    profile reproducible).  STV_CONV_TUNE=0 makes the library ignore the table (analytic choice); =1 re-measures
    shapes the table does not hold.  A missing file is fine: analytic choices."""
    import json  # noqa: PLC0415
    import warnings  # noqa: PLC0415
    if not os.path.exists(TILE_TABLE_PATH):
        return

    def give_up(why: str) -> None:
        # a table the library cannot take (a tile index that no longer exists, a malformed entry, another device's
        # measurements) must not make the package unusable: forget it and run on the analytic choices
        lib.stv_conv_tune_import(None, 0)
        tile_table_info.update(source=None, entries=0, ignored=f"{os.path.basename(TILE_TABLE_PATH)}: {why}")
        warnings.warn(f"conv tile table {TILE_TABLE_PATH} ignored ({why}): analytic tile choices", RuntimeWarning, stacklevel=3)
    try:
        with open(TILE_TABLE_PATH) as fh:
            doc = json.load(fh)
        rows = [int(v) for e in doc.get("entries", []) for v in (e["H"], e["W"], e["cin"], e["cout"], e["taps"], e["elem_bytes"], e["cfg"])]
    except (OSError, ValueError, KeyError, TypeError, AttributeError) as exc:
        give_up(f"unreadable: {exc!r}")
        return
    if not rows:
        return
    arch = _device_arch()
    measured_on = str(doc.get("arch") or "")
    if arch is not None and measured_on and arch != measured_on:
        give_up(f"measured on {measured_on}, this device is {arch}")
        return
    arr = (c_int * len(rows))(*rows)
    rc = lib.stv_conv_tune_import(arr, len(rows) // 7)
    if rc != 0:
        give_up(f"stv_conv_tune_import: {_ERRORS.get(rc, rc)}")
        return
    tile_table_info.update(source=os.path.basename(TILE_TABLE_PATH), entries=len(rows) // 7, measured_on=doc.get("device"),
                           tool=doc.get("tool"))


def _device_arch() -> str | None:
    """gcnArchName of the current GPU ("gfx950"), or None when there is none (host-only use of the library)."""
    import torch  # noqa: PLC0415
    try:
        if torch.cuda.device_count() == 0 or not torch.cuda.is_available():
            return None
        return str(torch.cuda.get_device_properties(torch.cuda.current_device()).gcnArchName).split(":")[0]
    except (RuntimeError, AttributeError, AssertionError):
        return None


def export_tile_table() -> list[dict]:
    """The library's current tile table (imported + measured in this process) as a list of dicts."""
    lib = load()
    n = int(lib.stv_conv_tune_export(None, 0))
    arr = (c_int * (7 * max(n, 1)))()
    n = min(n, int(lib.stv_conv_tune_export(arr, n)))
    keys = ("H", "W", "cin", "cout", "taps", "elem_bytes", "cfg")
    return [dict(zip(keys, (int(arr[7 * i + k]) for k in range(7)), strict=True)) for i in range(n)]


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = f"{what} failed: {_ERRORS.get(rc, rc)}"
        raise RuntimeError(msg)
